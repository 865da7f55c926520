"""The replay buffer on the GPU (csrc/mpe_replay.hip): one-launch push, one-launch sampled gather, the closed loop and its graph.
Both kernels only move data, so every comparison is equality -- bit-equal floats, equal integers -- against the NumPy ring and the
draw rule restated in tests/_replay_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop
from multiagent_particle_envs_amd.replay import ReplayBuffer

import _replay_ref as R

pytestmark = pytest.mark.gpu


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def push_coded(buf, T):
    """T synthetic steps into buf and into a NumPy ring of the same shape -> the NumPy ring."""
    ring = R.NumpyRing(buf.S, buf.B, buf.obs_widths, buf.dim_c)
    for t in range(T):
        obs, moves, utter, nxt, rew, done = R.coded_step(t, buf.B, buf.obs_widths, buf.dim_c)
        action = (dev(moves), dev(utter)) if buf.dim_c else dev(moves)
        buf.push([dev(o) for o in obs], action, [dev(o) for o in nxt], dev(rew), dev(done))
        ring.push(obs, moves, utter, nxt, rew, done)
    torch.cuda.synchronize()
    return ring


def assert_ring_equal(buf, ring):
    assert int(buf.head.item()) == buf.count == ring.count
    assert int(buf._ticket.item()) == 0
    for s in range(buf.S):
        for i in range(buf.A):
            assert np.array_equal(buf.obs_n[s][i].cpu().numpy(), ring.obs[s][i]), ("obs", s, i)
            assert np.array_equal(buf.next_obs_n[s][i].cpu().numpy(), ring.next_obs[s][i]), ("next_obs", s, i)
    assert np.array_equal(buf.act.cpu().numpy(), ring.act)
    assert np.array_equal(buf.rew.cpu().numpy(), ring.rew)
    assert np.array_equal(buf.done.cpu().numpy(), ring.done)
    if buf.dim_c:
        assert np.array_equal(buf.utter.cpu().numpy(), ring.utter)


@pytest.mark.parametrize("name,B", [("simple_adversary", 5), ("simple_speaker_listener", 7), ("simple_reference", 7),
                                    ("simple_adversary", 64)])
def test_push_fills_the_ring_through_two_wraps(name, B):
    """S = 3, 7 steps: slots hold steps 6, 4, 5.  B = 5 / 7: agent blocks and slots at 4-byte alignment only (the dword path), the
    done bytes aligned to nothing (the byte path); B = 64: everything 16-byte aligned (the vector path)."""
    env = mpe.make_env(name, batch_size=B, seed=1)
    buf = ReplayBuffer(env, steps=3)
    ring = push_coded(buf, 7)
    assert buf.count == 7 and len(buf) == 3 * B
    assert_ring_equal(buf, ring)
    assert float(buf.act[0, 0, 0, 0]) == R.coded(6, "act", 0, B, 5)[0, 0]      # slot 0 holds step 6


def test_push_takes_env_step_outputs_as_they_are():
    """push(obs_n, action, *env.step(action)[:3]): per-agent reward / done rows of one [A,B] tensor, no copies in front."""
    B = 6
    env = mpe.make_env("simple_spread", batch_size=B, seed=3)
    obs_n = [o.clone() for o in env.reset()]
    buf = ReplayBuffer(env, steps=2)
    act = dev(np.eye(5, dtype=np.float32)[np.random.RandomState(0).randint(0, 5, size=(3, B))])
    nxt, rew, done, _ = env.step(act)
    buf.push(obs_n, act, nxt, rew, done)
    torch.cuda.synchronize()
    assert all(torch.equal(buf.obs_n[0][i], obs_n[i]) and torch.equal(buf.next_obs_n[0][i], nxt[i]) for i in range(3))
    assert torch.equal(buf.act[0], act) and torch.equal(buf.rew[0], torch.stack(rew)) and torch.equal(buf.done[0], torch.stack(done))
    assert len(buf._ptrs) == 1
    with pytest.raises(_abi.MpeError, match="obs_n\\[0\\]"):
        buf.push([o[:, :5].contiguous() for o in obs_n], act, nxt, rew, done)
    assert buf.count == 1 and int(buf.head.item()) == 1


@pytest.fixture(scope="module")
def rings():
    """simple_speaker_listener (an immovable speaker, a silent listener) at B = 7, S = 3: one ring with count < S, one wrapped."""
    out = {}
    for tag, T in (("partial", 2), ("wrapped", 7)):
        env = mpe.make_env("simple_speaker_listener", batch_size=7, seed=1)
        buf = ReplayBuffer(env, steps=3, seed=0xC0FFEE12345)
        out[tag] = (buf, push_coded(buf, T))
    return out


@pytest.mark.parametrize("tag", ["partial", "wrapped"])
@pytest.mark.parametrize("M", [1, 7, 257, 1000])
def test_sample_matches_the_restated_draw_and_the_numpy_gather(rings, tag, M):
    buf, ring = rings[tag]
    draw = 3 + M
    b = buf.sample(M, draw=draw, joint=True)
    torch.cuda.synchronize()
    want = R.draw_indices(buf.seed, draw, M, ring.n_valid())
    assert ring.n_valid() == len(buf) == (14 if tag == "partial" else 21)
    assert b.idx.cpu().tolist() == want
    g = ring.gather(want)
    for i in range(buf.A):
        assert np.array_equal(b.obs_n[i].cpu().numpy(), g["obs_n"][i]), i
        assert np.array_equal(b.next_obs_n[i].cpu().numpy(), g["next_obs_n"][i]), i
    for f in ("act", "utter", "rew", "done"):
        assert np.array_equal(getattr(b, f).cpu().numpy(), g[f]), f
    assert b.done.dtype == torch.bool
    # joint: every agent's observation, then the speaker's utterance row (it cannot move), then the listener's move row
    assert buf.movable == [False, True] and buf.speaks == [True, False]
    assert torch.equal(b.joint, torch.cat([b.obs_n[0], b.obs_n[1], b.utter[0], b.act[1]], dim=1))
    assert torch.equal(b.joint_next, torch.cat(b.next_obs_n, dim=1))
    assert b.joint.shape == (M, buf.joint_width) and buf.joint_width == sum(buf.obs_widths) + 3 + 5


def test_sample_is_a_function_of_seed_and_draw(rings):
    buf, ring = rings["wrapped"]
    a = buf.sample(257, draw=11)
    keep = [a.idx.clone(), a.act.clone(), a.rew.clone()] + [o.clone() for o in a.obs_n]
    b = buf.sample(257, draw=12)
    assert b is a and not torch.equal(b.idx, keep[0])
    c = buf.sample(257, draw=11)
    assert all(torch.equal(x, y) for x, y in zip([c.idx, c.act, c.rew] + list(c.obs_n), keep))
    assert c.joint is None
    d0 = buf._draw      # draw=None: the internal counter
    i1 = buf.sample(257).idx.clone()
    assert buf._draw == d0 + 1 and i1.cpu().tolist() == R.draw_indices(buf.seed, d0, 257, ring.n_valid())
    # simple_adversary: every agent moves, nobody speaks -> joint = obs rows then move rows
    env = mpe.make_env("simple_adversary", batch_size=5, seed=1)
    buf2 = ReplayBuffer(env, steps=3, seed=9)
    ring2 = push_coded(buf2, 4)
    s = buf2.sample(100, draw=0, joint=True)
    assert s.idx.cpu().tolist() == R.draw_indices(9, 0, 100, ring2.n_valid()) and s.utter is None
    assert torch.equal(s.joint, torch.cat(list(s.obs_n) + [s.act[i] for i in range(3)], dim=1))
    assert np.array_equal(s.rew.cpu().numpy(), ring2.gather(s.idx.cpu().tolist())["rew"])


def actors(env):
    torch.manual_seed(3)
    return [torch.nn.Sequential(torch.nn.Linear(d, 32), torch.nn.ReLU(), torch.nn.Linear(32, 5)).cuda() for d in
            [o.shape[1] for o in env.reset()]]


def spread_loop(mods=None, B=6):
    env = mpe.make_env("simple_spread", batch_size=B, seed=11)
    mods = actors(env) if mods is None else mods
    env.reset()
    return env, PolicyLoop(env, Actors(env, mods, mode="sample", seed=5), episode_len=4), mods


def test_loop_pushes_every_step_and_episode_boundaries_fall_out_of_the_call_order():
    env, loop, mods = spread_loop()
    buf = ReplayBuffer(env, steps=16)
    traj = loop.run(10, replay=buf)
    torch.cuda.synchronize()
    assert buf.count == 10 and int(buf.head.item()) == 10
    assert torch.equal(buf.act[:10], traj.act) and torch.equal(buf.rew[:10], traj.rew) and torch.equal(buf.done[:10], traj.done)
    assert torch.equal(buf.next_obs[:10], traj.obs_flat)
    assert not buf.obs[10:].any() and not buf.next_obs[10:].any()
    env2, loop2, _ = spread_loop(mods)
    for t in range(10):
        if t % 4:
            assert torch.equal(buf.obs[t], buf.next_obs[t - 1]), t
        else:      # the first step of an episode was decided on the observation of the reset state
            reset_obs = loop2.device_reset(t // 4)
            torch.cuda.synchronize()
            assert all(torch.equal(buf.obs_n[t][i], reset_obs[i]) for i in range(3)), t
            if t:
                assert not torch.equal(buf.obs[t], buf.next_obs[t - 1]), t
    # replay=None changes nothing: the same run without a buffer gives the same trajectory
    env3, loop3, _ = spread_loop(mods)
    traj3 = loop3.run(10)
    assert torch.equal(traj3.obs_flat, traj.obs_flat) and torch.equal(traj3.act, traj.act) and torch.equal(traj3.rew, traj.rew)


def test_captured_loop_moves_to_new_slots_at_every_replay():
    env, loop, mods = spread_loop()
    buf = ReplayBuffer(env, steps=16)
    g = loop.capture(8, replay=buf)
    torch.cuda.synchronize()
    assert buf.count == 0 and int(buf.head.item()) == 0      # the warm-up steps' pushes were taken back
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert buf.count == 16 and int(buf.head.item()) == 16 and len(buf) == 16 * 6 and int(buf._ticket.item()) == 0
    env2, loop2, _ = spread_loop(mods)
    eager = ReplayBuffer(env2, steps=16)
    loop2.run(8, record=False, replay=eager)
    torch.cuda.synchronize()
    for f in ("obs", "next_obs", "act", "rew", "done"):
        ring, want = getattr(buf, f), getattr(eager, f)
        assert torch.equal(ring[:8], ring[8:]), f      # a replay repeats its keys
        assert torch.equal(ring[:8], want[:8]), f
    assert buf.act[:8].any() and buf.next_obs[:8].any()


def raw_ring(A, B, S, D, skew):
    """A ring in plain tensors whose every field starts `skew` elements into its allocation (so 4 * skew bytes, or skew bytes for
    done, past a 16-byte boundary), with guard elements on both sides -> (descriptor, fields {name: (whole tensor, view)})."""
    shapes = {"obs": (S, A * D * B), "next_obs": (S, A * D * B), "act": (S, A, B, 5), "rew": (S, A, B), "done": (S, A, B)}
    f = {}
    for name, shape in shapes.items():
        n = int(np.prod(shape))
        whole = torch.full((n + 2 * 16,), 77, dtype=torch.uint8 if name == "done" else torch.float32, device="cuda")
        f[name] = (whole, whole[skew: skew + n].view(shape))
    d = _abi.MpeReplay()
    d.n_agents, d.B, d.S, d.dim_c = A, B, S, 0
    for i in range(A):
        d.obs_width[i], d.movable[i] = D, 1
    for name in shapes:
        setattr(d, name, f[name][1].data_ptr())
    head, ticket = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    d.head, d.ticket = head.data_ptr(), ticket.data_ptr()
    f["head"], f["ticket"] = (head, head), (ticket, ticket)
    return d, f


def test_push_peels_the_ends_of_a_congruent_but_unaligned_segment():
    """Source and ring both 12 bytes past a 16-byte boundary (done: 3 bytes), B = 4, D = 3: obs blocks of 48 bytes in 16-byte units
    with 4 bytes peeled in front and 12 behind; guard elements around every field stay as they were."""
    A, B, S, D, skew = 2, 4, 2, 3, 3
    d, f = raw_ring(A, B, S, D, skew)
    L = _abi.lib()
    ring = R.NumpyRing(S, B, [D] * A, 0)
    keep = []
    for t in range(3):
        obs, moves, _, nxt, rew, done = R.coded_step(t, B, [D] * A, 0)

        def skewed(x, dtype):
            x = np.ascontiguousarray(x)
            whole = torch.zeros(x.size + 32, dtype=dtype, device="cuda")
            view = whole[skew: skew + x.size].view(x.shape)
            view.copy_(torch.as_tensor(x))
            keep.append(whole)
            return view
        o = [skewed(x, torch.float32) for x in obs]
        n = [skewed(x, torch.float32) for x in nxt]
        mv, rw, dn = skewed(moves, torch.float32), skewed(rew, torch.float32), skewed(done.astype(np.uint8), torch.uint8)
        assert all(v.data_ptr() % 16 == 12 for v in o + n + [mv, rw]) and dn.data_ptr() % 16 == 3
        rc = L.mpe_replay_push(C.byref(d), (C.c_void_p * A)(*[x.data_ptr() for x in o]), (C.c_void_p * A)(*[x.data_ptr() for x in n]),
                               mv.data_ptr(), None, rw.data_ptr(), dn.data_ptr(), None)
        assert rc == 0, L.mpe_last_error()
        ring.push(obs, moves, None, nxt, rew, done)
    torch.cuda.synchronize()
    assert int(f["head"][0].item()) == 3 and int(f["ticket"][0].item()) == 0
    for s in range(S):
        for i in range(A):
            lo = i * D * B
            assert np.array_equal(f["obs"][1][s, lo: lo + D * B].view(B, D).cpu().numpy(), ring.obs[s][i])
            assert np.array_equal(f["next_obs"][1][s, lo: lo + D * B].view(B, D).cpu().numpy(), ring.next_obs[s][i])
    assert np.array_equal(f["act"][1].cpu().numpy(), ring.act) and np.array_equal(f["rew"][1].cpu().numpy(), ring.rew)
    assert np.array_equal(f["done"][1].cpu().numpy().astype(bool), ring.done)
    for name in ("obs", "next_obs", "act", "rew", "done"):
        whole, view = f[name]
        assert (whole[:skew] == 77).all() and (whole[skew + view.numel():] == 77).all(), name


def test_abi_refuses_every_invalid_call_by_name_and_leaves_the_ring_alone():
    A, B, S, D = 2, 4, 2, 3
    d, f = raw_ring(A, B, S, D, 0)
    L = _abi.lib()
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device="cuda")      # noqa: E731
    obs, nxt = [z(B, D) + 1 for _ in range(A)], [z(B, D) + 2 for _ in range(A)]
    mv, ut, rw, dn = z(A, B, 5) + 3, z(A, B, 4) + 4, z(A, B) + 5, z(A, B, dt=torch.uint8) + 1
    po, pn = (C.c_void_p * A)(*[x.data_ptr() for x in obs]), (C.c_void_p * A)(*[x.data_ptr() for x in nxt])
    out = {"idx": z(8, dt=torch.int64), "obs": z(A * D * 8), "next_obs": z(A * D * 8), "act": z(A, 8, 5), "utter": z(A, 8, 4),
           "rew": z(A, 8), "done": z(A, 8, dt=torch.uint8), "joint": z(8, A * D + A * 5), "joint_next": z(8, A * D)}

    def push(desc, utter=None, **kw):
        a = {"obs": po, "next": pn, "moves": mv.data_ptr(), "rew": rw.data_ptr(), "done": dn.data_ptr()}
        a.update(kw)
        return L.mpe_replay_push(C.byref(desc), a["obs"], a["next"], a["moves"], utter, a["rew"], a["done"], None)

    def sample(desc, M=8, **kw):
        a = {k: v.data_ptr() for k, v in out.items()}
        a["utter"] = None
        a.update(kw)
        return L.mpe_replay_sample(C.byref(desc), M, 0, a["idx"], a["obs"], a["next_obs"], a["act"], a["utter"], a["rew"], a["done"],
                                   a["joint"], a["joint_next"], None)

    def edited(**kw):
        e = _abi.MpeReplay.from_buffer_copy(d)
        for k, v in kw.items():
            setattr(e, k, v)
        return e
    assert push(d) == 0 and sample(d) == 0, L.mpe_last_error()      # the valid calls, once
    torch.cuda.synchronize()
    before = {k: v[0].clone() for k, v in f.items()}
    outs = {k: v.clone() for k, v in out.items()}
    assert int(before["head"].item()) == 1
    speaker = edited(dim_c=4, utter=ut.data_ptr())
    speaker.speaks[0] = 1
    mute = edited()
    mute.speaks[0] = 1
    headless = edited()
    headless.movable[1] = 0
    cases = [(lambda: push(edited(obs=None)), b"replay->obs is NULL"), (lambda: sample(edited(next_obs=None)), b"replay->next_obs is NULL"),
             (lambda: push(edited(act=None)), b"replay->act is NULL"), (lambda: push(edited(rew=None)), b"replay->rew is NULL"),
             (lambda: sample(edited(done=None)), b"replay->done is NULL"), (lambda: push(edited(head=None)), b"replay->head is NULL"),
             (lambda: push(edited(ticket=None)), b"replay->ticket is NULL"),
             (lambda: sample(edited(dim_c=4), utter=out["utter"].data_ptr()), b"replay->utter is NULL"),
             (lambda: push(edited(S=0)), b"S = 0"), (lambda: sample(edited(S=-1)), b"S = -1"),
             (lambda: push(edited(B=0)), b"B = 0"), (lambda: sample(edited(B=0)), b"B = 0"),
             (lambda: sample(d, M=0), b"M = 0"), (lambda: sample(d, M=-3), b"M = -3"),
             (lambda: push(edited(S=2 ** 38)), b"2^40"), (lambda: sample(edited(S=2 ** 38)), b"2^40"),
             (lambda: push(mute), b"speaks but dim_c = 0"), (lambda: sample(headless), b"no head"), (lambda: push(headless), b"no head"),
             (lambda: push(speaker, utter=None), b"utter is NULL but an agent speaks"),
             (lambda: sample(speaker, utter=None), b"utter is NULL"),
             (lambda: push(d, obs=None), b"obs_ptrs is NULL"), (lambda: push(d, moves=None), b"moves is NULL"),
             (lambda: sample(d, joint=None), b"joint and joint_next"), (lambda: sample(d, idx=None), b"idx is NULL")]
    for call, word in cases:
        rc = call()
        assert rc < 0 and word in L.mpe_last_error(), (rc, word, L.mpe_last_error())
    torch.cuda.synchronize()
    assert all(torch.equal(f[k][0], before[k]) for k in f) and all(torch.equal(out[k], outs[k]) for k in out)
