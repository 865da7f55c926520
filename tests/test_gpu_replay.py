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
    # back to back: four more pushes and a sample queued with nothing between them (every source is on the device beforehand), so
    # each launch reads the `head` the launch before it advanced
    steps = [R.coded_step(t % 8, B, buf.obs_widths, buf.dim_c) for t in range(7, 11)]
    on_dev = [([dev(o) for o in st[0]], (dev(st[1]), dev(st[2])) if buf.dim_c else dev(st[1]), [dev(o) for o in st[3]], dev(st[4]),
               dev(st[5])) for st in steps]
    torch.cuda.synchronize()
    for args in on_dev:
        buf.push(*args)
    b = buf.sample(130, draw=2, joint=True)
    torch.cuda.synchronize()
    for st in steps:
        ring.push(*st)
    assert buf.count == 11
    assert_ring_equal(buf, ring)
    idx = R.draw_indices(buf.seed, 2, 130, ring.n_valid())
    g = ring.gather(idx)
    assert b.idx.cpu().tolist() == idx
    assert all(np.array_equal(b.obs_n[i].cpu().numpy(), g["obs_n"][i]) and np.array_equal(b.next_obs_n[i].cpu().numpy(), g["next_obs_n"][i])
               for i in range(buf.A))
    assert all(np.array_equal(getattr(b, k).cpu().numpy(), g[k]) for k in ("act", "rew", "done") + (("utter",) if buf.dim_c else ()))


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


def test_gather_of_a_never_pushed_slot_reads_the_ring_one_step_and_transition_0_n_step():
    """The one place where the one-step and the n-step gather differ on purpose (include/mpe_hip.h): B = 7, S = 4, 3 pushes, so
    transitions [21, 28) are in the ring but were never pushed.  mpe_replay_gather returns what the ring holds there (a pattern
    written straight into slot 3) and transition 0 only outside [0, S * B); mpe_replay_gather_nstep returns transition 0 for both."""
    B, S = 7, 4
    env = mpe.make_env("simple_speaker_listener", batch_size=B, seed=1)
    buf = ReplayBuffer(env, steps=S, seed=5)
    ring = push_coded(buf, 3)
    assert len(buf) == ring.n_valid() == 21 and buf.dim_c == 3
    obs, moves, utter, nxt, rew, _ = R.coded_step(5, B, buf.obs_widths, buf.dim_c)      # step 5: in no pushed slot, nowhere zero
    done_u8 = (1 + np.arange(buf.A * B, dtype=np.uint8)).reshape(buf.A, B)              # a byte of its own per (agent, world)
    for i in range(buf.A):
        buf.obs_n[3][i].copy_(dev(obs[i]))
        buf.next_obs_n[3][i].copy_(dev(nxt[i]))
        ring.obs[3][i][...], ring.next_obs[3][i][...] = obs[i], nxt[i]
    buf.act[3].copy_(dev(moves)), buf.utter[3].copy_(dev(utter)), buf.rew[3].copy_(dev(rew)), buf._done_u8[3].copy_(dev(done_u8))
    ring.act[3], ring.utter[3], ring.rew[3] = moves, utter, rew
    ring_done = buf._done_u8.cpu().numpy()
    assert all((x != 0).all() for x in obs + nxt + [moves, utter, rew, done_u8])
    idx = torch.tensor([3, 21, 27, 28, -1, 2 ** 62, 0], dtype=torch.int64).cuda()

    def check(b, want):
        g = ring.gather(want)
        sl, wd = [j // B for j in want], [j % B for j in want]
        for i in range(buf.A):
            assert np.array_equal(b.obs_n[i].cpu().numpy(), g["obs_n"][i]), i
            assert np.array_equal(b.next_obs_n[i].cpu().numpy(), g["next_obs_n"][i]), i
            assert np.array_equal(b._done_u8[i].cpu().numpy(), ring_done[sl, i, wd]), i
        for f in ("act", "utter", "rew"):
            assert np.array_equal(getattr(b, f).cpu().numpy(), g[f]), f
        assert torch.equal(b.joint, torch.cat([b.obs_n[0], b.obs_n[1], b.utter[0], b.act[1]], dim=1))
        assert torch.equal(b.joint_next, torch.cat(b.next_obs_n, dim=1))

    b = buf.gather(idx, joint=True)
    torch.cuda.synchronize()
    check(b, [3, 21, 27, 0, 0, 0, 0])
    assert b.idx is idx
    assert np.array_equal(b.rew[:, 1:3].cpu().numpy(), rew[:, [0, 6]])      # 21 and 27: slot 3's pattern, worlds 0 and 6
    assert np.array_equal(b._done_u8[:, 1:3].cpu().numpy(), done_u8[:, [0, 6]])
    assert np.array_equal(b.joint[1:3, :buf.obs_widths[0]].cpu().numpy(), obs[0][[0, 6]])
    nb = buf.gather(idx, joint=True, n_step=1, gamma=0.5)
    torch.cuda.synchronize()
    check(nb, [3, 0, 0, 0, 0, 0, 0])
    assert nb.last.cpu().tolist() == [3, 0, 0, 0, 0, 0, 0] and nb.n_used.cpu().tolist() == [1] * 7
    assert torch.equal(nb.ret, nb.rew) and nb.discount.cpu().tolist() == [0.5] * 7
    assert torch.equal(idx.cpu(), torch.tensor([3, 21, 27, 28, -1, 2 ** 62, 0]))      # (read, never written)


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


def test_loop_pushes_utterances():
    """simple_reference at B = 6: both agents move and speak, so every step of the loop pushes (moves, utterances)."""
    B = 6
    env = mpe.make_env("simple_reference", batch_size=B, seed=11)
    torch.manual_seed(3)
    mods = [torch.nn.Sequential(torch.nn.Linear(d, 32), torch.nn.ReLU(), torch.nn.Linear(32, 5 + env.world.dim_c)).cuda() for d in
            [o.shape[1] for o in env.reset()]]
    loop = PolicyLoop(env, Actors(env, mods, mode="sample", seed=5), episode_len=4)
    buf = ReplayBuffer(env, steps=8)
    assert buf.dim_c == env.world.dim_c == 10 and buf.speaks == [True, True] and buf.movable == [True, True]
    traj = loop.run(6, replay=buf)
    torch.cuda.synchronize()
    assert buf.count == 6 and int(buf.head.item()) == 6 and int(buf._ticket.item()) == 0
    assert traj.utter.shape == (6, 2, B, 10) and torch.equal(buf.utter[:6], traj.utter) and torch.equal(buf.act[:6], traj.act)
    assert bool((traj.utter.sum(-1) == 1).all()) and bool((traj.act.sum(-1) == 1).all())      # one-hot heads: something was said
    assert len(set(traj.utter.argmax(-1).flatten().tolist())) > 1
    assert torch.equal(buf.rew[:6], traj.rew) and torch.equal(buf.done[:6], traj.done) and torch.equal(buf.next_obs[:6], traj.obs_flat)
    assert not buf.utter[6:].any() and not buf.act[6:].any()


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


GUARD, FILL = 16, 77      # guard elements on both sides of every raw tensor, and what they (and untouched outputs) hold


def guarded(shape, dtype, skew=0):
    """A `shape` view inside a FILL-filled allocation: GUARD elements, then `whole` = [skew elements | the view | GUARD - skew
    elements and GUARD more] -> (whole, view).  whole starts on a 16-byte boundary, so the view lies skew elements past one."""
    n = int(np.prod(shape))
    assert 0 <= skew <= GUARD
    base = torch.full((n + 3 * GUARD,), FILL, dtype=dtype, device="cuda")
    whole = base[GUARD:]
    assert whole.data_ptr() % 16 == 0 and whole._base is base
    return whole, whole[skew: skew + n].view(shape)


def guards_untouched(whole, view):
    """Everything of the allocation outside the view still holds FILL: at least GUARD elements on either side."""
    base = whole._base
    lo = (view.data_ptr() - base.data_ptr()) // base.element_size()
    assert lo >= GUARD and base.numel() - (lo + view.numel()) >= GUARD
    return bool((base[:lo] == FILL).all()) and bool((base[lo + view.numel():] == FILL).all())


def raw_ring(A, B, S, D, skew, dim_c=0, speaks=None, movable=None, skew_done=None, seed=0):
    """A ring in plain tensors, no env.  D: one observation width for every agent, or the A widths.  Every float field starts
    `skew` elements into its allocation (4 * skew bytes past a 16-byte boundary) and the done bytes `skew_done` (default: skew)
    bytes, with guard elements on both sides -> (descriptor, fields {name: (whole tensor, view)})."""
    widths = [D] * A if isinstance(D, int) else list(D)
    assert len(widths) == A
    skew_done = skew if skew_done is None else skew_done
    shapes = {"obs": (S, sum(widths) * B), "next_obs": (S, sum(widths) * B), "act": (S, A, B, 5), "rew": (S, A, B), "done": (S, A, B)}
    if dim_c:
        shapes["utter"] = (S, A, B, dim_c)
    f = {}
    for name, shape in shapes.items():
        f[name] = guarded(shape, torch.uint8, skew_done) if name == "done" else guarded(shape, torch.float32, skew)
    d = _abi.MpeReplay()
    d.n_agents, d.B, d.S, d.dim_c, d.seed = A, B, S, dim_c, seed
    for i in range(A):
        d.obs_width[i] = widths[i]
        d.movable[i] = 1 if movable is None else int(movable[i])
        d.speaks[i] = 0 if speaks is None else int(speaks[i])
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


# ---- the raw C entry points at the shapes where the kernels' index arithmetic matters; floats are distinct bit patterns (bits_step) ----
PER_BLOCK = 1024      # units a block of k_replay_push copies; output floats a pass of gather_rows covers
TILE = 64             # samples per block of k_replay_sample


def plan(src, dst, stride, nbytes):
    """What replay_push_plan decides for a segment, from its addresses: -> (unit, whole units, blocks)."""
    apart = ((src - dst) % 16) | (stride % 16)
    unit = 16 if apart % 16 == 0 else 4 if apart % 4 == 0 else 1
    units = nbytes // unit
    return unit, units, max(1, -(-units // PER_BLOCK))


def device_step(step, skew=0, skew_done=0):
    """A step of _replay_ref on the device, every tensor `skew` elements (done: skew_done bytes) past a 16-byte boundary, with
    guards -> (obs views, next views, moves, utter or None, rew, done uint8, the allocations to keep alive)."""
    obs, moves, utter, nxt, rew, done = step
    keep = []

    def put(x, dtype, k):
        x = np.ascontiguousarray(x)
        whole, view = guarded(x.shape, dtype, k)
        view.copy_(torch.as_tensor(x.view(np.int32) if dtype == torch.float32 else x).cuda().view(dtype))
        keep.append(whole)
        return view
    o, n = [put(x, torch.float32, skew) for x in obs], [put(x, torch.float32, skew) for x in nxt]
    ut = put(utter, torch.float32, skew) if utter is not None and utter.size else None
    mv, rw, dn = put(moves, torch.float32, skew), put(rew, torch.float32, skew), put(done.astype(np.uint8), torch.uint8, skew_done)
    return o, n, mv, ut, rw, dn, keep


def raw_push(d, o, n, mv, ut, rw, dn):
    A, L = d.n_agents, _abi.lib()
    rc = L.mpe_replay_push(C.byref(d), (C.c_void_p * A)(*[x.data_ptr() for x in o]), (C.c_void_p * A)(*[x.data_ptr() for x in n]),
                           mv.data_ptr(), ut.data_ptr() if ut is not None else None, rw.data_ptr(), dn.data_ptr(), None)
    assert rc == 0, L.mpe_last_error()


def dev_bits(t):
    """A float32 device tensor -> its bit patterns as a NumPy int32 array (no float compare: NaNs are data here)."""
    return t.contiguous().view(torch.int32).cpu().numpy()


def assert_raw_ring_equal(f, ring):
    """Every field of the raw ring against the NumPy ring, floats as bit patterns; guards around every field untouched."""
    B, off = ring.B, np.concatenate([[0], np.cumsum(ring.widths)])
    for s in range(ring.S):
        for i, w in enumerate(ring.widths):
            for name, want in (("obs", ring.obs), ("next_obs", ring.next_obs)):
                got = f[name][1][s, off[i] * B: off[i + 1] * B].view(B, w)
                assert np.array_equal(dev_bits(got), R.bits(want[s][i])), (name, s, i)
    assert np.array_equal(dev_bits(f["act"][1]), R.bits(ring.act)) and np.array_equal(dev_bits(f["rew"][1]), R.bits(ring.rew))
    if ring.dim_c:
        assert np.array_equal(dev_bits(f["utter"][1]), R.bits(ring.utter))
    assert np.array_equal(f["done"][1].cpu().numpy(), ring.done.astype(np.uint8))
    for name, (whole, view) in f.items():
        if name not in ("head", "ticket"):
            assert guards_untouched(whole, view), name


def assert_patterns_distinct(steps):
    """What the steps push tells agents, worlds, columns, fields and steps apart: every float field of T steps of n floats holds
    at least T * (n - 5) different bit patterns (all but each step's five SPECIALS), and rew, obs and next_obs share none but those."""
    T = len(steps)
    for k, name in ((0, "obs"), (3, "next_obs"), (1, "act"), (2, "utter"), (4, "rew")):
        arrays = [a for st in steps for a in (st[k] if isinstance(st[k], list) else [st[k]])]
        n = sum(a.size for a in arrays) // T
        assert R.distinct_patterns(arrays) >= T * (n - 5), name
    both = [a for st in steps for a in st[0] + st[3] + [st[4]]]
    assert R.distinct_patterns(both) >= sum(a.size for a in both) - 15 * T


# want: segment -> (unit, bytes, blocks), the figures of the shape; lead / tail: bytes peeled off obs segment 0
PUSH_CASES = {
    "vector": dict(A=2, widths=(33, 5), B=136, dim_c=25, skew=0, skew_done=0, lead=0, tail=0, blocks=11,
                   want={"obs0": (16, 17952, 2), "obs1": (16, 2720, 1), "act": (16, 5440, 1), "utter": (16, 27200, 2),
                         "done": (16, 272, 1)}),
    "vector-skewed": dict(A=2, widths=(33, 5), B=136, dim_c=25, skew=3, skew_done=3, lead=4, tail=12, blocks=11,
                          want={"obs0": (16, 17952, 2), "obs1": (16, 2720, 1), "act": (16, 5440, 1), "utter": (16, 27200, 2),
                                "done": (16, 272, 1)}),
    "dword": dict(A=2, widths=(33, 5), B=135, dim_c=25, skew=0, skew_done=0, lead=0, tail=0, blocks=23,
                  want={"obs0": (4, 17820, 5), "obs1": (4, 2700, 1), "act": (4, 5400, 2), "utter": (4, 27000, 7),
                        "done": (1, 270, 1)}),
    "byte": dict(A=15, widths=(3,) * 15, B=69, dim_c=0, skew=0, skew_done=0, lead=0, tail=0, blocks=40,
                 want={"obs0": (4, 828, 1), "act": (4, 20700, 6), "rew": (4, 4140, 2), "done": (1, 1035, 2)}),
    "byte-vector": dict(A=16, widths=(1,) * 16, B=272, dim_c=0, skew=0, skew_done=0, lead=0, tail=0, blocks=41,
                        want={"obs0": (16, 1088, 1), "act": (16, 87040, 6), "rew": (16, 17408, 2), "done": (16, 4352, 1)}),
}


@pytest.mark.parametrize("case", sorted(PUSH_CASES))
def test_push_segments_longer_than_one_block(case):
    """S = 2, three pushes (a wrap) of bit-pattern steps through the C entry point, at shapes where a segment needs more than one
    block of 1024 units on each unit size.  The unit, byte count and block count of the named segments follow from the addresses
    and are asserted here against the figures of PUSH_CASES:
      vector / vector-skewed  obs of agent 0: 17 952 B = 1122 sixteen-byte units, 2 blocks, the second partly full; utterances
                              27 200 B = 1700 units, 2 blocks; skewed: everything 12 bytes (done: 3) past a 16-byte boundary,
                              so 4 bytes are peeled in front of obs segment 0, 1121 whole units follow, 12 bytes behind
      dword                   slot stride 20 520 B = 8 mod 16: obs of agent 0 is 4455 dwords, 5 blocks; utterances 6750, 7 blocks
      byte                    1035 done bytes (odd: unit 1), 2 blocks
      byte-vector             4352 done bytes, 16-congruent: 272 sixteen-byte units
    The grids are 11, 11, 23, 40 and 41 blocks, each of which takes a ticket.  (A 27 200-byte segment at A = 2, B = 136 cannot be
    `act`, which is 2 * 136 * 5 * 4 = 5440 bytes there: dim_c = 25 utterances supply a whole-field segment of that size, in the
    dword case too.)"""
    c = PUSH_CASES[case]
    A, B, widths, dim_c, S = c["A"], c["B"], list(c["widths"]), c["dim_c"], 2
    d, f = raw_ring(A, B, S, widths, c["skew"], dim_c=dim_c, speaks=[1] * A if dim_c else None, skew_done=c["skew_done"])
    ring = R.NumpyRing(S, B, widths, dim_c)
    keep, steps = [], []
    for t in range(3):
        step = R.bits_step(t, A, B, widths, dim_c)
        o, n, mv, ut, rw, dn, k = device_step(step, c["skew"], c["skew_done"])
        keep.append(k)
        # the segments as mpe_replay_push lays them out: (source, slot 0 of the ring's field, slot stride, bytes)
        dsum, off = sum(widths), np.concatenate([[0], np.cumsum(widths)])
        segs = {}
        for i in range(A):
            segs["obs%d" % i] = (o[i].data_ptr(), f["obs"][1].data_ptr() + int(off[i]) * B * 4, dsum * B * 4, widths[i] * B * 4)
            segs["next%d" % i] = (n[i].data_ptr(), f["next_obs"][1].data_ptr() + int(off[i]) * B * 4, dsum * B * 4, widths[i] * B * 4)
        segs["act"] = (mv.data_ptr(), f["act"][1].data_ptr(), A * B * 20, A * B * 20)
        if dim_c:
            segs["utter"] = (ut.data_ptr(), f["utter"][1].data_ptr(), A * B * dim_c * 4, A * B * dim_c * 4)
        segs["rew"] = (rw.data_ptr(), f["rew"][1].data_ptr(), A * B * 4, A * B * 4)
        segs["done"] = (dn.data_ptr(), f["done"][1].data_ptr(), A * B, A * B)
        plans = {k_: plan(*v) for k_, v in segs.items()}
        for name, (unit, nbytes, blocks) in c["want"].items():
            assert (plans[name][0], segs[name][3], plans[name][2]) == (unit, nbytes, blocks), (name, plans[name], segs[name])
        assert sum(p[2] for p in plans.values()) == c["blocks"] > 10
        assert all(v.data_ptr() % 16 == 4 * c["skew"] for v in o + n + [mv, rw]) and dn.data_ptr() % 16 == c["skew_done"]
        assert f["obs"][1].data_ptr() % 16 == 4 * c["skew"] and f["done"][1].data_ptr() % 16 == c["skew_done"]
        lead = -segs["obs0"][1] % 16 if plans["obs0"][0] == 16 else 0
        assert lead == c["lead"] and ((segs["obs0"][3] - lead) % 16 if plans["obs0"][0] == 16 else 0) == c["tail"]
        raw_push(d, o, n, mv, ut, rw, dn)
        ring.push(*step)
        # the path the case names, from this push's own addresses: more than one block of that unit size, the last partly full
        name, unit = {"vector": ("obs0", 16), "vector-skewed": ("obs0", 16), "dword": ("obs0", 4), "byte": ("done", 1),
                      "byte-vector": ("done", 16)}[case]
        whole = (segs[name][3] - (lead if name == "obs0" else 0)) // unit
        assert plans[name][0] == unit and (case == "byte-vector" or (whole > PER_BLOCK and whole % PER_BLOCK))
        if case == "dword":
            assert segs["obs0"][2] % 16 == 8
        if case == "byte":
            assert segs["done"][3] % 2 == 1
        steps.append(step)
    assert_patterns_distinct(steps)
    torch.cuda.synchronize()
    assert int(f["head"][0].item()) == 3 and int(f["ticket"][0].item()) == 0
    assert_raw_ring_equal(f, ring)


def raw_sample(d, widths, M, draw, joint_width):
    """mpe_replay_sample into FILL-filled, guarded outputs -> (return code, {name: (whole, view)})."""
    A, dsum, dim_c, f32 = d.n_agents, sum(widths), d.dim_c, torch.float32
    out = {"idx": guarded((M,), torch.int64), "obs": guarded((dsum * M,), f32), "next_obs": guarded((dsum * M,), f32),
           "act": guarded((A, M, 5), f32), "rew": guarded((A, M), f32), "done": guarded((A, M), torch.uint8),
           "joint": guarded((M, joint_width), f32), "joint_next": guarded((M, dsum), f32)}
    if dim_c:
        out["utter"] = guarded((A, M, dim_c), f32)
    p = {k: v[1].data_ptr() for k, v in out.items()}
    rc = _abi.lib().mpe_replay_sample(C.byref(d), M, draw, p["idx"], p["obs"], p["next_obs"], p["act"], p.get("utter"), p["rew"], p["done"],
                                      p["joint"], p["joint_next"], None)
    return rc, out


def assert_sample_equal(out, ring, idx, M, joint_cols):
    """Every output of a raw sample against the NumPy gather at idx, floats as bit patterns; joint_cols: the joint row as a list
    of ("obs" | "act" | "utter", agent) in column order; guards behind (and in front of) every output untouched."""
    g = ring.gather(idx)
    off = np.concatenate([[0], np.cumsum(ring.widths)])
    for i, w in enumerate(ring.widths):
        for name, key in (("obs", "obs_n"), ("next_obs", "next_obs_n")):
            got = out[name][1][off[i] * M: off[i + 1] * M].view(M, w)
            assert np.array_equal(dev_bits(got), R.bits(g[key][i])), (name, i)
    for name in ("act", "rew") + (("utter",) if ring.dim_c else ()):
        assert np.array_equal(dev_bits(out[name][1]), R.bits(g[name])), name
    assert np.array_equal(out["done"][1].cpu().numpy(), g["done"].astype(np.uint8))
    part = {"obs": lambda i: g["obs_n"][i], "act": lambda i: g["act"][i], "utter": lambda i: g["utter"][i]}
    want = np.concatenate([R.bits(part[kind](i)) for kind, i in joint_cols], axis=1)
    assert np.array_equal(dev_bits(out["joint"][1]), want)
    assert np.array_equal(dev_bits(out["joint_next"][1]), np.concatenate([R.bits(x) for x in g["next_obs_n"]], axis=1))
    for name, (whole, view) in out.items():
        assert guards_untouched(whole, view), name


def filled_raw_ring(A, B, S, widths, T, dim_c=0, speaks=None, movable=None, seed=0):
    """T bit-pattern steps pushed into a raw ring and into a NumPy ring of the same shape -> (descriptor, fields, NumPy ring)."""
    d, f = raw_ring(A, B, S, widths, 0, dim_c=dim_c, speaks=speaks, movable=movable, seed=seed)
    ring = R.NumpyRing(S, B, widths, dim_c)
    keep, steps = [], []
    for t in range(T):
        step = R.bits_step(t, A, B, widths, dim_c)
        o, n, mv, ut, rw, dn, k = device_step(step)
        keep.append(k)
        steps.append(step)
        raw_push(d, o, n, mv, ut, rw, dn)
        ring.push(*step)
    assert_patterns_distinct(steps)
    torch.cuda.synchronize()
    assert int(f["head"][0].item()) == T and int(f["ticket"][0].item()) == 0
    return d, f, ring


WIDE = (1, 2, 3, 17, 33, _abi.MPE_REPLAY_MAX_WIDTH)


@pytest.fixture(scope="module")
def wide_ring():
    """Six agents of widths 1 (no reciprocal: row = element), 2, 3, 17, 33 and MPE_REPLAY_MAX_WIDTH; B = 3, S = 2, two pushes."""
    return filled_raw_ring(len(WIDE), 3, 2, list(WIDE), 2, seed=0x1234567890ABCDEF)


@pytest.mark.parametrize("M", [64, 65, 130])
def test_sample_gathers_wide_and_narrow_rows(wide_ring, M):
    """M = 64: one full tile; 65: a tile of one sample behind it; 130: three tiles.  A full tile of the widest agent is
    64 * 4096 = 262 144 output floats = 256 passes of gather_rows' 1024-float loop (e up to 2^18 - 1 through umulhi), of width 33
    2112 floats = 3 passes, of width 17 1088 floats = 2 passes; width 1 takes the magic == 0 branch, width 2 magic 2^31."""
    d, f, ring = wide_ring
    A, W = len(WIDE), _abi.MPE_REPLAY_MAX_WIDTH
    assert W == 4096 and TILE * W == 262144 and -(-TILE * W // PER_BLOCK) == 256      # passes of a full tile at the widest row
    assert TILE * 33 > PER_BLOCK and -(-TILE * 33 // PER_BLOCK) == 3 and -(-TILE * 17 // PER_BLOCK) == 2
    assert TILE * 1 <= PER_BLOCK and TILE * 3 <= PER_BLOCK      # the narrow rows: one pass
    # tiles, and the samples of the last one
    assert -(-M // TILE) == {64: 1, 65: 2, 130: 3}[M] and (M - 1) % TILE + 1 == {64: 64, 65: 1, 130: 2}[M]
    draw = 5 + M
    rc, out = raw_sample(d, WIDE, M, draw, sum(WIDE) + 5 * A)
    assert rc == 0, _abi.lib().mpe_last_error()
    torch.cuda.synchronize()
    want = R.draw_indices(d.seed, draw, M, ring.n_valid())
    assert ring.n_valid() == 6 and out["idx"][1].cpu().tolist() == want and set(want) == set(range(6))
    assert_sample_equal(out, ring, want, M, [("obs", i) for i in range(A)] + [("act", i) for i in range(A)])


def test_sample_rewards_and_dones_of_sixteen_agents():
    """A = MPE_REPLAY_MAX_AGENTS = 16: the last job's loop over A * 64 = 1024 (agent, sample) pairs takes four passes of 256 lanes;
    M = 70: a full tile and one of 6 samples.  S = 3 after 4 pushes: a wrapped ring."""
    A, B, S, M = _abi.MPE_REPLAY_MAX_AGENTS, 5, 3, 70
    assert A == 16 and A * TILE > 256 and -(-A * TILE // 256) == 4
    d, f, ring = filled_raw_ring(A, B, S, [2] * A, 4, seed=9)
    rc, out = raw_sample(d, [2] * A, M, 1, 2 * A + 5 * A)
    assert rc == 0, _abi.lib().mpe_last_error()
    torch.cuda.synchronize()
    want = R.draw_indices(9, 1, M, ring.n_valid())
    assert ring.n_valid() == 15 and out["idx"][1].cpu().tolist() == want
    assert ring.done.any() and not ring.done.all()
    assert_sample_equal(out, ring, want, M, [("obs", i) for i in range(A)] + [("act", i) for i in range(A)])


def test_joint_row_of_agents_with_both_heads():
    """Agent 0 moves and speaks, agent 1 only speaks, agent 2 only moves: the joint row is
    [obs0 obs1 obs2 | move0 utter0 | utter1 | move2] -- agent by agent, an agent's move row in front of its utterance row.  Then
    the same through ReplayBuffer on simple_reference, where both agents have both heads."""
    widths, dim_c, M = [3, 2, 4], 4, 70
    d, f, ring = filled_raw_ring(3, 5, 2, widths, 3, dim_c=dim_c, speaks=(1, 1, 0), movable=(1, 0, 1), seed=77)
    jw = sum(widths) + (5 + 4) + 4 + 5
    rc, out = raw_sample(d, widths, M, 2, jw)
    assert rc == 0, _abi.lib().mpe_last_error()
    torch.cuda.synchronize()
    want = R.draw_indices(77, 2, M, ring.n_valid())
    assert out["idx"][1].cpu().tolist() == want
    assert_sample_equal(out, ring, want, M, [("obs", 0), ("obs", 1), ("obs", 2), ("act", 0), ("utter", 0), ("utter", 1), ("act", 2)])
    # simple_reference: two agents, each movable and speaking with dim_c = 10
    env = mpe.make_env("simple_reference", batch_size=7, seed=1)
    buf = ReplayBuffer(env, steps=3, seed=21)
    ring2 = push_coded(buf, 4)
    assert buf.movable == [True, True] and buf.speaks == [True, True] and buf.n_act == [5 + buf.dim_c] * 2
    assert buf.joint_width == sum(buf.obs_widths) + 2 * (5 + buf.dim_c)
    b = buf.sample(100, draw=6, joint=True)
    torch.cuda.synchronize()
    idx = R.draw_indices(21, 6, 100, ring2.n_valid())
    g = ring2.gather(idx)
    assert b.idx.cpu().tolist() == idx
    assert np.array_equal(b.act.cpu().numpy(), g["act"]) and np.array_equal(b.utter.cpu().numpy(), g["utter"])
    assert b.joint.shape == (100, buf.joint_width)
    assert torch.equal(b.joint, torch.cat([b.obs_n[0], b.obs_n[1], b.act[0], b.utter[0], b.act[1], b.utter[1]], dim=1))
    assert np.array_equal(b.joint.cpu().numpy(), np.concatenate([g["obs_n"][0], g["obs_n"][1], g["act"][0], g["utter"][0], g["act"][1],
                                                                 g["utter"][1]], axis=1))
    assert torch.equal(b.joint_next, torch.cat(b.next_obs_n, dim=1))


def test_sample_of_an_empty_ring_writes_nothing():
    """head == 0 at the C entry point: the launch is made, returns 0, and every block leaves before it writes -- idx included."""
    A, widths, dim_c, M = 3, [3, 2, 4], 4, 70
    d, f = raw_ring(A, 5, 2, widths, 0, dim_c=dim_c, speaks=(1, 1, 0), movable=(1, 0, 1), seed=3)
    rc, out = raw_sample(d, widths, M, 0, sum(widths) + 9 + 4 + 5)
    assert rc == 0, _abi.lib().mpe_last_error()
    torch.cuda.synchronize()
    assert int(f["head"][0].item()) == 0 and int(f["ticket"][0].item()) == 0
    for name, (whole, view) in out.items():
        assert bool((whole._base == FILL).all()), name
    for name, (whole, view) in f.items():
        if name not in ("head", "ticket"):
            assert bool((whole._base == FILL).all()), name
