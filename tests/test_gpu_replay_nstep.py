"""n-step returns on the GPU (the NSTEP instantiations of k_replay_sample in csrc/mpe_replay.hip): one launch that draws or reads, walks,
sums and gathers.  The rule fixes the order of every float32 operation, so every comparison is equality -- bit-equal floats, equal
integers -- against the restatement in tests/_replay_nstep_ref.py."""
import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop
from multiagent_particle_envs_amd.replay import (NStepReplayBatch, PrioritizedNStepReplayBatch, PrioritizedReplayBuffer, ReplayBatch,
                                                 ReplayBuffer)

import _replay_ref as R
import _replay_nstep_ref as N

pytestmark = pytest.mark.gpu

GAMMA = 0.95


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def dev_bits(t):
    """A float32 device tensor -> its bit patterns as a NumPy int32 array (no float compare: NaNs may be data)."""
    return t.contiguous().view(torch.int32).cpu().numpy()


def push_steps(buf, T, step=N.sparse_step):
    """T synthetic steps into buf and into a NumPy ring of the same shape -> the NumPy ring."""
    ring = R.NumpyRing(buf.S, buf.B, buf.obs_widths, buf.dim_c)
    for t in range(T):
        obs, moves, utter, nxt, rew, done = step(t, buf.B, buf.obs_widths, buf.dim_c)
        action = (dev(moves), dev(utter)) if buf.dim_c else dev(moves)
        buf.push([dev(o) for o in obs], action, [dev(o) for o in nxt], dev(rew), dev(done))
        ring.push(obs, moves, utter, nxt, rew, done)
    torch.cuda.synchronize()
    return ring


RINGS = {"partial": ("simple_speaker_listener", 7, 4, 3), "wrapped": ("simple_speaker_listener", 7, 4, 9),
         "spread": ("simple_spread", 64, 8, 19), "adversary": ("simple_adversary", 5, 6, 15)}


@pytest.fixture(scope="module")
def rings():
    """name -> (buffer, NumPy ring), filled once with the sparse steps of _replay_nstep_ref and left unchanged by every test."""
    out = {}
    for tag, (name, B, S, T) in RINGS.items():
        env = mpe.make_env(name, batch_size=B, seed=1)
        buf = ReplayBuffer(env, steps=S, seed=0xC0FFEE12345)
        out[tag] = (buf, push_steps(buf, T))
    return out


def joint_of(buf, b):
    """The joint row from the batch's own per-agent tensors: every observation, then per agent its move and utterance rows."""
    cols = list(b.obs_n)
    for i in range(buf.A):
        cols += ([b.act[i]] if buf.movable[i] else []) + ([b.utter[i]] if buf.speaks[i] else [])
    return torch.cat(cols, dim=1)


def assert_batch_is(buf, b, want, joint=True, ret=True):
    """Every output of an n-step batch against the restatement's dict; ret=False: the float arithmetic is left out."""
    torch.cuda.synchronize()
    assert b.last.cpu().tolist() == want["last"].tolist()
    assert b.n_used.dtype == torch.int32 and b.n_used.cpu().tolist() == want["n_used"].tolist()
    assert b.last.dtype == torch.int64 and b.done.dtype == torch.bool
    if ret:
        assert np.array_equal(dev_bits(b.discount), R.bits(want["discount"]))
        assert np.array_equal(dev_bits(b.ret), R.bits(want["ret"]))
    assert np.array_equal(b.done.cpu().numpy(), want["done"])
    for i in range(buf.A):
        assert np.array_equal(dev_bits(b.next_obs_n[i]), R.bits(want["next_obs_n"][i])), i
        assert np.array_equal(dev_bits(b.obs_n[i]), R.bits(want["obs_n"][i])), i
    for f in ("act", "rew") + (("utter",) if buf.dim_c else ()):
        assert np.array_equal(dev_bits(getattr(b, f)), R.bits(want[f])), f
    if joint:
        assert torch.equal(b.joint_next.view(torch.int32), torch.cat(b.next_obs_n, dim=1).view(torch.int32))
        assert torch.equal(b.joint.view(torch.int32), joint_of(buf, b).view(torch.int32))
        assert b.joint.shape == (b.last.numel(), buf.joint_width)
    else:
        assert b.joint is None and b.joint_next is None


EVERY = [("partial", 3, 0, 0), ("wrapped", 1, 0, 0), ("wrapped", 3, 0, 0), ("wrapped", 4, 0, 0), ("spread", 5, 7, 0), ("spread", 5, 7, 3),
         ("adversary", 4, 5, 0)]


def test_every_transition_and_every_stop_cause(rings):
    """gather(arange(n_valid), n_step=n) of a partial ring, a ring wrapped twice, a full 64-sample tile on the 16-byte path with
    episode cuts at two phases, and an odd B with cuts: every valid transition's chain against the restatement.  Every stop cause
    -- done, cut, n, head -- occurs in the spread case and at least once over the cases, so no branch of the walk goes untested."""
    seen = {c: 0 for c in N.CAUSES}
    for tag, n, L, p in EVERY:
        buf, ring = rings[tag]
        nv = ring.n_valid()
        assert nv == len(buf) == min(RINGS[tag][3], buf.S) * buf.B
        idx = torch.arange(nv, dtype=torch.int64, device="cuda")
        b = buf.gather(idx, joint=True, n_step=n, gamma=GAMMA, episode_len=L, episode_phase=p)
        want = N.nstep(ring, list(range(nv)), n, GAMMA, L, p)
        assert type(b) is NStepReplayBatch and b.idx is idx
        assert_batch_is(buf, b, want)
        here = {c: want["cause"].count(c) for c in N.CAUSES}
        print(tag, n, L, p, here)
        assert sum(v > 0 for v in here.values()) >= (4 if tag == "spread" else 1 if n == 1 else 3), here
        assert int(b.n_used.max()) == min(n, buf.S, RINGS[tag][3]) and int(b.n_used.min()) == 1
        for c in N.CAUSES:
            seen[c] += here[c]
    assert all(v > 0 for v in seen.values()), seen


def test_n_step_1_is_todays_sample(rings):
    buf, ring = rings["wrapped"]
    M, draw = 257, 11
    a = buf.sample(M, draw=draw, joint=True)
    torch.cuda.synchronize()
    assert type(a) is ReplayBatch
    keep = {f: getattr(a, f).clone() for f in ("idx", "act", "utter", "rew", "done", "joint", "joint_next")}
    keep_obs, keep_next = [o.clone() for o in a.obs_n], [o.clone() for o in a.next_obs_n]
    b = buf.sample(M, draw=draw, joint=True, n_step=1, gamma=GAMMA)
    torch.cuda.synchronize()
    assert b is not a and type(b) is NStepReplayBatch
    for f, v in keep.items():
        got = getattr(b, f)
        assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got, v.view(torch.int32) if v.dtype == torch.float32 else v), f
    assert all(torch.equal(x, y) for x, y in zip(b.obs_n, keep_obs)) and all(torch.equal(x, y) for x, y in zip(b.next_obs_n, keep_next))
    assert torch.equal(b.ret.view(torch.int32), b.rew.view(torch.int32))
    assert np.array_equal(dev_bits(b.discount), R.bits(np.full(M, GAMMA, np.float32)))
    assert bool((b.n_used == 1).all()) and torch.equal(b.last, b.idx)
    assert b.idx.cpu().tolist() == R.draw_indices(buf.seed, draw, M, ring.n_valid())


@pytest.mark.parametrize("M", [1, 64, 65, 1000])
def test_uniform_draw_is_the_one_step_draw(rings, M):
    """M = 1, one full tile, a tile of one sample behind it, sixteen tiles: idx is mpe_replay_sample's for the same (seed, draw)."""
    buf, ring = rings["spread"]
    draw = 3 + M
    b = buf.sample(M, draw=draw, joint=(M != 65), n_step=3, gamma=GAMMA, episode_len=7, episode_phase=2)
    torch.cuda.synchronize()
    want_idx = R.draw_indices(buf.seed, draw, M, ring.n_valid())
    assert b.idx.cpu().tolist() == want_idx
    assert_batch_is(buf, b, N.nstep(ring, want_idx, 3, GAMMA, 7, 2), joint=(M != 65))
    assert buf.sample(M, draw=draw, joint=(M != 65), n_step=3, gamma=GAMMA, episode_len=7, episode_phase=2) is b      # cached per shape


def test_bad_indices_behave_as_transition_0(rings):
    """The partial ring: 21 valid transitions of S * B = 28.  -1, n_valid, a never-pushed slot, S * B and 2^62 read transition 0."""
    buf, ring = rings["partial"]
    nv, cap = ring.n_valid(), buf.S * buf.B
    assert (nv, cap) == (21, 28)
    idx = [3, -1, nv, 20, cap - 1, cap, 2 ** 62, 0, -2 ** 63, 14]
    t = dev(np.array(idx, np.int64))
    b = buf.gather(t, joint=True, n_step=3, gamma=GAMMA)
    want = N.nstep(ring, idx, 3, GAMMA)
    assert want["idx"] == [3, 0, 0, 20, 0, 0, 0, 0, 0, 14]
    assert_batch_is(buf, b, want)
    assert b.idx is t and t.cpu().tolist() == idx      # the caller's tensor, left alone
    zero = [k for k, j in enumerate(want["idx"]) if j == 0]
    assert len(set(b.last[zero].cpu().tolist())) == 1 and len(set(dev_bits(b.ret[0, zero]).tolist())) == 1


def test_moved_fields_keep_their_bits():
    """Steps of distinct bit patterns (NaNs with payloads, denormals, -0.0, inf): everything the launch only moves comes back bit
    for bit, from the transition the walk names.  ret and discount are arithmetic on those patterns and are not compared."""
    env = mpe.make_env("simple_speaker_listener", batch_size=7, seed=1)
    buf = ReplayBuffer(env, steps=4)
    ring = push_steps(buf, 6, step=lambda t, B, widths, dim_c: R.bits_step(t, len(widths), B, widths, dim_c))
    nv = ring.n_valid()
    walks = [N.walk(ring, j, 3, 5, 1) for j in range(nv)]
    want = ring.gather(list(range(nv)))
    at_last = ring.gather([w[2] for w in walks])
    want["next_obs_n"], want["done"] = at_last["next_obs_n"], at_last["done"]
    want["last"], want["n_used"] = np.array([w[2] for w in walks], np.int64), np.array([w[1] for w in walks], np.int32)
    assert len(set(w[1] for w in walks)) >= 2 and ring.done.any() and not ring.done.all()
    b = buf.gather(torch.arange(nv, dtype=torch.int64, device="cuda"), joint=True, n_step=3, gamma=GAMMA, episode_len=5, episode_phase=1)
    assert_batch_is(buf, b, want, ret=False)


def test_prioritized_sample_with_n_step():
    B, S, M = 7, 4, 130
    env = mpe.make_env("simple_speaker_listener", batch_size=B, seed=1)
    buf = PrioritizedReplayBuffer(env, steps=S, seed=5)
    ring = push_steps(buf, 6)
    nv = ring.n_valid()
    buf.update_priorities(torch.arange(nv, dtype=torch.int64, device="cuda"), dev((1.0 + np.arange(nv) % 5).astype(np.float32)))
    u24 = dev(((np.arange(M, dtype=np.int64) * 2654435761) % (1 << 24)).astype(np.int32))
    a = buf.sample(M, draw=4, joint=True, u24=u24)
    torch.cuda.synchronize()
    keep = (a.idx.clone(), a.prio.clone(), a.total.clone(), a.n_valid.clone())
    b = buf.sample(M, draw=4, joint=True, u24=u24, n_step=3, gamma=GAMMA)
    torch.cuda.synchronize()
    assert type(b) is PrioritizedNStepReplayBatch and b is not a
    assert torch.equal(b.idx, keep[0]) and torch.equal(b.prio, keep[1]) and torch.equal(b.total, keep[2]) and torch.equal(b.n_valid, keep[3])
    assert len(set(b.idx.cpu().tolist())) > 10
    assert_batch_is(buf, b, N.nstep(ring, b.idx.cpu().tolist(), 3, GAMMA))
    w = b.weights(0.5)
    assert w.shape == (M,) and float(w.max()) == 1.0
    before = buf.priorities.clone()
    buf.update_td(b.idx, b.ret[1] - b.discount)
    torch.cuda.synchronize()
    assert not torch.equal(buf.priorities, before)


def test_graph_of_push_and_n_step_sample_follows_the_pushes():
    """{push, sample(64, draw=5, n_step=3, episode_len=4)} captured once and replayed 5 times with new step data copied into the
    captured source tensors: head is read on the device, so the last replay's batch is the restatement's at head = 5 + 1."""
    B, S, M = 6, 4, 64
    env = mpe.make_env("simple_spread", batch_size=B, seed=3)
    buf = ReplayBuffer(env, steps=S, seed=9)
    ring = R.NumpyRing(S, B, buf.obs_widths, 0)

    def host(t):
        st = N.sparse_step(t, B, buf.obs_widths, 0)
        return st, list(st[0]) + [st[1]] + list(st[3]) + [st[4], st[5]]
    st, flat = host(0)
    src = [dev(x) for x in flat]
    A = buf.A
    args = (src[:A], src[A], src[A + 1: 2 * A + 1], src[2 * A + 1], src[2 * A + 2])

    def iteration():
        buf.push(*args)
        return buf.sample(M, draw=5, joint=True, n_step=3, gamma=GAMMA, episode_len=4)
    iteration()      # the warm-up push: code objects and the batch's tensors outside the capture
    ring.push(*st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b = iteration()
    buf.count -= 1      # (the captured push has not run)
    for t in range(1, 6):
        st, flat = host(t)
        for d, x in zip(src, flat):
            d.copy_(dev(x))
        g.replay()
        buf.count += 1
        ring.push(*st)
    torch.cuda.synchronize()
    assert int(buf.head.item()) == buf.count == ring.count == 6 and int(buf._ticket.item()) == 0
    want_idx = R.draw_indices(9, 5, M, ring.n_valid())
    assert b.idx.cpu().tolist() == want_idx
    want = N.nstep(ring, want_idx, 3, GAMMA, 4, 0)
    assert_batch_is(buf, b, want)
    assert set(want["cause"]) >= {"cut", "head"}


def test_closed_loop_chains_stop_at_the_loops_restarts():
    """PolicyLoop(episode_len=5) restarts worlds on the device and reports no done: with episode_len=5 no chain crosses a restart."""
    B, S, T, L, n = 16, 16, 12, 5, 4
    env = mpe.make_env("simple_spread", batch_size=B, seed=11)
    torch.manual_seed(3)
    mods = [torch.nn.Sequential(torch.nn.Linear(d, 32), torch.nn.ReLU(), torch.nn.Linear(32, 5)).cuda() for d in
            [o.shape[1] for o in env.reset()]]
    env.reset()
    loop = PolicyLoop(env, Actors(env, mods, mode="sample", seed=5), episode_len=L)
    buf = ReplayBuffer(env, steps=S)
    loop.run(T, replay=buf)
    torch.cuda.synchronize()
    assert buf.count == T and not bool(buf.done.any())
    nv = len(buf)
    b = buf.gather(torch.arange(nv, dtype=torch.int64, device="cuda"), n_step=n, gamma=GAMMA, episode_len=L)
    torch.cuda.synchronize()
    m, idx = b.n_used.cpu().tolist(), list(range(nv))
    for j in idx:
        t0 = j // B      # (no wrap: slot = step)
        chain = list(range(t0, t0 + m[j]))
        assert all((t + 1) % L for t in chain[:-1]), (j, chain)
        assert m[j] == n or (chain[-1] + 1) % L == 0 or chain[-1] == T - 1, (j, chain)
    assert set(m) == {1, 2, 3, 4}
    ring = R.NumpyRing(S, B, buf.obs_widths, 0)      # the restatement applied to what the loop pushed
    ring.count = T
    ring.rew, ring.done, ring.act = buf.rew.cpu().numpy(), buf.done.cpu().numpy(), buf.act.cpu().numpy()
    ring.obs = [[o.cpu().numpy() for o in row] for row in buf.obs_n]
    ring.next_obs = [[o.cpu().numpy() for o in row] for row in buf.next_obs_n]
    want = N.nstep(ring, idx, n, GAMMA, L, 0)
    assert "done" not in want["cause"] and {"cut", "n", "head"} <= set(want["cause"])
    assert_batch_is(buf, b, want, joint=False)
    assert len(set(dev_bits(b.ret).reshape(-1).tolist())) > nv // 2      # (the agents share one reward; the worlds differ)
