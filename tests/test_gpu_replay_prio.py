"""Prioritized replay on the GPU (csrc/mpe_replay_prio.hip, mpe_replay_gather): the kernels move floats and add non-negative
floats in one fixed order, so every comparison is equality -- the whole tree, pmax, idx, prio, total, n_valid and every gathered
field -- against the NumPy restatement of tests/_replay_prio_ref.py and the NumPy ring of tests/_replay_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.replay import PrioritizedReplayBuffer, ReplayBuffer

import _replay_prio_ref as P
import _replay_ref as R
from test_gpu_replay import (FILL, assert_sample_equal, dev, device_step, guarded, guards_untouched, push_coded, raw_push, raw_ring,
                             spread_loop)

pytestmark = pytest.mark.gpu

WIDTHS = [3, 2]      # two agents, both movable, nobody speaks


def raw_prio(S, B):
    """The priorities of an S x B ring in plain tensors: a zeroed tree with guards, pmax = 1, ticket = 0 -> (descriptor, fields)."""
    off, n = _abi.replay_prio_layout(S * B)
    whole, tree = guarded((n,), torch.float32)
    tree.zero_()
    pmax, ticket = torch.ones(1, dtype=torch.float32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    p = _abi.MpeReplayPrio()
    p.n_leaves, p.tree, p.pmax, p.ticket = S * B, tree.data_ptr(), pmax.data_ptr(), ticket.data_ptr()
    return p, {"tree": (whole, tree), "pmax": pmax, "ticket": ticket, "off": off}


class Rig(object):
    """A raw ring with priorities, the NumPy ring and the NumPy tree beside it."""

    def __init__(self, S, B, seed=0):
        self.S, self.B, self.A = S, B, len(WIDTHS)
        self.d, self.f = raw_ring(self.A, B, S, WIDTHS, 0, seed=seed)
        self.p, self.pf = raw_prio(S, B)
        self.ring, self.ref = R.NumpyRing(S, B, WIDTHS, 0), P.PrioTree(S, B)
        self.keep, self.L, self.seed = [], _abi.lib(), seed

    def push(self):
        t = self.ring.count
        step = R.bits_step(t % 32, self.A, self.B, WIDTHS, 0)
        o, n, mv, ut, rw, dn, k = device_step(step)
        self.keep.append(k)
        rc = self.L.mpe_replay_prio_push(C.byref(self.d), C.byref(self.p), None)
        assert rc == 0, self.L.mpe_last_error()
        raw_push(self.d, o, n, mv, ut, rw, dn)
        self.ring.push(*step)
        self.ref.push()

    def update(self, idx, prio):
        i, v = dev(np.asarray(idx, dtype=np.int64)), dev(np.asarray(prio, dtype=np.float32))
        rc = self.L.mpe_replay_prio_update(C.byref(self.d), C.byref(self.p), len(idx), i.data_ptr(), v.data_ptr(), None)
        assert rc == 0, self.L.mpe_last_error()
        torch.cuda.synchronize()
        self.ref.update(idx, prio)

    def check_tree(self, what=""):
        torch.cuda.synchronize()
        whole, tree = self.pf["tree"]
        assert np.array_equal(R.bits(tree.cpu().numpy()), R.bits(self.ref.tree())), what
        assert guards_untouched(whole, tree), what
        assert float(self.pf["pmax"].item()) == float(self.ref.pmax), what
        assert int(self.pf["ticket"].item()) == 0 and int(self.f["head"][0].item()) == self.ref.head == self.ring.count, what

    def draw(self, M, draw_no, u24=None):
        """mpe_replay_prio_draw into guarded, FILL-filled outputs -> {name: (whole, view)}"""
        out = {"idx": guarded((M,), torch.int64), "prio": guarded((M,), torch.float32), "total": guarded((1,), torch.float32),
               "n_valid": guarded((1,), torch.int64)}
        u = dev(np.asarray(u24, dtype=np.int64).astype(np.uint32).view(np.int32)) if u24 is not None else None
        rc = self.L.mpe_replay_prio_draw(C.byref(self.d), C.byref(self.p), M, draw_no, u.data_ptr() if u is not None else None,
                                         out["idx"][1].data_ptr(), out["prio"][1].data_ptr(), out["total"][1].data_ptr(),
                                         out["n_valid"][1].data_ptr(), None)
        assert rc == 0, self.L.mpe_last_error()
        torch.cuda.synchronize()
        return out

    def check_draw(self, M, draw_no, u24=None, gather=True):
        out = self.draw(M, draw_no, u24)
        idx, prio, total, fired = self.ref.draw(M, self.seed, draw_no, u24)
        assert out["idx"][1].cpu().tolist() == idx.tolist(), (M, draw_no)
        assert np.array_equal(R.bits(out["prio"][1].cpu().numpy()), R.bits(prio))
        assert R.bits(out["total"][1].cpu().numpy())[0] == R.bits(total) and int(out["n_valid"][1].item()) == self.ref.n_valid()
        assert all(guards_untouched(*v) for v in out.values())
        assert (prio > 0).all() and idx.max() < self.ref.n_valid()
        if gather:
            self.check_gather(out["idx"][1], idx.tolist(), M)
        return idx, fired

    def check_gather(self, idx_dev, idx, M):
        """mpe_replay_gather at idx_dev into guarded outputs against the NumPy ring's gather."""
        A, dsum, f32 = self.A, sum(WIDTHS), torch.float32
        jw = dsum + 5 * A
        out = {"obs": guarded((dsum * M,), f32), "next_obs": guarded((dsum * M,), f32), "act": guarded((A, M, 5), f32),
               "rew": guarded((A, M), f32), "done": guarded((A, M), torch.uint8), "joint": guarded((M, jw), f32),
               "joint_next": guarded((M, dsum), f32)}
        q = {k: v[1].data_ptr() for k, v in out.items()}
        before = idx_dev.clone()
        rc = self.L.mpe_replay_gather(C.byref(self.d), M, idx_dev.data_ptr(), q["obs"], q["next_obs"], q["act"], None, q["rew"], q["done"],
                                      q["joint"], q["joint_next"], None)
        assert rc == 0, self.L.mpe_last_error()
        torch.cuda.synchronize()
        assert torch.equal(idx_dev, before)
        assert_sample_equal(out, self.ring, idx, M, [("obs", i) for i in range(A)] + [("act", i) for i in range(A)])


def nasty_update(rs, n, M):
    """M (idx, priority) pairs: duplicates, indices outside [0, n), and priorities of every kind the clamp has a rule for."""
    idx = rs.randint(0, n, size=M).astype(np.int64)
    prio = (2.0 ** rs.randint(-3, 4, size=M) * (1.0 + rs.rand(M))).astype(np.float32)
    with np.errstate(over="ignore"):
        specials = np.array([np.nan, np.inf, -np.inf, 0.0, -2.0, 1e-30, 1e30, 2.0 ** -40, 2.0 ** 40, 1e-45], np.float32)
    k = min(M, len(specials))
    prio[:k] = specials[:k]
    if M >= 16:
        idx[10:14] = [-1, n, n + 5, 2 ** 40]
        idx[14] = idx[15]                      # a duplicate for certain
        idx[:3] = idx[3]                       # NaN, inf and -inf on one leaf with a plain value: the leaf takes MAX
    return idx, prio


SHAPES = [(S, B) for B in (1, 5, 16, 17, 257) for S in (1, 3, 7)] + [(4, 4097)]


@pytest.mark.parametrize("S,B", SHAPES)
def test_push_update_draw_gather_equal_the_restatement(S, B):
    """Pushes through two wraps of the ring with updates between them, the whole tree compared after every step; draws (and the
    gather at the drawn indices) on the partly filled and on the full ring.  B = 1 with S = 1: level 0 only; B = 5, 17, 257: level-1
    nodes that straddle slots; 16, 17, 257 and 4097: level boundaries; 4 x 4097: five levels."""
    rig = Rig(S, B, seed=0xABCDEF0123 + S * B)
    rs = np.random.RandomState(S * 10007 + B)
    n = S * B
    assert len(rig.pf["off"]) - 1 == len(P.level_sizes(n)) and (n != 16388 or len(P.level_sizes(n)) == 5)
    pushes = 2 * S + 1
    for t in range(pushes):
        rig.push()
        rig.check_tree(("push", t))
        if t == 0:
            # the partly filled ring (S > 1): still-zero leaves are named too and must stay zero
            idx, prio = nasty_update(rs, n, 1000)
            rig.update(idx, prio)
            rig.check_tree("update on the first slot")
            assert S == 1 or not rig.ref.leaves[B:].any()
            rig.check_draw(65, 1)
        if t == S:
            rig.update(*nasty_update(rs, n, 1))      # M = 1: a NaN
            rig.check_tree("update of one")
            rig.update(*nasty_update(rs, n, 257))
            rig.check_tree("update after the first wrap")      # the next push writes the raised pmax
    assert float(rig.ref.pmax) == 2.0 ** 40
    idx, prio = rs.randint(0, n, size=4 * n), (2.0 ** rs.randint(-3, 4, size=4 * n) * (1.0 + rs.rand(4 * n))).astype(np.float32)
    rig.update(idx, prio)      # (priorities of one scale again, as a learner leaves them)
    rig.check_tree("last update")
    for M in (1, 63, 64, 65, 1000):
        rig.check_draw(M, 100 + M)


def test_u24_override_and_the_searched_last_child_case():
    rig = Rig(1, 16)
    rig.push()
    p = P.find_last_child_case(seed=0)
    rig.update(np.arange(16), p)
    rig.check_tree()
    idx, fired = rig.check_draw(1, 0, u24=[0xFFFFFF])
    assert fired == 1 and idx.tolist() == [15]
    # the bits above the low 24 are not looked at; M = 1000 caller-chosen values
    rs = np.random.RandomState(5)
    u = rs.randint(0, 2 ** 32, size=1000, dtype=np.int64)
    a, _ = rig.check_draw(1000, 3, u24=u)
    b, _ = rig.check_draw(1000, 9, u24=u & 0xFFFFFF, gather=False)
    assert a.tolist() == b.tolist()      # (the draw number plays no part either)
    rig2 = Rig(3, 257, seed=77)
    for _ in range(2):
        rig2.push()
    rig2.update(*nasty_update(rs, 3 * 257, 500))
    rig2.check_draw(1000, 0, u24=u)
    rig2.check_draw(64, 0, u24=np.full(64, 0xFFFFFF))
    rig2.check_draw(64, 0, u24=np.zeros(64, np.int64))


@pytest.mark.parametrize("S,B", [(1, 1), (3, 5), (7, 257), (4, 4097)])
def test_update_in_one_launch_gives_the_same_tree(S, B, monkeypatch):
    """MPE_REPLAY_PRIO_UPDATE=ticket: the repair form kept for measurement (the last-ticket block climbs alone), same rule."""
    rig = Rig(S, B)
    rs = np.random.RandomState(S + B)
    for _ in range(S):
        rig.push()
    monkeypatch.setenv("MPE_REPLAY_PRIO_UPDATE", "ticket")
    for M in (1, 257, 1000):
        rig.update(*nasty_update(rs, S * B, M))
        rig.check_tree(M)
    monkeypatch.delenv("MPE_REPLAY_PRIO_UPDATE")
    rig.update(*nasty_update(rs, S * B, 300))
    rig.check_tree("per-level again")


def test_empty_ring_writes_nothing():
    rig = Rig(2, 5)
    out = rig.draw(70, 0)
    for name, (whole, view) in out.items():
        assert bool((whole._base == FILL).all()), name
    A, dsum, M = rig.A, sum(WIDTHS), 70
    g = {"obs": guarded((dsum * M,), torch.float32), "next_obs": guarded((dsum * M,), torch.float32),
         "act": guarded((A, M, 5), torch.float32), "rew": guarded((A, M), torch.float32), "done": guarded((A, M), torch.uint8)}
    rc = rig.L.mpe_replay_gather(C.byref(rig.d), M, out["idx"][1].data_ptr(), g["obs"][1].data_ptr(), g["next_obs"][1].data_ptr(),
                                 g["act"][1].data_ptr(), None, g["rew"][1].data_ptr(), g["done"][1].data_ptr(), None, None, None)
    assert rc == 0, rig.L.mpe_last_error()
    torch.cuda.synchronize()
    assert all(bool((whole._base == FILL).all()) for whole, view in g.values())
    assert not rig.pf["tree"][1].any() and float(rig.pf["pmax"].item()) == 1.0


def test_gather_on_a_plain_buffer_equals_the_numpy_gather():
    env = mpe.make_env("simple_speaker_listener", batch_size=7, seed=1)
    buf = ReplayBuffer(env, steps=3, seed=4)
    ring = push_coded(buf, 5)
    rs = np.random.RandomState(1)
    for M in (1, 64, 65, 300):
        idx = rs.randint(0, 21, size=M).astype(np.int64)
        if M > 2:
            idx[1] = idx[0]
        t = dev(idx)
        b = buf.gather(t, joint=True)
        torch.cuda.synchronize()
        g = ring.gather(idx.tolist())
        assert b.idx is t and t.cpu().tolist() == idx.tolist()
        for i in range(buf.A):
            assert np.array_equal(b.obs_n[i].cpu().numpy(), g["obs_n"][i]) and np.array_equal(b.next_obs_n[i].cpu().numpy(), g["next_obs_n"][i])
        for f in ("act", "utter", "rew", "done"):
            assert np.array_equal(getattr(b, f).cpu().numpy(), g[f]), f
        assert torch.equal(b.joint, torch.cat([b.obs_n[0], b.obs_n[1], b.utter[0], b.act[1]], dim=1))
        assert torch.equal(b.joint_next, torch.cat(b.next_obs_n, dim=1))
    # gather's tensors are not sample's: a sample of the same shape leaves the gathered batch alone
    keep = b.rew.clone()
    s = buf.sample(300, draw=0, joint=True)
    assert s is not b and torch.equal(b.rew, keep) and s.idx is not b.idx
    # an index outside the ring gathers transition 0
    out = buf.gather(dev(np.array([-1, 21, 2 ** 41, 0], np.int64)))
    torch.cuda.synchronize()
    assert torch.equal(out.rew[:, :3], out.rew[:, 3:].expand(-1, 3)) and np.array_equal(out.rew.cpu().numpy()[:, 3], ring.gather([0])["rew"][:, 0])


def tree_of(buf):
    torch.cuda.synchronize()
    return buf.tree.cpu().numpy().copy(), float(buf.pmax.item()), int(buf.head.item())


def assert_tree_is(buf, ref):
    tree, pmax, head = tree_of(buf)
    assert np.array_equal(R.bits(tree), R.bits(ref.tree())) and pmax == float(ref.pmax) and head == ref.head == buf.count
    assert int(buf._prio_ticket.item()) == 0 and int(buf._ticket.item()) == 0


def test_buffer_sample_weights_and_updates():
    """PrioritizedReplayBuffer on an env: sample() = the restated draw + the NumPy gather; weights(); update_td() = the power in
    torch, then the update rule."""
    B, S = 6, 5
    env = mpe.make_env("simple_spread", batch_size=B, seed=3)
    buf = PrioritizedReplayBuffer(env, steps=S, seed=11, alpha=0.5, eps=0.25)
    ring = push_coded(buf, 7)
    ref = P.PrioTree(S, B)
    for _ in range(7):
        ref.push()
    assert_tree_is(buf, ref)
    assert torch.equal(buf.priorities, torch.ones(S, B, device="cuda")) and float(buf.level(2)[0]) == 30.0 and len(buf.level(1)) == 2
    td = torch.linspace(-3, 3, 40, device="cuda")
    idx = dev(np.random.RandomState(2).randint(0, S * B, size=40).astype(np.int64))
    buf.update_td(idx, td)
    ref.update(idx.cpu().numpy(), ((td.abs() + 0.25) ** 0.5).cpu().numpy())
    assert_tree_is(buf, ref)
    b = buf.sample(130, draw=4, joint=True)
    torch.cuda.synchronize()
    want, prio, total, _ = ref.draw(130, 11, 4)
    assert b.idx.cpu().tolist() == want.tolist() and np.array_equal(b.prio.cpu().numpy(), prio)
    assert float(b.total.item()) == float(total) and int(b.n_valid.item()) == 30 == len(buf)
    g = ring.gather(want.tolist())
    assert all(np.array_equal(b.obs_n[i].cpu().numpy(), g["obs_n"][i]) for i in range(3))
    assert np.array_equal(b.act.cpu().numpy(), g["act"]) and np.array_equal(b.rew.cpu().numpy(), g["rew"])
    assert torch.equal(b.joint, torch.cat(list(b.obs_n) + [b.act[i] for i in range(3)], dim=1))
    w = b.weights(0.4).cpu().numpy().astype(np.float64)
    ideal = (30 * prio.astype(np.float64) / float(total)) ** -0.4
    assert np.allclose(w, ideal / ideal.max(), rtol=1e-5) and w.max() == 1.0
    d0 = buf._draw
    assert buf.sample(130).idx.cpu().tolist() == ref.draw(130, 11, d0)[0].tolist() and buf._draw == d0 + 1
    with pytest.raises(_abi.MpeError, match="priority is a contiguous float32 \\[40\\]"):
        buf.update_priorities(idx, td[:39].contiguous())
    with pytest.raises(_abi.MpeError, match="obs_n\\[0\\]"):      # a refused push enqueues nothing: the tree stays as it was
        buf.push([o[:, :5].contiguous() for o in buf.obs_n[0]], buf.act[0], buf.next_obs_n[0], buf.rew[0], buf.done[0])
    assert_tree_is(buf, ref)


def test_loop_run_and_captured_loop_with_a_prioritized_buffer():
    """PolicyLoop.run(T, replay=prio_buf) pushes priorities with every step; capture(T, replay=prio_buf) leaves head, tree and pmax
    exactly as they were (the two warm-up pushes are taken back, a raised pmax included), and each replay moves T slots on."""
    B, S, T = 6, 16, 4
    env, loop, mods = spread_loop()
    buf = PrioritizedReplayBuffer(env, steps=S, seed=1)
    loop.run(3, replay=buf)
    ref = P.PrioTree(S, B)
    for _ in range(3):
        ref.push()
    assert_tree_is(buf, ref)
    idx, pr = dev(np.array([0, 7, 17, 40], np.int64)), dev(np.array([0.5, 3.0, 0.125, 9.0], np.float32))      # leaf 40: still zero
    buf.update_priorities(idx, pr)
    ref.update(idx.cpu().numpy(), pr.cpu().numpy())
    assert float(ref.pmax) == 3.0
    assert_tree_is(buf, ref)
    before = tree_of(buf)
    g = loop.capture(T, replay=buf)
    after = tree_of(buf)
    assert np.array_equal(R.bits(before[0]), R.bits(after[0])) and before[1:] == after[1:] and buf.count == 3
    assert not buf.priorities[3:].any()      # no never-recorded slot became drawable
    for k in range(3):
        g.replay()
        for _ in range(T):
            ref.push()
        assert_tree_is(buf, ref)
    assert buf.count == 3 + 3 * T and bool((buf.priorities[3:15] == 3.0).all()) and not buf.priorities[15:].any()
    b = buf.sample(64, draw=2)
    torch.cuda.synchronize()
    assert b.idx.cpu().tolist() == ref.draw(64, 1, 2)[0].tolist()
    # capture across the wrap of a small ring: the two warm-up slots are the last and the first
    env2, loop2, _ = spread_loop(mods)
    small = PrioritizedReplayBuffer(env2, steps=3, seed=1)
    loop2.run(2, replay=small)
    small.update_priorities(dev(np.array([1, 8], np.int64)), dev(np.array([5.0, 0.25], np.float32)))
    before = tree_of(small)
    loop2.capture(2, replay=small)
    after = tree_of(small)
    assert np.array_equal(R.bits(before[0]), R.bits(after[0])) and before[1:] == after[1:]


def test_one_graph_holds_push_sample_and_update():
    B, S, M = 6, 4, 64
    env = mpe.make_env("simple_spread", batch_size=B, seed=3)
    bufs = [PrioritizedReplayBuffer(env, steps=S, seed=9, alpha=0.7) for _ in range(2)]
    st = R.coded_step(1, B, bufs[0].obs_widths, 0)
    args = ([dev(o) for o in st[0]], dev(st[1]), [dev(o) for o in st[3]], dev(st[4]), dev(st[5]))

    def iteration(buf):
        buf.push(*args)
        b = buf.sample(M, draw=7)
        buf.update_td(b.idx, b.rew[0] * b.weights(0.5) + b.prio)
        return b
    graphed, eager = bufs
    iteration(graphed)      # code objects and the batch's tensors outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b = iteration(graphed)
    graphed.count -= 1      # (the captured push has not run)
    outs = []
    for _ in range(3):
        g.replay()
        graphed.count += 1
        torch.cuda.synchronize()
        outs.append((b.idx.clone(), b.prio.clone(), b.total.clone(), b.n_valid.clone()))
    want = []
    for _ in range(4):
        e = iteration(eager)
        torch.cuda.synchronize()
        want.append((e.idx.clone(), e.prio.clone(), e.total.clone(), e.n_valid.clone()))
    for got, exp in zip(outs, want[1:]):
        assert all(torch.equal(x, y) for x, y in zip(got, exp))
    assert [int(o[3].item()) for o in outs] == [12, 18, 24]      # each replay moved one slot on
    assert torch.equal(graphed.tree, eager.tree) and torch.equal(graphed.pmax, eager.pmax) and torch.equal(graphed.head, eager.head)
    assert float(graphed.pmax.item()) > 1.0 and int(graphed.head.item()) == 4 == graphed.count


def test_abi_refuses_every_invalid_call_by_name_and_leaves_the_tree_alone():
    rig = Rig(3, 5)
    rig.push()
    rig.update(np.arange(5), np.array([1, 2, 3, 4, 5], np.float32))
    L, d, p = rig.L, rig.d, rig.p
    idx, pr = dev(np.arange(4, dtype=np.int64)), dev(np.ones(4, np.float32))
    o = {"idx": torch.full((8,), FILL, dtype=torch.int64, device="cuda"), "prio": torch.full((8,), FILL, dtype=torch.float32, device="cuda"),
         "total": torch.full((1,), FILL, dtype=torch.float32, device="cuda"), "n_valid": torch.full((1,), FILL, dtype=torch.int64, device="cuda")}
    torch.cuda.synchronize()
    before = {"tree": rig.pf["tree"][0]._base.clone(), "pmax": rig.pf["pmax"].clone(), "ticket": rig.pf["ticket"].clone(),
              "head": rig.f["head"][0].clone()}

    def ep(**kw):
        e = _abi.MpeReplayPrio.from_buffer_copy(p)
        for k, v in kw.items():
            setattr(e, k, v)
        return C.byref(e)

    def ed(**kw):
        e = _abi.MpeReplay.from_buffer_copy(d)
        for k, v in kw.items():
            setattr(e, k, v)
        return C.byref(e)

    def draw(pd=None, M=8, **kw):
        a = {k: v.data_ptr() for k, v in o.items()}
        a.update(kw)
        return L.mpe_replay_prio_draw(C.byref(d), pd or C.byref(p), M, 0, None, a["idx"], a["prio"], a["total"], a["n_valid"], None)

    def update(pd=None, M=4, i=idx.data_ptr(), v=pr.data_ptr()):
        return L.mpe_replay_prio_update(C.byref(d), pd or C.byref(p), M, i, v, None)
    tree_ptr = rig.pf["tree"][1].data_ptr()
    cases = [(lambda: L.mpe_replay_prio_push(C.byref(d), None, None), b"mpe_replay_prio_push: prio is NULL"),
             (lambda: L.mpe_replay_prio_push(ed(head=None), C.byref(p), None), b"replay->head is NULL"),
             (lambda: L.mpe_replay_prio_push(ed(S=0), C.byref(p), None), b"S = 0"),
             (lambda: L.mpe_replay_prio_push(ed(S=4), C.byref(p), None), b"prio->n_leaves = 15, the ring has S * B = 20"),
             (lambda: L.mpe_replay_prio_push(C.byref(d), ep(n_leaves=16), None), b"prio->n_leaves = 16"),
             (lambda: L.mpe_replay_prio_push(C.byref(d), ep(tree=None), None), b"prio->tree is NULL"),
             (lambda: L.mpe_replay_prio_push(C.byref(d), ep(tree=tree_ptr + 4), None), b"not 16-byte aligned"),
             (lambda: L.mpe_replay_prio_push(C.byref(d), ep(pmax=None), None), b"prio->pmax is NULL"),
             (lambda: L.mpe_replay_prio_push(C.byref(d), ep(ticket=None), None), b"prio->ticket is NULL"),
             (lambda: draw(M=0), b"mpe_replay_prio_draw: M = 0"), (lambda: draw(M=2 ** 31), b"at most 2^31 - 1"),
             (lambda: draw(idx=None), b"idx is NULL"), (lambda: draw(prio=None), b"prio_out is NULL"),
             (lambda: draw(total=None), b"total is NULL"), (lambda: draw(n_valid=None), b"n_valid is NULL"),
             (lambda: draw(pd=ep(tree=None)), b"mpe_replay_prio_draw: prio->tree is NULL"),
             (lambda: update(M=0), b"mpe_replay_prio_update: M = 0"), (lambda: update(i=None), b"idx is NULL"),
             (lambda: update(v=None), b"prio_in is NULL"), (lambda: update(pd=ep(pmax=None)), b"prio->pmax is NULL"),
             (lambda: L.mpe_replay_prio_repair(C.byref(d), C.byref(p), 11, 5, None), b"mpe_replay_prio_repair: leaves [11, 11 + 5) of 15"),
             (lambda: L.mpe_replay_prio_repair(C.byref(d), C.byref(p), 0, 0, None), b"leaves [0"),
             (lambda: L.mpe_replay_gather(C.byref(d), 4, None, *([None] * 9)), b"mpe_replay_gather: idx is NULL")]
    for call, word in cases:
        rc = call()
        assert rc < 0 and word in L.mpe_last_error(), (rc, word, L.mpe_last_error())
    torch.cuda.synchronize()
    assert torch.equal(rig.pf["tree"][0]._base, before["tree"]) and torch.equal(rig.pf["pmax"], before["pmax"])
    assert torch.equal(rig.pf["ticket"], before["ticket"]) and torch.equal(rig.f["head"][0], before["head"])
    assert all(bool((v == FILL).all()) for v in o.values())
    rig.check_tree()
    # and the valid repair: leaves written by hand, every ancestor recomputed
    rig.pf["tree"][1][3:9] = torch.tensor([0.5, 0.0, 7.0, 0.25, 0.0, 2.0], device="cuda")
    rig.ref.leaves[3:9] = [0.5, 0.0, 7.0, 0.25, 0.0, 2.0]
    assert L.mpe_replay_prio_repair(C.byref(d), C.byref(p), 3, 6, None) == 0, L.mpe_last_error()
    rig.check_tree()
