"""Prioritized replay without a GPU: the NumPy restatement (tests/_replay_prio_ref.py) is a proportional sampler, the last-child
rule fires where rounding asks for it, the host-only layout entry point agrees with the restatement, the MpeReplayPrio binding
agrees with the header, and every refusal that is decided on the host before anything is launched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.replay import PrioritizedReplayBuffer, ReplayBuffer

import _replay_prio_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_priorities(rs, n):
    """2^k * (1 + r), k in [-3, 3]"""
    return (2.0 ** rs.randint(-3, 4, size=n) * (1.0 + rs.rand(n))).astype(np.float32)


@pytest.mark.parametrize("S,B,filled,M", [(3, 257, 3, 65536), (7, 5, 4, 65536), (1, 1, 1, 65536), (1, 16, 1, 65536), (1, 17, 1, 65536),
                                          (4, 4097, 2, 20000)])
def test_reference_is_a_proportional_sampler(S, B, filled, M):
    """M stratified draws: no unfilled leaf is ever drawn, and every leaf's count is within 3 of M * p_j / total.  Stratification
    alone gives +-2 (the leaf's interval of the cumulative sum cuts at most two strata partly); 3 leaves room for the float32
    running sums of the descent.  The rule is deterministic: the six shapes give at most 1.87."""
    rs = np.random.RandomState(S * 1000 + B)
    t = P.PrioTree(S, B)
    for _ in range(filled):
        t.push()
    t.leaves[:filled * B] = random_priorities(rs, filled * B)
    idx, prio, total, fired = t.draw(M, seed=0xC0FFEE, draw_no=S + B)
    assert idx.min() >= 0 and idx.max() < filled * B == t.n_valid()
    assert np.array_equal(prio, t.leaves[idx]) and (prio > 0).all()
    counts = np.bincount(idx, minlength=S * B).astype(np.float64)
    expect = M * t.leaves.astype(np.float64) / t.leaves.astype(np.float64).sum()
    worst = float(np.abs(counts - expect).max())
    print("S=%d B=%d: worst |count - M p| = %.3f, last-child rule fired %d times" % (S, B, worst, fired))
    assert not counts[filled * B:].any()
    assert worst <= 3.0
    assert abs(float(total) - float(t.leaves.astype(np.float64).sum())) <= 1e-5 * float(total)


def test_last_child_rule_fires_where_the_pairwise_total_exceeds_the_sequential_sum():
    p = P.find_last_child_case(seed=0)
    seq = np.float32(0)
    for c in p:
        seq = np.float32(seq + c)
    t = P.PrioTree(1, 16)
    t.push()
    t.leaves[:] = p
    assert t.levels()[1][0] == P.pair_sum(p[None, :])[0] > seq
    idx, prio, total, fired = t.draw(1, u24=[0xFFFFFF])
    assert fired == 1 and total == t.levels()[1][0]
    assert idx[0] == 15 and prio[0] == p[15] > 0
    # the last POSITIVE child: with the tail of the node never pushed, the rule lands on the last leaf that holds a priority
    t2 = P.PrioTree(1, 17)
    t2.push()
    t2.leaves[:16] = p
    t2.leaves[12:] = 0
    t2.leaves[16] = 0
    x = t2.draw(1, u24=[0xFFFFFF])
    assert x[0][0] < 12 and x[1][0] > 0


@pytest.mark.parametrize("n", [1, 2, 16, 17, 256, 257, 4096, 4097, 2 ** 40 - 1])
def test_layout_entry_point_equals_the_reference(n):
    off, floats = _abi.replay_prio_layout(n)
    want_off, want_floats = P.layout(n)
    assert off == want_off and floats == want_floats
    sizes = P.level_sizes(n)
    assert len(off) == len(sizes) + 1 <= _abi.MPE_REPLAY_PRIO_MAX_LEVELS + 1 and sizes[-1] == 1
    assert all(o % 16 == 0 for o in off) and all(off[l + 1] - off[l] >= sizes[l] for l in range(len(sizes)))
    if n == 1:
        assert off == [0, 16]
    if n == 17:
        assert off == [0, 32, 48, 64]


def test_layout_refuses_by_name():
    L = _abi.lib()
    for n in (0, -1, 2 ** 40):
        assert L.mpe_replay_prio_layout(n, None, None, None) < 0 and b"n_leaves" in L.mpe_last_error()
    assert L.mpe_replay_prio_layout(5, None, None, None) == 0      # every output is optional


def test_header_names_the_constants():
    hdr = open(os.path.join(ROOT, "include", "mpe_hip.h")).read()
    assert int(re.search(r"#define MPE_STREAM_REPLAY_PRIO (0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == _abi.MPE_STREAM_REPLAY_PRIO \
        == P.STREAM_REPLAY_PRIO == int.from_bytes(b"RPRO", "big")
    assert int(re.search(r"#define MPE_REPLAY_PRIO_FANOUT (\d+)", hdr).group(1)) == _abi.MPE_REPLAY_PRIO_FANOUT == P.FANOUT
    assert int(re.search(r"#define MPE_REPLAY_PRIO_MAX_LEVELS (\d+)", hdr).group(1)) == _abi.MPE_REPLAY_PRIO_MAX_LEVELS
    assert float.fromhex(re.search(r"#define MPE_REPLAY_PRIO_MIN (\S+)f", hdr).group(1)) == _abi.MPE_REPLAY_PRIO_MIN == float(P.PRIO_MIN)
    assert float.fromhex(re.search(r"#define MPE_REPLAY_PRIO_MAX (\S+)f", hdr).group(1)) == _abi.MPE_REPLAY_PRIO_MAX == float(P.PRIO_MAX)
    assert len(P.level_sizes(2 ** 40 - 1)) == _abi.MPE_REPLAY_PRIO_MAX_LEVELS


def test_binding_layout_matches_the_header(tmp_path):
    names = [f[0] for f in _abi.MpeReplayPrio._fields_]
    assert names == ["n_leaves", "tree", "pmax", "ticket"]
    src = tmp_path / "prio_layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mpe_hip.h\"\nint main(void) {\n"
                   "  printf(\"sizeof %zu\\n\", sizeof(MpeReplayPrio));\n"
                   "  printf(\"replay %zu\\n\", sizeof(MpeReplay));\n" +
                   "".join("  printf(\"%s %%zu\\n\", offsetof(MpeReplayPrio, %s));\n" % (n, n) for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "prio_layout")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict((ln.split()[0], int(ln.split()[1])) for ln in r.stdout.strip().splitlines())
    assert got.pop("sizeof") == C.sizeof(_abi.MpeReplayPrio) == _abi.lib().mpe_sizeof_replay_prio() == 32      # pinned
    assert got.pop("replay") == C.sizeof(_abi.MpeReplay) == _abi.lib().mpe_sizeof_replay()      # the ring's descriptor kept its size
    assert got == {n: getattr(_abi.MpeReplayPrio, n).offset for n in names}


def test_clamp_and_nan_rule():
    with np.errstate(over="ignore"):
        got = P.clamp(np.array([0.0, -1.0, np.nan, -np.inf, np.inf, 1e-30, 2.0 ** -40, 2.0 ** -41, 2.0 ** 40, 2.0 ** 41, 1.5, 1e-45],
                               dtype=np.float32))
    lo, hi = np.float32(2.0 ** -40), np.float32(2.0 ** 40)
    assert got.dtype == np.float32
    assert got.tolist() == [lo, lo, lo, lo, hi, lo, lo, lo, hi, hi, 1.5, lo]
    t = P.PrioTree(2, 3)
    t.push()
    t.update([0, 1, 1, 1, 2, 3, 7, -1], np.array([np.nan, 2.0, 5.0, 3.0, np.inf, 9.0, 9.0, 9.0], np.float32))
    assert t.leaves.tolist() == [lo, 5.0, hi, 0.0, 0.0, 0.0] and t.pmax == hi      # leaf 3: still zero; 7, -1: outside
    t.update([1], np.array([0.25], np.float32))      # an update replaces: not max(old, new)
    assert t.leaves[1] == 0.25 and t.pmax == hi
    t.push()
    assert t.leaves.tolist() == [lo, 0.25, hi, hi, hi, hi]


def _desc(B=4, S=3):
    d = _abi.MpeReplay()
    d.n_agents, d.dim_c, d.B, d.S = 2, 0, B, S
    for i in range(2):
        d.obs_width[i], d.movable[i] = 6, 1
    for name in ("obs", "next_obs", "act", "rew", "done", "head", "ticket"):      # fake, aligned, never dereferenced
        setattr(d, name, 4096)
    return d


def test_null_pointers_are_refused_before_any_launch():
    """No device memory exists here: every call returns from the host-side checks."""
    L = _abi.lib()
    d = _desc()
    p = _abi.MpeReplayPrio()
    p.n_leaves, p.tree, p.pmax, p.ticket = 12, 4096, 4096, 4096
    dp, pp = C.byref(d), C.byref(p)

    def edited(**kw):
        e = _abi.MpeReplayPrio.from_buffer_copy(p)
        for k, v in kw.items():
            setattr(e, k, v)
        return C.byref(e)
    cases = [(lambda: L.mpe_replay_prio_push(dp, None, None), b"prio is NULL"),
             (lambda: L.mpe_replay_prio_push(None, pp, None), b"replay is NULL"),
             (lambda: L.mpe_replay_prio_push(dp, edited(n_leaves=11), None), b"prio->n_leaves = 11"),
             (lambda: L.mpe_replay_prio_push(dp, edited(tree=None), None), b"prio->tree is NULL"),
             (lambda: L.mpe_replay_prio_push(dp, edited(tree=4100), None), b"prio->tree is NULL or not 16-byte aligned"),
             (lambda: L.mpe_replay_prio_push(dp, edited(pmax=None), None), b"prio->pmax is NULL"),
             (lambda: L.mpe_replay_prio_push(dp, edited(ticket=None), None), b"prio->ticket is NULL"),
             (lambda: L.mpe_replay_prio_draw(dp, pp, 0, 0, None, 4096, 4096, 4096, 4096, None), b"M = 0"),
             (lambda: L.mpe_replay_prio_draw(dp, pp, 8, 0, None, None, 4096, 4096, 4096, None), b"idx is NULL"),
             (lambda: L.mpe_replay_prio_draw(dp, pp, 8, 0, None, 4096, None, 4096, 4096, None), b"prio_out is NULL"),
             (lambda: L.mpe_replay_prio_draw(dp, pp, 8, 0, None, 4096, 4096, None, 4096, None), b"total is NULL"),
             (lambda: L.mpe_replay_prio_draw(dp, pp, 8, 0, None, 4096, 4096, 4096, None, None), b"n_valid is NULL"),
             (lambda: L.mpe_replay_prio_draw(dp, pp, 8, 0, 4098, 4096, 4096, 4096, 4096, None), b"u24 is not 4-byte aligned"),
             (lambda: L.mpe_replay_prio_update(dp, pp, -2, 4096, 4096, None), b"M = -2"),
             (lambda: L.mpe_replay_prio_update(dp, pp, 8, None, 4096, None), b"idx is NULL"),
             (lambda: L.mpe_replay_prio_update(dp, pp, 8, 4096, None, None), b"prio_in is NULL"),
             (lambda: L.mpe_replay_prio_repair(dp, pp, -1, 4, None), b"leaves [-1"),
             (lambda: L.mpe_replay_prio_repair(dp, pp, 9, 4, None), b"leaves [9"),
             (lambda: L.mpe_replay_prio_repair(dp, pp, 0, 0, None), b"leaves [0"),
             (lambda: L.mpe_replay_gather(dp, 0, 4096, *([None] * 9)), b"mpe_replay_gather: M = 0"),
             (lambda: L.mpe_replay_gather(dp, 8, None, *([None] * 9)), b"mpe_replay_gather: idx is NULL")]
    for call, word in cases:
        rc = call()
        assert rc < 0 and word in L.mpe_last_error(), (rc, word, L.mpe_last_error())


def test_constructor_and_argument_refusals():
    env = mpe.make_env("simple_adversary", batch_size=4, device="cpu")
    buf = PrioritizedReplayBuffer(env, steps=3, seed=5)
    assert isinstance(buf, ReplayBuffer) and (buf.A, buf.B, buf.S, buf.count, len(buf)) == (3, 4, 3, 0, 0)
    assert (buf.alpha, buf.eps, buf.n_leaves) == (0.6, 1e-6, 12) and (buf.level_off, buf.n_floats) == ([0, 16, 32], 32)
    with pytest.raises(_abi.MpeError, match="empty"):
        buf.sample(8)
    with pytest.raises(_abi.MpeError, match="M = 0"):
        buf.sample(0)
    with pytest.raises(_abi.MpeError, match="steps = 0"):
        PrioritizedReplayBuffer(env, steps=0)
    with pytest.raises(_abi.MpeError, match="2\\^40"):
        PrioritizedReplayBuffer(env, steps=2 ** 38)
    with pytest.raises(_abi.MpeError, match="alpha"):
        PrioritizedReplayBuffer(env, steps=3, alpha=-0.1)
    with pytest.raises(_abi.MpeError, match="eps"):
        PrioritizedReplayBuffer(env, steps=3, eps=0.0)
    with pytest.raises(_abi.MpeError, match="gather: idx"):
        ReplayBuffer(env, steps=3).gather([0, 1])
    assert set(("PrioritizedReplayBuffer", "PrioritizedReplayBatch")) <= set(mpe.__all__)
