"""n-step returns without a GPU: the rule's restatement (tests/_replay_nstep_ref.py) against a brute-force loop over absolute step
numbers that never wraps, the MpeReplayNStep binding against the header, and every refusal that is decided on the host before
anything is launched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.replay import PrioritizedReplayBuffer, ReplayBuffer

import _replay_ref as R
import _replay_nstep_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def filled(S, B, widths, dim_c, T):
    """T sparse steps into a NumpyRing -> (the ring, every pushed step in a list that is never overwritten)."""
    ring, steps = R.NumpyRing(S, B, widths, dim_c), []
    for t in range(T):
        st = N.sparse_step(t, B, widths, dim_c)
        ring.push(*st)
        steps.append(st)
    return ring, steps


def brute(steps, S, B, g, world, n, gamma, L, p):
    """The chain that starts at ABSOLUTE step g of `world`, from the list of all pushed steps: -> (m, last step, cause, ret per
    agent, discount).  No slot, no modulus by S: a step is in reach while it was pushed (t < h)."""
    h, A = len(steps), steps[0][4].shape[0]
    assert h - min(h, S) <= g < h
    used, t = [], g
    while True:
        used.append(t)
        if steps[t][5][:, world].any():
            cause = "done"
        elif L > 0 and (t + 1 + p) % L == 0:
            cause = "cut"
        elif len(used) == n:
            cause = "n"
        elif t + 1 == h:
            cause = "head"
        else:
            t += 1
            continue
        break
    rets = [N.chain_returns([steps[u][4][i, world] for u in used], gamma) for i in range(A)]
    return len(used), used[-1], cause, [r[0] for r in rets], rets[0][1]


CASES = [(4, 7, 3, 3, 0, 0), (4, 7, 9, 1, 0, 0), (4, 7, 9, 3, 0, 0), (4, 7, 9, 4, 0, 0), (8, 64, 19, 5, 7, 0), (8, 64, 19, 5, 7, 3),
         (6, 5, 15, 4, 5, 0), (1, 3, 4, 16, 0, 0), (5, 2, 23, 16, 3, 2)]


@pytest.mark.parametrize("S,B,T,n,L,p", CASES)
def test_restatement_equals_the_brute_force_walk_over_absolute_steps(S, B, T, n, L, p):
    widths, gamma = [2, 3, 1], 0.95
    ring, steps = filled(S, B, widths, 0, T)
    nv = ring.n_valid()
    out = N.nstep(ring, list(range(nv)), n, gamma, L, p)
    assert out["idx"] == list(range(nv))
    for j in range(nv):
        slot, world = divmod(j, B)
        g = max(t for t in range(T) if t % S == slot)      # the newest pushed step that lives in this slot
        m, last_t, cause, ret, disc = brute(steps, S, B, g, world, n, gamma, L, p)
        assert (int(out["n_used"][j]), int(out["last"][j]), out["cause"][j]) == (m, (last_t % S) * B + world, cause), j
        assert np.array_equal(R.bits(out["ret"][:, j]), R.bits(np.array(ret, np.float32))), j
        assert R.bits(out["discount"][j]) == R.bits(disc) and 1 <= m <= min(n, S)
        assert np.array_equal(out["done"][:, j], steps[last_t][5][:, world])
        assert all(np.array_equal(out["next_obs_n"][i][j], steps[last_t][3][i][world]) for i in range(3))
        assert all(np.array_equal(out["obs_n"][i][j], steps[g][0][i][world]) for i in range(3))


def test_the_gpu_cases_reach_every_stop_cause():
    """The shapes of tests/test_gpu_replay_nstep.py's first test, on the restatement alone: the spread case has all four causes,
    every other case at least three (n = 1 can only stop on n... or earlier: done and cut come first in CAUSES)."""
    spread = filled(8, 64, [18] * 3, 0, 19)[0]
    for p in (0, 3):
        causes = N.nstep(spread, list(range(spread.n_valid())), 5, 0.95, 7, p)["cause"]
        counts = {c: causes.count(c) for c in N.CAUSES}
        print(p, counts)
        assert all(35 <= v for v in counts.values()), counts
    sl = filled(4, 7, [3, 11], 3, 9)[0]
    assert len(set(N.nstep(sl, list(range(28)), 3, 0.95)["cause"])) == 3
    adv = filled(6, 5, [8, 10, 10], 0, 15)[0]
    assert len(set(N.nstep(adv, list(range(30)), 4, 0.95, 5, 0)["cause"])) >= 3


def test_rounding_order_matters_for_the_coded_rewards():
    """ret in float32 step by step differs from the float64 sum rounded once for some chain of the sparse steps: a kernel that
    fused or reordered the operations would not pass an equality test built on them."""
    ring, _ = filled(8, 64, [2] * 3, 0, 19)
    out = N.nstep(ring, list(range(ring.n_valid())), 5, 0.95, 0, 0)
    differ = 0
    for j in range(ring.n_valid()):
        slot, world = divmod(j, 64)
        m = int(out["n_used"][j])
        exact = sum(float(np.float32(0.95)) ** k * float(ring.rew[(slot + k) % 8, 0, world]) for k in range(m))
        differ += int(np.float32(exact) != out["ret"][0, j])
    assert differ > 20, differ


def test_out_of_range_indices_are_transition_0():
    ring, _ = filled(4, 7, [2, 2], 0, 3)      # a partial ring: 21 valid of 28
    bad = [-1, 21, 27, 28, 2 ** 62]
    out = N.nstep(ring, bad + [0], 3, 0.5)
    assert out["idx"] == [0] * 6 and len(set(out["last"].tolist())) == 1 and len(set(R.bits(out["ret"][0]).tolist())) == 1


def test_header_names_the_constant_and_states_the_rule():
    hdr = open(os.path.join(ROOT, "include", "mpe_hip.h")).read()
    assert int(re.search(r"#define MPE_REPLAY_MAX_NSTEP (\d+)", hdr).group(1)) == _abi.MPE_REPLAY_MAX_NSTEP == N.MAX_NSTEP == 16
    for phrase in ("ahead = (h - 1 - slot) mod S", "(g + k + 1 + p) mod L == 0", "d_k = d_{k-1} * gamma", "discount [M] float32 = d_{m-1} * gamma"):
        assert phrase in hdr, phrase
    assert set(("NStepReplayBatch", "PrioritizedNStepReplayBatch")) <= set(mpe.__all__)


def test_nstep_binding_layout_matches_the_header(tmp_path):
    names = [f[0] for f in _abi.MpeReplayNStep._fields_]
    src = tmp_path / "nstep_layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mpe_hip.h\"\nint main(void) {\n"
                   "  printf(\"sizeof %zu\\n\", sizeof(MpeReplayNStep));\n" +
                   "".join("  printf(\"%s %%zu\\n\", offsetof(MpeReplayNStep, %s));\n" % (n, n) for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "nstep_layout")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict((ln.split()[0], int(ln.split()[1])) for ln in r.stdout.strip().splitlines())
    assert got.pop("sizeof") == C.sizeof(_abi.MpeReplayNStep) == _abi.lib().mpe_sizeof_replay_nstep() == 24
    assert got == {n: getattr(_abi.MpeReplayNStep, n).offset for n in names}


def _desc(A=2, B=4, S=3):
    d = _abi.MpeReplay()
    d.n_agents, d.dim_c, d.B, d.S = A, 0, B, S
    for i in range(A):
        d.obs_width[i], d.movable[i] = 6, 1
    for name in ("obs", "next_obs", "act", "rew", "done", "head", "ticket"):      # (fake, aligned, never dereferenced: the checks stop first)
        setattr(d, name, 4096)
    return d


def _ns(n=3, gamma=0.9, L=0, p=0):
    ns = _abi.MpeReplayNStep()
    ns.n, ns.gamma, ns.episode_len, ns.episode_phase = n, gamma, L, p
    return ns


@pytest.mark.parametrize("entry", ["mpe_replay_sample_nstep", "mpe_replay_gather_nstep"])
def test_abi_refuses_by_name_before_any_launch(entry):
    """No device exists here: each call returns from the host-side checks.  The output pointers are fake and aligned."""
    L = _abi.lib()
    d = _desc()
    outs = {k: 4096 for k in ("idx", "obs", "next_obs", "act", "utter", "rew", "done", "joint", "joint_next", "ret", "discount", "n_used", "last")}

    def call(ns, M=8, **kw):
        o = dict(outs)
        o.update(kw)
        tail = [o[k] for k in ("idx", "obs", "next_obs", "act", "utter", "rew", "done", "joint", "joint_next", "ret", "discount", "n_used", "last")]
        lead = (C.byref(d), C.byref(ns) if ns is not None else None, M) + ((0,) if entry == "mpe_replay_sample_nstep" else ())
        return getattr(L, entry)(*(lead + tuple(tail) + (None,)))
    cases = [(lambda: call(_ns(n=0)), b"nstep->n = 0"), (lambda: call(_ns(n=17)), b"nstep->n = 17"),
             (lambda: call(_ns(n=-1)), b"MPE_REPLAY_MAX_NSTEP = 16"),
             (lambda: call(_ns(gamma=float("nan"))), b"nstep->gamma"), (lambda: call(_ns(gamma=float("inf"))), b"is not finite"),
             (lambda: call(_ns(L=-1)), b"nstep->episode_len = -1"), (lambda: call(_ns(L=5, p=5)), b"nstep->episode_phase = 5"),
             (lambda: call(_ns(L=0, p=1)), b"nstep->episode_phase = 1"), (lambda: call(_ns(L=5, p=-1)), b"nstep->episode_phase = -1"),
             (lambda: call(_ns(), ret=None), b"%s: ret is NULL" % entry.encode()), (lambda: call(_ns(), discount=None), b"discount is NULL"),
             (lambda: call(_ns(), n_used=None), b"n_used is NULL"), (lambda: call(_ns(), last=None), b"last is NULL"),
             (lambda: call(_ns(), last=4100), b"last is not 8-byte aligned"), (lambda: call(_ns(), idx=None), b"idx is NULL"),
             (lambda: call(_ns(), M=0), b"M = 0"), (lambda: call(None), b"nstep is NULL"),
             (lambda: call(_ns(), joint=None), b"joint and joint_next")]
    for fn, word in cases:
        rc = fn()
        assert rc == -1 and word in L.mpe_last_error() and entry.encode() in L.mpe_last_error(), (rc, word, L.mpe_last_error())


def test_python_refusals_come_before_anything_else():
    env = mpe.make_env("simple_adversary", batch_size=4, device="cpu")
    for buf, who in ((ReplayBuffer(env, steps=3), "ReplayBuffer.sample"), (PrioritizedReplayBuffer(env, steps=3), "PrioritizedReplayBuffer.sample")):
        with pytest.raises(_abi.MpeError, match="%s: gamma is required when n_step is given" % who):
            buf.sample(8, n_step=3)
        for kw, word in ((dict(n_step=0), "n_step = 0"), (dict(n_step=17), "n_step = 17"), (dict(n_step=3, gamma=float("nan")), "not finite"),
                         (dict(n_step=3, episode_len=-1), "episode_len = -1"), (dict(n_step=3, episode_len=4, episode_phase=4), "episode_phase = 4"),
                         (dict(n_step=3, episode_phase=1), "episode_phase = 1")):
            kw.setdefault("gamma", 0.9)
            with pytest.raises(_abi.MpeError, match=word):
                buf.sample(8, **kw)
        with pytest.raises(_abi.MpeError, match="empty"):      # valid n-step arguments: the next check is today's
            buf.sample(8, n_step=3, gamma=0.9, episode_len=4, episode_phase=3)
        with pytest.raises(_abi.MpeError, match="empty"):      # n_step=None: today's path, whatever gamma says
            buf.sample(8, gamma=0.9)
    with pytest.raises(_abi.MpeError, match="ReplayBuffer.gather: gamma is required"):
        ReplayBuffer(env, steps=3).gather(None, n_step=2)
