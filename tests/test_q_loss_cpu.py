"""The value-based learners' device pieces without a GPU: the float64 form of THE Q LOSS RULE against torch float64
autograd (gather, max / double-Q gather, mse), the statistics of THE EXPLORATION RULE on the draws' own bits, every refusal of
mpe_q_loss, mpe_q_loss_work and mpe_actor_act_explore in the header's order, the host layer's argument checks, and the host walk of
every block, wave and lane of both launches under the sanitizers (tests/c/q_loss_host_walk.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.learner import QLoss, QTargets, RowsLayout, q_loss_tensors
from multiagent_particle_envs_amd.replay import NStepReplayBatch, ReplayBatch

import _q_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x10000      # a plausible, 16-byte aligned address (no refused call reads it)
CASE_IDS = sorted(R.CASES)


# ---- (a) against torch float64 autograd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted,nstep", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("mix", sorted(R.MIXES))
@pytest.mark.parametrize("name", CASE_IDS)
def test_restatement_is_torch_float64_autograd(name, mix, double, weighted, nstep):
    """loss, dL/dlogits and |td| of the float64 form within 1e-12 of each output's largest magnitude; the float32 restatement is
    that form to float32 rounding"""
    case, M = R.CASES[name], 65
    x = R.make_inputs(case, M)
    ref = R.q_loss64(case, x, R.MIXES[mix], double, weighted, nstep)
    t64 = R.torch_q(case, x, R.MIXES[mix], double, weighted, nstep, torch.float64)
    for i in range(case.A):
        assert np.abs(ref["dq_n"][i] - t64["dq_n"][i]).max() <= 1e-12 * np.abs(ref["dq_n"][i]).max(), i
    assert np.abs(ref["td_abs"] - t64["td_abs"]).max() <= 1e-12 * np.abs(ref["td_abs"]).max()
    assert abs(ref["loss"] - t64["loss"]) <= 1e-12 * abs(ref["loss"])
    b32 = R.q_loss32(case, x, R.MIXES[mix], double, weighted, nstep)
    assert abs(float(b32["loss"]) - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    for i in range(case.A):
        assert np.array_equal(b32["dq_n"][i] != 0, ref["dq_n"][i] != 0)
        assert np.abs(b32["dq_n"][i] - ref["dq_n"][i]).max() <= 1e-5 * np.abs(ref["dq_n"][i]).max()


def test_inputs_hold_the_edges_the_sweeps_promise():
    """argmax ties in S and in the action rows, all-done and no-done rows, softmax rows, and (nan=True) a NaN in one q"""
    case, M = R.CASES["reference"], 257
    x = R.make_inputs(case, M, nan=True)
    m = np.arange(M)
    for i in range(case.A):
        for k0, n, rows in case.heads(i):
            S = x["no"][i][:, k0:k0 + n]
            assert ((S == S.max(axis=1, keepdims=True)).sum(axis=1) > 1).any()
            a = x[rows][i]
            assert ((a == a.max(axis=1, keepdims=True)).sum(axis=1) > 1).any()      # a tie in the rows that choose
            assert ((a > 0).sum(axis=1) > 1).any() and ((a == 1).sum(axis=1) == 1).any()      # softmax rows and one-hot rows
    assert x["done"][:, m % 5 == 0].all() and not x["done"][:, m % 5 == 1].any()
    assert np.isnan(x["q_n"][0][M // 2]).all() and sum(int(np.isnan(z).any(axis=1).sum()) for z in x["q_n"]) == 1


# ---- THE EXPLORATION RULE's statistics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [65536 // 4, 65536 // 2])
def test_exploration_rule_statistics(E):
    """over 65 536 draws the explored share lies within 5 binomial sigma of E / 65536, and each of the n = 5 indices within 5 sigma
    of 1 / 5 of the explored draws (a check of the rule on the SAMPLE draws' own bits, not of the kernel)"""
    N, n = 65536, 5
    bits = R.head_bits(0x504F4C49, 12345, N, 7, 1, 1000)
    idx, explored = R.explore_pick(bits, n, E, np.full(N, -1))
    p = E / 65536.0
    k = int(explored.sum())
    assert abs(k - N * p) <= 5 * np.sqrt(N * p * (1 - p)), (k, N * p)
    assert (idx[~explored] == -1).all() and ((idx[explored] >= 0) & (idx[explored] < n)).all()
    for j in range(n):
        c = int((idx[explored] == j).sum())
        assert abs(c - k / n) <= 5 * np.sqrt(k * (1 / n) * (1 - 1 / n)), (j, c, k / n)
    assert R.explore_E(0.0) == 0 and R.explore_E(1.0) == 65536 and R.explore_E(2.0 ** -16) == 1 and R.explore_E(0.5) == 32768
    assert R.explore_E(2.0 ** -18) == 0 and R.explore_E(2.0 ** -17) == 1
    all_, ex = R.explore_pick(bits, n, 65536, np.full(N, -1))
    assert ex.all() and np.array_equal(all_, ((bits & 0xFFFF).astype(np.int64) * n) >> 16)
    assert not R.explore_pick(bits, n, 0, np.full(N, -1))[1].any()


# ---- refusals: one ladder per entry point, the order include/mpe_hip.h states -------------------------------------------------------
def _climb(ladder, state, call):
    L_ = _abi.lib()
    last = None
    for n, (repair, rc_want, msg_want) in enumerate(ladder):
        exec(repair, {"PTR": PTR}, {"s": state})
        rc = call(state)
        msg = L_.mpe_last_error().decode()
        assert (rc, msg) == (rc_want, msg_want), "rung %d (%r): %d %s" % (n, repair, rc, msg)
        if rc == 0:
            assert msg == last, "a call that returns 0 leaves the last error alone"
        last = msg
    assert ladder[-1][1] == 0


def _arr(on, v):
    return (C.c_void_p * 16)(*v) if on else None


Q_ = "mpe_q_loss: "
Q_ALIGN = Q_ + "every float tensor must be 4-byte and work 8-byte aligned"
Q_TOP = ("cfg", "q_ptrs", "next_target", "td", "dq_ptrs", "q_taken", "y", "work", "stats", "loss")
Q_LADDER = [("pass", -1, Q_ + "cfg is NULL")] + [("s['%s'] = PTR" % a, -1, Q_ + "%s is NULL" % b) for a, b in zip(Q_TOP, Q_TOP[1:])] + [
    ("s['loss'] = PTR", -1, Q_ + "A = 17 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
    ("s['A'] = 0", -1, Q_ + "A = 0 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
    ("s['A'] = 2", -1, Q_ + "dim_c = 17 (0..16)"),
    ("s['dim_c'] = -1", -1, Q_ + "dim_c = -1 (0..16)"),
    ("s['dim_c'] = 0", -1, Q_ + "mix = 2 (MPE_Q_INDEPENDENT / MPE_Q_VDN)"),
    ("s['mix'] = 1", -1, Q_ + "agent 0 has no head (neither movable nor speaking with dim_c > 0)"),
    ("s['movable'][:2] = [1, 1]; s['speaks'][:2] = [0, 1]; s['dim_c'] = 12", -2,
     Q_ + "agent 1: 17 logits (5 * movable + dim_c * speaks) > MPE_ACTOR_MAX_OUT = 16"),
    ("s['dim_c'] = 3", -1, Q_ + "act is NULL and an agent moves"),
    ("s['act'] = PTR", -1, Q_ + "utter is NULL and an agent speaks"),
    ("s['utter'] = PTR", -1, Q_ + "M = -1"),
    ("s['M'] = 1 << 30", -1, Q_ + "td->ret is NULL"),
    ("s['ret'] = PTR", -1, Q_ + "td->done is NULL"),
    ("s['done'] = PTR + 1", -1, Q_ + "td->gamma = nan is not finite (and td->discount is NULL)"),
    ("s['gamma'] = 0.95", -1, Q_ + "q_ptrs[1] is NULL"),
    ("s['q'] = [PTR, PTR]; s['dq'] = [None, PTR]", -1, Q_ + "dq_ptrs[0] is NULL"),
    ("s['dq'] = [PTR, PTR + 2]", -1, Q_ALIGN),
    ("s['dq'] = [PTR, PTR + 4]; s['next_online'] = PTR + 1", -1, Q_ALIGN),
    ("s['next_online'] = PTR; s['weights'] = PTR + 2", -1, Q_ALIGN),
    ("s['weights'] = PTR + 4; s['td_abs'] = PTR + 3", -1, Q_ALIGN),
    ("s['td_abs'] = None; s['discount'] = PTR + 2", -1, Q_ALIGN),
    ("s['discount'] = PTR; s['gamma'] = float('nan'); s['work'] = PTR + 4", -1, Q_ALIGN),
    ("s['work'] = PTR + 8", -1, Q_ + "A * M = 2 * 1073741824 (need A * M < 2^31)"),
    ("s['M'] = 0", 0, Q_ + "A * M = 2 * 1073741824 (need A * M < 2^31)"),
]


def test_q_loss_refusal_ladder():
    s = dict(cfg=None, q_ptrs=None, next_target=None, next_online=None, act=None, utter=None, td=None, weights=None, dq_ptrs=None,
             q_taken=None, y=None, td_abs=None, work=None, stats=None, loss=None, q=[PTR, None], dq=[PTR, PTR], A=17, dim_c=17, mix=2,
             movable=[0] * 16, speaks=[0] * 16, M=-1, ret=None, done=None, discount=None, gamma=float("nan"))

    def call(s):
        cfg = td = None
        if s["cfg"]:
            cfg = _abi.MpeQLoss()
            cfg.n_agents, cfg.dim_c, cfg.mix = s["A"], s["dim_c"], s["mix"]
            for i in range(16):
                cfg.movable[i], cfg.speaks[i] = s["movable"][i], s["speaks"][i]
        if s["td"]:
            td = _abi.MpeTdTarget()
            td.ret, td.done, td.discount, td.gamma = s["ret"], s["done"], s["discount"], s["gamma"]
        return _abi.lib().mpe_q_loss(C.byref(cfg) if cfg is not None else None, _arr(s["q_ptrs"], s["q"]), s["next_target"],
                                     s["next_online"], s["act"], s["utter"], C.byref(td) if td is not None else None, s["weights"],
                                     s["M"], _arr(s["dq_ptrs"], s["dq"]), s["q_taken"], s["y"], s["td_abs"], s["work"], s["stats"],
                                     s["loss"], None)
    _climb(Q_LADDER, s, call)
    assert _abi.lib().mpe_sizeof_q_loss() == C.sizeof(_abi.MpeQLoss) == 16 + 32


def test_q_loss_work_refusal_ladder_and_counts():
    L_, fn, name = _abi.lib(), _abi.lib().mpe_q_loss_work, "mpe_q_loss_work"
    for A, M, rc, msg in ((0, -5, -1, "A = 0 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"), (17, -5, -1, "A = 17 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
                          (3, -5, -1, "M = -5"), (3, 715827883, -1, "A * M = 3 * 715827883 (need A * M < 2^31)")):
        assert (fn(A, M), L_.mpe_last_error().decode()) == (rc, "%s: %s" % (name, msg))
    assert [fn(3, M) for M in (0, 1, 256, 257, 6400)] == [0, 18, 18, 36, 18 * 25]
    assert fn(16, 1025) == 6 * 16 * 5


E_ = "mpe_actor_act_explore: "
E_MODE = "mode %d (%s; exploration replaces the choice of a MPE_POLICY_GREEDY set)"
EXPLORE_LADDER = [
    ("pass", -1, E_ + "set is NULL"),
    ("s['set'] = True; s['mode'] = 3", -1, E_ + "mode 3 (MPE_POLICY_GREEDY / SAMPLE / SOFTMAX)"),
    ("s['mode'] = 1", -1, E_ + E_MODE % (1, "MPE_POLICY_SAMPLE")),
    ("s['mode'] = 2", -1, E_ + E_MODE % (2, "MPE_POLICY_SOFTMAX")),
    ("s['mode'] = 0", -1, E_ + "epsilon = -0.1 (need 0 <= epsilon <= 1)"),
    ("s['epsilon'] = 1.5", -1, E_ + "epsilon = 1.5 (need 0 <= epsilon <= 1)"),
    ("s['epsilon'] = float('nan')", -1, E_ + "epsilon = nan (need 0 <= epsilon <= 1)"),
    ("s['epsilon'] = float('inf')", -1, E_ + "epsilon = inf (need 0 <= epsilon <= 1)"),
    ("s['epsilon'] = 0.25", -1, E_ + "B = -1"),
    ("s['B'] = 4", -1, E_ + "set->weights is NULL or not 16-byte aligned"),
    ("s['weights'] = PTR + 4", -1, E_ + "set->weights is NULL or not 16-byte aligned"),
    ("s['weights'] = PTR", -1, E_ + "obs_ptrs is NULL"),
    ("s['obs_ptrs'] = True", -1, E_ + "moves is NULL"),
    ("s['moves'] = PTR", -1, E_ + "logits is not 16-byte aligned"),
    ("s['logits'] = PTR + 64", -1, E_ + "obs_ptrs[0] is NULL"),
    ("s['obs'] = [PTR]; s['B'] = 0", 0, E_ + "obs_ptrs[0] is NULL"),
]


def test_actor_act_explore_refusal_ladder():
    """a set that is not GREEDY is refused by its mode's name; epsilon = -0.1, 1.5, NaN and inf by theirs; the NULLs"""
    s = dict(set=False, mode=0, epsilon=-0.1, B=-1, weights=None, obs_ptrs=False, obs=[None], moves=None, logits=PTR + 4)

    def call(s):
        aset = None
        if s["set"]:
            aset = _abi.MpeActorSet()
            aset.n_agents, aset.mode, aset.weights, aset.dim_c = 1, s["mode"], s["weights"], 0
            aset.n_layers[0], aset.width[0][0], aset.width[0][1], aset.movable[0] = 1, 4, 5, 1
        return _abi.lib().mpe_actor_act_explore(C.byref(aset) if aset is not None else None, _arr(s["obs_ptrs"], s["obs"]), s["B"], 0, 0,
                                                s["epsilon"], s["moves"], None, None, None, s["logits"], None)
    _climb(EXPLORE_LADDER, s, call)
    assert _abi.MPE_ABI_VERSION == _abi.lib().mpe_abi_version()


# ---- the host layer's argument checks -----------------------------------------------------------------------------------------------
def _batch(A, M, dim_c, nstep=False):
    b = (NStepReplayBatch if nstep else ReplayBatch)()
    b.act, b.utter = torch.zeros((A, M, 5)), torch.zeros((A, M, dim_c)) if dim_c else None
    b.rew, b._done_u8 = torch.zeros((A, M)), torch.zeros((A, M), dtype=torch.uint8)
    if nstep:
        b.ret, b.discount = torch.zeros((A, M)), torch.zeros(M)
    return b


def test_host_layer_checks_name_the_argument():
    assert set(("QLoss", "QLossResult", "QTargets", "q_loss_tensors")) <= set(mpe.__all__)
    z = torch.zeros
    lay = RowsLayout(22, 3, [14, 17], [False, True], [True, False])      # speaker_listener: n = [3, 5]
    who = "q_loss_tensors: "
    good = dict(layout=lay, q_n=[z((4, 3)), z((4, 5))], batch=_batch(2, 4, 3), next_target=z((2, 4, 16)), gamma=0.95)
    bad_done = _batch(2, 4, 3)
    bad_done._done_u8 = z((2, 5), dtype=torch.uint8)
    bad_act = _batch(2, 4, 3)
    bad_act.act = z((2, 4, 4))
    bad_utter = _batch(2, 4, 3)
    bad_utter.utter = None
    for match, kw in ((who + "layout is an Actors or a RowsLayout", dict(layout=None)),
                      (who + "mix is one of", dict(mix="qmix")),
                      (who + "q_n is a list of 2 tensors", dict(q_n=[z((4, 3))])),
                      (who + r"q_n\[0\] is a contiguous float32 \[M, 3\] tensor", dict(q_n=[z(4), z((4, 5))])),
                      (who + r"q_n\[1\] is a contiguous float32 \[4, 5\] tensor", dict(q_n=[z((4, 3)), z((4, 6))])),
                      (who + "batch is a ReplayBatch", dict(batch=object())),
                      (who + "gamma is required for a one-step batch", dict(gamma=None)),
                      (who + "gamma = nan is not finite", dict(gamma=float("nan"))),
                      (who + "an n-step batch carries its own discount", dict(batch=_batch(2, 4, 3, nstep=True))),
                      (who + r"batch.done is a contiguous \[2, 4\] tensor", dict(batch=bad_done)),
                      (who + r"batch.act is a contiguous float32 \[2, 4, 5\] tensor", dict(batch=bad_act)),
                      (who + r"batch.utter is a contiguous float32 \[2, 4, 3\] tensor", dict(batch=bad_utter)),
                      (who + r"next_target is a contiguous float32 \[2, 4, 16\] tensor", dict(next_target=z((2, 4, 8)))),
                      (who + r"next_online is a contiguous float32 \[2, 4, 16\] tensor", dict(next_online=z((2, 4, 16)).double())),
                      (who + r"weights is a contiguous float32 \[4\] tensor", dict(weights=z(5))),
                      (who + "out is a QLossResult of the same heads, mix and M = 4", dict(out=object())),
                      (who + r"q_n\[0\] is on cpu \(the tensors live on a GPU: there is no CPU path\)", dict())):
        a = dict(good)
        a.update(kw)
        with pytest.raises(_abi.MpeError, match=match):
            q_loss_tensors(**a)
    with pytest.raises(_abi.MpeError, match="QLoss: layout is an Actors or a RowsLayout"):
        QLoss(object())
    with pytest.raises(_abi.MpeError, match="QLoss: mix is one of"):
        QLoss(lay, mix="sum")
    head = QLoss(lay, mix="vdn", double=True)
    with pytest.raises(_abi.MpeError, match="QLoss: q_n is a list of 2 tensors"):
        head([z((4, 3))], good["batch"], good["next_target"])
    with pytest.raises(_abi.MpeError, match=r"QLoss: q_n\[1\] is not a tensor"):
        head([z((4, 3)), None], good["batch"], good["next_target"])
    with pytest.raises(_abi.MpeError, match="QLoss: double=True needs next_online"):
        head(good["q_n"], good["batch"], good["next_target"], gamma=0.95)
    with pytest.raises(_abi.MpeError, match="QLoss: double=False takes the target net's own maximum"):
        QLoss(lay, double=False)(good["q_n"], good["batch"], good["next_target"], z((2, 4, 16)), gamma=0.95)
    with pytest.raises(_abi.MpeError, match="QLoss: next_target requires grad"):
        head(good["q_n"], good["batch"], z((2, 4, 16), requires_grad=True), z((2, 4, 16)), gamma=0.95)
    with pytest.raises(_abi.MpeError, match=r"q_loss_tensors: q_n\[0\] is on cpu"):
        head([z((4, 3), requires_grad=True), z((4, 5))], good["batch"], good["next_target"], z((2, 4, 16)), gamma=0.95)
    with pytest.raises(_abi.MpeError, match="QTargets: target_actors is an Actors"):
        QTargets(object())


def test_actors_epsilon_checks():
    """Actors' own checks of epsilon, on an env without a device (the constructor reads only the world's agents)"""
    from multiagent_particle_envs_amd.policy import Actors
    pi = Actors.__new__(Actors)
    pi.mode = "greedy"
    for eps in (-0.1, 1.5, float("nan"), "x", None):
        pi.epsilon = eps
        with pytest.raises(_abi.MpeError, match=r"Actors.act: epsilon = .* \(a number in \[0, 1\]\)"):
            pi._epsilon("Actors.act")
    pi.epsilon = 0.25
    assert pi._epsilon("Actors.act") == 0.25
    for mode in ("sample", "softmax"):
        pi.mode = mode
        with pytest.raises(_abi.MpeError, match="Actors: epsilon = 0.25 with mode '%s'" % mode):
            pi._epsilon("Actors")
        pi.epsilon = 0.0
        assert pi._epsilon("Actors") == 0.0
        pi.epsilon = 0.25


# ---- the host walk ------------------------------------------------------------------------------------------------------------------
WALK_FLAGS = ["-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path_factory.mktemp("q_loss_walk") / "q_loss_host_walk")
    cmd = [cxx, "-std=c++17"] + WALK_FLAGS + ["-I", os.path.join(ROOT, "multiagent_particle_envs_amd", "csrc"),
                                              os.path.join(ROOT, "tests", "c", "q_loss_host_walk.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("name", CASE_IDS)
@pytest.mark.parametrize("M", R.ROWS)
def test_host_walk_every_block_wave_and_lane_under_the_sanitizers(M, name, nan, host_walk, tmp_path):
    """Both launches of all eight passes on exact-size heap buffers at both alignments (the walk itself asserts that both write the
    same bytes and that every output float is stored exactly once): bit-equal to restatement (b) in every output"""
    case = R.CASES[name]
    x = R.make_inputs(case, M, nan=nan)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    R.write_walk_input(src, case, M, x)
    r = subprocess.run([host_walk, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (name, M, r.stdout[-500:], r.stderr[-4000:])
    assert "%d chunks" % ((M + 255) // 256) in r.stdout and "stored once, both alignments equal" in r.stdout
    for (mix, double, weighted, nstep), got in zip(R.VARIANTS, R.read_walk_output(dst, case, M)):
        want = R.q_loss32(case, x, mix, double, weighted, nstep)
        tag = (name, M, mix, double, weighted)
        for i in range(case.A):
            assert R.same_bits(got["dq_n"][i], want["dq_n"][i]), tag + ("dq", i)
        for k in ("q_taken", "y", "td_abs", "stats"):
            assert R.same_bits(got[k], want[k]), tag + (k,)
        assert R.same_bits(got["loss"], want["loss"]), tag + ("loss",)
        if nan:      # the NaN reaches td_abs and the loss and no other row's gradient
            m = M // 2
            assert np.isnan(got["td_abs"][m]) and np.isnan(got["loss"]) and int(np.isnan(got["td_abs"]).sum()) == 1
            for i in range(case.A):
                assert not np.isnan(np.delete(got["dq_n"][i], m, axis=0)).any()
