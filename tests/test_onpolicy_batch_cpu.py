"""On-policy minibatches without a GPU: the C++ permutation against the NumPy restatement, the restatement's uniformity, the
statistics rule against float64 NumPy, every refusal of the three entry points, the host layer's argument checks, and the host walk
of every index of both kernels under the sanitizers (tests/c/onpolicy_host_walk.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.onpolicy import GaeResult, Minibatches, adv_stats, perm

import _onpolicy_batch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x10000      # a plausible, 16-byte aligned address (no refused call reads it)


# ---- the permutation --------------------------------------------------------------------------------------------------------------
PERM_N = [1, 2, 3, 5, 7, 12, 64, 65, 84, 257, 1625, 25600]
PERM_EPOCHS = [0, 1, 2 ** 32 + 5]
PERM_SEEDS = [77, R.SEED]


@pytest.mark.parametrize("N", PERM_N)
def test_perm_is_the_restatement_and_a_bijection(N):
    fn = _abi.lib().mpe_onpolicy_perm
    for seed in PERM_SEEDS:
        for epoch in PERM_EPOCHS:
            want = R.perm(N, seed, epoch)
            got = np.array([fn(N, seed, epoch, q) for q in range(N)], np.int64)
            assert np.array_equal(got, want.astype(np.int64)), (N, seed, epoch)
            assert np.array_equal(np.sort(got), np.arange(N)), (N, seed, epoch)
    assert perm(N, PERM_SEEDS[1], 1, N - 1) == int(R.perm(N, PERM_SEEDS[1], 1)[N - 1])


def test_perm_depends_on_seed_and_epoch_and_refuses_by_name():
    a, b, c = R.perm(1625, 77, 0), R.perm(1625, 77, 1), R.perm(1625, 78, 0)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    assert not np.array_equal(R.perm(1625, 77, 5), R.perm(1625, 77, 2 ** 32 + 5))      # the epoch's high word is keyed
    assert not np.array_equal(R.perm(1625, 77, 0), R.perm(1625, 77 + 2 ** 32, 0))      # and the seed's
    L_ = _abi.lib()
    for args, msg in (((0, 0, 0, 0), "mpe_onpolicy_perm: N = 0 (1..2^40)"),
                      (((1 << 40) + 1, 0, 0, 0), "mpe_onpolicy_perm: N = 1099511627777 (1..2^40)"),
                      ((5, 0, 0, 5), "mpe_onpolicy_perm: q = 5 (need 0 <= q < N = 5)"),
                      ((5, 0, 0, -1), "mpe_onpolicy_perm: q = -1 (need 0 <= q < N = 5)")):
        assert L_.mpe_onpolicy_perm(*args) == -1 and L_.mpe_last_error().decode() == msg
    with pytest.raises(_abi.MpeError, match="mpe_onpolicy_perm: q = 9"):
        perm(5, 0, 0, 9)
    assert L_.mpe_onpolicy_perm(1 << 40, 3, 4, (1 << 40) - 1) >= 0      # the largest N walks and ends


def test_perm_uniformity_of_the_restatement():
    """N = 1625, seed 77, epochs 0..1999: counts of (source bucket q / 125, destination bucket perm(q) / 125) in a 13 x 13 table
    against the flat table; the bound 205 is about the 0.999 quantile of chi^2 with 144 degrees of freedom (the seed is fixed: a
    condition, not a coin toss)."""
    N, n_ep = 1625, 2000
    table = np.zeros((13, 13), np.int64)
    src = np.arange(N) // 125
    for e in range(n_ep):
        np.add.at(table, (src, (R.perm(N, 77, e) // np.uint64(125)).astype(np.int64)), 1)
    expect = N * n_ep / 169.0
    chi2 = float(((table - expect) ** 2 / expect).sum())
    print("chi^2 = %.1f (144 degrees of freedom)" % chi2)
    assert chi2 < 205.0


# ---- the statistics ---------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


@pytest.mark.parametrize("N", [1, 2, 255, 256, 4096, 4097, 4098, 12289])
def test_statistics_rule_against_float64_numpy(N):
    rs = np.random.RandomState(N)
    x = (0.3 + 2.0 * rs.standard_normal(N)).astype(np.float32)
    st = R.adv_stats(x.reshape(N, 1, 1))
    assert st.shape == (1, 2) and st.dtype == np.float32
    x64 = x.astype(np.float64)
    assert _ulps(st[0, 0], np.float32(np.mean(x64))) <= 1
    if N == 1:
        assert st[0, 1] == np.float32(1.0) / np.float32(R.EPS)
    else:
        want = np.float32(1.0) / (np.float32(np.std(x64, ddof=1)) + np.float32(R.EPS))
        assert _ulps(st[0, 1], want) <= 1, (st[0, 1], want)
    same = np.full(N, x[0], np.float32)
    mean, var = R.moments(same)
    assert var == 0.0 and np.float32(mean) == x[0]
    assert R.adv_stats(same.reshape(N, 1, 1))[0, 1] == np.float32(1.0) / np.float32(R.EPS)


def test_statistics_elements_run_over_steps_then_worlds():
    T, A, B = 3, 2, 1366
    adv = R.make_traj((T, A, B, [1, 1], 0, 1))["adv"]
    st = R.adv_stats(adv)
    for i in range(A):
        assert R.same_bits(st[i], R.adv_stats(adv[:, i:i + 1, :])[0])
    assert not R.same_bits(st[0], st[1])


# ---- refusals: one ladder per entry point, the order include/mpe_hip.h states ----------------------------------------------------
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


SIZE = " (need A * B < 2^31, T < 2^31 and T * A * B <= 2^40)"
STATS_LADDER = [
    ("pass", -1, "mpe_adv_stats: T = 0 steps (need at least 1)"),
    ("s['T'] = 25", -1, "mpe_adv_stats: A = 17 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
    ("s['A'] = 0", -1, "mpe_adv_stats: A = 0 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
    ("s['A'] = 3", -1, "mpe_adv_stats: B = -1"),
    ("s['B'] = 1 << 30", -1, "mpe_adv_stats: adv is NULL"),
    ("s['adv'] = PTR + 2", -1, "mpe_adv_stats: work is NULL"),
    ("s['work'] = PTR + 4", -1, "mpe_adv_stats: stats is NULL"),
    ("s['stats'] = PTR", -1, "mpe_adv_stats: adv and stats must be 4-byte and work 8-byte aligned"),
    ("s['adv'] = PTR", -1, "mpe_adv_stats: adv and stats must be 4-byte and work 8-byte aligned"),
    ("s['work'] = PTR; s['stats'] = PTR + 1", -1, "mpe_adv_stats: adv and stats must be 4-byte and work 8-byte aligned"),
    ("s['stats'] = PTR", -1, "mpe_adv_stats: T * A * B = 25 * 3 * 1073741824" + SIZE),
    ("s['B'] = 1 << 28; s['T'] = 1 << 12", -1, "mpe_adv_stats: T * A * B = 4096 * 3 * 268435456" + SIZE),
    ("s['B'] = 1; s['A'] = 1; s['T'] = 1 << 31", -1, "mpe_adv_stats: T * A * B = 2147483648 * 1 * 1" + SIZE),
    ("s['T'] = 25; s['A'] = 3; s['B'] = 7", -1, "mpe_adv_stats: eps = nan (need a finite value >= 0)"),
    ("s['eps'] = float('inf')", -1, "mpe_adv_stats: eps = inf (need a finite value >= 0)"),
    ("s['eps'] = -1.0", -1, "mpe_adv_stats: eps = -1 (need a finite value >= 0)"),
    ("s['eps'] = 0.0; s['B'] = 0", 0, "mpe_adv_stats: eps = -1 (need a finite value >= 0)"),
]


def test_adv_stats_refusal_ladder():
    s = dict(T=0, A=17, B=-1, adv=None, work=None, stats=None, eps=float("nan"))
    _climb(STATS_LADDER, s, lambda s: _abi.lib().mpe_adv_stats(s["T"], s["A"], s["B"], s["adv"], s["eps"], s["work"], s["stats"], None))


def test_adv_stats_work_counts_and_refuses():
    L_ = _abi.lib()
    assert L_.mpe_adv_stats_work(25, 3, 65) == 2 * 3 * 1 and L_.mpe_adv_stats_work(3, 2, 1366) == 2 * 2 * 2
    assert L_.mpe_adv_stats_work(1, 16, 4096) == 2 * 16 and L_.mpe_adv_stats_work(1, 1, 4097) == 4 and L_.mpe_adv_stats_work(5, 2, 0) == 0
    for args, msg in (((0, 3, 7), "mpe_adv_stats_work: T = 0 steps (need at least 1)"),
                      ((1, 0, 7), "mpe_adv_stats_work: A = 0 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
                      ((1, 3, -2), "mpe_adv_stats_work: B = -2"),
                      ((1, 3, 1 << 30), "mpe_adv_stats_work: T * A * B = 1 * 3 * 1073741824" + SIZE)):
        assert L_.mpe_adv_stats_work(*args) == -1 and L_.mpe_last_error().decode() == msg


B_ = "mpe_onpolicy_batch: "
ALIGN = B_ + "every float tensor must be 4-byte, idx and epoch_add 8-byte aligned"
TRAJ_PTRS = ("obs_in", "act", "adv", "ret", "val")
OUT_PTRS = ("idx", "obs", "act", "adv", "ret", "val")
BATCH_LADDER = [
    ("pass", -1, B_ + "traj is NULL"),
    ("s['traj'] = True", -1, B_ + "T = 0 steps (need at least 1)"),
    ("s['T'] = 25", -1, B_ + "A = 17 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
    ("s['A'] = 3", -1, B_ + "B = -1"),
    ("s['B'] = 1 << 30", -1, B_ + "obs_width[0] = 0 (1..MPE_REPLAY_MAX_WIDTH = 4096)"),
    ("s['w'] = [18, 4097, 18]", -1, B_ + "obs_width[1] = 4097 (1..MPE_REPLAY_MAX_WIDTH = 4096)"),
    ("s['w'] = [18, 4096, 1]", -1, B_ + "dim_c = -1 (0..MPE_REPLAY_MAX_WIDTH = 4096)"),
    ("s['dim_c'] = 4", -1, B_ + "M = -1"),
    ("s['M'] = 5", -1, B_ + "first = -1, M = 5 (need 0 <= first and first + M <= T * B = 26843545600)"),
    ("s['first'] = 26843545596", -1, B_ + "first = 26843545596, M = 5 (need 0 <= first and first + M <= T * B = 26843545600)"),
    ("s['first'] = 26843545595", -1, B_ + "traj->obs_in is NULL"),
] + [("s['t_%s'] = PTR" % a, -1, B_ + "traj->%s is NULL" % b) for a, b in zip(TRAJ_PTRS, TRAJ_PTRS[1:])] + [
    ("s['t_val'] = PTR", -1, B_ + "idx is NULL"),
] + [("s['%s'] = PTR" % a, -1, B_ + "%s is NULL" % b) for a, b in zip(OUT_PTRS, OUT_PTRS[1:])] + [
    ("s['val'] = PTR", -1, B_ + "traj->utter is NULL and dim_c = 4"),
    ("s['t_utter'] = PTR", -1, B_ + "utter is NULL and dim_c = 4"),
    ("s['utter'] = PTR; s['t_logp'] = PTR", -1, B_ + "traj->logp is given and logp is NULL (both, or neither)"),
    ("s['t_logp'] = None; s['logp'] = PTR", -1, B_ + "logp is given and traj->logp is NULL (both, or neither)"),
    ("s['t_logp'] = PTR + 2", -1, ALIGN),
    ("s['t_logp'] = PTR; s['joint'] = PTR + 1", -1, ALIGN),
    ("s['joint'] = PTR; s['stats'] = PTR + 3", -1, ALIGN),
    ("s['stats'] = PTR; s['idx'] = PTR + 4", -1, ALIGN),
    ("s['idx'] = PTR; s['epoch_add'] = PTR + 4", -1, ALIGN),
    ("s['epoch_add'] = PTR", -1, B_ + "T * A * B = 25 * 3 * 1073741824" + SIZE),
    ("s['B'] = 1 << 28; s['T'] = 1 << 12; s['first'] = 0", -1, B_ + "T * A * B = 4096 * 3 * 268435456" + SIZE),
    ("s['T'] = 25; s['B'] = 7; s['M'] = 0; s['first'] = 175", 0, B_ + "T * A * B = 4096 * 3 * 268435456" + SIZE),
    ("s['first'] = 0; s['M'] = 1", -1, B_ + "first = 0, M = 1 (need 0 <= first and first + M <= T * B = 0)"),
    ("s['M'] = 0", 0, B_ + "first = 0, M = 1 (need 0 <= first and first + M <= T * B = 0)"),
]
# (the rung in front of the last two sets B = 0: a trajectory without worlds holds no pair, and only M = 0 is let through)
BATCH_LADDER[-2] = ("s['B'] = 0; " + BATCH_LADDER[-2][0],) + BATCH_LADDER[-2][1:]


def _batch_call(s):
    tr = None
    if s["traj"]:
        tr = _abi.MpeOnPolicyTraj()
        tr.T, tr.A, tr.B, tr.dim_c = s["T"], s["A"], s["B"], s["dim_c"]
        for i, d in enumerate(s["w"]):
            tr.obs_width[i] = d
        for k in TRAJ_PTRS + ("utter", "logp"):
            setattr(tr, k, s["t_" + k])
    return _abi.lib().mpe_onpolicy_batch(C.byref(tr) if tr is not None else None, s["M"], s["first"], 1, 2, s["epoch_add"], s["stats"], s["idx"],
                                         s["obs"], s["act"], s["utter"], s["logp"], s["adv"], s["ret"], s["val"], s["joint"], None)


def test_onpolicy_batch_refusal_ladder():
    s = dict(traj=False, T=0, A=17, B=-1, w=[0] * 16, dim_c=-1, M=-1, first=-1, epoch_add=None, stats=None, joint=None, utter=None, logp=None,
             t_utter=None, t_logp=None)
    s.update({"t_" + k: None for k in TRAJ_PTRS})
    s.update({k: None for k in OUT_PTRS})
    _climb(BATCH_LADDER, s, _batch_call)
    assert _abi.lib().mpe_sizeof_onpolicy_traj() == C.sizeof(_abi.MpeOnPolicyTraj) == 144


# ---- the host layer's argument checks ---------------------------------------------------------------------------------------------
class _Traj(object):
    pass


def _cpu_traj(T=4, A=2, B=3, widths=(5, 2), dim_c=0, logp=True):
    tr = _Traj()
    tr.obs_in_flat = torch.zeros((T, sum(widths) * B))
    off = np.concatenate([[0], np.cumsum(widths)])
    tr.obs_in = [[tr.obs_in_flat[t, off[i] * B:off[i + 1] * B].view(B, widths[i]) for i in range(A)] for t in range(T)]
    tr.act, tr.val = torch.zeros((T, A, B, 5)), torch.zeros((T, A, B))
    tr.utter = torch.zeros((T, A, B, dim_c)) if dim_c else None
    tr.logp = torch.zeros((T, A, B)) if logp else None
    return tr, GaeResult(torch.zeros((T, A, B)), torch.zeros((T, A, B)))


def test_host_layer_checks_name_the_tensor():
    assert set(("adv_stats", "Minibatches", "OnPolicyBatch")) <= set(mpe.__all__)
    tr, g = _cpu_traj()
    with pytest.raises(_abi.MpeError, match="Minibatches: g is a GaeResult"):
        Minibatches(tr, (g.adv, g.ret), 4)
    with pytest.raises(_abi.MpeError, match="Minibatches: traj holds no decision observations"):
        Minibatches(object(), g, 4)
    with pytest.raises(_abi.MpeError, match="Minibatches: g.adv is a contiguous float32 .T, A, B. tensor"):
        Minibatches(tr, GaeResult(g.adv.double(), g.ret), 4)
    with pytest.raises(_abi.MpeError, match=r"Minibatches: g.ret is a contiguous float32 \[4, 2, 3\] tensor"):
        Minibatches(tr, GaeResult(g.adv, g.ret[:3]), 4)
    for name, bad in (("val", torch.zeros((4, 2, 4))), ("act", torch.zeros((4, 2, 3, 4))), ("logp", torch.zeros((4, 2, 3)).double()),
                      ("obs_in_flat", torch.zeros((4, 22)))):
        tr2, _ = _cpu_traj()
        setattr(tr2, name, bad)
        with pytest.raises(_abi.MpeError, match="Minibatches: traj.%s is a contiguous float32" % name):
            Minibatches(tr2, g, 4)
    tr3, _ = _cpu_traj(dim_c=4)
    tr3.utter = torch.zeros((4, 2, 2, 4))
    with pytest.raises(_abi.MpeError, match=r"Minibatches: traj.utter is a contiguous float32 \[4, 2, 3, 4\] tensor"):
        Minibatches(tr3, g, 4)
    with pytest.raises(_abi.MpeError, match="Minibatches: M = 0 rows"):
        Minibatches(tr, g, 0)
    with pytest.raises(_abi.MpeError, match="Minibatches: epoch_counter is a uint64"):
        Minibatches(tr, g, 4, epoch_counter=torch.zeros(1))
    with pytest.raises(_abi.MpeError, match="Minibatches: g.adv is on cpu"):      # every shape is right: the device is not
        Minibatches(tr, g, 4)
    with pytest.raises(_abi.MpeError, match="adv_stats: adv is a contiguous float32 .T, A, B. tensor"):
        adv_stats(g.adv[0])
    with pytest.raises(_abi.MpeError, match="adv_stats: adv is a contiguous float32"):
        adv_stats(GaeResult(g.adv.double(), g.ret))
    with pytest.raises(_abi.MpeError, match=r"adv_stats: eps = -1"):
        adv_stats(g, eps=-1)
    with pytest.raises(_abi.MpeError, match=r"adv_stats: out is a contiguous float32 \[2, 2\] tensor"):
        adv_stats(g, out=torch.zeros((3, 2)))
    with pytest.raises(_abi.MpeError, match="adv_stats: adv is on cpu"):
        adv_stats(g)


# ---- the host walk ----------------------------------------------------------------------------------------------------------------
WALK_FLAGS = ["-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path_factory.mktemp("onpolicy_walk") / "onpolicy_host_walk")
    cmd = [cxx, "-std=c++17"] + WALK_FLAGS + ["-I", os.path.join(ROOT, "multiagent_particle_envs_amd", "csrc"),
                                              os.path.join(ROOT, "tests", "c", "onpolicy_host_walk.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.SHAPE_IDS)
def test_host_walk_every_block_job_and_lane_under_the_sanitizers(shape, host_walk, tmp_path):
    T, A, B, widths, dim_c, M = shape
    tr = R.make_traj(shape)
    stats = R.adv_stats(tr["adv"])
    epoch = 3
    keys = R.round_keys(R.SEED, epoch)
    order = R.perm(T * B, R.SEED, epoch).astype(np.int64)
    for want_logp, want_stats, want_joint in ((True, True, True), (False, False, False)):
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        R.write_walk_input(src, tr, shape, keys, want_logp, want_stats, want_joint)
        r = subprocess.run([host_walk, src, dst], capture_output=True, text=True)
        assert r.returncode == 0, (shape, r.stdout[-500:], r.stderr[-4000:])
        got_stats, outs = R.read_walk_output(dst, shape, want_logp, want_joint)
        assert R.same_bits(got_stats, stats), (got_stats, stats)
        parts = R.minibatches(T * B, M)
        assert "%d minibatches" % len(parts) in r.stdout and "%d statistics chunks" % ((T * B + 4095) // 4096) in r.stdout
        for (first, m), got in zip(parts, outs):
            want = R.batch(tr, shape, order[first:first + m], stats if want_stats else None)
            if not want_logp:
                want["logp"] = None
            if not want_joint:
                want["joint"] = None
            assert R.first_difference(got, want) is None, (shape, first, R.first_difference(got, want))
        assert np.array_equal(np.sort(np.concatenate([o["idx"] for o in outs])), np.arange(T * B))
