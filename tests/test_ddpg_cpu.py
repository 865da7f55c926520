"""The off-policy update's device pieces without a GPU: the float64 restatements of THE TD LOSS RULE, THE POLICY ROWS RULE and THE
POLICY ROWS GRADIENT RULE against torch float64 autograd of the MADDPG example's own formulas, every refusal of the entry points in
the header's order, the host layer's argument checks, PolyakTargets' refusals, and the host walk of every block, wave and lane of
all launches under the sanitizers (tests/c/ddpg_host_walk.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.learner import (ActorLoss, RowsLayout, TdLoss, policy_rows_grad_tensors, policy_rows_tensors,
                                                  td_loss_tensors)
from multiagent_particle_envs_amd.optim import PolyakTargets

import _ddpg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x10000      # a plausible, 16-byte aligned address (no refused call reads it)
LAYOUT_IDS = sorted(R.LAYOUTS)


# ---- (a) against torch float64 autograd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("M", [1, 65, 257])
def test_td_restatement_is_torch_float64_autograd(M, weighted):
    """weighted MSE per agent, summed: loss, means, dq and |td| within 1e-12 of each output's largest magnitude"""
    x = R.make_inputs(R.LAYOUTS["L69"], M)
    ref, t64 = R.td_loss64(x["q"], x["y"], x["w"] if weighted else None), R.torch_td(x, weighted, torch.float64)
    for name in ("dq", "td_abs", "stats"):
        assert np.abs(ref[name] - t64[name]).max() <= 1e-12 * np.abs(ref[name]).max(), name
    assert abs(ref["loss"] - t64["loss"]) <= 1e-12 * abs(ref["loss"])
    b32 = R.td_loss32(x["q"], x["y"], x["w"] if weighted else None)      # (b) is (a) to float32 rounding
    assert np.abs(b32["dq"] - ref["dq"]).max() <= 4 * np.spacing(np.float32(np.abs(ref["dq"]).max()))
    assert np.array_equal(b32["td_abs"], np.abs(x["q"] - x["y"]).max(axis=0))


@pytest.mark.parametrize("reg_coef", [0.0, 1e-3])
@pytest.mark.parametrize("name", LAYOUT_IDS)
def test_rows_restatements_are_torch_float64_autograd(name, reg_coef):
    """softmax into the window under an upstream gradient, and the regulariser: rows, dlogits, stats and loss"""
    lay, M = R.LAYOUTS[name], 65
    x = R.make_inputs(lay, M)
    R.check_logits(lay, x)
    t64 = R.torch_rows(lay, x, reg_coef, torch.float64, q=x["q"])
    rows, ref = R.rows64(lay, x), R.rows_grad64(lay, x, reg_coef, q=x["q"])
    for i in range(lay.A):
        ok = ~np.isnan(rows[i])
        assert np.array_equal(ok, ~np.isnan(t64["rows"][i])) and (~ok).sum() == 1
        assert np.abs(rows[i][ok] - t64["rows"][i][ok]).max() <= 1e-12 * np.abs(rows[i][ok]).max()
        assert np.abs(ref["dlogits"][i] - t64["dlogits"][i]).max() <= 1e-12 * np.abs(ref["dlogits"][i]).max()
    assert np.abs(ref["stats"] - t64["stats"]).max() <= 1e-12 * np.abs(ref["stats"]).max()
    assert abs(ref["loss"] - t64["loss"]) <= 1e-12 * abs(ref["loss"])


def test_polyak_restatement_is_torch_lerp():
    """torch.lerp's branch form: torch's CPU kernel may contract t * d into a fused multiply-add, the rule rounds every operation,
    so the two agree to one ulp of the larger operand, and exactly at tau = 0 and 1 and on padding."""
    rs = np.random.RandomState(5)
    x, w = rs.standard_normal(4096).astype(np.float32), rs.standard_normal(4096).astype(np.float32)
    x[:16], w[:16] = 0.0, 0.0      # padding stays +0.0
    for tau in R.POLYAK_TAU + [0.25, 0.75]:
        got = R.polyak32(x, w, tau)
        want = torch.lerp(torch.from_numpy(x), torch.from_numpy(w), float(np.float32(tau))).numpy()
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.maximum(np.abs(x), np.abs(w)))), tau
        if tau in (0.0, 1.0):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), tau
        assert not got[:16].view(np.uint32).any()
    assert np.array_equal(R.polyak32(x, w, 1.0).view(np.uint32), w.view(np.uint32))
    assert np.array_equal(R.polyak32(x, w, 0.0).view(np.uint32), x.view(np.uint32))


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


T_ = "mpe_td_loss: "
T_ALIGN = T_ + "every float tensor must be 4-byte and work 8-byte aligned"
T_TOP = ("q_ptrs", "y", "dq", "work", "stats", "loss")
TD_LADDER = [("pass", -1, T_ + "q_ptrs is NULL")] + [("s['%s'] = PTR" % a, -1, T_ + "%s is NULL" % b) for a, b in zip(T_TOP, T_TOP[1:])] + [
    ("s['loss'] = PTR", -1, T_ + "A = 17 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
    ("s['A'] = 0", -1, T_ + "A = 0 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
    ("s['A'] = 2", -1, T_ + "M = -1"),
    ("s['M'] = 1 << 30", -1, T_ + "q_ptrs[1] is NULL"),
    ("s['q'] = [PTR, PTR + 2]", -1, T_ALIGN),
    ("s['q'] = [PTR, PTR + 4]; s['w'] = PTR + 1", -1, T_ALIGN),
    ("s['w'] = PTR; s['td_abs'] = PTR + 2", -1, T_ALIGN),
    ("s['td_abs'] = PTR + 4; s['work'] = PTR + 4", -1, T_ALIGN),
    ("s['work'] = PTR + 8", -1, T_ + "A * M = 2 * 1073741824 (need A * M < 2^31)"),
    ("s['M'] = 0", 0, T_ + "A * M = 2 * 1073741824 (need A * M < 2^31)"),
]


def test_td_loss_refusal_ladder():
    s = dict(q_ptrs=None, q=[PTR, None], y=None, w=None, dq=None, td_abs=None, work=None, stats=None, loss=None, A=17, M=-1)
    _climb(TD_LADDER, s, lambda s: _abi.lib().mpe_td_loss(s["A"], _arr(s["q_ptrs"], s["q"]), s["y"], s["w"], s["M"], s["dq"], s["td_abs"],
                                                          s["work"], s["stats"], s["loss"], None))


@pytest.mark.parametrize("name", ["mpe_td_loss_work", "mpe_policy_rows_grad_work"])
def test_work_refusal_ladders_and_counts(name):
    L_, fn = _abi.lib(), getattr(_abi.lib(), name)
    for A, M, rc, msg in ((0, -5, -1, "A = 0 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"), (17, -5, -1, "A = 17 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
                          (3, -5, -1, "M = -5"), (3, 715827883, -1, "A * M = 3 * 715827883 (need A * M < 2^31)")):
        assert (fn(A, M), L_.mpe_last_error().decode()) == (rc, "%s: %s" % (name, msg))
    assert [fn(3, M) for M in (0, 1, 256, 257, 6400)] == [0, 18, 18, 36, 18 * 25]
    assert fn(16, 1025) == 6 * 16 * 5


def _rows_cfg(s):
    if not s["cfg"]:
        return None
    cfg = _abi.MpePolicyRows()
    cfg.n_agents, cfg.W, cfg.dim_c, cfg.reg_coef = s["A"], s["W"], s["dim_c"], s["reg_coef"]
    for i in range(16):
        cfg.movable[i], cfg.speaks[i], cfg.col[i], cfg.ld[i] = s["movable"][i], s["speaks"][i], s["col"][i], s["ld"][i]
    return cfg


def _layout_rungs(P_):
    """the checks mpe_policy_rows and mpe_policy_rows_grad share: A, dim_c, the heads, the windows, W, M"""
    return [
        ("s['A'] = 0", -1, P_ + "A = 0 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
        ("s['A'] = 2", -1, P_ + "dim_c = 17 (0..16)"),
        ("s['dim_c'] = -1", -1, P_ + "dim_c = -1 (0..16)"),
        ("s['dim_c'] = 0", -1, P_ + "agent 0 has no head (neither movable nor speaking with dim_c > 0)"),
        ("s['movable'][:2] = [1, 1]; s['speaks'][:2] = [0, 1]; s['dim_c'] = 12", -2,
         P_ + "agent 1: 17 logits (5 * movable + dim_c * speaks) > MPE_ACTOR_MAX_OUT = 16"),
        ("s['dim_c'] = 3", -1, P_ + "agent 0: the window of 5 columns from -1 leaves the row of W = 300"),
        ("s['col'][:2] = [295, 293]", -1, P_ + "agent 1: the window of 8 columns from 293 leaves the row of W = 300"),
        ("s['col'][:2] = [10, 15]", -1, P_ + "W = 300 (1..MPE_ACTOR_MAX_INPUT = 256)"),
        ("s['W'] = 23", -1, P_ + "M = -1"),
    ]


P_ = "mpe_policy_rows: "
R_TOP = ("cfg", "joint", "logits_ptrs", "out_ptrs")
ROWS_LADDER = [("pass", -1, P_ + "cfg is NULL")] + [("s['%s'] = PTR" % a, -1, P_ + "%s is NULL" % b) for a, b in zip(R_TOP, R_TOP[1:])] + [
    ("s['out_ptrs'] = PTR", -1, P_ + "A = 17 agents (1..MPE_ACTOR_MAX_AGENTS = 16)")] + _layout_rungs(P_) + [
    ("s['M'] = 1 << 30", -1, P_ + "logits_ptrs[1] is NULL"),
    ("s['logits'] = [PTR, PTR]; s['out'] = [None, PTR]", -1, P_ + "out_ptrs[0] is NULL"),
    ("s['out'] = [PTR, PTR + 2]", -1, P_ + "every pointer must be 4-byte aligned"),
    ("s['out'] = [PTR, PTR + 4]; s['joint'] = PTR + 1", -1, P_ + "every pointer must be 4-byte aligned"),
    ("s['joint'] = PTR + 4", -1, P_ + "A * M = 2 * 1073741824 (need A * M < 2^31)"),
    ("s['M'] = 0", 0, P_ + "A * M = 2 * 1073741824 (need A * M < 2^31)"),      # (M * W >= 2^40 cannot be reached: W <= 256)
]


def _rows_state():
    return dict(cfg=None, joint=None, logits_ptrs=None, out_ptrs=None, g_ptrs=None, dlogits_ptrs=None, logits=[PTR, None], out=[PTR, PTR],
                g=[PTR, PTR], dlogits=[PTR, PTR], A=17, W=300, dim_c=17, reg_coef=float("nan"), movable=[0] * 16, speaks=[0] * 16,
                col=[-1] * 16, ld=[0] * 16, M=-1, q=None, work=None, stats=None, loss=None)


def test_policy_rows_refusal_ladder():
    def call(s):
        cfg = _rows_cfg(s)
        return _abi.lib().mpe_policy_rows(C.byref(cfg) if cfg is not None else None, s["joint"], _arr(s["logits_ptrs"], s["logits"]), s["M"],
                                          _arr(s["out_ptrs"], s["out"]), None)
    _climb(ROWS_LADDER, _rows_state(), call)
    assert _abi.lib().mpe_sizeof_policy_rows() == C.sizeof(_abi.MpePolicyRows) == 16 + 64 + 32 + 128 + 8


G_ = "mpe_policy_rows_grad: "
G_ALIGN = G_ + "every float tensor must be 4-byte and work 8-byte aligned"
G_TOP = ("cfg", "logits_ptrs", "g_ptrs", "dlogits_ptrs")
GRAD_LADDER = [("pass", -1, G_ + "cfg is NULL")] + [("s['%s'] = PTR" % a, -1, G_ + "%s is NULL" % b) for a, b in zip(G_TOP, G_TOP[1:])] + [
    ("s['dlogits_ptrs'] = PTR; s['stats'] = PTR", -1, G_ + "work, stats and loss are given together or not at all"),
    ("s['work'] = PTR + 4", -1, G_ + "work, stats and loss are given together or not at all"),
    ("s['loss'] = PTR", -1, G_ + "stats is given and q is NULL"),
    ("s['q'] = PTR", -1, G_ + "A = 17 agents (1..MPE_ACTOR_MAX_AGENTS = 16)")] + _layout_rungs(G_) + [
    ("s['M'] = 1 << 30", -1, G_ + "reg_coef = nan (need a finite value >= 0)"),
    ("s['reg_coef'] = float('inf')", -1, G_ + "reg_coef = inf (need a finite value >= 0)"),
    ("s['reg_coef'] = -1e-3", -1, G_ + "reg_coef = -0.001 (need a finite value >= 0)"),
    ("s['reg_coef'] = 1e-3", -1, G_ + "agent 0: ld = 0 (need >= n = 5)"),
    ("s['ld'][:2] = [5, 7]", -1, G_ + "agent 1: ld = 7 (need >= n = 8)"),
    ("s['ld'][:2] = [5, 23]", -1, G_ + "logits_ptrs[1] is NULL"),
    ("s['logits'] = [PTR, PTR]; s['g'] = [None, PTR]", -1, G_ + "g_ptrs[0] is NULL"),
    ("s['g'] = [PTR, PTR]; s['dlogits'] = [PTR, None]", -1, G_ + "dlogits_ptrs[1] is NULL"),
    ("s['dlogits'] = [PTR, PTR + 2]", -1, G_ALIGN),
    ("s['dlogits'] = [PTR, PTR + 4]; s['q'] = PTR + 1", -1, G_ALIGN),
    ("s['q'] = PTR + 4", -1, G_ALIGN),
    ("s['work'] = PTR + 8", -1, G_ + "A * M = 2 * 1073741824 (need A * M < 2^31)"),
    ("s['M'] = 1 << 20; s['ld'][1] = 1 << 20", -1, G_ + "agent 1: M * ld = 1048576 * 1048576 floats (need M * ld < 2^40)"),
    ("s['M'] = 0", 0, G_ + "agent 1: M * ld = 1048576 * 1048576 floats (need M * ld < 2^40)"),
]


def test_policy_rows_grad_refusal_ladder():
    def call(s):
        cfg = _rows_cfg(s)
        return _abi.lib().mpe_policy_rows_grad(C.byref(cfg) if cfg is not None else None, _arr(s["logits_ptrs"], s["logits"]),
                                               _arr(s["g_ptrs"], s["g"]), s["M"], _arr(s["dlogits_ptrs"], s["dlogits"]), s["q"], s["work"],
                                               s["stats"], s["loss"], None)
    _climb(GRAD_LADDER, _rows_state(), call)


K_ = "mpe_polyak: "
POLYAK_LADDER = [
    ("pass", -1, K_ + "cfg is NULL"),
    ("s['cfg'] = True", -1, K_ + "n_sets = 0 (1..MPE_ADAM_MAX_SETS = 8)"),
    ("s['n_sets'] = 9", -1, K_ + "n_sets = 9 (1..MPE_ADAM_MAX_SETS = 8)"),
    ("s['n_sets'] = 2", -1, K_ + "set[0].target is NULL"),
    ("s['target'] = [PTR + 4, None]", -1, K_ + "set[0].online is NULL"),
    ("s['online'] = [PTR + 4096, None]", -1, K_ + "set[0].target is not 16-byte aligned"),
    ("s['target'][0] = PTR", -1, K_ + "set[0].n = 8 floats (a multiple of 16, at least 16)"),
    ("s['n'][0] = 40", -1, K_ + "set[0].n = 40 floats (a multiple of 16, at least 16)"),
    ("s['n'][0] = 1024", -1, K_ + "set[1].target is NULL"),
    ("s['target'][1] = PTR + 8192; s['online'][1] = PTR + 8192 + 8", -1, K_ + "set[1].online is not 16-byte aligned"),
    ("s['online'][1] = PTR + 4096 + 4080; s['n'][1] = 16", -1, K_ + "set[0].online and set[1].online overlap"),
    ("s['online'][1] = PTR + 8192 + 48", -1, K_ + "set[1].target and set[1].online overlap"),
    ("s['online'][1] = PTR + 8192 + 64; s['n'] = [1 << 30, 1 << 30]; s['target'] = [PTR, PTR + (1 << 34)]; "
     "s['online'] = [PTR + (1 << 33), PTR + (3 << 33)]", -1, K_ + "the sets hold 2^31 floats or more (need N < 2^31)"),
    ("s['n'] = [1024, 16]", -1, K_ + "tau = nan (need 0 <= tau <= 1)"),
    ("s['tau'] = 1.5", -1, K_ + "tau = 1.5 (need 0 <= tau <= 1)"),
    ("s['tau'] = -0.01", -1, K_ + "tau = -0.01 (need 0 <= tau <= 1)"),
    ("s['tau_ptr'] = PTR + 2", -1, K_ + "tau_ptr is not 4-byte aligned"),
]


def test_polyak_refusal_ladder():
    def call(s):
        if not s["cfg"]:
            return _abi.lib().mpe_polyak(None, None)
        cfg = _abi.MpePolyak()
        cfg.tau, cfg.tau_ptr, cfg.n_sets = s["tau"], s["tau_ptr"], s["n_sets"]
        for k in range(2):
            cfg.set[k].target, cfg.set[k].online, cfg.set[k].n = s["target"][k], s["online"][k], s["n"][k]
        return _abi.lib().mpe_polyak(C.byref(cfg), None)
    s = dict(cfg=False, n_sets=0, target=[None, None], online=[None, None], n=[8, 8], tau=float("nan"), tau_ptr=None)
    L_ = _abi.lib()
    for n, (repair, rc_want, msg_want) in enumerate(POLYAK_LADDER):      # (no rung returns 0: a valid call launches)
        exec(repair, {"PTR": PTR}, {"s": s})
        assert (call(s), L_.mpe_last_error().decode()) == (rc_want, msg_want), "rung %d (%r): %s" % (n, repair, L_.mpe_last_error().decode())
    assert L_.mpe_sizeof_polyak() == C.sizeof(_abi.MpePolyak) == 24 + 8 * 24


# ---- the host layer's argument checks -----------------------------------------------------------------------------------------------
def test_host_layer_checks_name_the_argument():
    assert set(("TdLoss", "TdLossResult", "td_loss_tensors", "ActorLoss", "RowsLayout", "policy_rows_tensors", "policy_rows_grad_tensors",
                "PolyakTargets")) <= set(mpe.__all__)
    z = torch.zeros
    who = "td_loss_tensors: "
    for match, kw in ((who + "q_n is a list of 1..MPE_ACTOR_MAX_AGENTS = 16 tensors", dict(q_n=[])),
                      (who + r"q_n\[0\] is a contiguous float32 \[M\] or \[M, 1\] tensor", dict(q_n=[z((4, 1, 1)), z(4)])),
                      (who + r"q_n\[1\] is a contiguous float32 \[4\] or \[4, 1\] tensor", dict(q_n=[z(4), z(5)])),
                      (who + r"y is a contiguous float32 \[2, 4\] tensor", dict(y=z((2, 5)))),
                      (who + r"weights is a contiguous float32 \[4\] tensor", dict(weights=z(4).double())),
                      (who + "out is a TdLossResult of 2 agents and M = 4", dict(out=object())),
                      (who + r"q_n\[0\] is on cpu \(the tensors live on a GPU: there is no CPU path\)", dict())):
        a = dict(q_n=[z(4), z((4, 1))], y=z((2, 4)))
        a.update(kw)
        with pytest.raises(_abi.MpeError, match=match):
            td_loss_tensors(**a)
    with pytest.raises(_abi.MpeError, match="TdLoss: q_n is a list of tensors"):
        TdLoss()([], z((2, 4)))
    with pytest.raises(_abi.MpeError, match=r"TdLoss: q_n\[1\] is not a tensor"):
        TdLoss()([z(4), None], z((2, 4)))
    with pytest.raises(_abi.MpeError, match="TdLoss: y requires grad"):
        TdLoss()([z(4), z(4)], z((2, 4), requires_grad=True))
    with pytest.raises(_abi.MpeError, match=r"td_loss_tensors: q_n\[0\] is on cpu"):
        TdLoss()([z(4, requires_grad=True), z(4)], z((2, 4)))
    ref = R.LAYOUTS["L22"]
    lay = RowsLayout(ref.W, ref.dim_c, ref.col, ref.movable, ref.speaks)
    assert lay.n == ref.n == [3, 5] and lay.A == 2
    with pytest.raises(_abi.MpeError, match="RowsLayout: col, movable and speaks are lists"):
        RowsLayout(22, 3, [14, 17], [False], [True, False])
    zs = [z((4, 3)), z((4, 5))]
    who = "policy_rows_tensors: "
    for match, kw in ((who + "layout is an Actors or a RowsLayout", dict(layout=None)),
                      (who + "logits_n is a list of 2 tensors", dict(logits_n=zs[:1])),
                      (who + r"logits_n\[1\] is a contiguous float32 \[4, 5\] tensor", dict(logits_n=[zs[0], z((4, 6))])),
                      (who + r"joint is a contiguous float32 \[4, 22\] tensor", dict(joint=z((4, 23)))),
                      (who + "out is a list of 2 tensors", dict(out=[z((4, 22))])),
                      (who + r"out\[1\] is a contiguous float32 \[4, 22\] tensor", dict(out=[z((4, 22)), z((5, 22))])),
                      (who + r"joint is on cpu \(the tensors live on a GPU: there is no CPU path\)", dict())):
        a = dict(layout=lay, joint=z((4, 22)), logits_n=zs)
        a.update(kw)
        with pytest.raises(_abi.MpeError, match=match):
            policy_rows_tensors(**a)
    who = "policy_rows_grad_tensors: "
    full = z((4, 22))
    for match, kw in ((who + "g_n is a list of 2 tensors", dict(g_n=[full])),
                      (who + r"g_n\[0\] is a float32 \[4, >= 3\] tensor", dict(g_n=[z((4, 2)), z((4, 5))])),
                      (who + r"g_n\[1\] is a float32 \[4, >= 5\] tensor", dict(g_n=[z((4, 3)), z((5, 4)).t()])),
                      (who + "reg_coef = -1", dict(reg_coef=-1)),
                      (who + "reg_coef = nan", dict(reg_coef=float("nan"))),
                      (who + r"q is a contiguous float32 \[2, 4\] tensor", dict(q=z((4, 2)))),
                      (who + "out is a PolicyRowsGradResult", dict(out=object())),
                      (who + r"logits_n\[0\] is on cpu", dict())):
        a = dict(layout=lay, logits_n=zs, g_n=[full[:, 14:17], full[:, 17:22]])
        a.update(kw)
        with pytest.raises(_abi.MpeError, match=match):
            policy_rows_grad_tensors(**a)
    with pytest.raises(_abi.MpeError, match="ActorLoss: critics is a Critics"):
        ActorLoss(lay, object())
    with pytest.raises(_abi.MpeError, match="ActorLoss: layout is an Actors or a RowsLayout"):
        ActorLoss(object(), object())


def test_polyak_targets_refusals():
    who = "PolyakTargets: "
    for pairs in (None, [], [(1, 2)] * 9, [(1,)], [1]):
        with pytest.raises(_abi.MpeError, match=who + r"pairs is a list of 1..MPE_ADAM_MAX_SETS = 8 \(online_net, target_net\) pairs"):
            PolyakTargets(pairs, 0.01)
    with pytest.raises(_abi.MpeError, match=who + r"pairs\[0\]'s online net is an Actors, a Values or a Critics"):
        PolyakTargets([(object(), object())], 0.01)


# ---- the host walk ------------------------------------------------------------------------------------------------------------------
WALK_FLAGS = ["-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path_factory.mktemp("ddpg_walk") / "ddpg_host_walk")
    cmd = [cxx, "-std=c++17"] + WALK_FLAGS + ["-I", os.path.join(ROOT, "multiagent_particle_envs_amd", "csrc"),
                                              os.path.join(ROOT, "tests", "c", "ddpg_host_walk.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]
    return exe


def _polyak_cases(M):
    """every n with every tau, spread over the row counts so that each walk stays short: the M-th slice of the 20 pairs"""
    rs = np.random.RandomState(77 + M)
    pairs = [(n, tau) for n in R.POLYAK_N for tau in R.POLYAK_TAU]
    k = R.ROWS.index(M)
    mine = pairs[k::len(R.ROWS)]
    out = []
    for n, tau in mine:
        x, w = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
        x[-5:], w[-5:] = 0.0, 0.0      # padding
        out.append((x, w, tau))
    return out


def test_polyak_cases_cover_every_size_and_tau():
    seen = set()
    for M in R.ROWS:
        seen |= set((len(x), tau) for x, _, tau in _polyak_cases(M))
    assert seen == set((n, tau) for n in R.POLYAK_N for tau in R.POLYAK_TAU)


@pytest.mark.parametrize("name", LAYOUT_IDS)
@pytest.mark.parametrize("M", R.ROWS)
def test_host_walk_every_block_wave_and_lane_under_the_sanitizers(M, name, host_walk, tmp_path):
    """All launches on exact-size heap buffers at both alignments (the walk itself asserts that both write the same bytes and that
    every output float of mpe_policy_rows is stored exactly once).  TD loss and Polyak: bit-equal to restatement (b).  The rows
    outside the windows: joint's bits.  What an exponential goes into (libm's on the host): p within LOGP_TOL on log p; dlogits,
    the stats and the loss within the parity bound (4 x the deviation of float32 torch autograd, here on the CPU; floor 2 ulps)."""
    lay, reg = R.LAYOUTS[name], 1e-3
    x = R.make_inputs(lay, M)
    R.check_logits(lay, x)
    polyak = _polyak_cases(M)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    R.write_walk_input(src, lay, M, x, reg, polyak)
    r = subprocess.run([host_walk, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (name, M, r.stdout[-500:], r.stderr[-4000:])
    assert "%d chunks, %d groups" % ((M + 255) // 256, (M + 63) // 64) in r.stdout and "both alignments equal" in r.stdout
    out = R.read_walk_output(dst, lay, M, polyak)
    for tag, w in (("td_w", x["w"]), ("td", None)):
        want = R.td_loss32(x["q"], x["y"], w)
        for k in ("dq", "td_abs", "stats"):
            assert np.array_equal(out[tag][k].view(np.uint32), want[k].view(np.uint32)), (tag, k)
        assert np.float32(out[tag]["loss"]).view(np.uint32) == want["loss"].view(np.uint32)
    for got, (xs, ws, tau) in zip(out["polyak"], polyak):
        assert np.array_equal(got.view(np.uint32), R.polyak32(xs, ws, tau).view(np.uint32)), (len(xs), tau)
    assert R.outside_equal(lay, out["rows"], x)
    assert R.logp_deviation(lay, out["rows"], x) <= R.LOGP_TOL
    ref = R.rows_grad64(lay, x, reg, q=x["q"])
    bound = R.bounds(R.grad_deviations(lay, R.torch_rows(lay, x, reg, torch.float32, q=x["q"]), ref))
    for tag in ("grad_packed", "grad_inplace", "grad_nostats"):
        for k, (dev, _) in R.grad_deviations(lay, out[tag], ref).items():
            assert dev <= bound[k], (name, M, tag, k, dev, bound[k])
    for i in range(lay.A):      # the window's source and the stats change no bit of dlogits
        assert np.array_equal(out["grad_packed"]["dlogits"][i].view(np.uint32), out["grad_inplace"]["dlogits"][i].view(np.uint32))
        assert np.array_equal(out["grad_packed"]["dlogits"][i].view(np.uint32), out["grad_nostats"]["dlogits"][i].view(np.uint32))
    assert np.array_equal(out["grad_packed"]["stats"].view(np.uint32), out["grad_inplace"]["stats"].view(np.uint32))
    assert np.all(out["grad_packed"]["stats"][:, [3, 4, 5, 7]] == 0)
