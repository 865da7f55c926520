"""The PPO loss head without a GPU: the float64 restatement of THE PPO LOSS RULE against torch float64 autograd (the select rule is
torch's), every refusal of the two entry points in the header's order, the host layer's argument checks, the host walk of every
block, wave and lane of both launches under the sanitizers (tests/c/ppo_loss_host_walk.cpp), and the band condition of the GPU
test's fixed inputs."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.onpolicy import OnPolicyBatch, PpoLoss, PpoLossResult, ppo_loss_tensors

import _ppo_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x10000      # a plausible, 16-byte aligned address (no refused call reads it)


# ---- (a) against torch float64 autograd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GPU_CASES, ids=R.GPU_IDS)
def test_restatement_is_torch_float64_autograd(case):
    """The rule's select gradients are what torch.min / clamp / torch.max hand back: loss, per-row terms and every gradient agree
    with float64 autograd on the example's formula (plus the clipped-value and entropy terms) within 1e-12 of each output's largest
    magnitude."""
    x = R.make_inputs(case)
    ref, t64 = R.rule64(case, x), R.torch_loss(case, x, torch.float64)
    ref = dict(ref, band=np.zeros_like(ref["band"]))      # every row: float64 against float64 has no band
    for name, (dev, mag) in R.deviations(case, t64, ref).items():
        assert dev <= 1e-12 * mag, (case.name, name, dev, mag)
    assert float(ref["clipped"].mean()) > 0.1 or case.M == 1      # a good share of the rows clips
    if case.M >= 257:
        for sign in (1, -1):      # on each side, under both advantage signs
            assert ((ref["ratio"] > 1.2) & (sign * x["adv"] > 0)).any() and ((ref["ratio"] < 0.8) & (sign * x["adv"] > 0)).any()
        assert (x["adv"] == 0).any() and (ref["ratio"] > 5).any() and (ref["ratio"] < 0.2).any()


def test_gradient_select_at_ties_and_inclusive_bounds():
    """ratio exactly on a clamp bound (inclusive: the gradient passes) and adv == 0 (both branches tie at 0), in float64 torch."""
    clip = float(np.float32(0.2))
    for ratio, adv in ((1.0 + clip, 1.0), (1.0 - clip, -1.0), (1.0 + clip, -1.0), (1.0 - clip, 1.0), (2.0, 0.0), (2.0, 1.0), (0.5, -1.0)):
        r = torch.tensor(ratio, dtype=torch.float64, requires_grad=True)
        a = torch.tensor(adv, dtype=torch.float64)
        torch.min(r * a, r.clamp(1 - clip, 1 + clip) * a).backward()
        s1, s2 = ratio * adv, min(max(ratio, 1 - clip), 1 + clip) * adv
        g = adv if (1 - clip <= ratio <= 1 + clip) or s1 < s2 else 0.0
        assert float(r.grad) == g, (ratio, adv, float(r.grad), g)


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


P_ = "mpe_ppo_loss: "
ALIGN = P_ + "every float tensor must be 4-byte and work 8-byte aligned"
TOP = ("cfg", "logits_ptrs", "logp_old", "adv", "dlogits_ptrs", "work", "stats", "loss")
LOSS_LADDER = [("pass", -1, P_ + "cfg is NULL")] + [
    ("s['%s'] = PTR" % a, -1, P_ + "%s is NULL" % b) for a, b in zip(TOP, TOP[1:])] + [
    ("s['loss'] = PTR", -1, P_ + "A = 17 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
    ("s['A'] = 0", -1, P_ + "A = 0 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
    ("s['A'] = 2", -1, P_ + "dim_c = 17 (0..16)"),
    ("s['dim_c'] = -1", -1, P_ + "dim_c = -1 (0..16)"),
    ("s['dim_c'] = 0", -1, P_ + "agent 0 has no head (neither movable nor speaking with dim_c > 0)"),
    ("s['movable'] = [1, 1]; s['speaks'] = [0, 1]; s['dim_c'] = 12", -2,
     P_ + "agent 1: 17 logits (5 * movable + dim_c * speaks) > MPE_ACTOR_MAX_OUT = 16"),
    ("s['dim_c'] = 3", -1, P_ + "M = -1"),
    ("s['M'] = 1 << 30", -1, P_ + "clip = nan (need a finite value >= 0)"),
    ("s['clip'] = float('inf')", -1, P_ + "clip = inf (need a finite value >= 0)"),
    ("s['clip'] = -0.5", -1, P_ + "clip = -0.5 (need a finite value >= 0)"),
    ("s['clip'] = 0.2", -1, P_ + "vf_coef = nan is not finite"),
    ("s['vf_coef'] = 0.5", -1, P_ + "ent_coef = inf is not finite"),
    ("s['ent_coef'] = 0.0", -1, P_ + "value_clip is NaN (negative: off)"),
    ("s['value_clip'] = -1.0; s['value_ptrs'] = [PTR, PTR]", -1, P_ + "value_ptrs is given and val_old is NULL"),
    ("s['val_old'] = PTR", -1, P_ + "value_ptrs is given and ret is NULL"),
    ("s['ret'] = PTR", -1, P_ + "value_ptrs is given and dvalues is NULL"),
    ("s['dvalues'] = PTR", -1, P_ + "act is NULL and an agent is movable"),
    ("s['act'] = PTR", -1, P_ + "utter is NULL and an agent speaks"),
    ("s['utter'] = PTR; s['logits'] = [PTR, None]; s['dlogits'] = [PTR, PTR]", -1, P_ + "logits_ptrs[1] is NULL"),
    ("s['logits'] = [PTR, PTR]; s['dlogits'] = [None, PTR]", -1, P_ + "dlogits_ptrs[0] is NULL"),
    ("s['dlogits'] = [PTR, PTR]; s['value_ptrs'] = [PTR, None]", -1, P_ + "value_ptrs[1] is NULL"),
    ("s['value_ptrs'] = [PTR, PTR + 2]", -1, ALIGN),
    ("s['value_ptrs'] = [PTR, PTR]; s['logits'] = [PTR + 1, PTR]", -1, ALIGN),
    ("s['logits'] = [PTR + 4, PTR]; s['rows'] = PTR + 3", -1, ALIGN),
    ("s['rows'] = PTR + 4; s['work'] = PTR + 4", -1, ALIGN),
    ("s['work'] = PTR + 8; s['adv'] = PTR + 2", -1, ALIGN),
    ("s['adv'] = PTR", -1, P_ + "A * M = 2 * 1073741824 (need A * M < 2^31)"),
    ("s['M'] = 0", 0, P_ + "A * M = 2 * 1073741824 (need A * M < 2^31)"),
]


def _loss_call(s):
    cfg = None
    if s["cfg"]:
        cfg = _abi.MpePpoLoss()
        cfg.n_agents, cfg.dim_c = s["A"], s["dim_c"]
        for i, (m, sp) in enumerate(zip(s["movable"], s["speaks"])):
            cfg.movable[i], cfg.speaks[i] = m, sp
        cfg.clip, cfg.value_clip, cfg.vf_coef, cfg.ent_coef = s["clip"], s["value_clip"], s["vf_coef"], s["ent_coef"]
    arr = lambda on, v: (C.c_void_p * 16)(*v) if on else None      # noqa: E731
    return _abi.lib().mpe_ppo_loss(C.byref(cfg) if cfg is not None else None, arr(s["logits_ptrs"], s["logits"]),
                                   arr(s["value_ptrs"] is not None, s["value_ptrs"] or []), s["M"], s["act"], s["utter"], s["logp_old"], s["adv"],
                                   s["ret"], s["val_old"], arr(s["dlogits_ptrs"], s["dlogits"]), s["dvalues"], s["rows"], s["work"], s["stats"],
                                   s["loss"], None)


def test_ppo_loss_refusal_ladder():
    s = dict(cfg=None, logits_ptrs=None, dlogits_ptrs=None, logits=[None, None], dlogits=[None, None], value_ptrs=None, A=17, dim_c=17,
             movable=[0] * 16, speaks=[0] * 16, M=-1, clip=float("nan"), value_clip=float("nan"), vf_coef=float("nan"), ent_coef=float("inf"),
             act=None, utter=None, logp_old=None, adv=None, ret=None, val_old=None, dvalues=None, rows=None, work=None, stats=None, loss=None)
    _climb(LOSS_LADDER, s, _loss_call)
    assert _abi.lib().mpe_sizeof_ppo_loss() == C.sizeof(_abi.MpePpoLoss) == 56


W_ = "mpe_ppo_loss_work: "
WORK_LADDER = [
    ("pass", -1, W_ + "A = 0 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
    ("s['A'] = 17", -1, W_ + "A = 17 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
    ("s['A'] = 3", -1, W_ + "M = -5"),
    ("s['M'] = 715827883", -1, W_ + "A * M = 3 * 715827883 (need A * M < 2^31)"),
    ("s['M'] = 715827882", 6 * 3 * 2796203, W_ + "A * M = 3 * 715827883 (need A * M < 2^31)"),
]


def test_ppo_loss_work_refusal_ladder_and_counts():
    L_ = _abi.lib()
    last = None
    s = dict(A=0, M=-5)
    for n, (repair, rc_want, msg_want) in enumerate(WORK_LADDER):
        exec(repair, {}, {"s": s})
        rc = L_.mpe_ppo_loss_work(s["A"], s["M"])
        assert (rc, L_.mpe_last_error().decode()) == (rc_want, msg_want), (n, rc, L_.mpe_last_error().decode())
        last = rc
    assert last > 0
    assert [L_.mpe_ppo_loss_work(3, M) for M in (0, 1, 256, 257, 6400)] == [0, 18, 18, 36, 18 * 25]
    assert L_.mpe_ppo_loss_work(16, 513) == 6 * 16 * 3


# ---- the host layer's argument checks -----------------------------------------------------------------------------------------------
def _cpu_args(A=2, M=4, dim_c=0, values=True):
    heads = dict(movable=[True] * A, speaks=[dim_c > 0] * A, dim_c=dim_c)
    n = 5 + dim_c
    a = dict(logits_n=[torch.zeros((M, n)) for _ in range(A)], values_n=[torch.zeros((M, 1)) for _ in range(A)] if values else None,
             act=torch.zeros((A, M, 5)), utter=torch.zeros((A, M, dim_c)) if dim_c else None, logp_old=torch.zeros((A, M)),
             adv=torch.zeros((A, M)), ret=torch.zeros((A, M)), val_old=torch.zeros((A, M)))
    a.update(heads)
    return a


def test_host_layer_checks_name_the_argument():
    assert set(("PpoLoss", "PpoLossResult", "ppo_loss_tensors")) <= set(mpe.__all__)
    who = "ppo_loss_tensors: "

    def refused(match, **kw):
        a = _cpu_args(**{k: kw.pop(k) for k in ("A", "M", "dim_c", "values") if k in kw})
        a.update(kw)
        with pytest.raises(_abi.MpeError, match=match):
            ppo_loss_tensors(**a)
    refused(who + "logits_n is a list of 1..MPE_ACTOR_MAX_AGENTS = 16 tensors", logits_n=[])
    refused(who + "logits_n is a list of 1..MPE_ACTOR_MAX_AGENTS = 16 tensors", logits_n=torch.zeros((4, 5)))
    refused(who + "3 movable and 2 speaks flags for 2 agents", movable=[True] * 3)
    refused(who + r"dim_c = 17 \(0..MPE_ACTOR_MAX_OUT = 16\)", dim_c=17)
    refused(who + "agent 1 has 0 logits", movable=[True, False])
    refused(who + "agent 0 has 17 logits", dim_c=12, logits_n=[torch.zeros((4, 17))] * 2)
    refused(who + r"logits_n\[0\] is a contiguous float32 \[M, 5\] tensor", logits_n=[torch.zeros(4), torch.zeros((4, 5))])
    refused(who + r"logits_n\[1\] is a contiguous float32 \[4, 5\] tensor", logits_n=[torch.zeros((4, 5)), torch.zeros((4, 6))])
    refused(who + r"logits_n\[0\] is a contiguous float32 \[4, 5\] tensor", logits_n=[torch.zeros((4, 5)).double(), torch.zeros((4, 5))])
    refused(who + r"logits_n\[1\] is a contiguous float32", logits_n=[torch.zeros((4, 5)), torch.zeros((5, 4)).t()])
    refused(who + "values_n is a list of 2 tensors", values_n=[torch.zeros(4)])
    refused(who + r"values_n\[1\] is a contiguous float32 \[4\] or \[4, 1\] tensor", values_n=[torch.zeros(4), torch.zeros((4, 2))])
    refused(who + r"act is a contiguous float32 \[2, 4, 5\] tensor", act=torch.zeros((2, 4, 4)))
    refused(who + r"utter is a contiguous float32 \[2, 4, 3\] tensor", dim_c=3, utter=None)
    for name in ("logp_old", "adv", "ret", "val_old"):
        refused(who + r"%s is a contiguous float32 \[2, 4\] tensor" % name, **{name: torch.zeros((2, 5))})
    refused(who + "clip = -0.1", clip=-0.1)
    refused(who + "clip = nan", clip=float("nan"))
    refused(who + "vf_coef = inf", vf_coef=float("inf"))
    refused(who + "value_clip = -1", value_clip=-1)
    refused(who + "out is a PpoLossResult", out=object())
    refused(who + r"logits_n\[0\] is on cpu \(the tensors live on a GPU: there is no CPU path\)")      # every shape is right
    refused(who + r"logits_n\[0\] is on cpu", values=False, ret=None, val_old=None)                    # a policy-only loss reads neither
    assert PpoLossResult.STATS[:6] == ("surrogate", "value_loss", "entropy", "approx_kl", "clip_fraction", "ratio")


def test_ppo_loss_object_checks_its_arguments():
    class _Agent(object):      # (what PpoLoss reads of an env: its agents' heads, as Actors does)
        movable, silent = True, True

    class _World(object):
        agents, dim_c = [_Agent(), _Agent(), _Agent()], 2

    class _Env(object):
        world = _World()
    env = _Env()
    with pytest.raises(_abi.MpeError, match="PpoLoss: clip = -1"):
        PpoLoss(env, clip=-1)
    with pytest.raises(_abi.MpeError, match="PpoLoss: value_clip = nan"):
        PpoLoss(env, value_clip=float("nan"))
    with pytest.raises(_abi.MpeError, match="PpoLoss: vf_coef = inf"):
        PpoLoss(env, vf_coef=float("inf"))
    head = PpoLoss(env, clip=0.1, value_clip=0.3, vf_coef=1.0, ent_coef=0.02)
    A = head.A
    assert head.n_out == [5] * A and head.dim_c == 0 and (head.clip, head.value_clip, head.vf_coef, head.ent_coef) == (0.1, 0.3, 1.0, 0.02)
    z = [torch.zeros((4, 5), requires_grad=True) for _ in range(A)]
    b = OnPolicyBatch()
    b.act, b.utter, b.logp = torch.zeros((A, 4, 5)), None, None
    b.adv = b.ret = b.val = torch.zeros((A, 4))
    with pytest.raises(_abi.MpeError, match="PpoLoss: logits_n is a list of %d tensors" % A):
        head(z[:1] if A > 1 else [], None, b)
    with pytest.raises(_abi.MpeError, match="PpoLoss: values_n is a list of %d tensors" % A):
        head(z, [torch.zeros(4)] * (A + 1), b)
    with pytest.raises(_abi.MpeError, match="PpoLoss: batch is an OnPolicyBatch"):
        head(z, None, object())
    with pytest.raises(_abi.MpeError, match="PpoLoss: batch.logp is None"):
        head(z, None, b)
    b.logp = torch.zeros((A, 4))
    with pytest.raises(_abi.MpeError, match=r"PpoLoss: logits_n\[0\] is not a tensor"):
        head([None] + z[1:], None, b)
    with pytest.raises(_abi.MpeError, match=r"ppo_loss_tensors: logits_n\[0\] is on cpu"):      # the last check: there is no CPU path
        head(z, None, b)


# ---- the host walk ------------------------------------------------------------------------------------------------------------------
WALK_FLAGS = ["-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path_factory.mktemp("ppo_loss_walk") / "ppo_loss_host_walk")
    cmd = [cxx, "-std=c++17"] + WALK_FLAGS + ["-I", os.path.join(ROOT, "multiagent_particle_envs_amd", "csrc"),
                                              os.path.join(ROOT, "tests", "c", "ppo_loss_host_walk.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("layout", sorted(R.WALK_LAYOUTS))
@pytest.mark.parametrize("M", R.WALK_M)
def test_host_walk_every_block_wave_and_lane_under_the_sanitizers(M, layout, A, host_walk, tmp_path):
    """Both launches on exact-size heap buffers: what they wrote against restatement (a) within the GPU test's bound (4 x the
    deviation of float32 torch autograd on the same inputs, here on the CPU; floor 2 ulps), and the sums against (b) exactly."""
    base = R.walk_case(layout, A, M)
    x = R.make_inputs(base)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for values, want_rows in ((True, True), (False, True), (True, False), (False, False)):
        case = base.but(base.name, values=values)
        xx = dict(x, values=x["values"] if values else None)
        R.write_walk_input(src, case, xx, want_rows)
        r = subprocess.run([host_walk, src, dst], capture_output=True, text=True)
        assert r.returncode == 0, (case.name, values, want_rows, r.stdout[-500:], r.stderr[-4000:])
        assert "%d chunks per agent, %d doubles" % ((M + 255) // 256, 6 * A * ((M + 255) // 256)) in r.stdout
        out = R.read_walk_output(dst, case, want_rows)
        ref = R.rule64(case, xx)
        got, bound = R.deviations(case, out, ref), R.bounds(R.deviations(case, R.torch_loss(case, xx, torch.float32), ref))
        for name, (dev, _) in got.items():
            assert dev <= bound[name], (case.name, values, want_rows, name, dev, bound[name])
        if not ref["band"].any():
            assert np.array_equal(out["stats"][:, 4], ref["stats"][:, 4].astype(np.float32))      # the clipped rows, counted
        assert np.all(out["stats"][:, 7] == 0)
        if not values:
            assert np.all(out["stats"][:, 1] == 0)
        if want_rows:
            stats, loss = R.fold_stats(case, out["rows"])
            cols = [0, 1, 2, 6]
            assert np.array_equal(out["stats"][:, cols].view(np.uint32), stats[:, cols].view(np.uint32)), (case.name, out["stats"], stats)
            assert np.float32(out["loss"]).view(np.uint32) == loss.view(np.uint32)


# ---- the band condition of the GPU test's fixed inputs ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GPU_CASES + R.PIECE_CASES, ids=R.GPU_IDS + R.PIECE_IDS)
def test_band_rows_are_at_most_a_thousandth(case):
    """Rows whose ratio lies within 1e-5 (relative) of 1 +- clip, whose |v - val_old| lies within 1e-6 of value_clip, or whose two
    value branches lie within 1e-6 (relative) of each other outside the clip may take the other side of a select in float32: the
    parity check leaves them out, and the seeds are picked so that they are at most 0.1 % of a case's rows."""
    ref = R.rule64(case, R.make_inputs(case))
    assert ref["band"].shape == (case.A, case.M)
    assert int(ref["band"].sum()) <= 0.001 * case.A * case.M, (case.name, int(ref["band"].sum()))


def test_host_walk_more_chunks_than_one_piece_of_the_second_launch(host_walk, tmp_path):
    """16 agents, 66 chunks: the second launch stages the partials in pieces of 64 chunks (6 144 doubles / (6 * 16)), so this walk
    takes a second, short piece, and a piece of one agent (384 doubles) is longer than the block is wide."""
    case = R.Case("move_A16_M16641", [R.MOVER] * 16, 0, 16641, 77)
    x = R.make_inputs(case)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    R.write_walk_input(src, case, x, True)
    r = subprocess.run([host_walk, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
    assert "66 chunks per agent, %d doubles of workspace, pieces of 64 chunks" % (6 * 16 * 66) in r.stdout
    out = R.read_walk_output(dst, case, True)
    stats, loss = R.fold_stats(case, out["rows"])
    cols = [0, 1, 2, 6]
    assert np.array_equal(out["stats"][:, cols].view(np.uint32), stats[:, cols].view(np.uint32))
    assert np.float32(out["loss"]).view(np.uint32) == loss.view(np.uint32)
    ref = R.rule64(case, x)
    cols = [0, 1, 2, 3, 5]      # (the means; the count of clipped rows may differ by a band row)
    assert np.abs(out["stats"][:, cols] - ref["stats"][:, cols]).max() < 1e-5
    assert np.abs(out["stats"][:, 4] - ref["stats"][:, 4]).max() <= 2.0 / case.M
