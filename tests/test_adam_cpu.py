"""The optimiser step without a device: the float64 form of THE ADAM RULE against float64 torch.optim.Adam / AdamW
with clip_grad_norm_, mpe_adam_step's refusal ladder and mpe_adam_work's counts, the argument checks of DeviceAdam, and the HOST WALK
-- csrc/mpe_adam.h's per-lane functions compiled by the host compiler under AddressSanitizer and UBSan and run for every lane of
every workgroup of both launches on exact-size buffers, BIT-EQUAL to the float32 restatement of tests/_adam_ref.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.optim import DeviceAdam
from multiagent_particle_envs_amd.train import Trainable

import _adam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the float64 form against torch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("max_grad_norm", [0.0, 0.5])
def test_float64_form_against_float64_torch(weight_decay, max_grad_norm):
    """20 steps, three tensors of 6416 floats together, gradient magnitudes 1e-4 .. 10; relative to each tensor's largest magnitude"""
    ns, steps, lr = (4000, 16, 2400), 20, 1e-2
    rng = np.random.RandomState(7)
    w0 = [rng.standard_normal(n) for n in ns]
    grads = [[10.0 ** rng.uniform(-4.0, 1.0, n) * rng.choice([-1.0, 1.0], n) for _ in range(steps)] for n in ns]
    cfg = dict(R.CFG, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
    sets = [dict(w=w.copy(), m=np.zeros_like(w), v=np.zeros_like(w)) for w in w0]
    got, log = R.run_ref(cfg, sets, grads, dtype=np.float64)
    params = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in w0]
    kind = torch.optim.AdamW if weight_decay else torch.optim.Adam
    opt = kind(params, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay, foreach=False)
    for t in range(steps):
        for p, gs in zip(params, grads):
            p.grad = torch.tensor(gs[t], dtype=torch.float64)
        if max_grad_norm:
            total = torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
            assert abs(float(total) - log[t][0][6]) <= 1e-12 * float(total)
            assert (log[t][0][7] < 1.0) == (float(total) + 1e-6 > max_grad_norm)
        opt.step()
    worst = 0.0
    for s, p in zip(got, params):
        ref = p.detach().numpy()
        worst = max(worst, float(np.abs(s["w"] - ref).max() / np.abs(ref).max()))
    print("float64 form against torch, wd %g clip %g: worst relative deviation %.3e" % (weight_decay, max_grad_norm, worst))
    assert worst <= 1e-12
    assert log[-1][0][3] == steps and log[-1][0][8] == 0


# ---- mpe_adam_work and the refusal ladder ------------------------------------------------------------------------------------------
_HOST = (C.c_float * 4096)()
_BASE = (C.addressof(_HOST) + 63) & ~63      # a 64-byte aligned host address: NO RUNG LAUNCHES (the last one fails on `work`)


def _cfg(ns, fill=True):
    c = _abi.MpeAdam()
    c.lr, c.beta1, c.beta2, c.eps, c.weight_decay, c.max_grad_norm = 3e-4, 0.9, 0.999, 1e-8, 0.0, 0.0
    c.n_sets = len(ns)
    at = 1 << 32      # (addresses only: mpe_adam_work reads no buffer)
    for k, n in enumerate(ns):
        c.set[k].n = n
        if fill:
            for name in ("weights", "grad", "m", "v"):
                setattr(c.set[k], name, at)
                at += 4 * n
    return c


def test_adam_work_counts_on_both_sides_of_a_span_change():
    L_ = _abi.lib()
    assert L_.mpe_sizeof_adam() == C.sizeof(_abi.MpeAdam) == 64 + 40 * 8
    cases = [((16,), 1, 1), ((1008,), 1, 1), ((1024,), 1, 1), ((1040,), 1, 2), ((262144,), 1, 256), ((262160,), 2, 129),
             ((6416, 16, 20000), 1, 7 + 1 + 20), ((32768,) * 8, 1, 256), ((32784,) * 8, 2, 8 * 17), ((38496,), 1, 38)]
    for ns, span, P in cases:
        assert R.span_of(ns) == span and sum(R.tiles_of(ns)) == P, ns
        assert L_.mpe_adam_work(C.byref(_cfg(ns))) == P, ns
    assert L_.mpe_adam_work(None) == -1 and L_.mpe_last_error().decode() == "mpe_adam_work: cfg is NULL"
    assert L_.mpe_adam_work(C.byref(_cfg((1 << 30, 1 << 30)))) == -1
    assert L_.mpe_last_error().decode() == "mpe_adam_work: the sets hold 2^31 floats or more (need N < 2^31)"
    big = ((1 << 30) - 16, 1 << 30)
    assert R.span_of(big) == 8192 and L_.mpe_adam_work(C.byref(_cfg(big))) == sum(R.tiles_of(big)) == 256


ADAM_LADDER = [
    ("", "mpe_adam_step: cfg is NULL"),
    ("s['cfg'] = s['C']", "mpe_adam_step: n_sets = 0 (1..MPE_ADAM_MAX_SETS = 8)"),
    ("s['C'].n_sets = 9", "mpe_adam_step: n_sets = 9 (1..MPE_ADAM_MAX_SETS = 8)"),
    ("s['C'].n_sets = 2", "mpe_adam_step: set[0].weights is NULL"),
    ("s['C'].set[0].weights = B + 4", "mpe_adam_step: set[0].grad is NULL"),
    ("s['C'].set[0].grad = B + 64", "mpe_adam_step: set[0].m is NULL"),
    ("s['C'].set[0].m = B + 128", "mpe_adam_step: set[0].v is NULL"),
    ("s['C'].set[0].v = B + 192", "mpe_adam_step: set[0].weights is not 16-byte aligned"),
    ("s['C'].set[0].weights = B", "mpe_adam_step: set[0].n = 8 floats (a multiple of 16, at least 16)"),
    ("s['C'].set[0].n = 24", "mpe_adam_step: set[0].n = 24 floats (a multiple of 16, at least 16)"),
    ("s['C'].set[0].n = 16", "mpe_adam_step: set[1].weights is NULL"),
    ("s['C'].set[1].weights = B + 256", "mpe_adam_step: set[1].grad is NULL"),
    ("s['C'].set[1].grad = B + 64 + 32", "mpe_adam_step: set[1].m is NULL"),
    ("s['C'].set[1].m = B + 1024", "mpe_adam_step: set[1].v is NULL"),
    ("s['C'].set[1].v = B + 2048 + 8", "mpe_adam_step: set[1].v is not 16-byte aligned"),
    ("s['C'].set[1].v = B + 2048", "mpe_adam_step: set[1].n = 0 floats (a multiple of 16, at least 16)"),
    ("s['C'].set[1].n = 32", "mpe_adam_step: set[0].grad and set[1].grad overlap"),
    ("s['C'].set[1].grad = B + 256 + 64", "mpe_adam_step: set[1].weights and set[1].grad overlap"),
    ("s['C'].set[1].grad = B + 512; s['C'].set[1].n = 1 << 31", "mpe_adam_step: set[1].weights and set[1].grad overlap"),
    # (N is checked behind the overlaps, so a rung that reaches it needs far-apart ADDRESSES: none is ever read)
    ("s['C'].set[1].n = 32; s['C'].set[0].n = (1 << 31) - 32; s['far'](s['C'].set[0], 1 << 40, 1 << 40)", "mpe_adam_step: the sets hold 2^31 floats or more (need N < 2^31)"),
    ("s['C'].set[0].n = 16; s['far'](s['C'].set[0], B, 64)", "mpe_adam_step: lr = nan is not finite"),
    ("s['C'].lr = -1.0", "mpe_adam_step: beta1 = inf is not finite"),
    ("s['C'].beta1 = 1.0", "mpe_adam_step: beta2 = nan is not finite"),
    ("s['C'].beta2 = -0.5", "mpe_adam_step: eps = inf is not finite"),
    ("s['C'].eps = 0.0", "mpe_adam_step: weight_decay = -inf is not finite"),
    ("s['C'].weight_decay = -0.01", "mpe_adam_step: max_grad_norm = nan is not finite"),
    ("s['C'].max_grad_norm = -0.5", "mpe_adam_step: beta1 = 1 (need 0 <= beta1 < 1)"),
    ("s['C'].beta1 = 0.9", "mpe_adam_step: beta2 = -0.5 (need 0 <= beta2 < 1)"),
    ("s['C'].beta2 = 0.999", "mpe_adam_step: eps = 0 (need eps > 0: a padding entry divides by it)"),
    ("s['C'].eps = 1e-8", "mpe_adam_step: lr = -1 (need >= 0)"),
    ("s['C'].lr = float('nan'); s['C'].lr_ptr = B + 3072 + 2", "mpe_adam_step: weight_decay = -0.01 (need >= 0)"),
    ("s['C'].weight_decay = 0.01", "mpe_adam_step: max_grad_norm = -0.5 (need >= 0; 0: no clipping)"),
    ("s['C'].max_grad_norm = 0.5", "mpe_adam_step: lr_ptr is not 4-byte aligned"),
    ("s['C'].lr_ptr = B + 3072", "mpe_adam_step: state is NULL"),
    ("s['state'] = B + 3200 + 4", "mpe_adam_step: work is NULL"),
    ("s['work'] = B + 3400", "mpe_adam_step: state and work must be 8-byte aligned"),
    ("s['state'] = B + 3200; s['work'] = B + 3400 + 4", "mpe_adam_step: state and work must be 8-byte aligned"),
]


def test_adam_refusal_ladder():
    """One repair per rung; the code and the whole message at every rung.  The call starts wrong in every checked way and NO RUNG
    PASSES EVERY CHECK: a call that did would launch two kernels on the host addresses below."""
    L_ = _abi.lib()
    c = _abi.MpeAdam()
    nan, inf = float("nan"), float("inf")
    c.lr, c.beta1, c.beta2, c.eps, c.weight_decay, c.max_grad_norm = nan, inf, nan, inf, -inf, nan
    c.set[0].n = 8
    def far(q, base, stride):
        q.weights, q.grad, q.m, q.v = base, base + stride, base + 2 * stride, base + 3 * stride
    s = dict(cfg=None, C=c, state=None, work=None, far=far)
    for n, (repair, msg_want) in enumerate(ADAM_LADDER):
        exec(repair, {"B": _BASE}, {"s": s})
        rc = L_.mpe_adam_step(C.byref(s["cfg"]) if s["cfg"] is not None else None, s["state"], s["work"], None)
        assert (rc, L_.mpe_last_error().decode()) == (-1, msg_want), "rung %d (%r)" % (n, repair)
    assert len(ADAM_LADDER) == 37


# ---- the host layer ----------------------------------------------------------------------------------------------------------------
def _mlp(D, n_out, hidden=(8,)):
    mods, k = [], D
    for h in hidden:
        mods += [nn.Linear(k, h), nn.Tanh()]
        k = h
    return nn.Sequential(*(mods + [nn.Linear(k, n_out)]))


def test_device_adam_checks_name_the_argument():
    assert "DeviceAdam" in mpe.__all__ and mpe.DeviceAdam is DeviceAdam
    env = mpe.make_env("simple_spread", batch_size=4, device="cpu")
    mods, vmods = [_mlp(18, 5) for _ in range(3)], [_mlp(18, 1) for _ in range(3)]
    pi, V = mpe.Actors(env, mods, logits=True), mpe.Values(env, vmods)
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam: nets is a list of 1..MPE_ADAM_MAX_SETS = 8"):
        DeviceAdam([])
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam: nets is a list of 1..MPE_ADAM_MAX_SETS = 8"):
        DeviceAdam(pi)
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam: nets is a list"):
        DeviceAdam([mpe.Values(env, [_mlp(18, 1) for _ in range(3)]) for _ in range(9)])
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam: nets\[1\] is an Actors, a Values or a Critics, or a Trainable of one \(got Sequential\)"):
        DeviceAdam([pi, mods[0]])
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam: nets\[1\] is nets\[0\] again"):
        DeviceAdam([pi, Trainable(pi)])
    behaviour = mpe.Actors(env, mods, mode="sample")
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam: nets\[0\] and nets\[2\] hold the same module object \(agent 0 of nets\[2\]\)"):
        DeviceAdam([pi, V, behaviour])
    shared = _mlp(18, 5)
    DeviceAdamRefused = pytest.raises(_abi.MpeError, match=r"DeviceAdam: nets\[0\] is on cpu \(the buffers live on a GPU: there is no CPU path\)")
    with DeviceAdamRefused:      # a module shared by the agents INSIDE one net is fine: the first refusal is the device's
        DeviceAdam([mpe.Actors(env, shared, logits=True)])
    frozen = mpe.Values(env, [_mlp(18, 1) for _ in range(3)])
    frozen._frozen = frozen.pack()
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam: nets\[1\] is already frozen"):
        DeviceAdam([pi, frozen])
    other = mpe.make_env("simple_spread", batch_size=4, device="cpu")
    V2 = mpe.Values(other, [_mlp(18, 1) for _ in range(3)])
    other.world.device = torch.device("meta")
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam: nets\[1\] is on meta, nets\[0\] on cpu"):
        DeviceAdam([pi, V2])
    for kw, name in ((dict(lr=float("nan")), "lr"), (dict(lr=-1e-3), "lr"), (dict(betas=(0.9, 1.0)), "betas"), (dict(eps=0.0), "eps"),
                     (dict(weight_decay=-0.1), "weight_decay"), (dict(max_grad_norm=float("inf")), "max_grad_norm")):
        with pytest.raises(_abi.MpeError, match=r"DeviceAdam: %s = " % name):
            DeviceAdam([pi, V], **kw)
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam: lr_tensor is a one-element float32 tensor on the nets' device"):
        DeviceAdam([pi, V], lr_tensor=torch.zeros(2))
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam: lr_tensor is a one-element float32 tensor"):
        DeviceAdam([pi, V], lr_tensor=torch.zeros(1, dtype=torch.float64))
    with DeviceAdamRefused:
        DeviceAdam([Trainable(pi), V])
    assert pi._frozen is None and V._frozen is None      # a refused constructor leaves the nets alone
    assert Trainable(pi).last_grad is None


def test_step_and_share_checks_name_the_argument():
    """step()'s and share()'s checks on an optimiser object without a device (the constructor allocates the device buffers)."""
    env = mpe.make_env("simple_spread", batch_size=4, device="cpu")
    mods = [_mlp(18, 5) for _ in range(3)]
    pi, V = Trainable(mpe.Actors(env, mods, logits=True)), mpe.Values(env, [_mlp(18, 1) for _ in range(3)])
    opt = object.__new__(DeviceAdam)
    opt.nets, opt._trainable, opt.device, opt._shared = [pi.net, V], [pi, None], torch.device("cpu"), []
    opt.weights = [pi.net.pack()[0], V.pack()[0]]
    opt._asets = [pi.net.pack()[1], V.pack()[1]]
    opt._cfg = _abi.MpeAdam()
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam.step: nets\[0\] no longer reads the optimiser's live buffer"):
        opt.step()
    pi.net._frozen, V._frozen = (opt.weights[0], opt._asets[0]), (opt.weights[1], opt._asets[1])
    V.freeze()      # the public freeze() replaces the live pair by a snapshot of the modules: refused, not silently stepped past
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam.step: nets\[1\] no longer reads the optimiser's live buffer \(freeze\(\) / unfreeze\(\)"):
        opt.step()
    V._frozen = (opt.weights[1], opt._asets[1])
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam.step: nets\[1\] was not given as a Trainable: pass grads="):
        opt.step()
    opt._trainable = [pi, Trainable(V)]
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam.step: nets\[0\].last_grad is None \(no backward\(\) since the last step\)"):
        opt.step()
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam.step: grads is a list of 2 MlpGradResult, one per net"):
        opt.step([None])
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam.step: grads\[0\] is the MlpGradResult of nets\[0\]"):
        opt.step([torch.zeros(4), torch.zeros(4)])
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam.share: net is none of this optimiser's nets"):
        opt.share(mpe.Values(env, [_mlp(18, 1) for _ in range(3)]), V)
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam.share: other is an Actors, a Values or a Critics \(got list\)"):
        opt.share(pi, mods)
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam.share: other is built over other modules than net"):
        opt.share(pi, mpe.Actors(env, [_mlp(18, 5) for _ in range(3)]))
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam.share: other is built over other modules than net"):
        opt.share(pi, mpe.Actors(env, mods[::-1]))
    behaviour = mpe.Actors(env, mods, mode="sample", seed=3)
    assert opt.share(pi, behaviour) is behaviour
    wts, aset = behaviour._frozen
    assert wts is opt.weights[0] and aset.mode == _abi.MPE_POLICY_SAMPLE and aset.seed == 3
    assert list(aset.offset) == list(opt._asets[0].offset)
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam.share: other is already frozen"):
        opt.share(pi, behaviour)
    behaviour.unfreeze()
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam.step: a set joined by share\(\) no longer reads the optimiser's live buffer"):
        opt.step()


# ---- the host walk -----------------------------------------------------------------------------------------------------------------
WALK_FLAGS = ["-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path_factory.mktemp("adam_walk") / "adam_host_walk")
    cmd = [cxx, "-std=c++17"] + WALK_FLAGS + ["-I", os.path.join(ROOT, "multiagent_particle_envs_amd", "csrc"),
                                              os.path.join(ROOT, "tests", "c", "adam_host_walk.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]
    return exe


def _same(a, b):
    """bit equality; a NaN equals a NaN (its payload is not part of the rule: only a skipped step's norm and partial hold one)"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and R.same_bits(np.where(nan, 0, a), np.where(nan, 0, b))


def _walk_equals_ref(exe, tmp_path, cfg, sets, grads, state=None, lr_values=None):
    ns = [s["w"].size for s in sets]
    state = R.fresh_state() if state is None else state
    want, wlog = R.run_ref(cfg, sets, grads, state=state, lr_values=lr_values)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    R.write_walk_input(src, cfg, sets, grads, state, lr_values)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (ns, r.stdout[-500:], r.stderr[-4000:])
    assert "span %d, %d tiles" % (R.span_of(ns), sum(R.tiles_of(ns))) in r.stdout, r.stdout
    got, glog = R.read_walk_output(dst, ns, len(grads[0]))
    for t, ((gs, gw), (ws, ww)) in enumerate(zip(glog, wlog)):
        assert _same(gs, ws), ("state", ns, t, gs, ws)
        assert _same(gw, ww), ("work", ns, t)
    for k, (g, w) in enumerate(zip(got, want)):
        for name in ("w", "m", "v"):
            assert R.same_bits(g[name], w[name]), (name, ns, k, int((g[name] != w[name]).sum()))
    return want, wlog


@pytest.mark.parametrize("ns", R.SHAPES, ids=R.SHAPE_IDS)
def test_host_walk_every_lane_under_the_sanitizers(ns, host_walk, tmp_path):
    sets, grads = R.make_sets(ns, seed=len(ns) * 1000 + ns[0])
    assert any((np.abs(g[0]) < 1e-19).any() for g in grads) or sum(ns) < 64      # g * g is denormal or zero in float32 somewhere
    for cfg in (R.CFG, dict(R.CFG, lr=1e-2, weight_decay=0.01, max_grad_norm=0.5)):
        want, log = _walk_equals_ref(host_walk, tmp_path, cfg, sets, grads)
        assert log[-1][0][3] == R.STEPS and log[-1][0][8] == 0
        for s, w in zip(sets, want):      # padding stays +0.0f bit for bit, also under weight decay
            for name in ("w", "m", "v"):
                assert not w[name][s["pad"]].view(np.uint32).any(), (name, ns)
            assert (w["w"][~s["pad"]] != s["w"][~s["pad"]]).any()


def test_host_walk_clipping(host_walk, tmp_path):
    """clip off, clip inactive, clip active, and norm == max_grad_norm exactly (the 1e-6 of clip_grad_norm_ makes that one active)"""
    sets, _ = R.make_sets((1040,), seed=5)
    g = np.zeros(1040, np.float32)
    g[0], g[1030] = 3.0, -4.0      # norm 5 exactly, across the two tiles
    grads = [[g] * R.STEPS]
    coefs = {}
    for mg in (0.0, 7.0, 0.5, 5.0):
        _, log = _walk_equals_ref(host_walk, tmp_path, dict(R.CFG, max_grad_norm=mg), sets, grads)
        assert log[0][0][6] == 5.0
        coefs[mg] = log[0][0][7]
    assert coefs[0.0] == 1.0 and coefs[7.0] == 1.0 and coefs[0.5] == 0.5 / (5.0 + 1e-6) and coefs[5.0] == 5.0 / (5.0 + 1e-6) < 1.0


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_host_walk_skip(bad, host_walk, tmp_path):
    """a non-finite gradient skips the step -- nothing changes, pending := committed -- and the next finite step goes on from there"""
    ns = (6416, 16, 20000)
    sets, grads = R.make_sets(ns, seed=11)
    poisoned = grads[2][1].copy()
    poisoned[17000] = bad
    grads[2][1] = poisoned
    want, log = _walk_equals_ref(host_walk, tmp_path, dict(R.CFG, max_grad_norm=0.5), sets, grads)
    assert [int(s[3]) for s, _ in log] == [1, 1, 2] and [int(s[8]) for s, _ in log] == [0, 1, 1]
    assert log[1][0][7] == 0.0 and not np.isfinite(log[1][0][6]) and log[2][0][7] > 0.0
    # the same three steps without the skipped one end in the same bits
    two = [[gs[0], gs[2]] for gs in grads]
    want2, log2 = R.run_ref(dict(R.CFG, max_grad_norm=0.5), sets, two)
    for a, b in zip(want, want2):
        assert all(R.same_bits(a[k], b[k]) for k in ("w", "m", "v"))
    assert R.same_bits(log[2][0][:6], log2[1][0][:6])


def test_host_walk_lr_ptr_is_read_from_memory(host_walk, tmp_path):
    sets, grads = R.make_sets((1008,), seed=3)
    lrs = [1e-2, 0.0, 3e-3]
    cfg = dict(R.CFG, lr=float("nan"), weight_decay=0.01)      # (lr itself is not read where lr_ptr is given)
    want, _ = _walk_equals_ref(host_walk, tmp_path, cfg, sets, grads, lr_values=lrs)
    fixed, _ = R.run_ref(dict(R.CFG, lr=1e-2, weight_decay=0.01), sets, grads)
    assert not R.same_bits(want[0]["w"], fixed[0]["w"])
    one, _ = R.run_ref(dict(cfg, lr=1.0), sets, [[gs[0]] for gs in grads], lr_values=lrs[:1])
    two, _ = R.run_ref(dict(cfg, lr=1.0), sets, [gs[:2] for gs in grads], lr_values=lrs[:2])
    assert R.same_bits(one[0]["w"], two[0]["w"]) and not R.same_bits(one[0]["m"], two[0]["m"])      # lr = 0 moves m and v only
