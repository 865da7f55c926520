"""On-policy returns without a device: the NumPy restatement of THE GAE RULE against an independent float64 textbook
form, mpe_gae_segments against a brute-force count, mpe_gae's refusal ladder, the wiring checks of Values / PolicyLoop.run(values=)
/ gae_tensors, and the HOST WALK -- csrc/mpe_gae.h's per-lane function compiled by the host compiler under AddressSanitizer and
UBSan and run for every lane of every shape of the GPU sweep, so that an index that leaves a tensor is found here."""
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
from multiagent_particle_envs_amd.onpolicy import Values, gae, gae_tensors, segments
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop

import _gae_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The float32 restatement against the float64 textbook form, max over adv and ret of |x32 - x64| / max(1, |x64|), on the finite
# inputs of the sweep (every shape; random, one_agent, all_done): worst measured on the CPU 1.4527681598819342e-06; the bar is 4 x
# that.  (The chains are at most 300 steps of |delta| ~ 3 with c = 0.855: a few dozen float32 roundings of values of a few units.)
RESTATEMENT_WORST = 1.4527681598819342e-06
RESTATEMENT_BAR = 4 * RESTATEMENT_WORST      # 5.811072639527737e-06


@pytest.mark.parametrize("shape", G.SHAPES, ids=G.SHAPE_IDS)
def test_restatement_against_the_float64_textbook_form(shape):
    T, A, B, L, p = shape
    worst = 0.0
    for kind in ("random", "one_agent", "all_done"):
        rew, done, val, boot = G.make_inputs(shape, kind)
        adv, ret = G.gae(rew, done, val, boot, G.GAMMA, G.LAM, L, p)
        a64, r64 = G.gae_textbook64(rew, done, val, boot, G.GAMMA, G.LAM, L, p)
        assert adv.dtype == ret.dtype == np.float32 and adv.shape == ret.shape == (T, A, B)
        worst = max(worst, float((np.abs(adv - a64) / np.maximum(1, np.abs(a64))).max()),
                    float((np.abs(ret - r64) / np.maximum(1, np.abs(r64))).max()))
        if kind == "all_done":
            assert G.same_bits(adv, rew - val)
    print("restatement %s: worst scaled deviation %.3e (bar %.3e)" % (shape, worst, RESTATEMENT_BAR))
    assert worst <= RESTATEMENT_BAR


def test_restatement_hides_a_nonfinite_boot_behind_own_rows():
    for shape in G.SHAPES:
        T, A, B, L, p = shape
        rew, done, val, boot = G.make_inputs(shape, "nonfinite")
        assert not np.isfinite(boot).all()
        adv, ret = G.gae(rew, done, val, boot, G.GAMMA, G.LAM, L, p)
        own = done != 0
        assert np.isfinite(adv).all() and np.isfinite(ret).all()
        assert G.same_bits(adv[own], (rew - val)[own])
        enders = [t for t in range(T) if G.ends(t, T, L, p)]
        assert len(enders) == boot.shape[0]
        for k, t in enumerate(enders):      # the non-finite entries sit behind own rows only
            assert (own[t] | np.isfinite(boot[k])).all() and G.boot_index(t, T, L, p) == k


def test_segments_against_a_brute_force_count():
    L_ = _abi.lib()
    n = 0
    for T in range(1, 61):
        for L in range(0, 13):
            for p in range(max(L, 1)):
                want = G.segments_brute(T, L, p)
                assert L_.mpe_gae_segments(T, L, p) == want == G.segments(T, L, p), (T, L, p)
                n += 1
    assert n == 60 * (1 + sum(range(1, 13)))
    for bad, msg in (((0, 5, 0), "mpe_gae_segments: T = 0 steps (need at least 1)"),
                     ((3, -1, 0), "mpe_gae_segments: episode_len = -1 (need >= 0)"),
                     ((3, 5, 5), "mpe_gae_segments: episode_phase = 5 (need 0 <= phase < max(episode_len, 1) = 5)"),
                     ((3, 0, 1), "mpe_gae_segments: episode_phase = 1 (need 0 <= phase < max(episode_len, 1) = 1)"),
                     ((3, 5, -1), "mpe_gae_segments: episode_phase = -1 (need 0 <= phase < max(episode_len, 1) = 5)")):
        assert L_.mpe_gae_segments(*bad) == -1 and L_.mpe_last_error().decode() == msg
    with pytest.raises(_abi.MpeError, match="episode_phase = 7"):
        segments(4, 5, 7)
    assert segments(12, 5, 3) == 3


# ---- the refusal ladder of mpe_gae, as tests/test_abi_refusals_cpu.py writes its ladders: the call starts wrong in every checked way
# and one thing is repaired per rung; the return code and the whole message are compared at every rung.  NO RUNG PASSES EVERY CHECK
# WITH B > 0 (that call would launch a kernel on the host addresses below); the last is B == 0 -> 0, which leaves the message alone.
_HOST = (C.c_float * 16)()
PTR = C.addressof(_HOST)
GAE_LADDER = [
    ("", -1, "mpe_gae: g is NULL"),
    ("s['g'] = s['G']", -1, "mpe_gae: T = 0 steps (need at least 1)"),
    ("s['T'] = 25", -1, "mpe_gae: A = 17 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
    ("s['A'] = 0", -1, "mpe_gae: A = 0 agents (1..MPE_ACTOR_MAX_AGENTS = 16)"),
    ("s['A'] = 3", -1, "mpe_gae: B = -1"),
    ("s['B'] = 7", -1, "mpe_gae: g->gamma = inf is not finite"),
    ("s['G'].gamma = 0.95", -1, "mpe_gae: g->lambda = nan is not finite"),
    ("s['G'].lambda_ = 0.9", -1, "mpe_gae: episode_len = -1 (need >= 0)"),
    ("s['G'].episode_len = 5", -1, "mpe_gae: episode_phase = 5 (need 0 <= phase < max(episode_len, 1) = 5)"),
    ("s['G'].episode_phase = 3", -1, "mpe_gae: rew is NULL"),
    ("s['rew'] = PTR + 2", -1, "mpe_gae: done is NULL"),
    ("s['done'] = PTR + 1", -1, "mpe_gae: val is NULL"),
    ("s['val'] = PTR", -1, "mpe_gae: boot is NULL"),
    ("s['boot'] = PTR", -1, "mpe_gae: adv and ret are both NULL: the launch would write nothing"),
    ("s['ret'] = PTR", -1, "mpe_gae: rew, val, boot, adv and ret must be 4-byte aligned"),
    ("s['rew'] = PTR; s['adv'] = PTR + 1; s['ret'] = None", -1, "mpe_gae: rew, val, boot, adv and ret must be 4-byte aligned"),
    ("s['adv'] = PTR; s['B'] = 1 << 30", -1, "mpe_gae: T * A * B = 25 * 3 * 1073741824 (need A * B < 2^31 and T * A * B <= 2^40)"),
    ("s['B'] = 1 << 28; s['T'] = 1 << 12", -1, "mpe_gae: T * A * B = 4096 * 3 * 268435456 (need A * B < 2^31 and T * A * B <= 2^40)"),
    ("s['B'] = 0", 0, "mpe_gae: T * A * B = 4096 * 3 * 268435456 (need A * B < 2^31 and T * A * B <= 2^40)"),
]


def test_gae_refusal_ladder():
    L_ = _abi.lib()
    G_ = _abi.MpeGae()
    G_.gamma, G_.lambda_, G_.episode_len, G_.episode_phase = float("inf"), float("nan"), -1, 5
    s = dict(g=None, G=G_, T=0, A=17, B=-1, rew=None, done=None, val=None, boot=None, adv=None, ret=None)
    last = None
    for n, (repair, rc_want, msg_want) in enumerate(GAE_LADDER):
        exec(repair, {"PTR": PTR}, {"s": s})
        if rc_want == 0:
            assert s["B"] == 0, (n, repair)      # the hard condition: a call that is let through does no work
        rc = L_.mpe_gae(C.byref(s["g"]) if s["g"] is not None else None, s["T"], s["A"], s["B"], s["rew"], s["done"], s["val"], s["boot"],
                        s["adv"], s["ret"], None)
        msg = L_.mpe_last_error().decode()
        assert (rc, msg) == (rc_want, msg_want), "rung %d (%r)" % (n, repair)
        if rc == 0:
            assert msg == last, "a call that returns 0 leaves the last error alone"
        last = msg
    assert GAE_LADDER[-1][1] == 0 and all(r[1] != 0 for r in GAE_LADDER[:-1])
    assert L_.mpe_sizeof_gae() == C.sizeof(_abi.MpeGae) == 24


# ---- wiring -----------------------------------------------------------------------------------------------------------------------
def _mlp(D, n_out, hidden=(8,)):
    mods, k = [], D
    for h in hidden:
        mods += [nn.Linear(k, h), nn.ReLU()]
        k = h
    return nn.Sequential(*(mods + [nn.Linear(k, n_out)]))


def test_values_refusals():
    env = mpe.make_env("simple_tag", batch_size=4, device="cpu")
    widths = [int(env._obs_off[i + 1] - env._obs_off[i]) for i in range(env.n)]
    assert len(set(widths)) == 2      # the prey's and the adversaries' observations differ
    V = Values(env, [_mlp(d, 1) for d in widths])
    assert V.in_widths == widths and not V.centralised
    wts, aset = V.pack()
    assert aset.mode == _abi.MPE_POLICY_VALUE and aset.n_agents == env.n and [aset.width[i][0] for i in range(env.n)] == widths
    assert all(aset.width[i][2] == 1 for i in range(env.n)) and wts.numel() % 16 == 0
    with pytest.raises(_abi.MpeError, match="Values: agent 3's critic takes %d inputs, its observation has %d" % (widths[0], widths[3])):
        Values(env, [_mlp(widths[0], 1) for _ in widths])
    with pytest.raises(_abi.MpeError, match=r"Values: the last Linear layer gives 2 outputs \(need 1\) \[agent 1's critic: one output\]"):
        Values(env, [_mlp(d, 1 + (i == 1)) for i, d in enumerate(widths)])
    with pytest.raises(_abi.MpeError, match="Values: 2 critics for 4 agents"):
        Values(env, [_mlp(d, 1) for d in widths[:2]])
    with pytest.raises(_abi.MpeError, match="Values: hidden width 65"):
        Values(env, [_mlp(d, 1, hidden=(65,)) for d in widths])
    total = sum(widths)
    Vc = Values(env, _mlp(total, 1), centralised=True)
    assert Vc.in_widths == [total] * env.n and Vc.shared
    with pytest.raises(_abi.MpeError, match="agent 0's critic takes %d inputs, the observations together have %d" % (widths[0], total)):
        Values(env, [_mlp(d, 1) for d in widths], centralised=True)
    wide = mpe.make_env("simple_spread", batch_size=4, device="cpu", num_agents=10)
    with pytest.raises(_abi.MpeError, match=r"Values\(centralised=True\): the observations together have 600 floats.*MPE_ACTOR_MAX_INPUT = 256"):
        Values(wide, _mlp(600, 1), centralised=True)
    Values(wide, _mlp(60, 1))      # decentralised, the same env is fine
    obs = [torch.zeros((6, d)) for d in widths]
    with pytest.raises(_abi.MpeError, match="Values.v: 2 observation blocks for 4 agents"):
        V.v(obs[:2])
    with pytest.raises(_abi.MpeError, match=r"Values.v: obs_n\[3\] is a contiguous float32 \[6, %d\]" % widths[3]):
        V.v(obs[:3] + [torch.zeros((6, widths[3] + 1))])
    with pytest.raises(_abi.MpeError, match=r"Values.v: obs_n\[1\] is a contiguous float32"):
        V.v([obs[0], obs[1].double()] + obs[2:])
    ref = V.reference(obs)
    assert ref.shape == (4, 6) and ref.dtype == torch.float64
    assert Vc.reference(obs).shape == (4, 6)


def _loop_without_a_device(env, episode_len):
    """A PolicyLoop as far as run()'s argument checks look at it (the constructor allocates the env's device buffers)."""
    loop = object.__new__(PolicyLoop)
    loop.env, loop.world, loop.pi = env, env.world, Actors(env, [_mlp(18, 5) for _ in range(3)])
    loop.episode_len, loop.t, loop.obs_n = episode_len, 0, None
    return loop


def test_run_values_argument_checks():
    env = mpe.make_env("simple_spread", batch_size=4, device="cpu")
    other = mpe.make_env("simple_spread", batch_size=4, device="cpu")
    loop = _loop_without_a_device(env, 5)
    V = Values(env, [_mlp(18, 1) for _ in range(3)])
    with pytest.raises(_abi.MpeError, match="PolicyLoop.run: values= records V along the trajectory; it needs record=True"):
        loop.run(3, record=False, values=V)
    with pytest.raises(_abi.MpeError, match=r"PolicyLoop.run: values is a Values\(env, modules\) built for this loop's env"):
        loop.run(3, values=Values(other, [_mlp(18, 1) for _ in range(3)]))
    with pytest.raises(_abi.MpeError, match="PolicyLoop.run: values is a Values"):
        loop.run(3, values=[_mlp(18, 1) for _ in range(3)])
    with pytest.raises(_abi.MpeError, match=r"PolicyLoop.run\(values=\): T = 0"):
        loop.run(0, values=V)
    assert loop.t == 0      # nothing ran


def test_gae_tensor_checks_name_the_tensor():
    T, A, B, L, p = 12, 3, 7, 5, 3
    rew, val = torch.zeros((T, A, B)), torch.zeros((T, A, B))
    done, boot = torch.zeros((T, A, B), dtype=torch.bool), torch.zeros((3, A, B))
    kw = dict(gamma=0.95, lam=0.9, episode_len=L, episode_phase=p)
    with pytest.raises(_abi.MpeError, match="gae_tensors: rew is a contiguous float32 .T, A, B. tensor"):
        gae_tensors(rew.double(), done, val, boot, **kw)
    with pytest.raises(_abi.MpeError, match="gae_tensors: rew is a contiguous float32"):
        gae_tensors(rew[0], done, val, boot, **kw)
    with pytest.raises(_abi.MpeError, match="gae_tensors: rew is a contiguous float32"):
        gae_tensors(rew.transpose(1, 2), done, val, boot, **kw)
    with pytest.raises(_abi.MpeError, match=r"gae_tensors: done is a contiguous bool / uint8 \[12, 3, 7\] tensor"):
        gae_tensors(rew, done.float(), val, boot, **kw)
    with pytest.raises(_abi.MpeError, match=r"gae_tensors: val is a contiguous float32 \[12, 3, 7\] tensor"):
        gae_tensors(rew, done, val[:, :2], boot, **kw)
    with pytest.raises(_abi.MpeError, match=r"gae_tensors: boot is a contiguous float32 \[3, 3, 7\] tensor"):
        gae_tensors(rew, done, val, torch.zeros((2, A, B)), **kw)
    with pytest.raises(_abi.MpeError, match=r"gae_tensors: boot is a contiguous float32 \[1, 3, 7\] tensor"):
        gae_tensors(rew, done, val, boot, gamma=0.95, lam=0.9)
    with pytest.raises(_abi.MpeError, match="gae_tensors: gamma = nan, lam = 0.9"):
        gae_tensors(rew, done, val, boot, gamma=float("nan"), lam=0.9, episode_len=L, episode_phase=p)
    with pytest.raises(_abi.MpeError, match="mpe_gae_segments: episode_phase = 5"):
        gae_tensors(rew, done, val, boot, gamma=0.95, lam=0.9, episode_len=5, episode_phase=5)
    with pytest.raises(_abi.MpeError, match="gae_tensors: out is a GaeResult"):
        gae_tensors(rew, done, val, boot, out=(rew, rew), **kw)
    with pytest.raises(_abi.MpeError, match="gae_tensors: rew is on cpu"):      # every shape is right: the device is not
        gae_tensors(rew, done, val, boot, **kw)
    with pytest.raises(_abi.MpeError, match="gae: traj holds no values"):
        gae(object(), 0.95, 0.9)


# ---- the host walk ----------------------------------------------------------------------------------------------------------------
WALK_FLAGS = ["-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path_factory.mktemp("gae_walk") / "gae_host_walk")
    cmd = [cxx, "-std=c++17"] + WALK_FLAGS + ["-I", os.path.join(ROOT, "multiagent_particle_envs_amd", "csrc"),
                                              os.path.join(ROOT, "tests", "c", "gae_host_walk.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]
    return exe


def _walk(exe, tmp_path, shape, kind, want_adv=True, want_ret=True, scalar=False):
    T, A, B, L, p = shape
    rew, done, val, boot = G.make_inputs(shape, kind)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    G.write_walk_input(src, rew, done, val, boot, G.GAMMA, G.LAM, L, p, want_adv, want_ret, scalar)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (shape, kind, r.stdout[-500:], r.stderr[-4000:])
    return G.read_walk_output(dst, (T, A, B), want_adv, want_ret), r.stdout


@pytest.mark.parametrize("shape", G.SHAPES, ids=G.SHAPE_IDS)
def test_host_walk_every_lane_under_the_sanitizers(shape, host_walk, tmp_path):
    T, A, B, L, p = shape
    for kind in G.KINDS:
        rew, done, val, boot = G.make_inputs(shape, kind)
        adv, ret = G.gae(rew, done, val, boot, G.GAMMA, G.LAM, L, p)
        (a, r), said = _walk(host_walk, tmp_path, shape, kind)
        assert ("16-byte" in said) == (B % 4 == 0), said      # the launch's own choice of path
        assert "K = %d" % G.segments_brute(T, L, p) in said
        assert G.same_bits(a, adv) and G.same_bits(r, ret), (shape, kind)
        (a1, r1), said = _walk(host_walk, tmp_path, shape, kind, scalar=True)
        assert "scalar" in said and G.same_bits(a1, adv) and G.same_bits(r1, ret), (shape, kind, "scalar path")
    (a, none), _ = _walk(host_walk, tmp_path, shape, "random", want_ret=False)
    (none2, r), _ = _walk(host_walk, tmp_path, shape, "random", want_adv=False)
    rew, done, val, boot = G.make_inputs(shape, "random")
    adv, ret = G.gae(rew, done, val, boot, G.GAMMA, G.LAM, L, p)
    assert none is None and none2 is None and G.same_bits(a, adv) and G.same_bits(r, ret)
