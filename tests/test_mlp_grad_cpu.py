"""The MLP weight gradients without a GPU: the float64 restatement of THE MLP GRADIENT RULE against torch float64 autograd, the
ReLU select at exactly 0, every refusal of the two entry points in the header's order, the host layer's argument checks, the host
walk of every chunk, wave, lane and step of both launches under the sanitizers (tests/c/mlp_grad_host_walk.cpp), and the band
condition of the GPU test's fixed inputs."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.train import MlpGradResult, Trainable, mlp_grad_tensors

import _mlp_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x10000      # a plausible, 16-byte aligned address (no refused call reads it)
EXTRA = [R.case("one_two_three_layers_nobias_shared_M37",
                [R.Net(7, (), 3, "tanh", True), R.Net(9, (11,), 4, "relu", False), R.Net(5, (6, 7), 2, "tanh", False),
                 R.Net(5, (6, 7), 2, "relu", True)], [0, 1, 2, 3, 2, 1], 37, 5)]


# ---- (a) against torch float64 autograd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GPU_CASES + EXTRA, ids=R.GPU_IDS + [c.name for c in EXTRA])
def test_restatement_is_torch_float64_autograd(case):
    """1, 2 and 3 layers, Tanh and ReLU, shared modules (torch accumulates over the agents too) and bias=False: every block within
    1e-12 of its largest magnitude."""
    x = R.make_inputs(case)
    ref, t64 = R.rule64(case, x), R.torch_grads(case, x, torch.float64)
    devs = R.deviations(case, t64, ref)
    assert len(devs) >= 2 * len(set(case.agents)) - sum(not case.nets[m].bias for m in set(case.agents))
    for key, (dev, mag) in devs.items():
        assert dev <= 1e-12 * mag, (case.name, key, dev, mag)


def test_relu_select_is_taken_on_the_output_and_zero_gets_zero():
    """torch's ReLU backward is grad * (output > 0): a unit at exactly 0 passes nothing, and so does the restatement."""
    z = torch.tensor([-1.0, 0.0, 2.0], dtype=torch.float64, requires_grad=True)
    torch.relu(z).backward(torch.tensor([5.0, 7.0, 11.0], dtype=torch.float64))
    assert z.grad.tolist() == [0.0, 0.0, 11.0]
    net = R.Net(2, (3,), 1, "relu", True)
    W0 = np.array([[1, 0, -1], [0, 0, 1]], R.F32)      # row (1, 1): pre-activations 1 + b, exactly 0, 0 + b
    params = [(W0, np.array([0.5, 0.0, -3.0], R.F32)), (np.array([[2.0], [3.0], [4.0]], R.F32), np.zeros(1, R.F32))]
    g = R.agent_grads64(net, params, np.ones((1, 2), R.F32), np.ones((1, 1), R.F32))
    assert g[0][1].tolist() == [2.0, 0.0, 0.0] and g[0][0].tolist() == [[2.0, 0.0, 0.0], [2.0, 0.0, 0.0]]
    assert g[1][0][:, 0].tolist() == [1.5, 0.0, 0.0]


# ---- refusals: one ladder per entry point, the order include/mpe_hip.h states -------------------------------------------------------
def _set(s):
    if s["set"] is None:
        return None
    a = _abi.MpeActorSet()
    a.n_agents, a.mode, a.weights = s["A"], s["mode"], s["weights"]
    for i in range(16):
        a.n_layers[i], a.activation[i], a.offset[i] = s["nl"][i], s["act"][i], s["off"][i]
        for l in range(4):
            a.width[i][l] = s["width"][i][l]
    return a


def _state():
    return dict(set=None, A=0, mode=7, weights=None, nl=[0] * 16, act=[5] * 16, off=[-16] * 16, width=[[0, 0, 0, 0] for _ in range(16)],
                M=-1, in_ptrs=None, dout_ptrs=None, ins=[None] * 16, douts=[None] * 16, grad=None, work=None)


def _ladder(P_):
    return [
        ("pass", -1, P_ + "set is NULL"),
        ("s['set'] = 1", -1, P_ + "n_agents = 0 (1..MPE_ACTOR_MAX_AGENTS = 16)"),
        ("s['A'] = 17", -1, P_ + "n_agents = 17 (1..MPE_ACTOR_MAX_AGENTS = 16)"),
        ("s['A'] = 3", -1, P_ + "mode 7 (MPE_POLICY_GREEDY / SAMPLE / SOFTMAX / VALUE)"),
        ("s['mode'] = 3", -1, P_ + "agent 0 has 0 Linear layers (1..3)"),
        ("s['nl'] = [3, 4, 3] + [0] * 13", -1, P_ + "agent 0: activation 5 (MPE_POLICY_RELU / TANH)"),
        ("s['act'] = [1] * 16", -1, P_ + "agent 0: input width 0 (1..MPE_ACTOR_MAX_INPUT = 256)"),
        ("s['width'][0] = [257, 65, 0, 17]", -1, P_ + "agent 0: input width 257 (1..MPE_ACTOR_MAX_INPUT = 256)"),
        ("s['width'][0][0] = 18", -1, P_ + "agent 0: hidden width 65 (1..MPE_POLICY_MAX_WIDTH = 64)"),
        ("s['width'][0][1] = 64", -1, P_ + "agent 0: hidden width 0 (1..MPE_POLICY_MAX_WIDTH = 64)"),
        ("s['width'][0][2] = 64", -1, P_ + "agent 0: the last layer gives 17 outputs (1..MPE_ACTOR_MAX_OUT = 16)"),
        ("s['width'][0][3] = 5", -1, P_ + "agent 0: offset -16 (a non-negative multiple of 16 floats, the block's end below 2^31)"),
        ("s['off'][0] = 8", -1, P_ + "agent 0: offset 8 (a non-negative multiple of 16 floats, the block's end below 2^31)"),
        ("s['off'][0] = 0x7fffffe0", -1, P_ + "agent 0: offset 2147483616 (a non-negative multiple of 16 floats, the block's end below 2^31)"),
        ("s['off'][0] = 0", -1, P_ + "agent 1 has 4 Linear layers (1..3)"),
        ("s['nl'][1] = 3; s['width'][1] = [18, 64, 64, 5]; s['width'][2] = [18, 64, 33, 5]; s['off'][1] = 6416; s['off'][2] = 0", -1,
         P_ + "agents 0 and 2 share offset 0 with different shapes (layers, widths or activation)"),
        ("s['width'][2] = [18, 64, 64, 5]; s['act'][2] = 0", -1, P_ + "agents 0 and 2 share offset 0 with different shapes (layers, widths or activation)"),
        ("s['act'][2] = 1; s['off'][1] = 6400", -1, P_ + "the blocks of agents 0 and 1 overlap (offsets 0 and 6400: a module is shared whole, at equal offsets, or not at all)"),
        ("s['off'][1] = 6416", -1, P_ + "M = -1"),
        ("s['M'] = 1 << 31", -1, P_ + "M = 2147483648 (need M < 2^31)"),
    ]


GRAD_LADDER = _ladder("mpe_mlp_grad: ") + [
    ("s['M'] = 65", -1, "mpe_mlp_grad: set->weights is NULL or not 16-byte aligned"),
    ("s['weights'] = PTR + 8", -1, "mpe_mlp_grad: set->weights is NULL or not 16-byte aligned"),
    ("s['weights'] = PTR", -1, "mpe_mlp_grad: in_ptrs is NULL"),
    ("s['in_ptrs'] = 1", -1, "mpe_mlp_grad: dout_ptrs is NULL"),
    ("s['dout_ptrs'] = 1", -1, "mpe_mlp_grad: grad is NULL"),
    ("s['grad'] = PTR", -1, "mpe_mlp_grad: work is NULL"),
    ("s['work'] = PTR", -1, "mpe_mlp_grad: in_ptrs[0] is NULL"),
    ("s['ins'] = [PTR, PTR, None] + [None] * 13", -1, "mpe_mlp_grad: dout_ptrs[0] is NULL"),
    ("s['douts'] = [PTR] * 16", -1, "mpe_mlp_grad: in_ptrs[2] is NULL"),
    ("s['ins'][2] = PTR + 2", -1, "mpe_mlp_grad: every pointer must be 4-byte aligned"),
    ("s['ins'][2] = PTR + 4; s['douts'][1] = PTR + 1", -1, "mpe_mlp_grad: every pointer must be 4-byte aligned"),
    ("s['douts'][1] = PTR + 4; s['grad'] = PTR + 3", -1, "mpe_mlp_grad: every pointer must be 4-byte aligned"),
    ("s['grad'] = PTR + 4; s['work'] = PTR + 6", -1, "mpe_mlp_grad: every pointer must be 4-byte aligned"),
]


def _climb(ladder, state, call):
    L_ = _abi.lib()
    for n, (repair, rc_want, msg_want) in enumerate(ladder):
        exec(repair, {"PTR": PTR}, {"s": state})
        rc = call(state)
        msg = L_.mpe_last_error().decode()
        assert (rc, msg) == (rc_want, msg_want), "rung %d (%r): %d %s" % (n, repair, rc, msg)


def _grad_call(s):
    a = _set(s)
    arr = lambda on, v: (C.c_void_p * 16)(*v) if on else None      # noqa: E731
    return _abi.lib().mpe_mlp_grad(C.byref(a) if a is not None else None, arr(s["in_ptrs"], s["ins"]), arr(s["dout_ptrs"], s["douts"]),
                                   s["M"], s["grad"], s["work"], None)


def test_mlp_grad_refusal_ladder():
    """Every rung refuses before any launch (no rung's pointers are real), in the header's order."""
    _climb(GRAD_LADDER, _state(), _grad_call)


def test_mlp_grad_work_refusal_ladder_and_counts():
    s = _state()
    _climb(_ladder("mpe_mlp_grad_work: "), s, lambda st: _abi.lib().mpe_mlp_grad_work(C.byref(_set(st)) if st["set"] else None, st["M"]))
    L_ = _abi.lib()
    size = 19 * 64 + 65 * 64 + 65 * 16
    assert size == R.module_size(R.ACTOR) == 6416
    for M, chunks, per in ((0, 0, 64), (1, 1, 64), (64, 1, 64), (65, 2, 64), (64 * 128, 128, 64), (64 * 128 + 1, 65, 128), (409600, 128, 3200)):
        s["M"] = M
        assert (R.chunks(M), R.span(M) * 64) == (chunks, per)
        assert L_.mpe_mlp_grad_work(C.byref(_set(s)), M) == 3 * (size + 144) * chunks      # (weights NULL: host only, not read)
    assert [(R.groups(c.M), R.span(c.M), R.chunks(c.M)) for c in R.SPAN_CASES] == [(131, 2, 66), (257, 3, 86), (131, 2, 66)]
    for c in R.GPU_CASES + R.SPAN_CASES + [R.WALK_EXTRA]:
        a = R.fill_set(_abi.MpeActorSet(), c, None, _abi.MPE_POLICY_VALUE if c.value else _abi.MPE_POLICY_GREEDY)
        assert L_.mpe_mlp_grad_work(C.byref(a), c.M) == R.work_floats(c), c.name


# ---- the host layer -----------------------------------------------------------------------------------------------------------------
class _Agent(object):
    movable, silent = True, True


class _World(object):
    def __init__(self, A, B):
        self.agents, self.batch_size, self.dim_c, self.device, self.world_offset = [_Agent() for _ in range(A)], B, 0, torch.device("cpu"), 0


class _Env(object):
    def __init__(self, A, D, B=4):
        self.world, self._obs_off = _World(A, B), [i * D for i in range(A + 1)]


def _actor(D=18, n=5, bias=True):
    import torch.nn as nn
    return nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, 64, bias=bias), nn.Tanh(), nn.Linear(64, n))


def test_host_layer_checks_name_the_argument():
    assert set(("Trainable", "MlpGradResult", "mlp_grad_tensors")) <= set(mpe.__all__)
    who = "mlp_grad_tensors: "
    env = _Env(2, 18)
    pi = mpe.Actors(env, [_actor(), _actor()], logits=True)
    V = mpe.Values(env, _actor(n=1))
    M, f = 6, torch.float32
    ok_in, ok_d = [torch.zeros((M, 18), dtype=f) for _ in range(2)], [torch.zeros((M, 5), dtype=f) for _ in range(2)]

    def refuses(msg, *a, **k):
        with pytest.raises(_abi.MpeError) as e:
            mlp_grad_tensors(*a, **k)
        assert str(e.value) == msg, str(e.value)
    refuses(who + "net is an Actors, a Values or a Critics (got list)", [], ok_in, ok_d)
    refuses(who + "in_n is a list of 2 tensors, one per agent, or one tensor every agent reads", pi, ok_in[:1], ok_d)
    refuses(who + "dout_n is a list of 2 tensors, one per agent", pi, ok_in, ok_d + ok_d)
    refuses(who + "in_n[0] is a contiguous float32 [M, 18] tensor on a GPU", pi, [None, ok_in[1]], ok_d)
    refuses(who + "in_n[1] is a contiguous float32 [6, 18] tensor on in_n[0]'s device", pi, [ok_in[0], torch.zeros((M, 17), dtype=f)], ok_d)
    refuses(who + "in_n[1] is a contiguous float32 [6, 18] tensor on in_n[0]'s device", pi, [ok_in[0], ok_in[1].double()], ok_d)
    refuses(who + "dout_n[0] is a contiguous float32 [6, 5] tensor on in_n[0]'s device", pi, ok_in, [torch.zeros((M, 16), dtype=f)[:, :5], ok_d[1]])
    refuses(who + "dout_n[1] is a contiguous float32 [6, 5] tensor on in_n[0]'s device", pi, ok_in, [ok_d[0], torch.zeros((M,), dtype=f)])
    refuses(who + "dout_n[0] is a contiguous float32 [6, 1] or [6] tensor on in_n[0]'s device", V, ok_in, ok_d)
    refuses(who + "in_n[0] is on cpu (the tensors live on a GPU: there is no CPU path)", pi, ok_in, ok_d)
    refuses(who + "in_n[0] is on cpu (the tensors live on a GPU: there is no CPU path)", V, ok_in, [torch.zeros((M,), dtype=f), torch.zeros((M, 1), dtype=f)])
    refuses(who + "in_n[0] is on cpu (the tensors live on a GPU: there is no CPU path)", pi, ok_in, ok_d, out=MlpGradResult())


def test_trainable_checks_its_arguments():
    env = _Env(2, 18)
    with pytest.raises(_abi.MpeError, match="net is an Actors, a Values or a Critics"):
        Trainable(_actor())
    with pytest.raises(_abi.MpeError, match="built without logits=True"):
        Trainable(mpe.Actors(env, [_actor(), _actor()]))
    shared = _actor(bias=False)
    t = Trainable(mpe.Actors(env, shared, logits=True))
    assert len(t.parameters()) == 5 and all(p is q for p, q in zip(t.parameters(), shared.parameters()))      # one copy; no bias of layer 1
    t = Trainable(mpe.Values(env, [_actor(n=1), _actor(n=1)]))
    assert len(t.parameters()) == 12
    x = [torch.zeros((3, 18)), torch.zeros((3, 18), requires_grad=True)]
    with pytest.raises(_abi.MpeError, match=r"obs_n\[1\] requires grad.*there is no dL/din"):
        t(x)


# ---- the host walk --------------------------------------------------------------------------------------------------------------------
WALK_FLAGS = ["-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path_factory.mktemp("mlp_grad_walk") / "mlp_grad_host_walk")
    cmd = [cxx, "-std=c++17"] + WALK_FLAGS + ["-I", os.path.join(ROOT, "multiagent_particle_envs_amd", "csrc"),
                                              os.path.join(ROOT, "tests", "c", "mlp_grad_host_walk.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]
    return exe


def _walk(exe, tmp_path, case):
    x = R.make_inputs(case)
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    R.write_walk_input(src, case, x)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (case.name, r.stdout[-500:], r.stderr[-4000:])
    assert "%d chunks of %d groups, %d floats of workspace" % (R.chunks(case.M), R.span(case.M), R.work_floats(case)) in r.stdout
    got, pad = R.unpack(case, R.read_walk_output(dst, case))
    assert pad.size and not pad.view(np.uint32).any(), "a padding entry is not +0.0f"
    ref = R.rule64(case, x)
    b = R.bounds(R.deviations(case, R.torch_grads(case, x, torch.float32), ref))
    for key, (dev, mag) in R.deviations(case, got, ref).items():
        assert dev <= b[key], (case.name, key, dev, b[key], mag)


@pytest.mark.parametrize("case", R.GPU_CASES, ids=R.GPU_IDS)
def test_host_walk_every_chunk_wave_and_lane_under_the_sanitizers(case, host_walk, tmp_path):
    """Both launches of every GPU case's shape on exact-size heap buffers (LDS arrays included), the MFMA replaced by its definition:
    what they wrote against the restatement within the GPU test's bound (4 x the deviation of float32 torch autograd on the same
    inputs, here on the CPU; floor 2 ulps), padding +0.0f, every float of work written once, no LDS float shared across lanes
    between two barriers."""
    _walk(host_walk, tmp_path, case)


def test_host_walk_most_chunks_and_a_span_of_two_groups(host_walk, tmp_path):
    """M = 64 * 128 + 65: 130 groups in 65 chunks of 2.  (The second launch stages nothing: a lane adds its entry's partials
    straight from work, so there is no piece to exceed; this walk takes the longest sum a lane of this span has.)"""
    assert (R.chunks(R.WALK_EXTRA.M), R.span(R.WALK_EXTRA.M)) == (65, 2)
    _walk(host_walk, tmp_path, R.WALK_EXTRA)


# ---- the fixture condition of the ReLU cases --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GPU_CASES + R.SPAN_CASES, ids=R.GPU_IDS + R.SPAN_IDS)
def test_no_relu_row_is_in_the_band(case):
    """A ReLU unit whose pre-activation lies within 1e-4 of 0 can flip between float32 and float64 and change the gradient by its
    whole contribution: make_inputs redraws such rows, and none is left."""
    x = R.make_inputs(case)
    n_relu = 0
    for i, m in enumerate(case.agents):
        net = case.nets[m]
        if net.act != "relu" or not net.hidden:
            continue
        n_relu += 1
        _, pre = R.forward64(net, x["params"][m], x["in"][i])
        assert min(float(np.abs(z).min()) for z in pre) >= R.BAND, (case.name, i)
    assert x["redrawn"] <= max(2, 0.05 * case.M * max(n_relu, 1)), (case.name, x["redrawn"])
