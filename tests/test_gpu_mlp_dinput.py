"""mpe_mlp_dinput on the GPU: every window of every case against the float64 restatement of THE MLP INPUT GRADIENT RULE within the
project's bar (4 x the deviation of float32 torch autograd on the same GPU, floor 2 float32 ulps of the window's largest magnitude),
sentinels around and between the rows of every output on the 4-byte store path, a second launch bit-equal, a row's result as a
function of that row alone (bit for bit: alone, at another position, permuted, as part of a wider window), MADDPG's actor loss on a
real env through Trainable(Actors) -> softmax -> Trainable(Critics, input_grad=True, weight_grad=False), and the actor update's
device half inside one HIP graph.  Every index of the launch was walked on the host first (tests/test_mlp_dinput_cpu.py, whose
docstring also says why the rule adds a hidden unit's bias last and cuts its sums into four chains).

A block of two groups runs on the device too (_mlp_dinput_ref.SPAN2: M = 32769, 257 blocks, the last of one group holding one row,
with a 256-wide net whose output takes several rounds of the stage tile): the second group's P2 writes the tile the first group's last
round was stored from, with one barrier between them.  It takes the parity and the sentinel checks on three windows, and the one
launch is held, bit for bit, against rows [0, 32768) (span 1) and row 32768 run as launches of their own.  Measured on an MI355X
(profiles/mlp_dinput_parity.json): the identity holds, and the closest window stands at 0.16 of its bound (window (30, 6), agent 0:
5.2e-13, torch 8.3e-13)."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.learner import Critics
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop
from multiagent_particle_envs_amd.replay import ReplayBuffer
from multiagent_particle_envs_amd.train import Trainable, mlp_dinput_tensors, mlp_grad_tensors

import _mlp_dinput_ref as D

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
PAD = 64      # sentinel floats in front of and behind every output


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _launch(case, x, win, sentinels=False, rows=None):
    """mpe_mlp_dinput at the ABI -> (per agent the window [M, ncol_i] as NumPy, True if nothing else was written).  sentinels: ld =
    ncol + 3, 64 sentinel floats around every din, in and dout 4 bytes into their allocations (every store is 4 bytes wide); else
    contiguous outputs.  rows: run these rows of the case's inputs (an index array) in place of all M."""
    dev = _dev()
    idx = np.arange(case.M) if rows is None else np.asarray(rows)
    A, M = len(case.agents), len(idx)
    w = torch.tensor(D.pack(case, x), device=dev)
    assert w.data_ptr() % 16 == 0
    shift = 1 if sentinels else 0
    held, ins, douts = [], [], []
    for i in range(A):
        for src, dst in ((x["in"][i][idx], ins), (x["dout"][i][idx], douts)):
            flat = torch.full((src.size + shift,), SENTINEL, dtype=torch.float32, device=dev)
            flat[shift:] = torch.tensor(np.ascontiguousarray(src), device=dev).reshape(-1)
            held.append(flat)
            dst.append(flat.data_ptr() + 4 * shift)
    aset = D.fill_set(_abi.MpeActorSet(), case, w.data_ptr(), _abi.MPE_POLICY_VALUE)
    desc, bufs, ptrs = _abi.MpeMlpDinput(), [], []
    for i, (c0, nc) in enumerate(win):
        ld = nc + 3 if sentinels else nc
        desc.col0[i], desc.ncol[i], desc.ld[i] = c0, nc, ld
        buf = torch.full((PAD + shift + (M + 2) * ld + PAD,), SENTINEL, dtype=torch.float32, device=dev)
        bufs.append((buf, ld))
        ptrs.append(buf.data_ptr() + 4 * (PAD + shift))
        assert (ptrs[-1] % 16 == 0) == (not sentinels)
    _abi.check(_abi.lib().mpe_mlp_dinput(C.byref(aset), C.byref(desc), (C.c_void_p * A)(*ins), (C.c_void_p * A)(*douts), M,
                                         (C.c_void_p * A)(*ptrs), _abi.raw_stream(dev)), "mpe_mlp_dinput")
    torch.cuda.synchronize()
    got, intact = [], True
    for (buf, ld), (c0, nc) in zip(bufs, win):
        flat = buf.cpu().numpy()
        body = flat[PAD + shift:PAD + shift + (M + 2) * ld].reshape(M + 2, ld)
        intact = intact and np.all(flat[:PAD + shift] == SENTINEL) and np.all(flat[flat.size - PAD:] == SENTINEL) and \
            np.all(body[:M, nc:] == SENTINEL) and np.all(body[M:] == SENTINEL) and not np.any(body[:M, :nc] == SENTINEL)
        got.append(body[:M, :nc].copy())
    for flat, src in zip(held, [a for i in range(A) for a in (x["in"][i][idx], x["dout"][i][idx])]):      # the inputs were only read
        intact = intact and np.array_equal(flat.cpu().numpy()[shift:], np.ascontiguousarray(src).reshape(-1))
    return got, bool(intact)


_cache = {}


def _case_run(case):
    """inputs, the float64 rule, the float32 torch yardstick on this GPU and the whole-row launch of one case: computed once, left unchanged"""
    hit = _cache.get(case.name)
    if hit is None:
        x = D.make_inputs(case)
        whole, intact = _launch(case, x, D.windows(case, "whole"))
        hit = _cache[case.name] = dict(x=x, ref=D.rule64(case, x), t32=D.torch_din(case, x, torch.float32, device=_dev()), whole=whole,
                                       intact=intact)
    return hit


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


SPAN2_RUNS = [(D.SPAN2, k) for k in D.SPAN2_KINDS]
SPAN2_SENTINEL_RUNS = [(D.SPAN2, k) for k in D.SPAN2_SENTINEL_KINDS]


@pytest.mark.parametrize("case,kind", D.runs() + SPAN2_RUNS, ids=[D.run_id(r) for r in D.runs() + SPAN2_RUNS])
def test_parity_with_the_float64_restatement(case, kind):
    """Every agent's window: |kernel - float64| <= max(4 x |float32 torch autograd on this GPU - float64|, 2 ulps of the window's
    largest magnitude).  tail_bias3_M65 is the test of the tail rows and of saturated Tanh units; mixed_M65 of D = 1, 31, 32, 33, 256
    and 5, of one, two and three layers and of modules without bias.  A window's values are, bit for bit, the same columns of the
    whole-row run."""
    run = _case_run(case)
    win = D.windows(case, kind)
    got, intact = (run["whole"], run["intact"]) if kind == "whole" else _launch(case, run["x"], win)
    assert intact
    dt = D.deviations(D.cut(run["t32"], win), run["ref"], win)
    b = D.bounds(dt)
    devs = D.deviations(got, run["ref"], win)
    for i, (dev, mag) in sorted(devs.items()):
        print("%s %s agent %d window %s kernel %.3e torch %.3e bound %.3e mag %.3e" % (case.name, kind, i, win[i], dev, dt[i][0], b[i], mag))
    if os.environ.get("MPE_MLP_DINPUT_PARITY_OUT"):      # tools/mlp_dinput_parity.py
        with open(os.environ["MPE_MLP_DINPUT_PARITY_OUT"], "a") as f:
            f.write(json.dumps({"case": case.name, "window": kind, "deviation": {"agent%d" % i: {
                "cols": list(win[i]), "kernel": d, "torch_float32": dt[i][0], "bound": b[i], "largest_magnitude": m} for i, (d, m) in devs.items()}}) + "\n")
    for i, (dev, mag) in devs.items():
        assert mag > 0 and dev <= b[i], (case.name, kind, i, dev, dt[i][0], b[i], mag)
    for g, wh, (c0, nc) in zip(got, run["whole"], win):
        assert np.array_equal(_bits(g), _bits(wh[:, c0:c0 + nc])), (case.name, kind)


@pytest.mark.parametrize("case,kind", D.runs() + SPAN2_SENTINEL_RUNS, ids=[D.run_id(r) for r in D.runs() + SPAN2_SENTINEL_RUNS])
def test_sentinels_and_a_second_run_on_the_four_byte_path(case, kind):
    """ld = ncol + 3, 64 sentinel floats around every din, two sentinel rows behind row M - 1, in and dout 4 bytes into their
    allocations: nothing outside the windows changes, the inputs are only read, two runs are bit-equal, and the values are those of
    the 16-byte path."""
    run = _case_run(case)
    win = D.windows(case, kind)
    a, intact_a = _launch(case, run["x"], win, sentinels=True)
    b, intact_b = _launch(case, run["x"], win, sentinels=True)
    assert intact_a and intact_b
    for ga, gb, wh, (c0, nc) in zip(a, b, run["whole"], win):
        assert np.array_equal(_bits(ga), _bits(gb)) and np.array_equal(_bits(ga), _bits(wh[:, c0:c0 + nc]))


def test_a_row_depends_on_that_row_alone_bit_for_bit():
    """critics_M129, the whole row: row r run alone (M = 1), row r at position 0 of an M = 65 batch of other rows, and a permutation
    of all rows give row r's bits of the M = 129 run."""
    case = D.CASES[4]
    assert case.name == "critics_M129"
    run = _case_run(case)
    win = D.windows(case, "whole")
    for r in (0, 31, 63, 64, 128):
        alone, ok = _launch(case, run["x"], win, rows=[r])
        assert ok
        others = [k for k in range(case.M) if k != r][:64]
        first, ok = _launch(case, run["x"], win, rows=[r] + others)
        assert ok and len(others) == 64
        for i in range(len(case.agents)):
            assert np.array_equal(_bits(alone[i][0]), _bits(run["whole"][i][r])), (r, i)
            assert np.array_equal(_bits(first[i]), _bits(run["whole"][i][[r] + others])), (r, i)
    perm = np.random.RandomState(3).permutation(case.M)
    got, ok = _launch(case, run["x"], win, rows=perm)
    assert ok and all(np.array_equal(_bits(g), _bits(wh[perm])) for g, wh in zip(got, run["whole"]))


def test_a_block_of_two_groups_is_its_groups_run_apart_bit_for_bit():
    """span2_M32769, the whole row: 257 blocks of two groups, the last of one group holding one row.  A row's result depends on that
    row alone, so the one launch equals, bit for bit, rows [0, 32768) run as a launch of their own (span 1, 512 blocks of one group)
    followed by row 32768 run alone -- unless a block's second group meets what its first left in the tiles."""
    case = D.SPAN2
    assert (D.span(case.M), D.blocks(case.M), D.span(case.M - 1), D.blocks(case.M - 1)) == (2, 257, 1, 512)
    run = _case_run(case)
    win = D.windows(case, "whole")
    head, ok_h = _launch(case, run["x"], win, rows=np.arange(case.M - 1))
    tail, ok_t = _launch(case, run["x"], win, rows=[case.M - 1])
    assert run["intact"] and ok_h and ok_t
    for i in range(len(case.agents)):
        assert np.array_equal(_bits(run["whole"][i]), _bits(np.concatenate([head[i], tail[i]]))), i


# ---- behind torch autograd, on a real env ---------------------------------------------------------------------------------------------
def _mlp(n_in, n_out):
    """Tanh nets: the test compares gradients with float64, and a ReLU unit within rounding of 0 would flip between the two"""
    return nn.Sequential(nn.Linear(n_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, n_out)).cuda()


@pytest.fixture(scope="module")
def spread():
    """simple_spread N = 3, 4 worlds, a filled replay ring, one joint batch of 65 transitions"""
    torch.manual_seed(11)
    env = mpe.make_env("simple_spread", batch_size=4, seed=5)
    buf = ReplayBuffer(env, steps=50)
    mu = [_mlp(w, 5) for w in buf.obs_widths]
    qs = [_mlp(buf.joint_width, 1) for _ in range(env.n)]
    PolicyLoop(env, Actors(env, mu, mode="sample", seed=2), episode_len=25).run(50, record=False, replay=buf)
    batch = buf.sample(65, draw=0, joint=True)
    col = Actors(env, mu, mode="softmax").col_move
    return dict(env=env, buf=buf, mu=mu, qs=qs, batch=batch, col=col, obs_n=[o.clone() for o in batch.obs_n], joint=batch.joint.clone())


def _torch_actor_grads(s, dtype):
    """the example's actor loss in plain torch -> the actors' parameter gradients, float64 NumPy"""
    mu, qs = [copy.deepcopy(m).to(dtype) for m in s["mu"]], [copy.deepcopy(m).to(dtype) for m in s["qs"]]
    loss = 0.0
    for i in range(3):
        joint = s["joint"].to(dtype).clone()
        joint[:, s["col"][i]:s["col"][i] + 5] = F.softmax(mu[i](s["obs_n"][i].to(dtype)), dim=1)
        loss = loss - qs[i](joint).mean()
    loss.backward()
    return [p.grad.double().cpu().numpy() for m in mu for p in m.parameters()], float(loss.detach())


def test_maddpg_actor_loss_through_the_critics(spread):
    """-Q_i(joint with agent i's action columns replaced by softmax(mu_i(obs_i))), i = 0..2, M = 65: Trainable(Actors, logits=True),
    torch's softmax and column write, Trainable(Critics, input_grad=True, weight_grad=False, cols=...).  Every actor parameter's
    .grad is within 4 x float32 torch's own deviation from the float64 chain (floor 2 ulps); the critics' parameters get none."""
    s = spread
    ref, loss64 = _torch_actor_grads(s, torch.float64)
    t32, _ = _torch_actor_grads(s, torch.float32)
    mu, qs = [copy.deepcopy(m) for m in s["mu"]], [copy.deepcopy(m) for m in s["qs"]]
    pi = Trainable(Actors(s["env"], mu, mode="softmax", logits=True))
    qc = Trainable(Critics(s["env"], qs), input_grad=True, weight_grad=False, cols=[(c, 5) for c in s["col"]])
    logits = pi(s["obs_n"])
    joints = []
    for i in range(3):
        joint = s["joint"].clone()
        joint[:, s["col"][i]:s["col"][i] + 5] = F.softmax(logits[i], dim=1)
        joints.append(joint)
    q = qc(joints)
    loss = -sum(q[i].mean() for i in range(3))
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - loss64) <= 1e-5 * max(1.0, abs(loss64))
    assert all(p.grad is None for m in qs for p in m.parameters()) and qc.last_grad is None
    params = [p for m in mu for p in m.parameters()]
    for k, (p, r, t) in enumerate(zip(params, ref, t32)):
        bound = max(4 * float(np.abs(t - r).max()), 2 * float(np.spacing(np.float32(np.abs(r).max()))))
        dev = float(np.abs(p.grad.double().cpu().numpy() - r).max())
        print("actor tensor %d: deviation %.3e (torch %.3e, bound %.3e, largest %.3e)" % (k, dev, float(np.abs(t - r).max()), bound, float(np.abs(r).max())))
        assert float(np.abs(r).max()) > 0 and dev <= bound, (k, dev, bound)


def test_input_and_weight_gradients_of_one_shared_joint_tensor(spread):
    """input_grad=True, weight_grad=True on ONE joint tensor every critic reads: the parameters get mpe_mlp_grad's gradients, the
    tensor the agents' windows added in ascending agent order, zeros outside them, in a tensor of its own."""
    s = spread
    qs = [copy.deepcopy(m) for m in s["qs"]]
    net = Critics(s["env"], qs)
    cols = [(0, 7), (3, 9), (s["col"][2], 5)]      # two windows overlap
    qc = Trainable(net, input_grad=True, cols=cols)
    joint = s["joint"].clone().requires_grad_()
    gout = [torch.full((65,), 0.25 * (i + 1), device=joint.device) for i in range(3)]
    q = qc(joint)
    torch.autograd.backward(q, gout)
    torch.cuda.synchronize()
    want_w = mlp_grad_tensors(net, joint.detach(), gout)
    for (m_views, m) in zip(want_w.modules, qs):
        lins = [l for l in m if isinstance(l, nn.Linear)]
        for (w, b), lin in zip(m_views, lins):
            assert torch.equal(lin.weight.grad, w) and torch.equal(lin.bias.grad, b)
    assert qc.last_grad is want_w
    din = [d.clone() for d in mlp_dinput_tensors(net, joint.detach(), gout, cols=cols)]
    want = torch.zeros_like(joint)
    for d, (c0, nc) in zip(din, cols):
        want[:, c0:c0 + nc] += d
    assert torch.equal(joint.grad, want) and float(joint.grad[:, 12:s["col"][2]].abs().max()) == 0 and float(joint.grad.abs().max()) > 0
    first = joint.grad.clone()
    torch.autograd.backward(qc(joint), gout)      # accumulated into, not aliased
    assert torch.equal(joint.grad, 2 * first)
    # and against float32 torch autograd of the same function
    tj = s["joint"].clone().requires_grad_()
    tq = []
    for i, (c0, nc) in enumerate(cols):      # only the window's columns of critic i's input carry gradient
        m_i = torch.zeros_like(tj)
        m_i[:, c0:c0 + nc] = 1
        tq.append(s["qs"][i](tj * m_i + (tj * (1 - m_i)).detach())[:, 0])
    torch.autograd.backward(tq, gout)
    assert float((tj.grad - first).abs().max()) <= 1e-5 * float(first.abs().max())


# ---- inside a HIP graph -------------------------------------------------------------------------------------------------------------
def test_actor_update_in_one_graph(spread):
    """{Actors.act_rows (logits), softmax, the column writes into three copies of the joint rows, Critics.q on the three, the backward:
    mlp_dinput_tensors over the action columns, the softmax Jacobian, mlp_grad_tensors of the actors} captured on one stream and
    replayed twice on refreshed inputs: bit for bit what the eager sequence gives on the same inputs."""
    s = spread
    env, dev, M = s["env"], s["joint"].device, 65
    pi, qc = Actors(env, s["mu"], mode="softmax", logits=True).freeze(), Critics(env, s["qs"]).freeze()
    cols = [(c, 5) for c in s["col"]]
    obs_n, joint = [o.clone() for o in s["obs_n"]], s["joint"].clone()
    joints = [torch.zeros_like(joint) for _ in range(3)]
    dq = [torch.full((M,), -1.0 / M, device=dev) for _ in range(3)]
    dlogits = [torch.zeros((M, 5), device=dev) for _ in range(3)]

    def call():
        pi.act_rows(obs_n)
        for i in range(3):
            p = F.softmax(pi.rows.logits[i, :, :5], dim=1)
            joints[i].copy_(joint)
            joints[i][:, cols[i][0]:cols[i][0] + 5] = p
        q = qc.q(joints)
        dp = mlp_dinput_tensors(qc, joints, dq, cols=cols)
        for i in range(3):
            p = joints[i][:, cols[i][0]:cols[i][0] + 5]
            dlogits[i].copy_(p * (dp[i] - (p * dp[i]).sum(dim=1, keepdim=True)))
        return q, dp, mlp_grad_tensors(pi, obs_n, dlogits)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(st):
            q, dp, ga = call()      # the code objects and the buffers outside the capture
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st):
                q1, dp1, ga1 = call()
                assert q1 is q and ga1 is ga and all(a.data_ptr() == b.data_ptr() for a, b in zip(dp, dp1))
        torch.cuda.current_stream().wait_stream(st)
        for draw in (1, 2):
            b = s["buf"].sample(M, draw=draw, joint=True)
            for dst, src in zip(obs_n + [joint], list(b.obs_n) + [b.joint]):
                dst.copy_(src)
            ga.packed.fill_(SENTINEL)
            graph.replay()
            torch.cuda.synchronize()
            snap = [t.clone() for t in [q, ga.packed] + list(dp)]
            assert float(snap[1].abs().max()) > 0 and not bool((snap[1] == SENTINEL).any())
            q2, dp2, ga2 = call()
            torch.cuda.synchronize()
            for a, b_ in zip(snap, [q2, ga2.packed] + list(dp2)):
                assert torch.equal(a.view(torch.int32), b_.view(torch.int32))
        assert not torch.equal(snap[0], torch.zeros_like(snap[0]))
    finally:
        pi.unfreeze(), qc.unfreeze()
