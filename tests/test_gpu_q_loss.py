"""The value-based learners' loss head on the GPU: mpe_q_loss BIT-EQUAL to the float32 restatement of
tests/_q_loss_ref.py on every shape, mix and target, at 16-byte aligned and unaligned gradient bases, sentinels around every gradient
block; a row's bits at any position and any M; QLoss's parameter gradients through Trainable within the project's parity bound (4 x
float32 torch autograd's deviation from the float64 chain on this GPU, floor 2 ulps); the prioritized buffer's round trip; a whole
update captured as ONE HIP graph; and the example's --device-update mode against its torch path.

The closest ratio to the parity bound is written to $MPE_Q_LOSS_PARITY_OUT when that is set (profiles/q_loss_parity.json)."""
import copy
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.learner import QLoss, QTargets, q_loss_tensors
from multiagent_particle_envs_amd.optim import DeviceAdam
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop
from multiagent_particle_envs_amd.replay import PrioritizedReplayBuffer, ReplayBuffer
from multiagent_particle_envs_amd.train import Trainable, mlp_grad_tensors

import _q_loss_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -777.25
PAD = 64      # sentinel floats (256 bytes: the 16-byte alignment stays) in front of and behind a gradient block
CASE_IDS = sorted(R.CASES)
PARITY = {}


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    return torch.tensor(np.asarray(a), device=_dev())


def _bits(t):
    return t.view(torch.int32)


@pytest.fixture(scope="module", autouse=True)
def _parity_out():
    yield
    if os.environ.get("MPE_Q_LOSS_PARITY_OUT"):
        with open(os.environ["MPE_Q_LOSS_PARITY_OUT"], "w") as f:
            f.write(json.dumps({"device": torch.cuda.get_device_name(0), "largest_fraction_of_bound": max(PARITY.values()) if PARITY else None,
                                "fraction_of_bound": PARITY}) + "\n")


class _Call(object):
    """the device tensors of one case's inputs, and mpe_q_loss on them through the C entry point"""

    def __init__(self, case, x):
        self.case, self.M = case, x["ret"].shape[1]
        self.t = {k: _t(x[k]) for k in ("nt", "no", "act", "utter", "ret", "done", "discount", "w")}
        self.q_n = [_t(z) for z in x["q_n"]]

    def run(self, mix, double, weighted, nstep, off=0):
        """-> dict of NumPy outputs; dq at PAD + off floats into over-allocated blocks whose sentinels are checked"""
        case, M, t, dev = self.case, self.M, self.t, _dev()
        A = case.A
        raw = [torch.full((PAD + off + M * n + PAD,), SENTINEL, dtype=torch.float32, device=dev) for n in case.n]
        dq = [r[PAD + off:PAD + off + M * n] for r, n in zip(raw, case.n)]
        o = dict(q_taken=torch.zeros((A, M), device=dev), y=torch.zeros((A, M), device=dev), td_abs=torch.zeros(M, device=dev),
                 stats=torch.full((A, 8), SENTINEL, device=dev), loss=torch.zeros(1, device=dev))
        work = torch.empty(max(int(_abi.lib().mpe_q_loss_work(A, M)), 1), dtype=torch.float64, device=dev)
        cfg, td = _abi.MpeQLoss(), _abi.MpeTdTarget()
        cfg.n_agents, cfg.dim_c, cfg.mix = A, case.dim_c, mix
        for i in range(A):
            cfg.movable[i], cfg.speaks[i] = int(case.movable[i]), int(case.speaks[i])
        td.ret, td.done, td.discount, td.gamma = t["ret"].data_ptr(), t["done"].data_ptr(), t["discount"].data_ptr() if nstep else None, R.GAMMA
        ptr = lambda ts: (C.c_void_p * A)(*[x_.data_ptr() for x_ in ts])      # noqa: E731
        _abi.check(_abi.lib().mpe_q_loss(
            C.byref(cfg), ptr(self.q_n), t["nt"].data_ptr(), t["no"].data_ptr() if double else None, t["act"].data_ptr(),
            t["utter"].data_ptr() if case.dim_c else None, C.byref(td), t["w"].data_ptr() if weighted else None, M, ptr(dq),
            o["q_taken"].data_ptr(), o["y"].data_ptr(), o["td_abs"].data_ptr(), work.data_ptr(), o["stats"].data_ptr(), o["loss"].data_ptr(),
            _abi.raw_stream(dev)), "mpe_q_loss")
        torch.cuda.synchronize()
        for r, n in zip(raw, case.n):
            h = r.cpu().numpy()
            assert np.all(h[:PAD + off] == SENTINEL) and np.all(h[PAD + off + M * n:] == SENTINEL), "a float outside a gradient block was written"
        out = {k: v.cpu().numpy() for k, v in o.items()}
        out["dq_n"] = [d.cpu().numpy().reshape(M, n) for d, n in zip(dq, case.n)]
        out["loss"] = out["loss"][0]
        return out


def _assert_equal(got, want, tag):
    for i, (a, b) in enumerate(zip(got["dq_n"], want["dq_n"])):
        assert R.same_bits(a, b), tag + ("dq", i)
        assert not np.signbit(a[a == 0]).any(), tag + ("dq holds a -0.0", i)
    for k in ("q_taken", "y", "td_abs", "stats", "loss"):
        assert R.same_bits(got[k], want[k]), tag + (k,)


# ---- bit-equal to the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("name", CASE_IDS)
@pytest.mark.parametrize("M", R.ROWS)
def test_q_loss_bit_equal_to_the_restatement(M, name, nan):
    """both mixes, plain and double-Q, with and without weights and per-row discounts, dq bases 16-byte aligned and 4 bytes off: every
    output's bits are the restatement's.  The inputs hold argmax ties in S and in the action rows, all-done and no-done rows,
    softmax action rows and (nan) a NaN in one q, which reaches td_abs and the loss and no other row's dq."""
    case = R.CASES[name]
    x = R.make_inputs(case, M, nan=nan)
    call = _Call(case, x)
    for mix, double, weighted, nstep in R.VARIANTS:
        want = R.q_loss32(case, x, mix, double, weighted, nstep)
        for off in (0, 1):
            got = call.run(mix, double, weighted, nstep, off)
            _assert_equal(got, want, (name, M, mix, double, weighted, off))
        if nan:
            m = M // 2
            assert np.isnan(got["td_abs"][m]) and np.isnan(got["loss"]) and int(np.isnan(got["td_abs"]).sum()) == 1
            for i in range(case.A):
                assert not np.isnan(np.delete(got["dq_n"][i], m, axis=0)).any()


@pytest.mark.parametrize("mix", sorted(R.MIXES))
@pytest.mark.parametrize("name", CASE_IDS)
def test_q_loss_same_bits_at_any_position_and_any_M(name, mix):
    """a row's q_taken, y, td_abs and dq depend on that row alone, up to the 1 / M of the gradient: rows 964.. of M = 1029 against the
    same 65 rows as a batch of their own -- q_taken, y and td_abs bit for bit; dq, whose rule divides by M, at the same columns and,
    scaled by M, equal to the rounding of the two quotients"""
    case = R.CASES[name]
    x = R.make_inputs(case, 1029)
    tail = {k: np.ascontiguousarray(v[..., 964:] if k in ("ret", "done") else v[964:] if k in ("discount", "w") else v[:, 964:])
            for k, v in x.items() if k != "q_n"}
    tail["q_n"] = [np.ascontiguousarray(z[964:]) for z in x["q_n"]]
    whole = _Call(case, x).run(R.MIXES[mix], True, True, True)
    part = _Call(case, tail).run(R.MIXES[mix], True, True, True)
    for k in ("q_taken", "y"):
        assert R.same_bits(whole[k][:, 964:], part[k]), k
    assert R.same_bits(whole["td_abs"][964:], part["td_abs"])
    for a, b in zip(whole["dq_n"], part["dq_n"]):
        assert np.array_equal(a[964:] != 0, b != 0)
        # (2 wd) / 1029 against (2 wd) / 65: each a correctly rounded quotient of the same numerator
        assert np.abs(a[964:].astype(np.float64) * 1029 - b.astype(np.float64) * 65).max() <= 2 * np.spacing(np.float32(np.abs(b).max() * 65))


# ---- QLoss through Trainable -------------------------------------------------------------------------------------------------------------
def _mlp(D, n_out, act=nn.Tanh):
    return nn.Sequential(nn.Linear(D, 64), act(), nn.Linear(64, 64), act(), nn.Linear(64, n_out)).cuda()


def _spread(batch_size=16, act=nn.Tanh):
    torch.manual_seed(11)
    env = mpe.make_env("simple_spread", batch_size=batch_size, seed=2)
    return env, [_mlp(18, 5, act) for _ in range(3)]


def _filled(env, nets, buf, steps=12, epsilon=0.5):
    loop = PolicyLoop(env, Actors(env, nets, mode="greedy", seed=2, epsilon=epsilon), episode_len=5)
    loop.run(steps, record=False, replay=buf)
    return loop


def _torch_chain(nets, targets, batch, mix, double, weights, dtype):
    """the learner's own torch formulas on modules of `dtype`: gather, max / double-Q gather, (weighted) mse -> the loss"""
    A = len(nets)
    f = lambda t: t.to(dtype)      # noqa: E731
    q, v = [], []
    for i in range(A):
        z = nets[i](f(batch.obs_n[i]))
        q.append(z.gather(1, batch.act[i].argmax(dim=1, keepdim=True))[:, 0])
        with torch.no_grad():
            zt = targets[i](f(batch.next_obs_n[i]))
            v.append(zt.gather(1, nets[i](f(batch.next_obs_n[i])).argmax(dim=1, keepdim=True))[:, 0] if double else zt.max(dim=1).values)
    live, ret, d = 1.0 - f(batch.done), f(batch.ret), f(batch.discount)
    w = None if weights is None else f(weights)
    if mix == "independent":
        return sum((F.mse_loss(q[i], ret[i] + d * live[i] * v[i]) if w is None else (w * (q[i] - (ret[i] + d * live[i] * v[i])) ** 2).mean())
                   for i in range(A))
    y = ret.sum(dim=0) / A + d * live.min(dim=0).values * sum(v)
    return F.mse_loss(sum(q), y) if w is None else (w * (sum(q) - y) ** 2).mean()


@pytest.mark.parametrize("mix", ["independent", "vdn"])
def test_q_loss_parameter_gradients_against_float64_autograd(mix):
    """simple_spread, a sampled 3-step batch of M = 65, Tanh nets, double-Q, weights: every parameter's gradient against float64
    autograd of the torch chain, within max(4 x float32 torch autograd on this GPU, 2 ulps of the tensor's largest magnitude); the
    loss likewise; the target nets get no gradient"""
    env, nets = _spread()
    targets = [copy.deepcopy(m) for m in nets]
    with torch.no_grad():
        for m in targets:
            for p in m.parameters():
                p.mul_(0.9)
    buf = ReplayBuffer(env, 8, seed=4)
    _filled(env, nets, buf)
    batch = buf.sample(65, n_step=3, gamma=0.95, episode_len=5)
    w = torch.rand(65, device=_dev()) + 0.5
    online = Actors(env, nets, mode="greedy", logits=True)
    pi = Trainable(online)
    qt = QTargets(Actors(env, targets, mode="greedy", logits=True), online)
    head = QLoss(online, mix=mix, double=True)
    nt, no = qt.compute(batch)
    loss = head(pi(batch.obs_n), batch, nt, no, weights=w)
    loss.backward()
    assert loss.stats.shape == (3, 8) and head.last.dq_n[0].shape == (65, 5) and head.last.td_abs.shape == (65,)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        n2, t2 = [copy.deepcopy(m).to(dtype) for m in nets], [copy.deepcopy(m).to(dtype) for m in targets]
        for m in n2:
            m.zero_grad()
        l2 = _torch_chain(n2, t2, batch, mix, True, w, dtype)
        l2.backward()
        grads[dtype] = ([p.grad.double().cpu().numpy() for m in n2 for p in m.parameters()], float(l2.detach()))
    ours = [p.grad.double().cpu().numpy() for m in nets for p in m.parameters()]
    (ref, lref), (t32, l32) = grads[torch.float64], grads[torch.float32]
    for k, (a, t, r) in enumerate(zip(ours, t32, ref)):
        dev, bound = float(np.abs(a - r).max()), max(4 * float(np.abs(t - r).max()), 2 * float(np.spacing(np.float32(np.abs(r).max()))))
        PARITY["param_grad_" + mix] = max(PARITY.get("param_grad_" + mix, 0.0), dev / bound)
        print("param %d: ours %.3e bound %.3e" % (k, dev, bound))
        assert dev <= bound, (k, dev, bound)
    dev, bound = abs(float(loss.detach()) - lref), max(4 * abs(l32 - lref), 2 * float(np.spacing(np.float32(abs(lref)))))
    PARITY["loss_" + mix] = max(PARITY.get("loss_" + mix, 0.0), dev / bound)
    print("loss: ours %.3e bound %.3e" % (dev, bound))
    assert dev <= bound
    assert all(p.grad is None for m in targets for p in m.parameters())
    stale = head(pi(batch.obs_n), batch, nt, no)
    head(pi(batch.obs_n), batch, nt, no)
    with pytest.raises(_abi.MpeError, match="QLoss: backward\\(\\) of a loss whose buffers a later forward"):
        stale.backward()


# ---- prioritized replay ----------------------------------------------------------------------------------------------------------------
def test_prioritized_replay_takes_td_abs_back():
    """sample -> weights(beta) -> QLoss -> update_td(batch.idx, head.last.td_abs): the head's outputs are the restatement's bits on
    the batch's own tensors, and the stored priorities are (|td| + eps)^alpha of them, to float32 rounding of the power"""
    env, nets = _spread(batch_size=7, act=nn.ReLU)
    buf = PrioritizedReplayBuffer(env, 8, seed=4, alpha=0.6, eps=1e-6)
    _filled(env, nets, buf)
    online = Actors(env, nets, mode="greedy", logits=True)
    qt = QTargets(Actors(env, [copy.deepcopy(m) for m in nets], mode="greedy", logits=True), online)
    batch = buf.sample(130, n_step=3, gamma=0.95, episode_len=5)
    nt, no = qt.compute(batch)
    pi, head = Trainable(online), QLoss(online, mix="independent", double=True)
    w = batch.weights(0.4).contiguous()
    q_n = pi(batch.obs_n)
    loss = head(q_n, batch, nt, no, weights=w)
    loss.backward()
    buf.update_td(batch.idx, head.last.td_abs)
    torch.cuda.synchronize()
    case = R.CASES["spread3"]
    h = lambda t: t.detach().cpu().numpy()      # noqa: E731
    x = dict(q_n=[h(q) for q in q_n], nt=h(nt), no=h(no), act=h(batch.act), utter=np.zeros((3, 130, 0), np.float32), ret=h(batch.ret),
             done=h(batch._done_u8), discount=h(batch.discount), w=h(w))
    want = R.q_loss32(case, x, R.INDEPENDENT, True, True, True)
    assert R.same_bits(h(head.last.td_abs), want["td_abs"]) and R.same_bits(h(loss), want["loss"])
    for i in range(3):
        assert R.same_bits(h(head.last.dq_n[i]), want["dq_n"][i])
    idx, ref = h(batch.idx), {}
    for j, t in zip(idx, want["td_abs"].astype(np.float64)):      # the largest where several samples name one transition
        ref[int(j)] = max(ref.get(int(j), 0.0), (t + 1e-6) ** 0.6)
    pr = h(buf.priorities.reshape(-1))
    for j, p in ref.items():
        assert abs(pr[j] - p) <= 4 * np.spacing(np.float32(p)), (j, pr[j], p)
    assert all(p.grad is not None for p in pi.parameters())


# ---- a whole update as ONE graph ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", ["independent", "vdn"])
def test_whole_update_as_one_graph(mix):
    """{sample, QTargets.compute, the online forward, mpe_q_loss, mpe_mlp_grad, DeviceAdam.step} captured as ONE HIP graph (one stream)
    and replayed three times: the weights, the moments and the optimiser state are bit-equal to the same three updates run eager"""
    env, nets0 = _spread(batch_size=7, act=nn.ReLU)
    dev, M = _dev(), 130
    buf = ReplayBuffer(env, 8, seed=4)
    _filled(env, nets0, buf)

    def build():
        nets = [copy.deepcopy(m) for m in nets0]
        pi = Actors(env, nets, mode="greedy", logits=True)
        pi_t = Actors(env, [copy.deepcopy(m) for m in nets], mode="greedy", logits=True)
        return dict(pi=pi, qt=QTargets(pi_t, pi), opt=DeviceAdam([pi], lr=1e-2), out={},
                    z_n=[torch.zeros((M, 5), dtype=torch.float32, device=dev) for _ in range(3)])

    def update(s):
        batch = buf.sample(M, draw=100, n_step=3, gamma=0.95, episode_len=5)
        nt, no = s["qt"].compute(batch)
        s["pi"].act_rows(batch.obs_n)
        for i in range(3):
            s["z_n"][i].copy_(s["pi"].rows.logits[i, :, :5])
        s["out"]["q"] = q_loss_tensors(s["pi"], s["z_n"], batch, nt, no, mix=mix, out=s["out"].get("q"))
        s["opt"].step([mlp_grad_tensors(s["pi"], batch.obs_n, s["out"]["q"].dq_n)])

    def state(s):
        return s["opt"].weights + s["opt"].m + s["opt"].v + [s["opt"].state]

    eager = build()
    start = [t.clone() for t in state(eager)]
    for _ in range(3):
        update(eager)
    torch.cuda.synchronize()
    g_ = build()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        before = [t.clone() for t in state(g_)]
        update(g_)      # the code objects and the buffers outside the capture
        for t, b in zip(state(g_), before):
            t.copy_(b)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            update(g_)
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert g_["opt"].t == 3 == eager["opt"].t
    for a, b in zip(state(g_), state(eager)):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int64), b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int64))
    assert not torch.equal(state(eager)[0], start[0])
    assert torch.equal(_bits(g_["out"]["q"].loss), _bits(eager["out"]["q"].loss)) and bool(torch.isfinite(eager["out"]["q"].loss))


# ---- the example -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["--mix", "vdn", "--double"], ["--mix", "independent", "--n-step", "3", "--prioritized"]])
def test_example_device_update_follows_its_torch_path(flags):
    """examples/vdn_spread.py: 20 updates with --device-update against the same 20 in plain torch, losses within 1e-6 relative"""
    runs = []
    for extra in (["--device-update"], []):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "vdn_spread.py"), "--worlds", "16", "--batch", "64", "--updates", "20"]
                           + flags + extra, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        runs.append([json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")])
    ours, theirs = runs
    assert len(ours) == len(theirs) == 20
    worst = 0.0
    for a, b in zip(ours, theirs):
        assert np.isfinite(a["loss"]) and np.isfinite(b["loss"])
        worst = max(worst, abs(a["loss"] - b["loss"]) / abs(b["loss"]))
    print("largest relative difference of the 20 losses: %.3e" % worst)
    assert worst <= 1e-6, worst
