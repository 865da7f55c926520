"""mpe_mlp_grad on the GPU: every gradient block against the float64 restatement of THE MLP GRADIENT RULE within the project's bar
(4 x the deviation of float32 torch autograd on the same GPU, floor 2 float32 ulps of the block's largest magnitude), sentinels
behind every output, every float of the workspace written, a second launch bit-equal, padding +0.0f, the tail rows' hazard with
biases of +-3, shared modules as the fixed-order sum of the per-agent partials, Trainable + PpoLoss through one SGD step, and the
whole minibatch update's device half inside one HIP graph.  Every index of both launches was walked on the host first
(tests/test_mlp_grad_cpu.py).

Chunks of more than one group run on the device too (_mlp_grad_ref.SPAN_CASES: M = 8321, span 2, and M = 16385, span 3, each with a
short last chunk that ends in a group of one row): a workgroup's second and third trip through its group loop reuse the three LDS
tiles with one barrier between the trips and carry the dW accumulators and the float64 bias sums across it, which a sequential host
walk cannot get wrong.  They take every check above, and a chunk's partial is held, bit for bit, against the ordered float32 sum of
its groups' partials from launches of their own; mlp_grad_tensors at span 2 against the ABI launch's bits.  Measured on an
MI355X (profiles/mlp_grad_parity.json): every identity holds, and the closest block of the three cases stands at 0.22 of its bound
(span2_M8321, db_0 of module 0: 4.2e-10, torch 4.8e-10; span3_M16385 0.22, shared_span2_M8321 0.18) -- the float32 carry over a
chunk's groups costs nothing that shows.

Recorded miss (before any GPU run, on the host walk, which uses libm's exp2f and an exact divide -- more accurate than the hardware's):
with the forward's Tanh, 1 - 2 / (exp2(x * 2 log2 e) + 1), in the recompute, the case tail_bias3_M65 missed the bound on block db0 of
the 18-33-5 Tanh net -- deviation 8.5e-09 against a bound of 7.4e-09 (4 x torch's 1.86e-09; largest magnitude 2.2e-03) -- and over
six seeds the hidden layers' blocks of the Tanh nets stood at 3..7 x torch's deviation, the ReLU nets at about 1 x.  With the
accurate tanhf in the recompute (the forward is untouched) the same blocks stand at 1..3 x.  The bound is unchanged."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.onpolicy import Minibatches, PpoLoss, Values, gae, ppo_loss_tensors
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop
from multiagent_particle_envs_amd.train import Trainable, mlp_grad_tensors

import _mlp_grad_ref as R
import _ppo_loss_ref as P

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
PAD = 64      # sentinel floats in front of and behind every output


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _launch(case, x, agents=None, rows=None):
    """mpe_mlp_grad at the ABI on sentinel-padded grad and work -> (grad, work as NumPy; the padding is intact and all of work was
    written).  agents: run only these agents of the case, as a set of their own (same packed weights, same offsets).  rows: run
    these rows of the case's inputs (an index array) in place of all M."""
    dev = _dev()
    sel = np.arange(case.M) if rows is None else np.asarray(rows)
    sub = case._replace(M=len(sel)) if agents is None else case._replace(agents=tuple(case.agents[i] for i in agents), M=len(sel))
    idx = list(range(len(case.agents))) if agents is None else list(agents)
    A, M = len(idx), len(sel)
    _, total = R.offsets(case)
    w = torch.tensor(R.pack(case, x), device=dev)
    assert w.data_ptr() % 16 == 0
    shift = 1 if case.shift else 0
    held, ins, douts = [], [], []
    for i in idx:
        for src, dst in ((x["in"][i] if rows is None else x["in"][i][sel], ins), (x["dout"][i] if rows is None else x["dout"][i][sel], douts)):
            flat = torch.full((src.size + shift,), SENTINEL, dtype=torch.float32, device=dev)
            flat[shift:] = torch.tensor(src, device=dev).reshape(-1)
            held.append(flat)
            dst.append(flat.data_ptr() + 4 * shift)
            assert not shift or dst[-1] % 16 == 4
    aset = R.fill_set(_abi.MpeActorSet(), sub, w.data_ptr(), _abi.MPE_POLICY_VALUE if case.value else _abi.MPE_POLICY_GREEDY)
    n_work = int(_abi.lib().mpe_mlp_grad_work(C.byref(aset), M))
    assert n_work == R.work_floats(sub)
    grad = torch.full((PAD + total + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    work = torch.full((PAD + n_work + PAD,), SENTINEL, dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().mpe_mlp_grad(C.byref(aset), (C.c_void_p * A)(*ins), (C.c_void_p * A)(*douts), M, grad.data_ptr() + 4 * PAD,
                                       work.data_ptr() + 4 * PAD, _abi.raw_stream(dev)), "mpe_mlp_grad")
    torch.cuda.synchronize()
    g, wk = grad.cpu().numpy(), work.cpu().numpy()
    intact = np.all(g[:PAD] == SENTINEL) and np.all(g[PAD + total:] == SENTINEL) and np.all(wk[:PAD] == SENTINEL) and \
        np.all(wk[PAD + n_work:] == SENTINEL) and not np.any(wk[PAD:PAD + n_work] == SENTINEL)
    for m, (o, net) in enumerate(zip(R.offsets(case)[0], case.nets)):      # a module none of the agents uses is not written
        blk = g[PAD + o:PAD + o + R.module_size(net)]
        intact = intact and (not np.any(blk == SENTINEL) if m in sub.agents else np.all(blk == SENTINEL))
    return g[PAD:PAD + total].copy(), wk[PAD:PAD + n_work].copy(), bool(intact)


_cache = {}


def _case_run(case):
    """inputs, the float64 reference, the float32 torch yardstick and the kernel's outputs of one case: computed once, left unchanged"""
    hit = _cache.get(case.name)
    if hit is None:
        x = R.make_inputs(case)
        grad, work, intact = _launch(case, x)
        hit = _cache[case.name] = dict(x=x, ref=R.rule64(case, x), t32=R.torch_grads(case, x, torch.float32, device=_dev()), grad=grad,
                                       work=work, intact=intact)
    return hit


@pytest.mark.parametrize("case", R.GPU_CASES + R.SPAN_CASES, ids=R.GPU_IDS + R.SPAN_IDS)
def test_parity_with_the_float64_restatement(case):
    """Every block of every module: |kernel - float64| <= max(4 x |float32 torch on this GPU - float64|, 2 ulps of the block's largest
    magnitude).  tail_bias3_M65 is the test of the tail rows: row 65's group has 63 rows beyond M whose hidden activations are
    act(+-3), and their delta must be zero."""
    run = _case_run(case)
    got, _ = R.unpack(case, run["grad"])
    dt = R.deviations(case, run["t32"], run["ref"])
    b = R.bounds(dt)
    devs = R.deviations(case, got, run["ref"])
    for key, (dev, mag) in sorted(devs.items()):
        print("%s %s kernel %.3e torch %.3e bound %.3e mag %.3e" % (case.name, key, dev, dt[key][0], b[key], mag))
    if os.environ.get("MPE_MLP_GRAD_PARITY_OUT"):      # tools/mlp_grad_parity.py
        with open(os.environ["MPE_MLP_GRAD_PARITY_OUT"], "a") as f:
            f.write(json.dumps({"case": case.name, "deviation": {"module%d_layer%d_%s" % k: {"kernel": d, "torch_float32": dt[k][0], "bound": b[k],
                                                                                           "largest_magnitude": m} for k, (d, m) in devs.items()}}) + "\n")
    for key, (dev, mag) in devs.items():
        assert mag > 0 and dev <= b[key], (case.name, key, dev, dt[key][0], b[key], mag)


@pytest.mark.parametrize("case", R.GPU_CASES + R.SPAN_CASES, ids=R.GPU_IDS + R.SPAN_IDS)
def test_deterministic_padding_zero_and_nothing_written_out_of_range(case):
    """64 sentinel floats in front of and behind grad and work are intact, every float of work was written, every padding entry of
    the packed gradient is bit-equal to +0.0f, and a second launch writes the same bits to grad and to work."""
    run = _case_run(case)
    assert run["intact"]
    _, pad = R.unpack(case, run["grad"])
    assert pad.size and not pad.view(np.uint32).any()
    grad, work, intact = _launch(case, run["x"])
    assert intact and np.array_equal(grad.view(np.uint32), run["grad"].view(np.uint32))
    assert np.array_equal(work.view(np.uint32), run["work"].view(np.uint32))


def _bias_slots(net):
    """(entry of the module's block, low-half slot) of every packed bias entry, as the header lays them out"""
    L, out, at = len(net.hidden) + 1, [], 0
    for l in range(L):
        n_in, wide = (net.D if l == 0 else R.HW), (R.LW if l == L - 1 else R.HW)
        slot0 = 0 if l == 0 else (2 * R.HW if l == L - 1 else R.HW)
        out += [(at + n_in * wide + j, slot0 + j) for j in range(wide)]
        at += (n_in + 1) * wide
    return out


@pytest.mark.parametrize("case", [c for c in R.GPU_CASES + R.SPAN_CASES if c.name.startswith("shared")], ids=lambda c: c.name)
def test_shared_module_is_the_fixed_order_sum_of_the_per_agent_partials(case):
    """Each agent run alone leaves its chunks' partials in work; the shared run's block of grad is, bit for bit, their sum in
    float64 -- agents ascending, each agent's chunks ascending, a bias entry's high halves and then its low halves -- rounded once."""
    run = _case_run(case)
    off, _ = R.offsets(case)
    chunks = R.chunks(case.M)
    for m in sorted(set(case.agents)):
        net, size = case.nets[m], R.module_size(case.nets[m])
        ps = size + R.BIAS_SLOTS
        slots = _bias_slots(net)
        s = np.zeros(size, np.float64)
        for i, mi in enumerate(case.agents):
            if mi != m:
                continue
            _, work, intact = _launch(case, run["x"], agents=[i])
            assert intact and work.size == chunks * ps
            part = work.reshape(chunks, ps).astype(np.float64)
            for c in range(chunks):
                s += part[c, :size]
            for e, slot in slots:
                for c in range(chunks):
                    s[e] += part[c, size + slot]
        want = s.astype(np.float32)
        got = run["grad"][off[m]:off[m] + size]
        mask = got.view(np.uint32) != 0      # (a padding entry is +0.0f whatever the partials hold)
        assert mask.sum() > size // 4 and np.array_equal(got[mask].view(np.uint32), want[mask].view(np.uint32)), (case.name, m)


# ---- a chunk of several groups ------------------------------------------------------------------------------------------------------
def _layer_of_slot(net):
    """(layer, unit) of every entry of _bias_slots(net), in its order"""
    L = len(net.hidden) + 1
    return [(l, j) for l in range(L) for j in range(R.LW if l == L - 1 else R.HW)]


@pytest.mark.parametrize("case", R.SPAN_CASES[:2], ids=R.SPAN_IDS[:2])
def test_a_chunks_partial_is_the_ordered_sum_of_its_groups_partials(case):
    """Chunk c of a span >= 2 launch against its groups launched alone (rows [64 g, min(64 g + 64, M)), one agent: span 1, one chunk,
    the launch the M = 1, 63 and 64 cases hold against float64), for every chunk of every agent, the short last chunk included.

    dW (every entry of the partial that is no bias entry): bit for bit ((+0 + p_g0) + p_g1) [+ p_g2] in float32 -- the chunk's
    accumulator starts at +0 and takes each group's four-chain sum whole, and so does a group's own launch.

    db: the chunk adds its 64 span tile values t_r ascending in float64 and splits once; the groups add 64 each and split each.  With
    u = 2^-53 and S = sum over the chunk's rows of |t_r|: the chunk's sum is off the exact one by at most 64 span u S, the groups'
    sums together by 64 u S; a split (hi = fl32(d), lo = fl32(d - hi)) returns d within 2^-48 |d| <= 2^-48 S, the chunk's and the
    groups' together 2 x 2^-48 S = 128 u S; hi + lo is exact in float64 (53 bits span both halves) and adding the groups' pairs here
    rounds span - 1 times, below span u S.  Together (65 span + 192) u S.  S is taken from the float64 restatement's delta rows and
    doubled, which covers the kernel's float32 t_r beside them (they agree to parts in 1e6 wherever the parity test holds):
    |(hi + lo)_chunk - sum_g (hi_g + lo_g)| <= 2 (65 span + 192) 2^-53 S_64, at span 3 8.6e-14 S_64 -- against a float32 ulp of a value of
    S's size, >= 6e-8 S: five orders of magnitude below it, which the test asserts.  Against an ulp of the ENTRY it depends on how far
    the chunk's rows cancel: the test asserts the bound of every bias block below a hundredth of a float32 ulp of the block's largest
    entry in that chunk and prints the largest such fraction (the float64 restatement alone gives 3.2e-05 and 3.4e-03 for the two cases)."""
    run = _case_run(case)
    x, M, span, chunks = run["x"], case.M, R.span(case.M), R.chunks(case.M)
    assert span >= 2 and M - (chunks - 1) * span * R.ROWS <= (span - 1) * R.ROWS and (M - 1) % R.ROWS == 0      # a short last chunk, one last row
    at, worst = 0, 0.0
    for i, m in enumerate(case.agents):
        net, size = case.nets[m], R.module_size(case.nets[m])
        ps = size + R.BIAS_SLOTS
        whole = run["work"][at:at + chunks * ps].reshape(chunks, ps)
        at += chunks * ps
        slots, where = _bias_slots(net), _layer_of_slot(net)
        hi_at, lo_at = [e for e, _ in slots], [size + s for _, s in slots]
        is_dw = np.ones(size, bool)
        is_dw[hi_at] = False
        w = R.widths(net)
        live = sum(w[l] * w[l + 1] for l in range(len(w) - 1))
        deltas = [np.abs(d) for d in R.agent_deltas64(net, x["params"][m], x["in"][i], x["dout"][i])]
        for c in range(chunks):
            g0, g1 = c * span, min((c + 1) * span, R.groups(M))
            acc, pairs = np.zeros(size, np.float32), np.zeros(len(slots), np.float64)
            for g in range(g0, g1):
                _, part, intact = _launch(case, x, agents=[i], rows=np.arange(g * R.ROWS, min((g + 1) * R.ROWS, M)))
                assert intact and part.size == ps
                acc = acc + part[:size]      # float32, groups ascending
                pairs = pairs + (part[hi_at].astype(np.float64) + part[lo_at].astype(np.float64))
            assert acc.dtype == np.float32
            assert np.array_equal(whole[c, :size][is_dw].view(np.uint32), acc[is_dw].view(np.uint32)), (case.name, i, c)
            assert np.count_nonzero(acc[is_dw]) >= live // 8      # (a ReLU net's one-row chunk leaves the dead units' entries at zero)
            got = whole[c, hi_at].astype(np.float64) + whole[c, lo_at].astype(np.float64)
            r0, r1 = g0 * R.ROWS, min(g1 * R.ROWS, M)
            sums = [d[r0:r1].sum(axis=0) for d in deltas]
            S = np.array([sums[l][j] if j < sums[l].size else 0.0 for l, j in where])
            bound = 2.0 * (65 * span + 192) * 2.0 ** -53 * S
            assert np.all(np.abs(got - pairs) <= bound), (case.name, i, c, float(np.abs(got - pairs).max()))
            for l in range(len(deltas)):
                blk = np.array([w[0] == l for w in where])
                ulp = float(np.spacing(np.float32(np.abs(got[blk]).max())))
                assert bound[blk].max() <= 1e-5 * float(np.spacing(np.float32(S[blk].max())))
                assert ulp > 0 and bound[blk].max() <= 1e-2 * ulp, (case.name, i, c, l, float(bound[blk].max()), ulp)
                worst = max(worst, float(bound[blk].max()) / ulp)
    assert at == run["work"].size
    print("%s: %d chunks; the largest db bound is %.2e of a float32 ulp of its block's largest entry" % (case.name, chunks, worst))


def test_mlp_grad_tensors_at_span_2_is_the_abi_launch():
    """mlp_grad_tensors at M = 8321 (66 chunks of 2 groups: the Python side's workspace size at span 2): the packed gradient and the
    workspace are the ABI launch's bits."""
    case = R.case("tensors_span2_M8321", [R.ACTOR] * 3, [0, 1, 2], R.SPAN_CASES[0].M, 44)
    assert (R.span(case.M), R.chunks(case.M)) == (2, 66)
    x = R.make_inputs(case)
    grad, work, intact = _launch(case, x)
    assert intact
    env = mpe.make_env("simple_spread", batch_size=4, seed=2)
    net = Actors(env, R.torch_modules(case, x, torch.float32, device=_dev()), mode="softmax", logits=True)
    res = mlp_grad_tensors(net, [torch.tensor(a, device=_dev()) for a in x["in"]], [torch.tensor(a, device=_dev()) for a in x["dout"]])
    torch.cuda.synchronize()
    assert res.work.numel() == work.size == R.work_floats(case)
    assert np.array_equal(res.packed.cpu().numpy().view(np.uint32), grad.view(np.uint32))
    assert np.array_equal(res.work.cpu().numpy().view(np.uint32), work.view(np.uint32))


# ---- behind torch autograd ----------------------------------------------------------------------------------------------------------
def _mlp(n_out):
    return nn.Sequential(nn.Linear(18, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, n_out)).cuda()


@pytest.fixture(scope="module")
def spread():
    """simple_spread, B = 64, T = 5: a recorded trajectory, its returns and one minibatch of all 320 rows"""
    torch.manual_seed(7)
    env = mpe.make_env("simple_spread", batch_size=64, seed=2)
    pi, vf = [_mlp(5) for _ in range(3)], [_mlp(1) for _ in range(3)]
    actors, values = Actors(env, pi, mode="sample", seed=4, logp=True, logits=True), Values(env, vf)
    traj = PolicyLoop(env, actors, episode_len=5).run(5, values=values)
    g = gae(traj, 0.95, 0.9)
    counter = torch.zeros(1, dtype=torch.int64, device=g.adv.device)
    mb = Minibatches(traj, g, 320, seed=6, epoch_counter=counter)
    return dict(env=env, pi=pi, vf=vf, actors=actors, values=values, traj=traj, g=g, mb=mb, counter=counter)


KW = dict(clip=0.2, value_clip=0.2, vf_coef=0.5, ent_coef=0.01)


def _torch_step(spread, batch, lr, dtype):
    """one SGD step of the torch modules on the torch loss from the same start -> (parameters after, gradients), float64 NumPy"""
    import copy
    case = P.Case("spread_B64_T5", [P.MOVER] * 3, 0, 320, 0, **KW)
    pi, vf = [copy.deepcopy(m).to(dtype) for m in spread["pi"]], [copy.deepcopy(m).to(dtype) for m in spread["vf"]]
    params = [p for m in pi + vf for p in m.parameters()]
    opt = torch.optim.SGD(params, lr=lr)
    loss = P.torch_loss_terms(case, [pi[i](batch.obs_n[i].to(dtype)) for i in range(3)], [vf[i](batch.obs_n[i].to(dtype)) for i in range(3)],
                              batch.act.to(dtype), None, batch.logp.to(dtype), batch.adv.to(dtype), batch.ret.to(dtype), batch.val.to(dtype))[0]
    opt.zero_grad()
    loss.backward()
    grads = [p.grad.double().cpu().numpy() for p in params]
    opt.step()
    return [p.detach().double().cpu().numpy() for p in params], grads


def test_trainable_and_ppo_loss_through_one_sgd_step(spread):
    """Trainable(Actors), Trainable(Values) and PpoLoss: forward, backward and one SGD step with no torch layer in between.  Every
    parameter tensor afterwards deviates from the float64 torch step by at most lr x (the parity bound of its gradient: 4 x the
    float32 torch step's gradient deviation, floor 2 ulps of the gradient's largest magnitude) + 1 ulp of the tensor's largest
    parameter (the update p - lr * g rounds once in either float32 step).  Two backward() calls without zero_grad leave exactly twice
    the gradient of one; an observation that requires grad and a backward behind a later forward of the same M are refused."""
    import copy
    batch, lr = spread["mb"].batch(0, 0), 0.5
    ref_p, ref_g = _torch_step(spread, batch, lr, torch.float64)
    t32_p, t32_g = _torch_step(spread, batch, lr, torch.float32)
    pi, vf = [copy.deepcopy(m) for m in spread["pi"]], [copy.deepcopy(m) for m in spread["vf"]]
    env = spread["env"]
    tp, tv = Trainable(Actors(env, pi, mode="sample", seed=4, logits=True)), Trainable(Values(env, vf))
    head = PpoLoss(env, **KW)
    params = [p for m in pi + vf for p in m.parameters()]
    assert all(a is b for a, b in zip(tp.parameters() + tv.parameters(), params))
    opt = torch.optim.SGD(params, lr=lr)

    def backward():
        logits_n, values_n = tp(batch.obs_n), tv(batch.obs_n)
        assert [tuple(z.shape) for z in logits_n] == [(320, 5)] * 3 and [tuple(v.shape) for v in values_n] == [(320,)] * 3
        head(logits_n, values_n, batch).backward()
    backward()
    torch.cuda.synchronize()
    once = [p.grad.clone() for p in params]
    backward()
    assert all(torch.equal(p.grad, 2 * g_) for p, g_ in zip(params, once))      # accumulated into, not aliased
    for p, g_ in zip(params, once):
        p.grad.copy_(g_)
    opt.step()
    torch.cuda.synchronize()
    for k, (p, g_, rp, rg, tg) in enumerate(zip(params, once, ref_p, ref_g, t32_g)):
        gb = max(4 * float(np.abs(tg - rg).max()), 2 * float(np.spacing(np.float32(np.abs(rg).max()))))
        gd = float(np.abs(g_.double().cpu().numpy() - rg).max())
        pd = float(np.abs(p.detach().double().cpu().numpy() - rp).max())
        print("tensor %d: gradient deviation %.3e (torch %.3e, bound %.3e), parameter deviation %.3e" % (k, gd, float(np.abs(tg - rg).max()), gb, pd))
        assert float(np.abs(rg).max()) > 0
        assert pd <= lr * gb + float(np.spacing(np.float32(np.abs(rp).max()))), (k, pd, gd, gb)
    with pytest.raises(_abi.MpeError, match="requires grad.*there is no dL/din"):
        tp([o.clone().requires_grad_() for o in batch.obs_n])
    first = tv(batch.obs_n)
    second = tv(batch.obs_n)
    torch.stack(second).sum().backward()
    with pytest.raises(_abi.MpeError, match="Trainable: backward\\(\\) behind a later forward with the same M"):
        torch.stack(first).sum().backward()
    # a None grad_output counts as zeros: only agent 0's output is used, the other modules' gradients are exactly zero
    for p in params:
        p.grad = None
    tv(batch.obs_n)[0].sum().backward()
    torch.cuda.synchronize()
    n0 = len(list(vf[0].parameters()))
    vparams = [p for m in vf for p in m.parameters()]
    assert all(float(p.grad.abs().max()) > 0 for p in vparams[:n0]) and all(float(p.grad.abs().max()) == 0 for p in vparams[n0:])


# ---- inside a HIP graph -------------------------------------------------------------------------------------------------------------
def test_minibatch_update_in_one_graph(spread):
    """{Minibatches.batch, Actors.act_rows, Values.v, ppo_loss_tensors, mlp_grad_tensors x 2} captured on one stream and replayed after
    the epoch counter was bumped: bit for bit what the eager sequence gives then."""
    counter, dev = spread["counter"], spread["g"].adv.device
    M = 96
    pi, V = spread["actors"].freeze(), spread["values"].freeze()
    counter.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(s):
            mb = Minibatches(spread["traj"], spread["g"], M, seed=6, epoch_counter=counter)
            z_n = [torch.zeros((M, 5), dtype=torch.float32, device=dev) for _ in range(3)]

            def call(out=None):
                b = mb.batch(3, 1)
                pi.act_rows(b.obs_n)
                for i in range(3):
                    z_n[i].copy_(pi.rows.logits[i, :, :5])
                v = V.v(b.obs_n)
                res = ppo_loss_tensors(z_n, [v[i] for i in range(3)], b.act, b.utter, b.logp, b.adv, b.ret, b.val, movable=[True] * 3,
                                       speaks=[False] * 3, dim_c=0, out=out, **KW)
                ga = mlp_grad_tensors(pi, b.obs_n, res.dlogits_n)
                gv = mlp_grad_tensors(V, b.obs_n, [res.dvalues[i] for i in range(3)])
                return b, res, ga, gv
            b0, res, ga, gv = call()      # the code objects and the buffers outside the capture
            first_idx = b0.idx.clone()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                _, r1, a1, v1 = call(res)
                assert r1 is res and a1 is ga and v1 is gv
        torch.cuda.current_stream().wait_stream(s)
        counter.add_(1)
        ga.packed.fill_(SENTINEL)
        gv.packed.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        snap = [t.clone() for t in (ga.packed, gv.packed, res.grads, b0.idx)]
        assert not torch.equal(snap[3], first_idx)       # the bumped counter drew other rows
        assert float(snap[0].abs().max()) > 0 and float(snap[1].abs().max()) > 0 and not bool((snap[0] == SENTINEL).any())
        _, res2, ga2, gv2 = call(res)
        torch.cuda.synchronize()
        for a, b in zip(snap, (ga2.packed, gv2.packed, res2.grads, b0.idx)):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
        # the views of the result are the modules' own shapes
        assert [tuple(w.shape) for w, _ in ga.modules[0]] == [(64, 18), (64, 64), (5, 64)] and len(ga.modules) == 3
        assert torch.equal(ga.modules[1][2][1], ga.packed[6416 + 19 * 64 + 65 * 64 + 64 * 16:][:5])
    finally:
        pi.unfreeze(), V.unfreeze()
        counter.zero_()
