"""The PPO loss head on the device (mpe_ppo_loss): parity of every output with the float64 restatement of THE PPO
LOSS RULE, bounded by the deviation of float32 torch autograd on the same inputs; the sums bit for bit against the fold restatement
applied to the kernel's own rows; determinism; nothing written out of range; the switches; PpoLoss behind torch autograd against the
torch loss through one SGD step; and {Minibatches.batch, ppo_loss_tensors} inside a HIP graph.  Every index of both launches was
walked on the CPU under AddressSanitizer first
(tests/test_ppo_loss_cpu.py::test_host_walk_every_block_wave_and_lane_under_the_sanitizers).

Parity figures measured on an MI355X (profiles/ppo_loss_parity.json): with __expf on the ratio path the case
spread_A3_M257 missed the bound (surr 4.689e-06 > 3.815e-06, dlogits 1.601e-08 > 1.523e-08), so the ratio uses the accurate expf;
every case then holds it, the largest fraction of a bound reached being 0.79 (mean surrogate at M = 320: 3.5e-08, torch 1.1e-08).

The second launch's loops run past their first trip on the device too (_ppo_loss_ref.PIECE_CASES: 16 agents at 65 chunks, a second
piece of one chunk; the speaker / listener pair at 342 chunks, a second trip of the piece's load; one agent at 1025 chunks, three
trips and a second piece): the staged piece is overwritten behind one barrier while the lanes' float64 sums carry on, so the check
that matters is the sums against the fold of the kernel's own rows, bit for bit.  Measured on an MI355X
(profiles/ppo_loss_parity.json): it holds in all three, and the largest fraction of a parity bound among them is 0.34 (the entropy
rows of pair_A2_M87297: 3.3e-07, torch 2.4e-07); their bands hold 9, 7 and 6 agent-rows, so their means are not compared."""
import copy
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

import _ppo_loss_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
PAD = 64      # sentinel floats behind every output


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _device_inputs(case, x):
    """the case's inputs on the device; the unaligned case's logits are views that start 4 bytes into their allocations"""
    dev = _dev()
    t = lambda a: torch.tensor(a, device=dev) if a is not None else None      # noqa: E731
    d = {k: t(x[k]) for k in ("act", "utter", "logp_old", "adv", "ret", "val_old")}
    d["logits"] = []
    for z in x["logits"]:
        if case.unaligned:
            flat = torch.zeros(z.size + 1, dtype=torch.float32, device=dev)
            flat[1:] = t(z).reshape(-1)
            d["logits"].append(flat[1:].view(z.shape))
            assert d["logits"][-1].data_ptr() % 16 == 4
        else:
            d["logits"].append(t(z))
    d["values"] = [t(v) for v in x["values"]] if case.values else None
    return d


def _launch(case, d, want_rows=True):
    """mpe_ppo_loss at the ABI on sentinel-padded outputs -> (outputs as NumPy, the padding is intact)"""
    dev, A, M = _dev(), case.A, case.M
    full = lambda n: torch.full((n + PAD,), SENTINEL, dtype=torch.float32, device=dev)      # noqa: E731
    off = 1 if case.unaligned else 0      # (the unaligned case's gradients start 4 bytes into their allocations as well)
    dl = [full(M * n + off) for n in case.n_out]
    dv, rows, stats, loss = full(A * M), full(A * M * 4), full(A * 8), full(1)
    work = torch.full((int(_abi.lib().mpe_ppo_loss_work(A, M)) + 8,), -1e300, dtype=torch.float64, device=dev)
    cfg = _abi.MpePpoLoss()
    cfg.n_agents, cfg.dim_c = A, case.dim_c
    for i, (mv, sp) in enumerate(case.heads):
        cfg.movable[i], cfg.speaks[i] = int(mv), int(sp)
    cfg.clip, cfg.value_clip, cfg.vf_coef, cfg.ent_coef = case.clip, -1.0 if case.value_clip is None else case.value_clip, case.vf_coef, case.ent_coef
    ptr = lambda x: x.data_ptr() if x is not None else None      # noqa: E731
    zp = (C.c_void_p * A)(*[z.data_ptr() for z in d["logits"]])
    vp = (C.c_void_p * A)(*[v.data_ptr() for v in d["values"]]) if case.values else None
    gp = (C.c_void_p * A)(*[g.data_ptr() + 4 * off for g in dl])
    _abi.check(_abi.lib().mpe_ppo_loss(C.byref(cfg), zp, vp, M, ptr(d["act"]), ptr(d["utter"]), ptr(d["logp_old"]), ptr(d["adv"]), ptr(d["ret"]),
                                       ptr(d["val_old"]), gp, ptr(dv) if case.values else None, ptr(rows) if want_rows else None, ptr(work),
                                       ptr(stats), ptr(loss), _abi.raw_stream(dev)), "mpe_ppo_loss")
    torch.cuda.synchronize()
    n = lambda a: a.cpu().numpy()      # noqa: E731
    out = dict(dlogits=[n(g)[off:off + M * k].reshape(M, k) for g, k in zip(dl, case.n_out)], dvalues=n(dv)[:A * M].reshape(A, M) if case.values else None,
               rows=n(rows)[:A * M * 4].reshape(A, M, 4) if want_rows else None, stats=n(stats)[:A * 8].reshape(A, 8), loss=n(loss)[0])
    intact = all(np.all(n(g)[off + M * k:] == SENTINEL) and np.all(n(g)[:off] == SENTINEL) for g, k in zip(dl, case.n_out))
    intact = intact and np.all(n(stats)[A * 8:] == SENTINEL) and np.all(n(loss)[1:] == SENTINEL)
    intact = intact and np.all(n(dv)[A * M if case.values else 0:] == SENTINEL) and np.all(n(rows)[A * M * 4 if want_rows else 0:] == SENTINEL)
    intact = intact and np.all(n(work)[-8:] == -1e300) and not np.any(n(work)[:-8] == -1e300)      # every entry written, none behind
    return out, bool(intact)


_cache = {}


def _case_run(case):
    """inputs, the float64 reference, the float32 torch yardstick and the kernel's outputs of one case: computed once, left unchanged"""
    hit = _cache.get(case.name)
    if hit is None:
        x = R.make_inputs(case)
        d = _device_inputs(case, x)
        out, intact = _launch(case, d)
        hit = _cache[case.name] = dict(x=x, d=d, ref=R.rule64(case, x), t32=R.torch_loss(case, x, torch.float32, device=_dev()), out=out, intact=intact)
    return hit


@pytest.mark.parametrize("case", R.GPU_CASES + R.PIECE_CASES, ids=R.GPU_IDS + R.PIECE_IDS)
def test_parity_with_the_float64_restatement(case):
    """rows, dlogits, dvalues, stats and loss against restatement (a), the band rows left out: logp within 1e-5; every other output
    within 4 x the deviation of the same loss in float32 torch autograd on this GPU from the same reference, with a floor of 2
    float32 ulps of the output's own largest magnitude (a single row that clips: _ppo_loss_ref.deviations)."""
    c = _case_run(case)
    got, yard = R.deviations(case, c["out"], c["ref"]), R.deviations(case, c["t32"], c["ref"])
    bound = R.bounds(yard)
    for name in got:
        print("%-24s %-10s kernel %.3e  torch float32 %.3e  bound %.3e" % (case.name, name, got[name][0], yard[name][0], bound[name]))
    path = os.environ.get("MPE_PPO_LOSS_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case.name, "A": case.A, "M": case.M, "n_out": case.n_out, "band_rows": int(c["ref"]["band"].sum()),
                                "deviation": {k: {"kernel": got[k][0], "torch_float32": yard[k][0], "bound": bound[k]} for k in got}}) + "\n")
    for name, (dev, _) in got.items():
        assert dev <= bound[name], (case.name, name, dev, yard[name][0], bound[name])
    if not c["ref"]["band"].any():
        assert np.array_equal(c["out"]["stats"][:, 4], c["ref"]["stats"][:, 4].astype(np.float32))      # the clipped rows, counted
    assert np.all(c["out"]["stats"][:, 7] == 0)


@pytest.mark.parametrize("case", R.GPU_CASES + R.PIECE_CASES, ids=R.GPU_IDS + R.PIECE_IDS)
def test_sums_are_the_fold_of_the_kernels_own_rows_bit_for_bit(case):
    c = _case_run(case)
    stats, loss = R.fold_stats(case, c["out"]["rows"])
    cols = [0, 1, 2, 6]
    assert np.array_equal(c["out"]["stats"][:, cols].view(np.uint32), stats[:, cols].view(np.uint32)), (c["out"]["stats"], stats)
    assert np.float32(c["out"]["loss"]).view(np.uint32) == loss.view(np.uint32)


@pytest.mark.parametrize("case", R.GPU_CASES + R.PIECE_CASES, ids=R.GPU_IDS + R.PIECE_IDS)
def test_deterministic_and_nothing_written_out_of_range(case):
    c = _case_run(case)
    assert c["intact"]
    again, intact = _launch(case, c["d"])
    assert intact
    for k in ("dvalues", "rows", "stats"):
        assert (again[k] is None and c["out"][k] is None) or np.array_equal(again[k].view(np.uint32), c["out"][k].view(np.uint32)), k
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again["dlogits"], c["out"]["dlogits"]))
    assert np.float32(again["loss"]).view(np.uint32) == np.float32(c["out"]["loss"]).view(np.uint32)
    bare, intact = _launch(case, c["d"], want_rows=False)      # rows is optional: the other outputs do not depend on it
    assert intact and np.array_equal(bare["stats"].view(np.uint32), c["out"]["stats"].view(np.uint32))


def test_switches_change_what_they_should():
    by = {c.name: c for c in R.GPU_CASES}
    on, no_clip, no_ent, no_val = (_case_run(by[k]) for k in ("spread_A3_M257", "spread_value_clip_off", "spread_ent_coef_0", "spread_no_values"))
    assert not np.array_equal(on["out"]["rows"][:, :, 2], no_clip["out"]["rows"][:, :, 2])            # the clipped value loss is another
    assert np.array_equal(on["out"]["rows"][:, :, 1], no_clip["out"]["rows"][:, :, 1])                # the surrogate is not
    assert np.array_equal(on["out"]["rows"], no_ent["out"]["rows"])                                   # ent_coef moves no row ..
    assert not np.array_equal(on["out"]["dlogits"][0], no_ent["out"]["dlogits"][0])                   # .. but the gradient and L_i
    assert np.all(on["out"]["stats"][:, 6] != no_ent["out"]["stats"][:, 6])
    assert no_val["out"]["dvalues"] is None and np.all(no_val["out"]["stats"][:, 1] == 0) and np.all(no_val["out"]["rows"][:, :, 2] == 0)
    assert np.array_equal(on["out"]["dlogits"][0], no_val["out"]["dlogits"][0])                       # the policy gradient does not see the values


def test_ppo_loss_tensors_is_the_abi_call_and_reuses_out():
    case = R.GPU_CASES[3]      # the speaker / listener pair
    c = _case_run(case)
    d = c["d"]
    kw = dict(movable=[h[0] for h in case.heads], speaks=[h[1] for h in case.heads], dim_c=case.dim_c, clip=case.clip, value_clip=case.value_clip,
              vf_coef=case.vf_coef, ent_coef=case.ent_coef)
    res = ppo_loss_tensors(d["logits"], [v.view(-1, 1) for v in d["values"]], d["act"], d["utter"], d["logp_old"], d["adv"], d["ret"], d["val_old"],
                           rows=True, **kw)
    again = ppo_loss_tensors(d["logits"], d["values"], d["act"], d["utter"], d["logp_old"], d["adv"], d["ret"], d["val_old"], rows=True, out=res, **kw)
    torch.cuda.synchronize()
    assert again is res and all(g.data_ptr() % 16 == 0 for g in res.dlogits_n)
    for i in range(case.A):
        assert np.array_equal(res.dlogits_n[i].cpu().numpy().view(np.uint32), c["out"]["dlogits"][i].view(np.uint32))
    assert np.array_equal(res.dvalues.cpu().numpy().view(np.uint32), c["out"]["dvalues"].view(np.uint32))
    assert np.array_equal(res.rows.cpu().numpy().view(np.uint32), c["out"]["rows"].view(np.uint32))
    assert np.array_equal(res.stats.cpu().numpy().view(np.uint32), c["out"]["stats"].view(np.uint32))
    assert res.loss.cpu().numpy()[0].view(np.uint32) == np.float32(c["out"]["loss"]).view(np.uint32)
    dv_before = res.dvalues.clone()
    res.dvalues.fill_(SENTINEL)
    policy_only = ppo_loss_tensors(d["logits"], None, d["act"], d["utter"], d["logp_old"], d["adv"], None, None, **kw)
    torch.cuda.synchronize()
    assert policy_only.dvalues is None and float(policy_only.stats[:, 1].abs().max()) == 0.0
    assert bool((res.dvalues == SENTINEL).all()) and dv_before.shape == res.dvalues.shape      # values_n=None: dvalues is untouched
    with pytest.raises(_abi.MpeError, match="ppo_loss_tensors: out is a PpoLossResult of the same heads"):
        ppo_loss_tensors(d["logits"], None, d["act"], d["utter"], d["logp_old"], d["adv"], None, None, out=res, **kw)


# ---- behind torch autograd ----------------------------------------------------------------------------------------------------------
def _mlp(n_in, n_out):
    return nn.Sequential(nn.Linear(n_in, 16), nn.Tanh(), nn.Linear(16, n_out)).cuda()


@pytest.fixture(scope="module")
def spread():
    """simple_spread, B = 8, T = 5: a recorded trajectory, its returns and one minibatch of all 40 rows"""
    torch.manual_seed(5)
    env = mpe.make_env("simple_spread", batch_size=8, seed=2)
    pi, vf = [_mlp(18, 5) for _ in range(3)], [_mlp(18, 1) for _ in range(3)]
    loop = PolicyLoop(env, Actors(env, pi, mode="sample", seed=4, logp=True), episode_len=5)
    traj = loop.run(5, values=Values(env, vf))
    g = gae(traj, 0.95, 0.9)
    counter = torch.zeros(1, dtype=torch.int64, device=g.adv.device)
    mb = Minibatches(traj, g, 40, seed=6, epoch_counter=counter)
    return dict(env=env, pi=pi, vf=vf, traj=traj, g=g, mb=mb, counter=counter)


def _sgd_step(case, pi, vf, batch, lr, dtype, head=None, scale=1.0):
    """one SGD step of copies of the modules from the same start -> (every parameter after the step, as float64 NumPy; the gradients)"""
    pi, vf = [copy.deepcopy(m).to(dtype) for m in pi], [copy.deepcopy(m).to(dtype) for m in vf]
    params = [p for m in pi + vf for p in m.parameters()]
    opt = torch.optim.SGD(params, lr=lr)
    logits_n = [pi[i](batch.obs_n[i].to(dtype)) for i in range(case.A)]
    values_n = [vf[i](batch.obs_n[i].to(dtype)) for i in range(case.A)]
    if head is not None:
        loss = head(logits_n, values_n, batch)
    else:
        loss = R.torch_loss_terms(case, logits_n, values_n, batch.act.to(dtype), None, batch.logp.to(dtype), batch.adv.to(dtype),
                                  batch.ret.to(dtype), batch.val.to(dtype))[0]
    opt.zero_grad()
    (scale * loss).backward()
    grads = [p.grad.clone() for p in params]
    opt.step()
    torch.cuda.synchronize()
    return [p.detach().double().cpu().numpy() for p in params], grads, loss


def test_autograd_one_sgd_step_agrees_with_the_torch_loss(spread):
    """After one SGD step from the same start every parameter agrees with the torch-loss step within the parity bound carried through
    the step: the deviation from the float64 step is at most 4 x that of the float32 torch-loss step, floor 2 ulps of the tensor's
    largest parameter.  A non-unit grad_output scales the gradients (0.5: exactly)."""
    case = R.Case("spread_B8_T5", [R.MOVER] * 3, 0, 40, 0, clip=0.2, value_clip=0.2, vf_coef=0.5, ent_coef=0.01)
    batch = spread["mb"].batch(0, 0)
    lr = 0.5
    head = PpoLoss(spread["env"], clip=case.clip, value_clip=case.value_clip, vf_coef=case.vf_coef, ent_coef=case.ent_coef)
    ref, _, loss64 = _sgd_step(case, spread["pi"], spread["vf"], batch, lr, torch.float64)
    t32, _, loss32 = _sgd_step(case, spread["pi"], spread["vf"], batch, lr, torch.float32)
    got, grads, loss = _sgd_step(case, spread["pi"], spread["vf"], batch, lr, torch.float32, head=head)
    assert loss.dim() == 0 and loss.stats.shape == (3, 8) and loss.stats.is_cuda
    assert abs(float(loss.detach()) - float(loss64.detach())) <= max(4 * abs(float(loss32.detach()) - float(loss64.detach())), 2 * float(np.spacing(np.float32(abs(float(loss64.detach()))))))
    start = [p.detach().double().cpu().numpy() for m in spread["pi"] + spread["vf"] for p in m.parameters()]
    moved = 0
    for k, (a, b, r, s) in enumerate(zip(got, t32, ref, start)):
        bound = max(4 * float(np.abs(b - r).max()), 2 * float(np.spacing(np.float32(np.abs(r).max()))))
        assert float(np.abs(a - r).max()) <= bound, (k, float(np.abs(a - r).max()), float(np.abs(b - r).max()), bound)
        moved += int(np.abs(r - s).max() > 1e-6)
    assert moved == len(got)      # the step moved every tensor: the comparison is of steps, not of starts
    _, half, _ = _sgd_step(case, spread["pi"], spread["vf"], batch, lr, torch.float32, head=head, scale=0.5)
    assert all(torch.equal(h, 0.5 * g_) for h, g_ in zip(half, grads))
    policy_only = head([m(batch.obs_n[i]) for i, m in enumerate(spread["pi"])], None, batch)
    torch.cuda.synchronize()
    assert float(policy_only.stats[:, 1].abs().max()) == 0.0
    # the buffers are cached per M: a backward behind a later forward of the same M would read that call's gradients, and is refused
    first = head([m(batch.obs_n[i]) for i, m in enumerate(spread["pi"])], None, batch)
    head([m(batch.obs_n[i]) for i, m in enumerate(spread["pi"])], None, batch).backward()
    with pytest.raises(_abi.MpeError, match="PpoLoss: backward\\(\\) of a loss whose buffers a later forward"):
        first.backward()


# ---- inside a HIP graph -------------------------------------------------------------------------------------------------------------
def test_batch_and_loss_in_a_graph_with_an_epoch_counter(spread):
    """{Minibatches.batch, ppo_loss_tensors} captured on one stream, replayed after the epoch counter was bumped and the logits
    rewritten: bit for bit what the eager calls give then."""
    counter, dev = spread["counter"], spread["g"].adv.device
    M, A = 16, 3
    gen = torch.Generator(device="cpu").manual_seed(1)
    logits_n = [torch.randn((M, 5), generator=gen).to(dev) for _ in range(A)]
    values_n = [torch.randn((M,), generator=gen).to(dev) for _ in range(A)]
    kw = dict(movable=[True] * A, speaks=[False] * A, dim_c=0, clip=0.2, value_clip=0.2, vf_coef=0.5, ent_coef=0.01, rows=True)
    counter.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mb = Minibatches(spread["traj"], spread["g"], M, seed=6, epoch_counter=counter)

        def call(out=None):
            b = mb.batch(3, 1)      # rows 16 .. 31 of epoch 3 + counter
            return b, ppo_loss_tensors(logits_n, values_n, b.act, b.utter, b.logp, b.adv, b.ret, b.val, out=out, **kw)
        b0, res = call()      # the code objects and the buffers outside the capture
        first_idx = b0.idx.clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            assert call(res)[1] is res
    torch.cuda.current_stream().wait_stream(s)
    counter.add_(1)                                  # the next replay draws epoch 4's rows ..
    for z in logits_n:
        z.mul_(-0.75).add_(0.125)                    # .. and reads the logits as they stand now
    res.grads.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    snap = [t.clone() for t in (res.grads, res.rows, res.stats, res.loss, b0.idx)]
    assert not torch.equal(snap[4], first_idx)       # the bumped counter drew other rows
    b1, eager = call()
    torch.cuda.synchronize()
    assert eager is not res and b1 is b0
    for a, b in zip(snap, (eager.grads, eager.rows, eager.stats, eager.loss, b1.idx)):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    counter.zero_()
