"""Time the optimiser step on the device (optim.DeviceAdam: mpe_adam_step's two launches for all sets) against what it replaces on the
torch path -- clip_grad_norm_, torch.optim.Adam over the modules' parameter tensors, and the two pack() calls the next forward makes
because nothing is frozen -- in ONE process, the legs alternating, three rounds, median with the range (the protocol of
tools/mlp_grad_rate.py).

    python tools/adam_rate.py [--steps 4] [--out profiles/adam_rate.json]

1. The step alone, at two parameter counts (independent of the number of worlds): the six simple_spread modules (3 x 18-64-64-5,
   3 x 18-64-64-1: 38 496 packed floats, through DeviceAdam) and sixteen 256-64-64-16 modules (346 368 packed floats, two sets of
   eight, at the ABI).  Clip 0.5 everywhere.
       ours / ours_eager                 two launches, as a graph and issued eagerly
       torch_foreach / torch_fused       clip_grad_norm_ + Adam(capturable=True; foreach, or fused=True) + the two packs, as a graph
       *_eager                           the same calls issued eagerly (capturable=False)
       *_adam_only                       torch's Adam alone as a graph: no clip, no packs -- how much is optimiser, how much repack
2. One minibatch update end to end, simple_spread at 1 024 and 65 536 worlds, T = 25, M = T * B / 4: from Minibatches.batch() to
   weights the next act can read.  No clipping (examples/ppo_spread.py uses none).
       fused_nets_eager    Trainable + PpoLoss, zero_grad / backward / torch Adam.step, then the two packs (the parent path)
       device_adam_eager   Trainable + PpoLoss, backward, DeviceAdam.step
       parent_graph        the device pieces {batch, a pack and the forward of each set, loss, both gradients on the forwards'
                           packed pairs}, the packed gradients copied to the parameters' .grad, Adam(capturable=True).step and the
                           two packs the next act / v make, as ONE graph: four set-packs per update, as the eager parent path
                           makes them -- the yardstick
       ours                {batch, both forwards, loss, both gradients, DeviceAdam.step} as ONE graph

One step of DeviceAdam and of clip_grad_norm_ + torch Adam from the same weights and gradients is compared before anything is timed
(1e-5 of each tensor's largest magnitude).  Figures are us per step / per update from device events around the calls.  The goal:
ours as a graph below the torch graph leg in every round (ours max < torch min), for the step at both sizes and for the whole update
at both world counts."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd import _abi  # noqa: E402
from multiagent_particle_envs_amd.onpolicy import Minibatches, PpoLoss, Values, gae, ppo_loss_tensors  # noqa: E402
from multiagent_particle_envs_amd.optim import DeviceAdam  # noqa: E402
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop, pack_actor16  # noqa: E402
from multiagent_particle_envs_amd.netset import module_views as _module_views  # noqa: E402
from multiagent_particle_envs_amd.train import MlpGradResult, Trainable, mlp_grad_tensors  # noqa: E402
from replay_rate import graph_of, rounds  # noqa: E402

T_STEPS, PARTS, CLIP = 25, 4, 0.5
ADAM = dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8)


def mlp(n_in, n_out):
    return nn.Sequential(nn.Linear(n_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, n_out)).cuda()


def torch_legs(params, packs, K):
    """the parent path's optimiser side: {clip, Adam, packs} and Adam alone, foreach and fused, graphs and eager"""
    legs, keep = {}, []
    for name, kw in (("torch_foreach", {}), ("torch_fused", dict(fused=True))):
        cap = torch.optim.Adam(params, capturable=True, **ADAM, **kw)
        only = torch.optim.Adam(params, capturable=True, **ADAM, **kw)
        eager = torch.optim.Adam(params, **ADAM, **kw)
        keep += [cap, only, eager]

        def full(k, opt=cap):
            torch.nn.utils.clip_grad_norm_(params, CLIP)
            opt.step()
            packs()
        legs[name] = graph_of(full, K)
        legs[name + "_adam_only"] = graph_of(lambda k, opt=only: opt.step(), K)
        legs[name + "_eager"] = lambda opt=eager: [full(0, opt) for _ in range(K)]
        legs[name + "_adam_only_eager"] = lambda opt=eager: [opt.step() for _ in range(K)]
    return legs, keep


def verdict(r, ours, yard):
    r["goal_met"] = all(r[ours]["max_us"] < r[y]["min_us"] for y in yard)
    for y in yard:
        r["speedup_over_" + y] = r[y]["median_us"] / r[ours]["median_us"]


def same_step_before_timing():
    """one step of both paths from the same weights and gradients -> the largest difference relative to each tensor's largest
    magnitude (float32 roundings in two orders: asserted below 1e-5)"""
    import copy
    torch.manual_seed(2)
    env = mpe.make_env("simple_spread", batch_size=64, seed=1)
    pm, vm = [mlp(18, 5) for _ in range(3)], [mlp(18, 1) for _ in range(3)]
    tm = [copy.deepcopy(m) for m in pm + vm]
    pi, V = Actors(env, pm, mode="sample", logits=True), Values(env, vm)
    opt = DeviceAdam([pi, V], max_grad_norm=CLIP, **ADAM)
    grads, tparams = [], [p for m in tm for p in m.parameters()]
    at = 0
    for net, w in zip((pi, V), opt.weights):
        g = MlpGradResult()
        g.packed, g.M, g.work, g.modules, g.shape = torch.zeros_like(w), 0, None, None, None
        for views in _module_views(net, g.packed)[0]:
            for w_, b_ in views:
                for view in (w_, b_):
                    view.copy_(torch.randn_like(view))
                    tparams[at].grad = view.clone()
                    at += 1
        grads.append(g)
    opt.step(grads)
    opt.write_back()
    torch.nn.utils.clip_grad_norm_(tparams, CLIP)
    torch.optim.Adam(tparams, **ADAM).step()
    worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip([p for m in pm + vm for p in m.parameters()], tparams))
    assert worst < 1e-5, worst
    return worst


def step_small(K, reps):
    torch.manual_seed(3)
    env = mpe.make_env("simple_spread", batch_size=64, seed=1)
    pm, vm = [mlp(18, 5) for _ in range(3)], [mlp(18, 1) for _ in range(3)]
    params = [p for m in pm + vm for p in m.parameters()]
    for p in params:
        p.grad = torch.randn_like(p)
    twin_pi, twin_V = Actors(env, pm, mode="sample", logits=True), Values(env, vm)      # the torch path's sets: packed at every call
    legs, keep = torch_legs(params, lambda: (twin_pi.pack(env.world.device), twin_V.pack(env.world.device)), K)
    pi, V = Actors(env, pm, mode="sample", logits=True), Values(env, vm)
    opt = DeviceAdam([pi, V], max_grad_norm=CLIP, **ADAM)
    grads = []
    for w in opt.weights:
        g = MlpGradResult()
        g.packed, g.M, g.work, g.modules, g.shape = torch.randn_like(w), 0, None, None, None
        grads.append(g)
    legs["ours"] = graph_of(lambda k: opt.step(grads), K)
    legs["ours_eager"] = lambda: [opt.step(grads) for _ in range(K)]
    r = rounds(legs, K, reps)
    r["packed_floats"] = sum(int(w.numel()) for w in opt.weights)
    verdict(r, "ours", ["torch_foreach", "torch_fused"])
    r["torch_share_that_is_optimiser"] = {k: r[k + "_adam_only"]["median_us"] / r[k]["median_us"] for k in ("torch_foreach", "torch_fused")}
    return r


def step_large(K, reps):
    torch.manual_seed(4)
    mods = [mlp(256, 16) for _ in range(16)]
    params = [p for m in mods for p in m.parameters()]
    for p in params:
        p.grad = torch.randn_like(p)

    def packs():      # what Actors.pack does on the device for two sets of eight modules
        return torch.cat([pack_actor16(m, 16) for m in mods[:8]]), torch.cat([pack_actor16(m, 16) for m in mods[8:]])
    legs, keep = torch_legs(params, packs, K)
    w = [t.contiguous() for t in packs()]
    g, m, v = ([torch.randn_like(t) if k == 0 else torch.zeros_like(t) for t in w] for k in range(3))
    cfg = _abi.MpeAdam()
    cfg.lr, (cfg.beta1, cfg.beta2), cfg.eps, cfg.max_grad_norm, cfg.n_sets = ADAM["lr"], ADAM["betas"], ADAM["eps"], CLIP, 2
    for k in range(2):
        s = cfg.set[k]
        s.weights, s.grad, s.m, s.v, s.n = w[k].data_ptr(), g[k].data_ptr(), m[k].data_ptr(), v[k].data_ptr(), w[k].numel()
    state = torch.zeros(_abi.MPE_ADAM_STATE_DOUBLES, dtype=torch.float64, device="cuda")
    state[[1, 2, 4, 5]] = 1.0
    work = torch.zeros(int(_abi.lib().mpe_adam_work(C.byref(cfg))), dtype=torch.float64, device="cuda")
    dev = w[0].device

    def ours(k):
        _abi.check(_abi.lib().mpe_adam_step(C.byref(cfg), state.data_ptr(), work.data_ptr(), _abi.raw_stream(dev)), "mpe_adam_step")
    legs["ours"] = graph_of(ours, K)
    legs["ours_eager"] = lambda: [ours(0) for _ in range(K)]
    r = rounds(legs, K, reps)
    r["packed_floats"] = sum(int(t.numel()) for t in w)
    verdict(r, "ours", ["torch_foreach", "torch_fused"])
    r["torch_share_that_is_optimiser"] = {k: r[k + "_adam_only"]["median_us"] / r[k]["median_us"] for k in ("torch_foreach", "torch_fused")}
    return r


def whole_update(B, K, reps):
    torch.manual_seed(5)
    env = mpe.make_env("simple_spread", batch_size=B, seed=1)
    dev, M = env.world.device, T_STEPS * B // PARTS
    pm0, vm0 = [mlp(18, 5) for _ in range(3)], [mlp(18, 1) for _ in range(3)]
    behaviour, V0 = Actors(env, pm0, mode="sample", seed=4, logp=True), Values(env, vm0)
    traj = PolicyLoop(env, behaviour, episode_len=T_STEPS).run(T_STEPS, values=V0)
    g = gae(traj, 0.95, 0.95)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    mb = Minibatches(traj, g, M, seed=6, epoch_counter=counter)
    head = PpoLoss(env, clip=0.2, vf_coef=0.5)
    KW = dict(clip=0.2, vf_coef=0.5)
    import copy

    def nets():
        pm, vm = [copy.deepcopy(m) for m in pm0], [copy.deepcopy(m) for m in vm0]
        return pm, vm, Actors(env, pm, mode="sample", seed=4, logits=True), Values(env, vm)
    # ---- the parent path, eager: Trainable + torch Adam + the packs the next act / v make
    pm, vm, pi_a, V_a = nets()
    tp_a, tv_a = Trainable(pi_a), Trainable(V_a)
    params_a = [p for m in pm + vm for p in m.parameters()]
    opt_a = torch.optim.Adam(params_a, **ADAM)

    def fused_nets(k):
        b = mb.batch(0, k % PARTS)
        loss = head(tp_a(b.obs_n), tv_a(b.obs_n), b)
        opt_a.zero_grad()
        loss.backward()
        opt_a.step()
        pi_a.pack(dev), V_a.pack(dev)
    # ---- the device path, eager
    pm, vm, pi_b, V_b = nets()
    tp_b, tv_b = Trainable(pi_b), Trainable(V_b)
    opt_b = DeviceAdam([tp_b, tv_b], **ADAM)

    params_b = [p for m in pm + vm for p in m.parameters()]

    def device_adam(k):
        b = mb.batch(0, k % PARTS)
        for p in params_b:      # (the example's zero_grad(): host only, so that autograd sets its views and does not accumulate)
            p.grad = None
        head(tp_b(b.obs_n), tv_b(b.obs_n), b).backward()
        opt_b.step()
    # ---- the device half as a straight line of launches, with either optimiser behind it
    z_n = [torch.zeros((M, 5), dtype=torch.float32, device=dev) for _ in range(3)]

    def device_half(pi, V, k, repack=False):
        """repack: the parent path -- nothing stays frozen, each set packs its modules ONCE per update in front of its forward and
        hands that pair to its backward (what _TrainFn.forward / backward do)"""
        b = mb.batch(0, k % PARTS)
        if repack:
            pi._frozen, V._frozen = pi.pack(dev), V.pack(dev)
        try:
            return _device_half(pi, V, b)
        finally:
            if repack:
                pi._frozen = V._frozen = None

    def _device_half(pi, V, b):
        pi.act_rows(b.obs_n)
        for i in range(3):
            z_n[i].copy_(pi.rows.logits[i, :, :5])
        v = V.v(b.obs_n)
        res = ppo_loss_tensors(z_n, [v[i] for i in range(3)], b.act, b.utter, b.logp, b.adv, b.ret, b.val, movable=[True] * 3,
                               speaks=[False] * 3, dim_c=0, **KW)
        return (mlp_grad_tensors(pi, b.obs_n, res.dlogits_n, packed=pi._frozen),
                mlp_grad_tensors(V, b.obs_n, [res.dvalues[i] for i in range(3)], packed=V._frozen))
    pm, vm, pi_c, V_c = nets()
    params_c = [p for m in pm + vm for p in m.parameters()]
    flat = [torch.zeros_like(pi_c.pack(dev)[0]), torch.zeros_like(V_c.pack(dev)[0])]
    at = 0
    for net, f in ((pi_c, flat[0]), (V_c, flat[1])):      # the parameters' .grad are views of a copy of the packed gradient, as _TrainFn hands them
        for views in _module_views(net, f)[0]:
            for w_, b_ in views:
                params_c[at].grad, params_c[at + 1].grad = w_, b_
                at += 2
    opt_c = torch.optim.Adam(params_c, capturable=True, **ADAM)

    def parent_graph(k):
        ga, gv = device_half(pi_c, V_c, k, repack=True)      # two packs here and the two below: four per update, as fused_nets_eager
        flat[0].copy_(ga.packed)
        flat[1].copy_(gv.packed)
        opt_c.step()
        pi_c.pack(dev), V_c.pack(dev)
    pm, vm, pi_d, V_d = nets()
    opt_d = DeviceAdam([pi_d, V_d], **ADAM)

    def ours(k):
        opt_d.step(list(device_half(pi_d, V_d, k)))
    legs = {"ours": graph_of(ours, K), "parent_graph": graph_of(parent_graph, K),
            "fused_nets_eager": lambda: [fused_nets(k) for k in range(K)], "device_adam_eager": lambda: [device_adam(k) for k in range(K)]}
    for leg in (legs["fused_nets_eager"], legs["device_adam_eager"]):
        leg()
    torch.cuda.synchronize()
    r = rounds(legs, K, reps)
    r["M"] = M
    verdict(r, "ours", ["parent_graph"])
    r["speedup_eager"] = r["fused_nets_eager"]["median_us"] / r["device_adam_eager"]["median_us"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "adam_rate.py measures on a GPU: there is no CPU path"
    res = {"device": torch.cuda.get_device_name(0), "equal_before_timing": {"one_step_max_relative_difference": same_step_before_timing()}, "steps_per_graph": a.steps, "graph_replays_per_timing": a.reps, "clip": CLIP,
           "unit": "us per optimiser step (step_alone) / per minibatch update (whole_update)",
           "step_alone": {"small_six_spread_modules": step_small(a.steps, a.reps), "large_sixteen_256_64_64_16": step_large(a.steps, a.reps)},
           "whole_update": {"B%d" % B: whole_update(B, a.steps, a.reps) for B in (1024, 65536)}}
    res["goal_met_everywhere"] = all(r["goal_met"] for part in ("step_alone", "whole_update") for r in res[part].values())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
