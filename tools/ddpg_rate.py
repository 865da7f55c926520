"""Time the off-policy update's device pieces against the torch ops they replace, in ONE process, every leg a HIP
graph, the legs alternating over three rounds, median with the range (the protocol of tools/mlp_dinput_rate.py).

    python tools/ddpg_rate.py [--steps 4] [--out profiles/ddpg_rate.json]

simple_spread, N = 3 (W = 69), M = 1 024 and 65 536 rows.
1. Per piece:
       rows            mpe_policy_rows + mpe_policy_rows_grad against A x (clone, softmax, column write) and its autograd backward
       rows_forward    mpe_policy_rows alone against the forward half, and against a device copy of its compulsory bytes (M * W
                       floats read, A * M * W written)
       td_loss         mpe_td_loss against A x F.mse_loss and its backward
       polyak          mpe_polyak on the two packed buffers against torch._foreach_lerp_ over the 36 parameter tensors
2. The whole update -- critic update, actor update, soft updates -- as ONE graph: --device-update's wiring (TdLoss's and ActorLoss's
   launches, DeviceAdam, PolyakTargets) against the --fused-nets wiring (Trainable, F.mse_loss, torch's softmax and column write,
   torch Adam (capturable) and lerp_), captured the same way.  Goal: ours below the parent in every round (ours max < parent min).
Figures are us per pass from device events around the replays."""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd.learner import (Critics, RowsLayout, policy_rows_grad_tensors, policy_rows_tensors,  # noqa: E402
                                                  td_loss_tensors)
from multiagent_particle_envs_amd.optim import DeviceAdam, PolyakTargets  # noqa: E402
from multiagent_particle_envs_amd.policy import Actors  # noqa: E402
from multiagent_particle_envs_amd.train import Trainable, mlp_dinput_tensors, mlp_grad_tensors  # noqa: E402
from replay_rate import graph_of, rounds  # noqa: E402

TAU, LR = 0.01, 1e-3


def mlp(n_in, n_out):
    return nn.Sequential(nn.Linear(n_in, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, n_out)).cuda()


def verdict(r, ours, yard):
    r["speedup_over_" + yard] = r[yard]["median_us"] / r[ours]["median_us"]
    r["goal_met"] = r[ours]["max_us"] < r[yard]["min_us"]
    return r


def pieces(env, mu, qs, M, K, reps):
    A, dev = env.n, torch.device("cuda")
    lay = RowsLayout.of(Actors(env, mu, mode="softmax"))
    W, col = lay.W, lay.col
    gen = torch.Generator(device="cuda").manual_seed(0)
    joint = torch.randn(M, W, generator=gen, device=dev)
    zs = [torch.randn(M, 5, generator=gen, device=dev) for _ in range(A)]
    G = [torch.randn(M, W, generator=gen, device=dev) for _ in range(A)]
    q, y = torch.randn(A, M, generator=gen, device=dev), torch.randn(A, M, generator=gen, device=dev)
    out = {}
    # ---- the relaxed rows and their gradient
    rows = policy_rows_tensors(lay, joint, zs)
    g_n = [g[:, c:c + 5] for g, c in zip(G, col)]
    res = policy_rows_grad_tensors(lay, zs, g_n)
    tz = [z.clone().requires_grad_() for z in zs]

    def torch_rows():
        js = []
        for i in range(A):
            j = joint.clone()
            j[:, col[i]:col[i] + 5] = F.softmax(tz[i], dim=1)
            js.append(j)
        return js

    def torch_both(k):
        return torch.autograd.grad(torch_rows(), tz, G)
    want = torch_both(0)
    torch.cuda.synchronize()
    worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(res.dlogits_n, want))
    assert worst < 1e-5, worst

    def ours_both(k):
        policy_rows_tensors(lay, joint, zs, out=rows)
        policy_rows_grad_tensors(lay, zs, g_n, out=res)
    r = rounds({"ours": graph_of(ours_both, K), "torch_graph": graph_of(torch_both, K)}, K, reps)
    r["equal_before_timing"] = {"dlogits_max_relative_difference": worst}
    out["rows"] = verdict(r, "ours", "torch_graph")
    big = torch.zeros((A, M, W), device=dev)

    def torch_forward(k):
        with torch.no_grad():
            torch_rows()
    r = rounds({"ours": graph_of(lambda k: policy_rows_tensors(lay, joint, zs, out=rows), K), "torch_graph": graph_of(torch_forward, K),
                "copy_floor": graph_of(lambda k: big.copy_(joint.unsqueeze(0).expand(A, M, W)), K)}, K, reps)
    r["compulsory_bytes"] = 4 * M * W * (1 + A)
    r["fraction_of_copy_floor"] = r["copy_floor"]["median_us"] / r["ours"]["median_us"]
    out["rows_forward"] = verdict(r, "ours", "torch_graph")
    # ---- the TD loss
    q_n = [q[i] for i in range(A)]
    td = td_loss_tensors(q_n, y)
    tq = q.clone().requires_grad_()

    def torch_td(k):
        return torch.autograd.grad(sum(F.mse_loss(tq[i], y[i]) for i in range(A)), tq)
    want = torch_td(0)[0]
    torch.cuda.synchronize()
    worst = float((td.dq - want).abs().max() / want.abs().max())
    assert worst < 1e-5, worst
    r = rounds({"ours": graph_of(lambda k: td_loss_tensors(q_n, y, out=td), K), "torch_graph": graph_of(torch_td, K)}, K, reps)
    r["equal_before_timing"] = {"dq_max_relative_difference": worst}
    out["td_loss"] = verdict(r, "ours", "torch_graph")
    # ---- the soft updates
    pi, Q = Actors(env, mu, mode="softmax", logits=True).freeze(), Critics(env, qs).freeze()
    pol = PolyakTargets([(pi, Actors(env, [copy.deepcopy(m) for m in mu], mode="softmax")), (Q, Critics(env, [copy.deepcopy(m) for m in qs]))], TAU)
    on = [p.detach() for m in mu + qs for p in m.parameters()]
    tg = [p.clone() for p in on]
    r = rounds({"ours": graph_of(lambda k: pol.step(), K), "torch_graph": graph_of(lambda k: torch._foreach_lerp_(tg, on, TAU), K)}, K, reps)
    r["packed_floats"], r["parameter_tensors"] = sum(int(w.numel()) for w in pol.weights), len(on)
    out["polyak"] = verdict(r, "ours", "torch_graph")
    return out


def whole_update(env, mu0, qs0, M, K, reps):
    A, dev = env.n, torch.device("cuda")
    gen = torch.Generator(device="cuda").manual_seed(1)
    obs_n = [torch.randn(M, 18, generator=gen, device=dev) for _ in range(A)]
    joint = torch.randn(M, 69, generator=gen, device=dev)
    y = torch.randn(A, M, generator=gen, device=dev)
    # ---- the parent commit's --fused-nets wiring: torch Adam and lerp_ over the parameters
    mu, qs = [copy.deepcopy(m) for m in mu0], [copy.deepcopy(m) for m in qs0]
    mu_t, q_t = copy.deepcopy(mu), copy.deepcopy(qs)
    col = Actors(env, mu, mode="softmax").col_move
    q_train, pi_train = Trainable(Critics(env, qs)), Trainable(Actors(env, mu, mode="softmax", logits=True))
    q_const = Trainable(Critics(env, qs), input_grad=True, weight_grad=False, cols=[(c, 5) for c in col])
    opt_q = torch.optim.Adam([p for m in qs for p in m.parameters()], lr=LR, capturable=True)
    opt_mu = torch.optim.Adam([p for m in mu for p in m.parameters()], lr=LR, capturable=True)

    def parent(k):
        q = q_train(joint)
        critic_loss = sum(F.mse_loss(q[i], y[i]) for i in range(A))
        opt_q.zero_grad(set_to_none=True)
        critic_loss.backward()
        opt_q.step()
        logits = pi_train(obs_n)
        js = []
        for i in range(A):
            j = joint.clone()
            j[:, col[i]:col[i] + 5] = F.softmax(logits[i], dim=1)
            js.append(j)
        actor_loss = 0.0
        for q_i in q_const(js):
            actor_loss = actor_loss - q_i.mean()
        opt_mu.zero_grad(set_to_none=True)
        actor_loss.backward()
        opt_mu.step()
        with torch.no_grad():
            for online, targ in zip(mu + qs, mu_t + q_t):
                for p, pt in zip(online.parameters(), targ.parameters()):
                    pt.lerp_(p, TAU)
    # ---- --device-update's wiring as a straight line of launches
    mu2, qs2 = [copy.deepcopy(m) for m in mu0], [copy.deepcopy(m) for m in qs0]
    pi, Q = Actors(env, mu2, mode="softmax", logits=True), Critics(env, qs2)
    o_q, o_mu = DeviceAdam([Q], lr=LR), DeviceAdam([pi], lr=LR)
    pol = PolyakTargets([(pi, Actors(env, copy.deepcopy(mu2), mode="softmax")), (Q, Critics(env, copy.deepcopy(qs2)))], TAU)
    lay = RowsLayout.of(pi)
    z_n = [torch.zeros((M, 5), device=dev) for _ in range(A)]
    dout = torch.full((M,), -1.0 / M, device=dev)
    o = {}

    def ours(k):
        q = Q.q(joint)
        o["td"] = td_loss_tensors([q[i] for i in range(A)], y, out=o.get("td"))
        o_q.step([mlp_grad_tensors(Q, joint, [o["td"].dq[i] for i in range(A)])])
        pi.act_rows(obs_n)
        for i in range(A):
            z_n[i].copy_(pi.rows.logits[i, :, :5])
        o["rows"] = policy_rows_tensors(lay, joint, z_n, out=o.get("rows"))
        qa = Q.q(o["rows"])
        g = mlp_dinput_tensors(Q, o["rows"], [dout] * A, cols=[(c, 5) for c in lay.col])
        o["grad"] = policy_rows_grad_tensors(lay, z_n, g, q=qa, out=o.get("grad"))
        o_mu.step([mlp_grad_tensors(pi, obs_n, o["grad"].dlogits_n)])
        pol.step()
    legs, notes = {"ours": graph_of(ours, K)}, {}
    try:
        legs["parent_graph"] = graph_of(parent, K)
    except Exception as e:      # (a capture the runtime refuses: the figure is then missing, said so)
        torch.cuda.synchronize()
        notes["parent_graph"] = "capture failed: %s" % (str(e).splitlines() or [""])[0]
    legs["parent_eager"] = lambda: [parent(0) for _ in range(K)]
    legs["ours_eager"] = lambda: [ours(0) for _ in range(K)]
    r = rounds(legs, K, reps)
    r.update(notes)
    r["M"] = M
    if not notes:
        verdict(r, "ours", "parent_graph")
    r["speedup_eager"] = r["parent_eager"]["median_us"] / r["ours_eager"]["median_us"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ddpg_rate.py measures on a GPU: there is no CPU path"
    torch.manual_seed(3)
    env = mpe.make_env("simple_spread", batch_size=64, seed=1)
    mu, qs = [mlp(18, 5) for _ in range(env.n)], [mlp(69, 1) for _ in range(env.n)]
    res = {"device": torch.cuda.get_device_name(0), "scenario": "simple_spread", "agents": env.n, "joint_width": 69, "passes_per_graph": a.steps,
           "graph_replays_per_timing": a.reps, "unit": "us per pass (pieces) / per update (whole_update)", "pieces": {}, "whole_update": {}}
    for M in (1024, 65536):
        res["pieces"]["M%d" % M] = pieces(env, mu, qs, M, a.steps, a.reps)
        res["whole_update"]["M%d" % M] = whole_update(env, mu, qs, M, a.steps, a.reps)
    res["whole_update_goal_met"] = all(r.get("goal_met", False) for r in res["whole_update"].values())
    res["pieces_that_lost"] = ["%s/%s" % (m, k) for m, p in res["pieces"].items() for k, r in p.items() if not r["goal_met"]]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
