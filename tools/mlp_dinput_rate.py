"""Time the MLP input gradients (train.mlp_dinput_tensors: mpe_mlp_dinput's one launch) against torch autograd's gradient with
respect to the input of the same modules, in ONE process, every leg a HIP graph of K passes replayed several times, the legs
alternating, three rounds (the protocol of tools/mlp_grad_rate.py): the three ReLU critics of simple_spread N = 3, W-64-64-1 with
W = 69 the env's joint row (3 x 18 observation floats and 3 x 5 action floats), M = 1024 and 65 536 joint rows per critic, the
window of 5 action columns and the whole row.

    python tools/mlp_dinput_rate.py [--steps 4] [--out profiles/mlp_dinput_rate.json]

Every leg starts from dL/dq [M] per agent and the agent's own joint rows [M, W] and ends at dL/d(joint rows) over the window.

    ours          mlp_dinput_tensors(critics, joints, dq, cols): one launch, the hidden activations recomputed; the set frozen
    torch_graph   torch.autograd.grad(q.sum-like, joint) on the same modules: forward AND backward (torch has no backward without a
                  forward of these inputs: the actor loss makes new joint rows at every update), captured as a graph: the yardstick
    torch_eager   the same calls issued eagerly;  ours_eager likewise
    copy_floor    one device copy of the compulsory bytes (in + dout + din) -- what a kernel bound by memory alone would take
    mfma_floor    the fp32 MFMA steps the kernel issues (csrc/mpe_mlp_dinput.h: P1, P2, P4, P6, P8), 4096 FLOP each, at 157 TFLOP/s
    actor_update  one whole actor update of examples/maddpg_spread.py as a graph -- forward, loss, backward, Adam step on the actors
                  -- with --fused-nets' wiring (Trainable(Actors), torch softmax, Trainable(Critics, input_grad=True,
                  weight_grad=False)) against the plain torch wiring of the default path

Both legs' gradients are compared before anything is timed (1e-4 of each tensor's largest magnitude).  Figures are us per pass from
device events around the replays (median of the rounds, min and max kept).  The goal: faster than the torch graph at both sizes in
every round (ours max < torch_graph min)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd.learner import Critics  # noqa: E402
from multiagent_particle_envs_amd.policy import Actors  # noqa: E402
from multiagent_particle_envs_amd.train import Trainable, mlp_dinput_tensors  # noqa: E402
from replay_rate import graph_of, rounds  # noqa: E402

PEAK = 157e12


def mlp(n_in, n_out):
    return nn.Sequential(nn.Linear(n_in, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, n_out)).cuda()


def mfma_steps_per_group(D, ncol):
    """v_mfma_f32_32x32x2_f32 steps a workgroup issues per 64 rows of a D-64-64-1 net and a window of ncol columns"""
    return 4 * ((D + 1) // 2) + 4 * 32 + 4 * 8 + 4 * 32 + 2 * 32 * ((ncol + 31) // 32)


def size(env, qs, mu, M, K, reps):
    A, dev = env.n, torch.device("cuda")
    net = Critics(env, qs).freeze()
    W = net.joint_width
    col = Actors(env, mu, mode="softmax").col_move
    gen = torch.Generator(device="cuda").manual_seed(0)
    joints = [torch.randn(M, W, generator=gen, device=dev) for _ in range(A)]
    obs_n = [torch.randn(M, 18, generator=gen, device=dev) for _ in range(A)]
    dq = [torch.full((M,), -1.0 / M, device=dev) for _ in range(A)]
    out = {"M": M, "joint_width": W, "windows": {}}
    for name, cols in (("actions_5", [(col[i], 5) for i in range(A)]), ("whole_row", [(0, W)] * A)):
        tj = [j.clone().requires_grad_() for j in joints]

        def ours(k):
            mlp_dinput_tensors(net, joints, dq, cols=cols)

        def torch_grad(k):
            return torch.autograd.grad([qs[i](tj[i])[:, 0] for i in range(A)], tj, dq)
        want = torch_grad(0)
        got = mlp_dinput_tensors(net, joints, dq, cols=cols)
        torch.cuda.synchronize()
        # (a ReLU unit within rounding of 0 may fall on either side in two float32 forwards: such a row differs by that unit's whole
        #  share, so the check is on the fraction of elements beyond 1e-4 of the largest magnitude, and the worst is recorded)
        rel = [(g - w_[:, c0:c0 + nc]).abs() / w_[:, c0:c0 + nc].abs().max() for g, w_, (c0, nc) in zip(got, want, cols)]
        worst, beyond = max(float(r_.max()) for r_ in rel), max(float((r_ > 1e-4).float().mean()) for r_ in rel)
        assert beyond <= 1e-5, (worst, beyond)
        nbytes = sum(4 * M * (W + 1 + nc) for _, nc in cols)
        a, b = torch.zeros(nbytes // 2, dtype=torch.uint8, device=dev), torch.zeros(nbytes // 2, dtype=torch.uint8, device=dev)
        legs = {"ours": graph_of(ours, K), "torch_graph": graph_of(torch_grad, K), "torch_eager": lambda: [torch_grad(0) for _ in range(K)],
                "ours_eager": lambda: [ours(0) for _ in range(K)], "copy_floor": graph_of(lambda k: b.copy_(a), K)}
        r = rounds(legs, K, reps)
        flops = 4096.0 * sum(mfma_steps_per_group(W, nc) for _, nc in cols) * ((M + 63) // 64)
        r.update(equal_before_timing={"max_relative_difference": worst, "fraction_beyond_1e-4": beyond}, compulsory_bytes=nbytes, mfma_flops_issued=flops,
                 mfma_floor_us=flops / PEAK * 1e6)
        r["fraction_of_mfma_floor"] = r["mfma_floor_us"] / r["ours"]["median_us"]
        r["fraction_of_copy_floor"] = r["copy_floor"]["median_us"] / r["ours"]["median_us"]
        r["speedup_over_torch_graph"] = r["torch_graph"]["median_us"] / r["ours"]["median_us"]
        r["speedup_over_torch_eager"] = r["torch_eager"]["median_us"] / r["ours_eager"]["median_us"]
        r["goal_met"] = r["ours"]["max_us"] < r["torch_graph"]["min_us"]
        out["windows"][name] = r
        del legs
    net.unfreeze()
    # ---- one whole actor update, both wirings as graphs (capturable Adam: its step count lives on the device)
    import copy
    mu_a, mu_b = [copy.deepcopy(m) for m in mu], [copy.deepcopy(m) for m in mu]
    joint = joints[0]
    cols = [(col[i], 5) for i in range(A)]
    pi = Trainable(Actors(env, mu_a, mode="softmax", logits=True))
    qc = Trainable(Critics(env, qs).freeze(), input_grad=True, weight_grad=False, cols=cols)      # (the critics do not change in an actor update)
    opt_a = torch.optim.Adam([p for m in mu_a for p in m.parameters()], lr=1e-3, capturable=True)
    opt_b = torch.optim.Adam([p for m in mu_b for p in m.parameters()], lr=1e-3, capturable=True)

    def fused(k):
        logits = pi(obs_n)
        js = []
        for i in range(A):
            j = joint.clone()
            j[:, col[i]:col[i] + 5] = F.softmax(logits[i], dim=1)
            js.append(j)
        q = qc(js)
        loss = -sum(q[i].mean() for i in range(A))
        opt_a.zero_grad(set_to_none=True)
        loss.backward()
        opt_a.step()

    def plain(k):
        loss = 0.0
        for i in range(A):
            j = joint.clone()
            j[:, col[i]:col[i] + 5] = F.softmax(mu_b[i](obs_n[i]), dim=1)
            loss = loss - qs[i](j).mean()
        opt_b.zero_grad(set_to_none=True)
        loss.backward()
        opt_b.step()
    legs, notes = {"fused_nets_eager": lambda: [fused(0) for _ in range(K)], "torch_eager": lambda: [plain(0) for _ in range(K)]}, {}
    for name, fn in (("fused_nets_graph", fused), ("torch_graph", plain)):
        try:
            legs[name] = graph_of(fn, K)
        except Exception as e:      # (a capture the runtime refuses: the figure is then missing, said so)
            torch.cuda.synchronize()
            notes[name] = "capture failed: %s" % (str(e).splitlines() or [""])[0]
    r = rounds(legs, K, reps)
    r.update(notes)
    if not notes:
        r["speedup_over_torch_graph"] = r["torch_graph"]["median_us"] / r["fused_nets_graph"]["median_us"]
        r["goal_met"] = r["fused_nets_graph"]["max_us"] < r["torch_graph"]["min_us"]
    r["speedup_over_torch_eager"] = r["torch_eager"]["median_us"] / r["fused_nets_eager"]["median_us"]
    out["actor_update"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mlp_dinput_rate.py measures on a GPU: there is no CPU path"
    torch.manual_seed(3)
    env = mpe.make_env("simple_spread", batch_size=64, seed=1)
    A = env.n
    mu = [mlp(18, 5) for _ in range(A)]
    W = Actors(env, mu, mode="softmax").joint_width
    qs = [mlp(W, 1) for _ in range(A)]
    res = {"scenario": "simple_spread", "agents": A, "modules": "3 x %d-64-64-1 ReLU critics (the joint row of N = 3: 3 x 18 + 3 x 5)" % W,
           "passes_per_graph": a.steps, "graph_replays_per_timing": a.reps, "peak_fp32_mfma_flops": PEAK,
           "unit": "us per pass: dL/dq of three critics to dL/d(joint rows) over the window", "sizes": {}}
    for M in (1024, 65536):
        res["sizes"]["M%d" % M] = size(env, qs, mu, M, a.steps, a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
