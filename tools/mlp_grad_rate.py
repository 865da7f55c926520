"""Time the MLP weight gradients (train.mlp_grad_tensors: mpe_mlp_grad's two launches per set) against torch autograd's backward of
the same modules, in ONE process, every leg a HIP graph of K backward passes replayed several times, the legs alternating, three
rounds (the protocol of tools/ppo_loss_rate.py): simple_spread N = 3, T = 25, B = 1024 and 65 536 worlds, one minibatch of
M = T * B / 4 rows, three 18-64-64-5 Tanh actors and three 18-64-64-1 Tanh critics.

    python tools/mlp_grad_rate.py [--steps 4] [--out profiles/mlp_grad_rate.json]

Every leg starts from dL/dlogits [M, 5] and dL/dvalues [M] per agent (what the loss head leaves) and ends at the gradients of all
six modules' weights and biases.

    ours          mlp_grad_tensors(actors, obs_n, dlogits_n) and mlp_grad_tensors(values, obs_n, dvalues rows): four launches, the
                  hidden activations recomputed; the sets frozen (packed once, as a learner packs them once per optimiser step)
    torch_graph   torch.autograd.backward of the six modules' outputs, the forward done once outside and its graph retained (the
                  saved activations are read, not recomputed), captured as a graph: the yardstick
    torch_eager   the same call issued eagerly;  ours_eager likewise
    torch_fwd_bwd_graph   forward and backward of the six modules in one graph (what a learner without a saved forward pays)

Both legs' gradients are compared before anything is timed (1e-4 of each tensor's largest magnitude: float32 sums of M terms in two
orders).  Figures are us per backward pass of all six modules from device events around the replays (median of the rounds, min and
max kept).  The goal: faster than the torch graph at both sizes in every round (ours max < torch_graph min).  Also recorded: the
fraction of the fp32 MFMA floor -- the padded recompute, delta and dW steps the kernel issues, 4096 FLOP each, against 157 TFLOP/s."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd.onpolicy import Values  # noqa: E402
from multiagent_particle_envs_amd.policy import Actors  # noqa: E402
from multiagent_particle_envs_amd.train import mlp_grad_tensors  # noqa: E402
from replay_rate import graph_of, rounds  # noqa: E402

T_STEPS, PARTS, PEAK = 25, 4, 157e12


def mlp(n_out):
    return nn.Sequential(nn.Linear(18, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, n_out)).cuda()


def mfma_steps_per_group(D):
    """v_mfma_f32_32x32x2_f32 steps a workgroup issues per 64 rows of a D-64-64-n net (csrc/mpe_mlp_grad.h: P1..P7)"""
    return 4 * ((D + 1) // 2) + 4 * 32 + 2 * 32 + 4 * 8 + 4 * 32 + 4 * 32 + 32 * 2 * ((D + 31) // 32)


def backward_graph(outs, douts, params, K, s):
    """K backward passes of a retained autograd graph as one HIP graph, on the stream the forward ran on"""
    def fn(k):
        for p in params:
            p.grad = None
        torch.autograd.backward(outs, douts, retain_graph=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        for k in range(2):
            fn(k)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for k in range(K):
                fn(k)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    return g, fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    K = a.steps
    assert torch.cuda.is_available(), "mlp_grad_rate.py measures on a GPU: there is no CPU path"
    res = {"scenario": "simple_spread", "agents": 3, "modules": "3 x 18-64-64-5 Tanh, 3 x 18-64-64-1 Tanh", "T": T_STEPS,
           "backward_passes_per_graph": K, "graph_replays_per_timing": a.reps, "peak_fp32_mfma_flops": PEAK,
           "unit": "us per backward pass of all six modules, dL/dlogits and dL/dvalues to every weight's and bias's gradient", "sizes": {}}
    for B in (1024, 65536):
        torch.manual_seed(3)
        env = mpe.make_env("simple_spread", batch_size=B, seed=1)
        A = env.n
        M = T_STEPS * B // PARTS
        pi_m, vf_m = [mlp(5) for _ in range(A)], [mlp(1) for _ in range(A)]
        params = [p for m in pi_m + vf_m for p in m.parameters()]
        gen = torch.Generator(device="cuda").manual_seed(0)
        obs_n = [torch.randn(M, 18, generator=gen, device="cuda") for _ in range(A)]
        dlogits_n = [torch.randn(M, 5, generator=gen, device="cuda") / M for _ in range(A)]
        dvalues = torch.randn(A, M, generator=gen, device="cuda") / M
        pi, V = Actors(env, pi_m, mode="sample", logits=True).freeze(), Values(env, vf_m).freeze()

        def ours(k):
            mlp_grad_tensors(pi, obs_n, dlogits_n)
            mlp_grad_tensors(V, obs_n, [dvalues[i] for i in range(A)])
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            outs = [m(o) for m, o in zip(pi_m + vf_m, obs_n + obs_n)]
        douts = dlogits_n + [dvalues[i].view(M, 1) for i in range(A)]
        note = None
        try:
            torch_graph, torch_bwd = backward_graph(outs, douts, params, K, s)
        except Exception as e:      # (a capture the runtime refuses: the figure is then missing, said so)
            note, torch_graph = "backward-only capture failed: %s" % (str(e).splitlines() or [""])[0], None
            torch.cuda.synchronize()

            def torch_bwd(k):
                for p in params:
                    p.grad = None
                torch.autograd.backward(outs, douts, retain_graph=True)

        def fwd_bwd(k):
            for p in params:
                p.grad = None
            torch.autograd.backward([m(o) for m, o in zip(pi_m + vf_m, obs_n + obs_n)], douts)
        # ---- the same gradients, before timing
        torch_bwd(0)
        ours(0)
        torch.cuda.synchronize()
        ga, gv = mlp_grad_tensors(pi, obs_n, dlogits_n), mlp_grad_tensors(V, obs_n, [dvalues[i] for i in range(A)])
        torch.cuda.synchronize()
        worst, at = 0.0, 0
        for views in ga.modules + gv.modules:
            for w, b_ in views:
                for got in (w, b_):
                    want = params[at].grad
                    worst = max(worst, float((got - want).abs().max() / want.abs().max()))
                    at += 1
        assert at == len(params) and worst < 1e-4, worst
        legs = {"ours": graph_of(ours, K), "torch_eager": lambda: [torch_bwd(0) for _ in range(K)],
                "ours_eager": lambda: [ours(0) for _ in range(K)], "torch_fwd_bwd_graph": graph_of(fwd_bwd, K)}
        if torch_graph is not None:
            legs["torch_graph"] = torch_graph
        r = rounds(legs, K, a.reps)
        flops = 4096.0 * (mfma_steps_per_group(18) * ((M + 63) // 64)) * 2 * A
        r["equal_before_timing"] = {"gradients_max_relative_difference": worst}
        r["M"] = M
        r["mfma_flops_issued"] = flops
        r["mfma_floor_us"] = flops / PEAK * 1e6
        r["fraction_of_mfma_floor"] = r["mfma_floor_us"] / r["ours"]["median_us"]
        if torch_graph is not None:
            r["speedup_over_torch_graph"] = r["torch_graph"]["median_us"] / r["ours"]["median_us"]
            r["goal_met"] = r["ours"]["max_us"] < r["torch_graph"]["min_us"]
        else:
            r["note"] = note
        r["speedup_over_torch_eager"] = r["torch_eager"]["median_us"] / r["ours_eager"]["median_us"]
        r["speedup_over_torch_fwd_bwd_graph"] = r["torch_fwd_bwd_graph"]["median_us"] / r["ours"]["median_us"]
        res["sizes"]["B%d" % B] = r
        del legs, outs, torch_graph
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
