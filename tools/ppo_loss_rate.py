"""Time the PPO loss head (onpolicy.PpoLoss: mpe_ppo_loss's two launches forward, one multiply backward) against the same loss in
torch autograd and against a device copy of the bytes it has to move, in ONE process, every leg as a HIP graph of K loss heads
replayed several times, the legs alternating, three rounds (the method of tools/onpolicy_batch_rate.py): simple_spread N = 3
(three movers, 5 logits each), T = 25, B = 1024 and 65 536 worlds, one minibatch of M = T * B / 4 rows.

    python tools/ppo_loss_rate.py [--steps 4] [--out profiles/ppo_loss_rate.json]

Every leg is the loss head ONLY, forward and backward: it starts from leaf logits_n [M, 5] / values_n [M, 1] tensors (what the
networks would have produced) and ends at their .grad.

    ours          PpoLoss(env, clip, vf_coef=0.5)(logits_n, values_n, batch) and loss.backward()
    torch_graph   losses() of examples/ppo_spread.py per agent (log_softmax, * act, sum, exp, clamp, min, mean, mse_loss), summed as
                  the example sums them, and backward() -- captured as a graph: the yardstick
    torch_eager   the same calls issued one by one
    copy_floor    one device copy that moves the compulsory bytes of the head: per row and agent the logits read and their gradient
                  written (8 * n_out), the move row read (20), logp_old, adv, ret, val_old and v read and dL/dv written (24)

Both legs are checked against each other before anything is timed (loss and gradients to 1e-5 of their largest magnitude).  Figures
are us per loss head from device events around the replays (median of the rounds, min and max kept).  The goal: faster than the
torch graph at both sizes in every round (ours max < torch_graph min).  The fraction of the copy floor reached is recorded, with no
bar."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd.onpolicy import OnPolicyBatch, PpoLoss  # noqa: E402
from replay_rate import graph_of, rounds  # noqa: E402

T_STEPS, PARTS, CLIP, VF = 25, 4, 0.2, 0.5


def synthetic(A, M, n_out):
    """leaf logits and values, and a minibatch's own tensors with a spread of ratios around the clip"""
    gen = torch.Generator(device="cuda").manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=gen, device="cuda")      # noqa: E731
    logits_n = [(1.5 * rn(M, n_out)).requires_grad_() for _ in range(A)]
    values_n = [rn(M, 1).requires_grad_() for _ in range(A)]
    b = OnPolicyBatch()
    b.M = M
    b.act = F.one_hot(torch.randint(0, n_out, (A, M), generator=gen, device="cuda"), n_out).float().contiguous()
    b.utter = None
    with torch.no_grad():
        lp = torch.stack([(F.log_softmax(logits_n[i], dim=-1) * b.act[i]).sum(-1) for i in range(A)])
    b.logp = (lp + 0.3 * rn(A, M)).contiguous()
    b.adv, b.ret, b.val = rn(A, M), rn(A, M), rn(A, M)
    return logits_n, values_n, b


def torch_losses(logits_n, values_n, b):
    """examples/ppo_spread.py: losses() per agent and the example's summation"""
    policy_loss = value_loss = 0.0
    for i in range(len(logits_n)):
        logp = (F.log_softmax(logits_n[i], dim=-1) * b.act[i]).sum(dim=-1)
        ratio = torch.exp(logp - b.logp[i])
        policy_loss = policy_loss - torch.min(ratio * b.adv[i], ratio.clamp(1 - CLIP, 1 + CLIP) * b.adv[i]).mean()
        value_loss = value_loss + F.mse_loss(values_n[i][..., 0], b.ret[i])
    return policy_loss + VF * value_loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    K = a.steps
    assert torch.cuda.is_available(), "ppo_loss_rate.py measures on a GPU: there is no CPU path"
    res = {"scenario": "simple_spread", "agents": 3, "n_out": 5, "T": T_STEPS, "loss_heads_per_graph": K, "graph_replays_per_timing": a.reps,
           "unit": "us per loss head, forward and backward, leaf logits / values to their .grad", "sizes": {}}
    for B in (1024, 65536):
        env = mpe.make_env("simple_spread", batch_size=B, seed=1)
        A, n_out = env.n, 5
        M = T_STEPS * B // PARTS
        logits_n, values_n, b = synthetic(A, M, n_out)
        leaves = logits_n + values_n
        head = PpoLoss(env, clip=CLIP, vf_coef=VF)

        def ours(k):
            for x in leaves:
                x.grad = None
            head(logits_n, values_n, b).backward()

        def theirs(k):
            for x in leaves:
                x.grad = None
            torch_losses(logits_n, values_n, b).backward()
        # ---- the same loss and gradients, before timing
        ours(0)
        mine = [float(head.last.loss)] + [x.grad.clone() for x in leaves]
        theirs(0)
        want = [float(torch_losses(logits_n, values_n, b))] + [x.grad.clone() for x in leaves]
        worst = abs(mine[0] - want[0]) / max(abs(want[0]), 1e-30)
        for g, w in zip(mine[1:], want[1:]):
            worst = max(worst, float((g - w).abs().max() / w.abs().max()))
        assert worst < 1e-5, worst
        torch.cuda.synchronize()
        row = 8 * n_out + 20 + 24
        nbytes = A * M * row
        src, dst = torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.zeros(nbytes // 2, dtype=torch.uint8, device="cuda")
        legs = {"ours": graph_of(ours, K),
                "torch_graph": graph_of(theirs, K),
                "torch_eager": lambda: [theirs(0) for _ in range(K)],
                "ours_eager": lambda: [ours(0) for _ in range(K)],
                "copy_floor": graph_of(lambda k: dst.copy_(src), K)}
        r = rounds(legs, K, a.reps)
        r["equal_before_timing"] = {"loss_and_gradients_max_relative_difference": worst}
        r["M"] = M
        r["compulsory_bytes_per_row_and_agent"] = row
        r["compulsory_bytes"] = nbytes
        r["speedup_over_torch_graph"] = r["torch_graph"]["median_us"] / r["ours"]["median_us"]
        r["speedup_over_torch_eager"] = r["torch_eager"]["median_us"] / r["ours_eager"]["median_us"]
        r["goal_met"] = r["ours"]["max_us"] < r["torch_graph"]["min_us"]
        r["fraction_of_copy_floor"] = r["copy_floor"]["median_us"] / r["ours"]["median_us"]
        r["ours_GB_per_s_compulsory"] = nbytes / r["ours"]["median_us"] * 1e-3
        res["sizes"]["B%d" % B] = r
        del legs, head
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
