"""Time one PPO epoch of shuffled minibatches (onpolicy.Minibatches: mpe_adv_stats once, then four one-launch minibatches of
mpe_onpolicy_batch) against the same result in torch and against device copies of the same bytes, in ONE process, every leg as a
HIP graph of K epochs replayed several times, the legs alternating, three rounds (the method of tools/gae_rate.py): simple_spread
N = 3, a T = 25 step trajectory, B = 1024 and 65 536 worlds, M = T * B / 4.

    python tools/onpolicy_batch_rate.py [--steps 4] [--out profiles/onpolicy_batch_rate.json]

    ours          restats() + batch(e, 0..3): 2 + 4 launches; the device epoch counter is bumped inside the graph, so every epoch
                  of a replay is another shuffle
    torch_graph   mean / std / normalise over [A, T * B], then per minibatch and agent one index_select per field (obs, act, logp,
                  adv, ret, val) over a slice of a permutation -- captured as a graph: the yardstick.  Two things favour the torch
                  leg.  It is handed per-agent CONTIGUOUS [T * B, .] copies of every field, made outside the timing (the
                  trajectory's own layout has no such view: an agent's observation block is [T][B][D_i] with a step stride of
                  sum D_i * B).  And its torch.randperm(T * B) is drawn ONCE per size, outside the timing: with the randperm
                  inside the captured epoch, replaying the graph at T * B = 1 638 400 ended in an illegal memory access inside
                  torch's own radix sort (rocprim onesweep_iteration_kernel), so the shuffle's cost is left out of both torch legs
    torch_eager   the same calls issued one by one
    copy_floor    four device copies, each of the bytes ONE minibatch moves (rows read and written once; idx written)

The torch leg is checked against the launch for the same index set before anything is timed: every gathered field BIT-EQUAL, the
normalised advantage to 1e-5 (torch divides by std + eps, the rule multiplies by its reciprocal).  Figures are us per epoch from
device events around the replays (median of the rounds, min and max kept).  The goal: faster than the torch graph in every round by
more than either leg's spread (ours max < torch_graph min).  The fraction of the copy floor reached is recorded, with no bar."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd.onpolicy import Minibatches, Values, gae  # noqa: E402
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop  # noqa: E402
from replay_rate import graph_of, rounds  # noqa: E402

T_STEPS, EPISODE, GAMMA, LAM, EPS, PARTS = 25, 25, 0.95, 0.9, 1e-8, 4


def mlp(n_in, n_out):
    return nn.Sequential(nn.Linear(n_in, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, n_out)).cuda()


class TorchEpoch(object):
    """The torch leg: its own contiguous per-agent [N, .] fields, and one set of outputs."""

    def __init__(self, traj, g, widths, M):
        T, A, B = g.adv.shape
        off = [0]
        for d in widths:
            off.append(off[-1] + d)
        self.A, self.N, self.M = A, T * B, M
        self.obs = [traj.obs_in_flat[:, off[i] * B:off[i + 1] * B].reshape(T * B, widths[i]).contiguous() for i in range(A)]
        self.act = [traj.act[:, i].reshape(T * B, 5).contiguous() for i in range(A)]
        self.scal = {k: x.permute(1, 0, 2).reshape(A, T * B).contiguous() for k, x in
                     (("logp", traj.logp), ("adv", g.adv), ("ret", g.ret), ("val", traj.val))}
        self.out = None
        self.order = torch.randperm(self.N, device="cuda")      # once, outside every timed region and every graph (see above)

    def stats(self):
        adv = self.scal["adv"]
        self.norm = (adv - adv.mean(dim=1, keepdim=True)) / (adv.std(dim=1, keepdim=True) + EPS)

    def gather(self, idx):
        out = {"obs": [torch.index_select(self.obs[i], 0, idx) for i in range(self.A)],
               "act": [torch.index_select(self.act[i], 0, idx) for i in range(self.A)]}
        for k in ("logp", "ret", "val"):
            out[k] = [torch.index_select(self.scal[k][i], 0, idx) for i in range(self.A)]
        out["adv"] = [torch.index_select(self.norm[i], 0, idx) for i in range(self.A)]
        return out

    def epoch(self):
        self.stats()
        for k in range(PARTS):
            self.out = self.gather(self.order[k * self.M:(k + 1) * self.M])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    K = a.steps
    assert torch.cuda.is_available(), "onpolicy_batch_rate.py measures on a GPU: there is no CPU path"
    res = {"scenario": "simple_spread", "agents": 3, "T": T_STEPS, "minibatches_per_epoch": PARTS, "epochs_per_graph": K,
           "graph_replays_per_timing": a.reps, "torch_legs_exclude_randperm": True, "unit": "us per epoch (statistics once, four minibatches)", "sizes": {}}
    for B in (1024, 65536):
        torch.manual_seed(0)
        env = mpe.make_env("simple_spread", batch_size=B, seed=1)
        widths = [int(env._obs_off[i + 1] - env._obs_off[i]) for i in range(env.n)]
        loop = PolicyLoop(env, Actors(env, [mlp(18, 5) for _ in range(3)], mode="sample", logp=True), episode_len=EPISODE)
        traj = loop.run(T_STEPS, values=Values(env, [mlp(18, 1) for _ in range(3)]))
        g = gae(traj, GAMMA, LAM)
        N = T_STEPS * B
        M = N // PARTS
        counter = torch.zeros(1, dtype=torch.int64, device="cuda")
        mb = Minibatches(traj, g, M, seed=1, eps=EPS, epoch_counter=counter)
        te = TorchEpoch(traj, g, widths, M)
        # ---- equal for the same index set, before timing
        te.stats()
        worst = 0.0
        for k in range(PARTS):
            ours = mb.batch(0, k)
            theirs = te.gather(ours.idx)
            for i in range(env.n):
                assert torch.equal(ours.obs_n[i], theirs["obs"][i]) and torch.equal(ours.act[i], theirs["act"][i]), (B, k, i)
                for f in ("logp", "ret", "val"):
                    assert torch.equal(getattr(ours, f)[i], theirs[f][i]), (B, k, i, f)
                worst = max(worst, float((ours.adv[i] - theirs["adv"][i]).abs().max()))
        assert worst < 1e-5, worst
        torch.cuda.synchronize()

        def ours_epoch(k):
            mb.restats()
            for j in range(PARTS):
                mb.batch(0, j)
            counter.add_(1)
        row = sum(widths) + 5 * env.n + 4 * env.n
        nbytes = M * (row * 4 + 8)
        src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        legs = {"ours": graph_of(ours_epoch, K),
                "torch_graph": graph_of(lambda k: te.epoch(), K),
                "torch_eager": lambda: [te.epoch() for _ in range(K)],
                "copy_floor": graph_of(lambda k: [dst.copy_(src) for _ in range(PARTS)], K)}
        r = rounds(legs, K, a.reps)
        r["equal_before_timing"] = {"fields_bit_equal": True, "normalised_adv_max_abs_difference": worst}
        r["M"] = M
        r["bytes_gathered_per_minibatch"] = nbytes
        r["speedup_over_torch_graph"] = r["torch_graph"]["median_us"] / r["ours"]["median_us"]
        r["goal_met"] = r["ours"]["max_us"] < r["torch_graph"]["min_us"]
        r["fraction_of_copy_floor"] = r["copy_floor"]["median_us"] / r["ours"]["median_us"]
        res["sizes"]["B%d" % B] = r
        del legs, te, mb
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
