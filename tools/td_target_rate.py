"""Time the two-launch TD target (learner.TdTargets: mpe_actor_act_rows, mpe_critic_q) against the same target in torch, in ONE
process, every leg as a HIP graph of K dependent computes replayed several times, the legs alternating, three rounds (the method
of tools/replay_rate.py): simple_spread N = 3, 64-64 target actors (softmax mode) and 64-64 centralised target critics, a
minibatch of M = 1024 and of 65 536 rows with 3-step returns.

    python tools/td_target_rate.py [--steps 20] [--out profiles/td_target_rate.json]

    td_targets    TdTargets.compute(batch): two launches, weights frozen
    torch_graph   the same target in torch -- A actor forwards with a softmax, a cat, A critic forwards, the target arithmetic
                  (the where of the y rule) -- captured as a graph: the yardstick
    torch_eager   the same calls issued one by one

The two are checked equal before anything is timed: the action columns within 1e-5 * max(1, max|z|), q within 1e-5 * max(1, |q|)
of torch's float32 pass on the kernel's own rows, y bit-equal to the rule on the kernel's own q.  Figures are us per compute from
device events around the replays (median of the rounds, min and max kept).  The goal is DESIGN.md 2.10's: faster than the torch
graph in each round by more than either leg's spread."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd.learner import Critics, TdTargets  # noqa: E402
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop  # noqa: E402
from multiagent_particle_envs_amd.replay import ReplayBuffer  # noqa: E402
from policy_rate import actors  # noqa: E402
from replay_rate import graph_of, rounds  # noqa: E402


def mlp(n_in, n_out):
    return nn.Sequential(nn.Linear(n_in, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, n_out)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    K = a.steps
    torch.manual_seed(0)
    env = mpe.make_env("simple_spread", batch_size=4096, seed=1)
    A = env.n
    loop = PolicyLoop(env, Actors(env, actors(env), mode="sample"), episode_len=25)
    buf = ReplayBuffer(env, steps=32)
    loop.run(40, record=False, replay=buf)
    mu_t = [mlp(18, 5) for _ in range(A)]
    q_t = [mlp(buf.joint_width, 1) for _ in range(A)]
    pi, cr = Actors(env, mu_t, mode="softmax", logits=True).freeze(), Critics(env, q_t).freeze()
    td = TdTargets(pi, cr)
    res = {"scenario": "simple_spread", "agents": A, "nets": "64-64", "computes_per_graph": K, "graph_replays_per_timing": a.reps, "sizes": {}}
    for M in (1024, 65536):
        batch = buf.sample(M, draw=7, joint=True, n_step=3, gamma=0.95, episode_len=25)
        ret, disc, done, nxt = batch.ret, batch.discount, batch.done, batch.next_obs_n

        def torch_target():
            with torch.no_grad():
                acts = [torch.softmax(mu_t[i](nxt[i]), dim=1) for i in range(A)]
                joint = torch.cat(list(nxt) + acts, dim=1)
                q = torch.stack([q_t[i](joint)[:, 0] for i in range(A)])
                return joint, q, torch.where(done, ret, ret + disc[None, :] * q)
        # ---- equal, before timing
        y = td.compute(batch, t=0)
        joint_t, _, _ = torch_target()
        z = pi.rows.logits[:, :, :5].abs().amax(dim=2).clamp(min=1)      # [A, M]
        err_a = max(float(((td.joint_next_act[:, 54 + 5 * i:59 + 5 * i] - joint_t[:, 54 + 5 * i:59 + 5 * i]).abs().amax(dim=1) / (1e-5 * z[i])).max())
                    for i in range(A))
        with torch.no_grad():
            q_own = torch.stack([q_t[i](td.joint_next_act)[:, 0] for i in range(A)])      # torch's critics on the kernel's own rows
        err_q = float(((td.q_next - q_own).abs() / (1e-5 * q_own.abs().clamp(min=1))).max())
        y_rule = torch.where(done, ret, ret + disc[None, :] * td.q_next)
        ok = torch.equal(td.joint_next_act[:, :54], batch.joint_next) and err_a < 1 and err_q < 1 and torch.equal(y, y_rule)
        assert ok, (M, err_a, err_q)
        legs = {"td_targets": graph_of(lambda k: td.compute(batch, t=k), K), "torch_graph": graph_of(lambda k: torch_target(), K),
                "torch_eager": lambda: [torch_target() for _ in range(K)]}
        r = rounds(legs, K, a.reps)
        r["equal_before_timing"] = {"action_columns_error_over_bar": err_a, "q_error_over_bar": err_q, "y_bit_equal_to_rule": True}
        r["speedup_over_torch_graph"] = r["torch_graph"]["median_us"] / r["td_targets"]["median_us"]
        r["goal_met"] = r["td_targets"]["max_us"] < r["torch_graph"]["min_us"]
        res["sizes"]["M%d" % M] = r
        del legs
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
