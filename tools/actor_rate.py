"""Per-step time of the closed loop with the standalone actor kernel (policy.PolicyLoop, eager and as a HIP graph) next to
tools/policy_rate.py's legs (PolicyRollout fused, the eager torch loop, the torch loop as a graph), measured in ONE process, three
times: simple_spread N = 3 at 65 536 worlds and simple_tag at 16 384 worlds, 18-64-64-5 style ReLU actors.

    python tools/actor_rate.py [--steps 50] [--out profiles/actor_rate.json]
    python tools/actor_rate.py --kernel-only        # the actor launch alone, for a `rocprofv3 --kernel-trace --stats` run

The actor kernel's own time comes from the kernel trace (k_actor), its floor from 5 568 multiply-adds per agent-world at the
157.3 TFLOP/s fp32 peak (13.9 us for simple_spread at 65 536 worlds)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop  # noqa: E402
from multiagent_particle_envs_amd.rollout import MlpPolicy, PolicyRollout  # noqa: E402
from policy_rate import PEAK, actors, timed  # noqa: E402


def torch_legs(env, pol, K):
    """tools/policy_rate.py's eager and graph legs: MlpPolicy.action -> torch.stack -> env.step"""
    obs = [o for o in env.reset()]

    def loop(n):
        nonlocal obs
        for _ in range(n):
            obs = env.step(torch.stack(pol.action(obs, mode="greedy")))[0]
    loop(3)
    torch.cuda.synchronize()
    eager = timed(lambda: loop(K), K)
    static_obs = [o.clone() for o in obs]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        for _ in range(2):
            out = env.step(torch.stack(pol.action(static_obs, mode="greedy")))[0]
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            out = env.step(torch.stack(pol.action(static_obs, mode="greedy")))[0]
            for i in range(env.n):
                static_obs[i].copy_(out[i])
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    return eager, timed(lambda: [g.replay() for _ in range(K)], K)


def loop_legs(env, mods, K):
    pi = Actors(env, mods, mode="greedy").freeze()
    loop = PolicyLoop(env, pi, episode_len=25)
    loop.run(K, record=False)
    torch.cuda.synchronize()
    eager = timed(lambda: loop.run(K, record=False), K)
    loop.t = 0
    g = loop.capture(K)
    g.replay()
    torch.cuda.synchronize()
    return eager, timed(lambda: [g.replay() for _ in range(2)], 2 * K)


def differing_rows(B=4000, T=30):
    """rows mpe_actor_act and mpe_rollout_policy choose differently on the same recorded inputs (sample mode, same seed)"""
    env = mpe.make_env("simple_spread", batch_size=B, seed=7)
    env.reset()
    mods = actors(env)
    traj = PolicyRollout(env, MlpPolicy(mods), mode="sample", episode_len=25, policy_seed=9).run(T, record_inputs=True)
    pi = Actors(env, mods, mode="sample", seed=9)
    n = sum(int((pi.act(traj.obs_in[t], t) != traj.act[t]).any(dim=-1).sum()) for t in range(T))
    return {"rows": T * env.n * B, "differ": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--kernel-us", type=float, help="k_actor's average time from the kernel trace (simple_spread shape), recorded")
    a = ap.parse_args()
    K = a.steps
    if a.kernel_only:
        env = mpe.make_env("simple_spread", batch_size=65536, seed=1)
        obs = env.reset()
        pi = Actors(env, actors(env), mode="greedy").freeze()
        for t in range(200):
            pi.act(obs, t)
        torch.cuda.synchronize()
        return
    res = {"steps": K, "shapes": []}
    for name, B in (("simple_spread", 65536), ("simple_tag", 16384)):
        env = mpe.make_env(name, batch_size=B, seed=1)
        env.reset()
        mods = actors(env)
        pol = MlpPolicy(mods)
        fmas = sum(sum(l.in_features * l.out_features for l in m if isinstance(l, torch.nn.Linear)) for m in mods)
        rec = {"scenario": name, "agents": env.n, "worlds": B, "actor": "D-64-64-5 relu", "fp32_floor_us": 2.0 * fmas * B / PEAK * 1e6,
               "runs": []}
        for _ in range(3):
            te, tg = torch_legs(env, pol, K)
            le, lg = loop_legs(env, mods, K)
            rec["runs"].append({"torch_eager_us": te, "torch_graph_us": tg, "policy_loop_eager_us": le, "policy_loop_graph_us": lg})
        if name == "simple_spread":
            roll = PolicyRollout(env, pol, episode_len=25)
            traj = roll.run(K)
            torch.cuda.synchronize()
            rec["policy_rollout_fused_us"] = timed(lambda: roll.run(K, trajectory=traj), K)
            if a.kernel_us:
                rec["actor_kernel_us"] = a.kernel_us
                rec["actor_kernel_fp32_peak_fraction"] = rec["fp32_floor_us"] / a.kernel_us
        tg = [r["torch_graph_us"] for r in rec["runs"]]
        lg = [r["policy_loop_graph_us"] for r in rec["runs"]]
        spread = max(max(tg) - min(tg), max(lg) - min(lg))
        rec["goal_met"] = all(r["torch_graph_us"] - r["policy_loop_graph_us"] > spread for r in rec["runs"])
        res["shapes"].append(rec)
    res["rows_differing_from_policy_rollout"] = differing_rows()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
