"""Time a 64-64 MLP actor in the loop with simple_spread (N = 3) at 65 536 worlds, three ways, and print one JSON line:

    python tools/policy_rate.py [--steps 50] [--worlds 65536] [--out FILE]

    fused   PolicyRollout.run(steps): one mpe_rollout_policy launch (actor, move, World.step, rewards, resets)
    eager   the loop a user writes today: MlpPolicy modules -> argmax -> one-hot -> env.step, eager torch
    graph   the same loop captured once with torch.cuda.graph (if it captures) and replayed

Per way: us per step, env-steps/s, and the actor's achieved fraction of the 157.3 TFLOP/s fp32 peak (2 FLOP per
multiply-add of the actor: 5 568 multiply-adds per agent-world-step for 18 -> 64 -> 64 -> 5)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd.rollout import MlpPolicy, PolicyRollout  # noqa: E402

PEAK = 157.3e12


def actors(env):
    torch.manual_seed(0)
    mods = []
    for i in range(env.n):
        D = int(env._obs_off[i + 1] - env._obs_off[i])
        mods.append(torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                                        torch.nn.Linear(64, 5)).cuda())
    return mods


def timed(fn, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--worlds", type=int, default=65536)
    ap.add_argument("--out")
    a = ap.parse_args()
    B, K = a.worlds, a.steps
    env = mpe.make_env("simple_spread", batch_size=B, seed=1)
    obs_n = env.reset()
    mods = actors(env)
    pol = MlpPolicy(mods)
    fmas = sum(l.in_features * l.out_features for l in mods[0] if isinstance(l, torch.nn.Linear))
    flop_step = 2.0 * fmas * env.n * B
    res = {"scenario": "simple_spread", "agents": env.n, "worlds": B, "steps": K, "actor": "18-64-64-5 relu",
           "fma_per_agent_world_step": fmas}

    roll = PolicyRollout(env, pol, episode_len=25)
    traj = roll.run(K)                       # warm-up (and the trajectory buffers, reused below)
    torch.cuda.synchronize()
    us = timed(lambda: roll.run(K, trajectory=traj), K)
    res["fused"] = {"us_per_step": us, "env_steps_per_s": B / (us * 1e-6), "fp32_peak_fraction": flop_step / (us * 1e-6) / PEAK}

    obs = [o for o in env.reset()]

    def loop(n):
        nonlocal obs
        for _ in range(n):
            rows = pol.action(obs, mode="greedy")
            obs = env.step(torch.stack(rows))[0]
    loop(3)
    torch.cuda.synchronize()
    us = timed(lambda: loop(K), K)
    res["eager"] = {"us_per_step": us, "env_steps_per_s": B / (us * 1e-6), "fp32_peak_fraction": flop_step / (us * 1e-6) / PEAK}

    try:
        static_obs = [o.clone() for o in obs]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            for _ in range(2):
                rows = pol.action(static_obs, mode="greedy")
                out = env.step(torch.stack(rows))[0]
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                rows = pol.action(static_obs, mode="greedy")
                out = env.step(torch.stack(rows))[0]
                for i in range(env.n):
                    static_obs[i].copy_(out[i])
        torch.cuda.current_stream().wait_stream(s)
        g.replay()
        torch.cuda.synchronize()

        def replay(n):
            for _ in range(n):
                g.replay()
        us = timed(lambda: replay(K), K)
        res["graph"] = {"us_per_step": us, "env_steps_per_s": B / (us * 1e-6), "fp32_peak_fraction": flop_step / (us * 1e-6) / PEAK}
    except Exception as e:       # (a loop the graph cannot capture is reported, not hidden)
        res["graph"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
