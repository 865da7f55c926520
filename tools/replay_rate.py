"""Time the replay buffer (replay.ReplayBuffer: mpe_replay_push / mpe_replay_sample) against what torch offers for the same work,
in ONE process, every leg as a HIP graph of K dependent launches replayed several times, the legs alternating, three rounds:
simple_spread N = 3 at 65 536 worlds and simple_tag at 16 384 worlds, a ring of S = 16 steps.

    python tools/replay_rate.py [--steps 50] [--out profiles/replay_rate.json]

    push     one mpe_replay_push per step   vs  the copy_ calls that store the same fields into a LoopTrajectory-shaped ring (five:
             obs, next obs, act, rew, done)  vs  ONE copy_ of the same byte count (the floor)
    sample   one mpe_replay_sample per minibatch (M = 1024 and 65 536, with and without the joint rows)  vs  torch: randint, one
             index_select per field per agent on per-agent [S * B, .] tensors (torch's best layout), cat for the joint rows --
             eager and as a graph
    loop     PolicyLoop.capture(T) with and without replay=

Every figure is us per push / per sample / per step from device events around the replays (median of the rounds, min and max kept)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop  # noqa: E402
from multiagent_particle_envs_amd.replay import ReplayBuffer  # noqa: E402
from policy_rate import actors, timed  # noqa: E402

S = 16


def graph_of(fn, K):
    """K calls of fn(k) as one graph (two really run first)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
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
    return g


def rounds(legs, K, reps, n=3):
    """legs {name: graph or callable running K units}: n rounds, the legs alternating -> {name: {median, min, max}} us per unit."""
    got = {k: [] for k in legs}
    for _ in range(n):
        for name, leg in legs.items():
            run = leg.replay if hasattr(leg, "replay") else leg
            got[name].append(timed(lambda: [run() for _ in range(reps)], reps * K))
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in got.items()}


def push_legs(env, K, reps):
    A, B, off = env.n, env.batch_size, env._obs_off
    act = torch.zeros((A, B, 5), device="cuda")
    act[..., 0] = 1
    flat0 = torch.cat([o.reshape(-1) for o in env.reset()])      # the pre-step observation, kept beside the env's two output sets
    obs_n = [flat0[off[i] * B: off[i + 1] * B].view(B, off[i + 1] - off[i]) for i in range(A)]
    nxt, rew, done, _ = env.step(act)
    o1 = env._sets[env._flip]
    buf = ReplayBuffer(env, steps=S)
    ours = graph_of(lambda k: buf.push(obs_n, act, nxt, rew, done), K)
    ring = {"obs": torch.zeros((S, int(off[-1]) * B), device="cuda"), "next": torch.zeros((S, int(off[-1]) * B), device="cuda"),
            "act": torch.zeros((S, A, B, 5), device="cuda"), "rew": torch.zeros((S, A, B), device="cuda"),
            "done": torch.zeros((S, A, B), dtype=torch.bool, device="cuda")}

    def copies(k):
        s = k % S
        ring["obs"][s].copy_(flat0)
        ring["next"][s].copy_(o1.obs)
        ring["act"][s].copy_(act)
        ring["rew"][s].copy_(o1.rew)
        ring["done"][s].copy_(o1.done)
    nbytes = 2 * flat0.numel() * 4 + act.numel() * 4 + o1.rew.numel() * 4 + o1.done.numel()
    a, b = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.zeros((S, nbytes), dtype=torch.uint8, device="cuda")
    res = rounds({"push": ours, "torch_copies": graph_of(copies, K), "one_copy_floor": graph_of(lambda k: b[k % S].copy_(a), K)}, K, reps)
    buf.count = int(buf.head.item())      # (graph replays advanced the device-side count)
    res["bytes_per_push"] = nbytes
    for k in ("push", "torch_copies", "one_copy_floor"):
        res[k]["GB_per_s_read_plus_write"] = 2 * nbytes / res[k]["median_us"] * 1e-3
    res["push_fraction_of_floor"] = res["one_copy_floor"]["median_us"] / res["push"]["median_us"]
    res["done"] = res["push"]["median_us"] <= res["torch_copies"]["median_us"]
    return res, buf


def sample_legs(env, buf, K, reps):
    """buf: a full ring (every slot pushed)."""
    A, B, off = env.n, env.batch_size, env._obs_off
    n_valid = S * B
    D = [int(off[i + 1] - off[i]) for i in range(A)]
    tr = {"obs": [torch.randn(n_valid, d, device="cuda") for d in D], "next": [torch.randn(n_valid, d, device="cuda") for d in D],
          "act": [torch.randn(n_valid, 5, device="cuda") for _ in D], "rew": [torch.randn(n_valid, device="cuda") for _ in D],
          "done": [torch.zeros(n_valid, dtype=torch.bool, device="cuda") for _ in D]}
    out = {}
    for M in (1024, 65536):
        for joint in (False, True):
            def torch_batch(k, M=M, joint=joint):
                idx = torch.randint(0, n_valid, (M,), device="cuda")
                b = {f: [t.index_select(0, idx) for t in tr[f]] for f in tr}
                if joint:
                    b["joint"] = torch.cat(b["obs"] + b["act"], dim=1)
                    b["joint_next"] = torch.cat(b["next"], dim=1)
                return b
            legs = {"sample": graph_of(lambda k, M=M, joint=joint: buf.sample(M, draw=k, joint=joint), K),
                    "torch_graph": graph_of(torch_batch, K), "torch_eager": lambda f=torch_batch: [f(k) for k in range(K)]}
            r = rounds(legs, K, reps)
            r["done"] = r["sample"]["median_us"] < r["torch_graph"]["median_us"]
            r["bytes_gathered"] = M * (2 * sum(D) * 4 + A * (5 * 4 + 4 + 1)) * (2 if joint else 1)
            out["M%d%s" % (M, "_joint" if joint else "")] = r
    return out


def loop_legs(env, K):
    mods = actors(env)
    res = {}
    for name, with_buf in (("capture", False), ("capture_replay", True), ("capture_again", False)):
        pi = Actors(env, mods, mode="greedy").freeze()
        loop = PolicyLoop(env, pi, episode_len=25)
        buf = ReplayBuffer(env, steps=S) if with_buf else None
        g = loop.capture(K, replay=buf)
        g.replay()
        torch.cuda.synchronize()
        v = [timed(lambda: [g.replay() for _ in range(2)], 2 * K) for _ in range(3)]
        res[name] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
        del g, buf
    res["replay_adds_us_per_step"] = res["capture_replay"]["median_us"] - min(res["capture"]["median_us"], res["capture_again"]["median_us"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    K = a.steps
    res = {"steps_per_graph": K, "graph_replays_per_timing": a.reps, "ring_steps": S, "shapes": []}
    for name, B in (("simple_spread", 65536), ("simple_tag", 16384)):
        env = mpe.make_env(name, batch_size=B, seed=1)
        rec = {"scenario": name, "agents": env.n, "worlds": B}
        rec["push"], buf = push_legs(env, K, a.reps)
        rec["sample"] = sample_legs(env, buf, K, a.reps)
        del buf
        rec["loop"] = loop_legs(env, K)
        res["shapes"].append(rec)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
