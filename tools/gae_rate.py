"""Time the one-launch GAE (onpolicy.gae_tensors: mpe_gae) against the same rule in torch and against a device copy of the same
bytes, in ONE process, every leg as a HIP graph of K computes replayed several times, the legs alternating, three rounds (the
method of tools/td_target_rate.py / tools/replay_rate.py): simple_spread N = 3, a T = 25 step trajectory of one whole episode
(episode_len = 25, phase 0), B = 1024 and 65 536 worlds.

    python tools/gae_rate.py [--steps 10] [--out profiles/gae_rate.json]

    gae           gae_tensors: one launch (B % 4 == 0 and torch's allocations are aligned: the 16-byte path)
    gae_scalar    the same launch writing to outputs that start 4 bytes past a 16-byte boundary: the scalar path, one chain per lane
    torch_graph   THE GAE RULE in torch -- a reverse loop over t of elementwise kernels (sub, mul, add, where, any) -- captured as a
                  graph: the yardstick
    torch_eager   the same calls issued one by one
    copy_floor    one device copy that moves as many bytes as the launch must: it reads rew, val (4 bytes each) and done (1) and
                  writes adv and ret (4 each), 17 bytes per (step, agent, world); the copy reads and writes 8.5 bytes per element

The torch rule and the launch are checked BIT-EQUAL before anything is timed.  Figures are us per compute from device events around
the replays (median of the rounds, min and max kept).  The goal: faster than the torch graph in every round by more than either
leg's spread (gae max < torch_graph min).  The fraction of the copy floor reached is recorded, with no bar.  Last, the closed loop's
us per step with and without values= (PolicyLoop.run(25), eager, host clock around a synchronise)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd.onpolicy import GaeResult, Values, gae_tensors, segments  # noqa: E402
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop  # noqa: E402
from replay_rate import graph_of, rounds  # noqa: E402

T_STEPS, EPISODE, GAMMA, LAM = 25, 25, 0.95, 0.9


def mlp(n_in, n_out):
    return nn.Sequential(nn.Linear(n_in, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, n_out)).cuda()


def torch_gae(rew, done, val, boot, L, p, out):
    """THE GAE RULE, one elementwise kernel per operation (torch fuses no multiply-add across them)."""
    T = rew.shape[0]
    g = torch.tensor(GAMMA, dtype=torch.float32)
    c = (g * torch.tensor(LAM, dtype=torch.float32)).item()
    g = g.item()
    k = segments(T, L, p) - 1
    adv, ret = out.adv, out.ret
    for t in range(T - 1, -1, -1):
        ends = t == T - 1 or (L > 0 and (p + t + 1) % L == 0)
        nv = boot[k] if ends else val[t + 1]
        delta = torch.where(done[t], rew[t] - val[t], (rew[t] + g * nv) - val[t])
        if ends:
            adv[t] = delta
            k -= 1
        else:
            adv[t] = torch.where(done[t].any(dim=0, keepdim=True), delta, delta + c * adv[t + 1])
        torch.add(adv[t], val[t], out=ret[t])
    return out


def loop_us_per_step(B, with_values, reps=5):
    torch.manual_seed(0)
    env = mpe.make_env("simple_spread", batch_size=B, seed=1)
    loop = PolicyLoop(env, Actors(env, [mlp(18, 5) for _ in range(3)], mode="sample", logp=True).freeze(), episode_len=EPISODE)
    V = Values(env, [mlp(18, 1) for _ in range(3)]).freeze() if with_values else None
    loop.run(T_STEPS, values=V)
    torch.cuda.synchronize()
    got = []
    for _ in range(reps):
        t0 = time.perf_counter()
        loop.run(T_STEPS, values=V)
        torch.cuda.synchronize()
        got.append((time.perf_counter() - t0) * 1e6 / T_STEPS)
    return {"median_us": statistics.median(got), "min_us": min(got), "max_us": max(got)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    K = a.steps
    assert torch.cuda.is_available(), "gae_rate.py measures on a GPU: there is no CPU path"
    res = {"scenario": "simple_spread", "agents": 3, "T": T_STEPS, "episode_len": EPISODE, "gamma": GAMMA, "lambda": LAM,
           "computes_per_graph": K, "graph_replays_per_timing": a.reps, "sizes": {}}
    for B in (1024, 65536):
        torch.manual_seed(0)
        env = mpe.make_env("simple_spread", batch_size=B, seed=1)
        loop = PolicyLoop(env, Actors(env, [mlp(18, 5) for _ in range(3)], mode="sample"), episode_len=EPISODE)
        traj = loop.run(T_STEPS, values=Values(env, [mlp(18, 1) for _ in range(3)]))
        rew, done, val, boot = traj.rew, traj.done, traj.val, traj.boot
        done = done | (torch.rand(done.shape, device=done.device) < 0.02)      # (the scenario never ends an episode: some dones, so both selects run)
        assert boot.shape[0] == 1 and traj.episode_phase == 0
        ours, theirs = GaeResult(torch.empty_like(rew), torch.empty_like(rew)), GaeResult(torch.empty_like(rew), torch.empty_like(rew))
        # ---- equal, before timing
        gae_tensors(rew, done, val, boot, GAMMA, LAM, EPISODE, 0, out=ours)
        torch_gae(rew, done, val, boot, EPISODE, 0, theirs)
        torch.cuda.synchronize()
        assert torch.equal(ours.adv, theirs.adv) and torch.equal(ours.ret, theirs.ret), B
        n = rew.numel()
        nbytes = (17 * n + 4 * boot.numel()) // 2
        src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        flat = [torch.empty(n + 1, dtype=torch.float32, device="cuda") for _ in range(2)]
        off16 = GaeResult(flat[0][1:].view(rew.shape), flat[1][1:].view(rew.shape))
        gae_tensors(rew, done, val, boot, GAMMA, LAM, EPISODE, 0, out=off16)
        assert torch.equal(off16.adv, ours.adv) and torch.equal(off16.ret, ours.ret), B
        legs = {"gae": graph_of(lambda k: gae_tensors(rew, done, val, boot, GAMMA, LAM, EPISODE, 0, out=ours), K),
                "gae_scalar": graph_of(lambda k: gae_tensors(rew, done, val, boot, GAMMA, LAM, EPISODE, 0, out=off16), K),
                "torch_graph": graph_of(lambda k: torch_gae(rew, done, val, boot, EPISODE, 0, theirs), K),
                "torch_eager": lambda: [torch_gae(rew, done, val, boot, EPISODE, 0, theirs) for _ in range(K)],
                "copy_floor": graph_of(lambda k: dst.copy_(src), K)}
        r = rounds(legs, K, a.reps)
        r["equal_before_timing"] = {"adv_bit_equal": True, "ret_bit_equal": True, "scalar_path_bit_equal": True, "done_fraction": float(done.float().mean())}
        r["bytes_moved_per_compute"] = 2 * nbytes
        for k in ("gae", "gae_scalar", "copy_floor"):
            r[k]["GB_per_s_read_plus_write"] = 2 * nbytes / r[k]["median_us"] * 1e-3
        r["speedup_over_torch_graph"] = r["torch_graph"]["median_us"] / r["gae"]["median_us"]
        r["goal_met"] = r["gae"]["max_us"] < r["torch_graph"]["min_us"]
        r["fraction_of_copy_floor"] = r["copy_floor"]["median_us"] / r["gae"]["median_us"]
        r["loop_us_per_step"] = {"without_values": loop_us_per_step(B, False), "with_values": loop_us_per_step(B, True)}
        res["sizes"]["B%d" % B] = r
        del legs
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
