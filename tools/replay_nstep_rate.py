"""Time the n-step sample (ReplayBuffer.sample(..., n_step=n): mpe_replay_sample_nstep) against the one-step sample
it extends and against the same work in torch, in ONE process with the method of tools/replay_rate.py: every leg a HIP graph of K
dependent launches replayed several times, the legs alternating, three rounds.  simple_spread N = 3 at 65 536 worlds, a full ring of
S = 64 steps, M = 1024 and 16 384, joint=True, gamma = 0.95, episode_len = 25.

    python tools/replay_nstep_rate.py [--steps 50] [--out profiles/replay_nstep_rate.json]

    one_step      ReplayBuffer.sample(M, joint=True): the yardstick
    nstep_n1/3/5  the same with n_step = 1, 3, 5: one launch each
    torch_*_n5    the n = 5 rule in torch on top of the one-step sample: the ring's rew / done indexed once per step, a masked scan,
                  and a second full gather (ReplayBuffer.gather) at the computed last index -- as a graph and eager
The torch restatement is checked against the kernel once (ret, discount, n_used, last: equal) before anything is timed.
Every figure is us per minibatch from device events around the replays (median of the rounds, min and max kept)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd.replay import ReplayBuffer  # noqa: E402
from replay_rate import graph_of, rounds  # noqa: E402

S, GAMMA, EPISODE = 64, 0.95, 25


def filled_ring(env):
    """A ring with every slot pushed: S real steps of the env under a fixed move, each pushed as env.step returns it."""
    A, B = env.n, env.batch_size
    buf = ReplayBuffer(env, steps=S, seed=7)
    act = torch.zeros((A, B, 5), device="cuda")
    act[..., 1] = 1
    obs_n = [o.clone() for o in env.reset()]
    for _ in range(S):
        nxt, rew, done, _ = env.step(act)
        buf.push(obs_n, act, nxt, rew, done)
        for o, x in zip(obs_n, nxt):
            o.copy_(x)
    torch.cuda.synchronize()
    assert int(buf.head.item()) == buf.count == S
    return buf


def torch_nstep(buf, M, draw, n, gamma, L, p=0):
    """The rule of include/mpe_hip.h in torch ops on device tensors only (capturable): -> (one-step batch, ret [A,M], discount [M],
    n_used [M], last [M], the batch gathered at last)."""
    b = buf.sample(M, draw=draw, joint=True)
    B = buf.B
    slot, world = b.idx // B, b.idx % B
    h = buf.head
    ahead = (h - 1 - slot) % S
    g = h - 1 - ahead
    gam = float(gamma)      # (a float32 tensor times a Python float is a float32 product)
    ret = buf.rew[slot, :, world].t().contiguous()      # [A,M]
    d = torch.ones(M, dtype=torch.float32, device=b.idx.device)
    m = torch.ones(M, dtype=torch.int64, device=b.idx.device)
    alive = torch.ones(M, dtype=torch.bool, device=b.idx.device)
    for k in range(1, n):
        prev = (slot + (k - 1)) % S
        stop = buf.done[prev, :, world].any(dim=1) | (ahead < k)
        if L > 0:
            stop = stop | ((g + k + p) % L == 0)
        alive = alive & ~stop
        dk = d * gam
        term = dk.unsqueeze(0) * buf.rew[(slot + k) % S, :, world].t()
        ret = torch.where(alive.unsqueeze(0), ret + term, ret)
        d = torch.where(alive, dk, d)
        m = m + alive.to(torch.int64)
    last = ((slot + m - 1) % S) * B + world
    return b, ret, d * gam, m, last, buf.gather(last, joint=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--worlds", type=int, default=65536)
    ap.add_argument("--out")
    a = ap.parse_args()
    K = a.steps
    env = mpe.make_env("simple_spread", batch_size=a.worlds, seed=1)
    buf = filled_ring(env)
    D = buf.obs_widths
    res = {"scenario": "simple_spread", "agents": buf.A, "worlds": buf.B, "ring_steps": S, "gamma": GAMMA, "episode_len": EPISODE,
           "steps_per_graph": K, "graph_replays_per_timing": a.reps, "joint": True, "sizes": {}}
    for M in (1024, 16384):
        # the restatement against the kernel, once, on the same draw
        nb = buf.sample(M, draw=3, joint=True, n_step=5, gamma=GAMMA, episode_len=EPISODE)
        _, ret, disc, m, last, at_last = torch_nstep(buf, M, 3, 5, GAMMA, EPISODE)
        torch.cuda.synchronize()
        same = bool(torch.equal(ret.view(torch.int32), nb.ret.view(torch.int32)) and torch.equal(disc, nb.discount) and
                    torch.equal(m.to(torch.int32), nb.n_used) and torch.equal(last, nb.last) and
                    torch.equal(at_last.joint_next, nb.joint_next))
        if not same:
            raise SystemExit("the torch restatement and the kernel disagree at M = %d" % M)
        legs = {"one_step": graph_of(lambda k, M=M: buf.sample(M, draw=k, joint=True), K)}
        for n in (1, 3, 5):
            legs["nstep_n%d" % n] = graph_of(lambda k, M=M, n=n: buf.sample(M, draw=k, joint=True, n_step=n, gamma=GAMMA,
                                                                             episode_len=EPISODE), K)
        legs["torch_graph_n5"] = graph_of(lambda k, M=M: torch_nstep(buf, M, k, 5, GAMMA, EPISODE), K)
        legs["torch_eager_n5"] = lambda M=M: [torch_nstep(buf, M, k, 5, GAMMA, EPISODE) for k in range(K)]
        r = rounds(legs, K, a.reps)
        one = r["one_step"]["median_us"]
        r["torch_restatement_equals_kernel"] = same
        r["mean_n_used_n5"] = float(nb.n_used.to(torch.float32).mean().item())
        r["row_bytes_read_per_sample"] = 2 * sum(D) * 4 + buf.A * (5 * 4 + 4 + 1)      # obs, next obs, move, reward, done of every agent
        r["nstep_extra_read_bytes_per_sample_at_most"] = {"n%d" % n: n * buf.A * 5 for n in (1, 3, 5)}
        for n in (1, 3, 5):
            r["nstep_n%d_over_one_step" % n] = r["nstep_n%d" % n]["median_us"] / one
        r["torch_graph_n5_over_nstep_n5"] = r["torch_graph_n5"]["median_us"] / r["nstep_n5"]["median_us"]
        r["within_1p5x"] = r["nstep_n5_over_one_step"] <= 1.5
        res["sizes"]["M%d" % M] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
