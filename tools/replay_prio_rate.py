"""Time prioritized replay (replay.PrioritizedReplayBuffer: mpe_replay_prio_push / _draw / _update, mpe_replay_gather) in ONE
process, every leg as a HIP graph of K dependent launches replayed several times, the legs alternating, three rounds (the method
of tools/replay_rate.py): `simple` (one agent, 4-float observations: the smallest ring per transition) at 65 536 worlds, a ring of
S = 1024 steps -- 67 M priorities, a tree of seven levels.

    python tools/replay_prio_rate.py [--steps 20] [--slots 1024] [--out profiles/replay_prio_rate.json]

    push     PrioritizedReplayBuffer.push (two launches)  vs  ReplayBuffer.push (one) on the same commit
    sample   the draw and the gather (M = 1024 and 65 536)  vs  a torch batch over the same priorities: cumsum over all S * B of them,
             M stratified targets, searchsorted, one index_select per field -- as a graph
    update   update_priorities with the per-level launches  vs  the single launch whose last block climbs alone
             (MPE_REPLAY_PRIO_UPDATE=ticket), M = 1024 and 65 536

Every figure is us per push / per sample / per update from device events around the replays (median of the rounds, min and max kept)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd.replay import PrioritizedReplayBuffer, ReplayBuffer  # noqa: E402
from replay_rate import graph_of, rounds  # noqa: E402


def step_tensors(env):
    A, B, off = env.n, env.batch_size, env._obs_off
    act = torch.zeros((A, B, 5), device="cuda")
    act[..., 0] = 1
    flat0 = torch.cat([o.reshape(-1) for o in env.reset()])
    obs_n = [flat0[off[i] * B: off[i + 1] * B].view(B, off[i + 1] - off[i]) for i in range(A)]
    nxt, rew, done, _ = env.step(act)
    return obs_n, act, nxt, rew, done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--worlds", type=int, default=65536)
    ap.add_argument("--out")
    a = ap.parse_args()
    K, S, B = a.steps, a.slots, a.worlds
    env = mpe.make_env("simple", batch_size=B, seed=1)
    args = step_tensors(env)
    plain, prio = ReplayBuffer(env, steps=S), PrioritizedReplayBuffer(env, steps=S, seed=3)
    res = {"steps_per_graph": K, "graph_replays_per_timing": a.reps, "ring_steps": S, "worlds": B, "leaves": S * B,
           "tree_levels": len(prio.level_off) - 1}
    # ---- push
    res["push"] = rounds({"prioritized": graph_of(lambda k: prio.push(*args), K), "plain": graph_of(lambda k: plain.push(*args), K)}, K, a.reps)
    res["push"]["priority_launch_adds_us"] = res["push"]["prioritized"]["median_us"] - res["push"]["plain"]["median_us"]
    # ---- fill every slot, then priorities of a learner's spread
    for _ in range(S):
        prio.push(*args)
    torch.cuda.synchronize()
    prio.count = int(prio.head.item())
    n = S * B
    all_idx = torch.arange(n, device="cuda")
    prio.update_priorities(all_idx, (torch.rand(n, device="cuda") * 4 + 0.01).contiguous())
    torch.cuda.synchronize()
    leaves = prio.tree[:n]
    # torch's side gathers the same bytes per transition by index_select, from per-field [S * B, .] tensors (its best layout)
    flat = {"obs": torch.randn(n, 4, device="cuda"), "next": torch.randn(n, 4, device="cuda"), "act": torch.randn(n, 5, device="cuda"),
            "rew": torch.randn(n, device="cuda"), "done": torch.zeros(n, dtype=torch.bool, device="cuda")}
    res["sample"], res["update"] = {}, {}
    for M in (1024, 65536):
        def torch_batch(k, M=M):
            c = torch.cumsum(leaves, 0)
            x = (torch.arange(M, device="cuda") + torch.rand(M, device="cuda")) * (c[-1] / M)
            idx = torch.searchsorted(c, x).clamp_(max=n - 1)
            return idx, leaves.index_select(0, idx), {f: t.index_select(0, idx) for f, t in flat.items()}
        legs = {"draw_gather": graph_of(lambda k, M=M: prio.sample(M, draw=k), K), "torch_cumsum_searchsorted": graph_of(torch_batch, K)}
        r = rounds(legs, K, a.reps)
        r["done"] = r["draw_gather"]["median_us"] < r["torch_cumsum_searchsorted"]["median_us"]
        res["sample"]["M%d" % M] = r
        idx = torch.randint(0, n, (M,), device="cuda")
        new = (torch.rand(M, device="cuda") * 4 + 0.01).contiguous()
        os.environ.pop("MPE_REPLAY_PRIO_UPDATE", None)
        per_level = graph_of(lambda k: prio.update_priorities(idx, new), K)
        os.environ["MPE_REPLAY_PRIO_UPDATE"] = "ticket"
        ticket = graph_of(lambda k: prio.update_priorities(idx, new), K)
        os.environ.pop("MPE_REPLAY_PRIO_UPDATE", None)
        res["update"]["M%d" % M] = rounds({"per_level_launches": per_level, "last_ticket_block": ticket}, K, a.reps)
    u = res["update"]
    faster = "per_level_launches" if u["M1024"]["per_level_launches"]["median_us"] <= u["M1024"]["last_ticket_block"]["median_us"] \
        else "last_ticket_block"
    other = "last_ticket_block" if faster == "per_level_launches" else "per_level_launches"
    res["update"]["keep"] = faster if u["M65536"][faster]["median_us"] <= 2 * u["M65536"][other]["median_us"] else other
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
