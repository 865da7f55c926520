"""Time the value-based learners' device pieces in ONE process, every leg as a HIP graph of K dependent passes
replayed several times, the legs alternating, three rounds, and print one JSON line:

    python tools/q_loss_rate.py [--steps 4] [--reps 10] [--out profiles/q_loss_rate.json] [--parent-loop FILE ...]
    python tools/q_loss_rate.py --greedy-loop-only            (one JSON line: the greedy closed loop alone)

    head    simple_spread N = 3, M = 1 024 and 65 536, double-Q, both mixes: q_loss_tensors (mpe_q_loss: the loss AND dL/dlogits)
            and the backward's one multiply  vs  the same rule in torch (gather, double-Q gather, mse, autograd.grad), eager and as a
            graph  vs  ONE copy_ that moves the head's compulsory bytes (the floor).  Checked equal before timing.
    loop    PolicyLoop.capture(T) at 65 536 worlds: epsilon = 0 (mpe_actor_act) and epsilon = 0.25 (mpe_actor_act_explore)  vs  the
            same loop with the exploration as a torch chain behind the greedy launch (rand, randint, one_hot, where), one graph too.

--greedy-loop-only times the epsilon = 0 loop alone and uses nothing this change added, so that it also runs on the PARENT commit's
tree: MPE_TREE=<a checkout of the parent, built> python tools/q_loss_rate.py --greedy-loop-only.  --parent-loop takes the JSON
lines of such runs (alternated with this tree's own by the caller): their spread is the yardstick of the loop goal.

Goals (recorded as met or missed, never tuned here): the head's slowest round is faster than the torch graph's fastest at both sizes;
the epsilon = 0 and epsilon > 0 loops' medians lie inside the parent's greedy loop's [min, max] widened by its own spread (max - min).
Every figure is us per pass / per step from device events around the replays (median of the rounds, min and max kept)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.environ.get("MPE_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop  # noqa: E402

WORLDS, T_LOOP, EPS = 65536, 25, 0.25


def mlp(n_in, n_out):
    return nn.Sequential(nn.Linear(n_in, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, n_out)).cuda()


def timed(fn, units):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / units


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


def greedy_loop(env, nets):
    """the epsilon = 0 closed loop as the parent commit runs it: Actors(mode="greedy"), PolicyLoop.capture"""
    loop = PolicyLoop(env, Actors(env, nets, mode="greedy"), episode_len=T_LOOP)
    return loop.capture(T_LOOP)


def loops(reps, parent_files):
    from multiagent_particle_envs_amd import _abi
    env = mpe.make_env("simple_spread", batch_size=WORLDS, seed=1)
    torch.manual_seed(0)
    nets = [mlp(18, 5) for _ in range(env.n)]
    legs = {"greedy": greedy_loop(env, nets)}
    pi = Actors(env, nets, mode="greedy", epsilon=EPS)
    legs["epsilon_greedy"] = PolicyLoop(env, pi, episode_len=T_LOOP).capture(T_LOOP)
    # the torch chain a learner wrote before: the greedy launch, then rand / randint / one_hot / where on its rows
    plain = Actors(env, nets, mode="greedy").freeze()
    A, B = env.n, WORLDS
    obs = [o.clone() for o in env.reset()]

    def torch_step(k):      # (torch's default generator: the one a capture advances by itself)
        rows = plain.act(obs, k)
        explore = torch.rand((A, B, 1), device="cuda") < EPS
        rand = F.one_hot(torch.randint(0, _abi.MPE_ACTION_DIM, (A, B), device="cuda"), _abi.MPE_ACTION_DIM).float()
        out = env.step(torch.where(explore, rand, rows))[0]
        for i in range(A):
            obs[i].copy_(out[i])
    try:
        legs["torch_chain"] = graph_of(torch_step, T_LOOP)
    except Exception as e:      # (a loop the runtime refuses to capture: the figure is then missing, said so)
        torch.cuda.synchronize()
        legs["torch_chain"] = lambda: [torch_step(k) for k in range(T_LOOP)]
        note = "torch_chain ran eager: capture failed: %s" % (str(e).splitlines() or [""])[0]
    else:
        note = None
    r = rounds(legs, T_LOOP, reps)
    r.update(worlds=WORLDS, steps_per_graph=T_LOOP, epsilon=EPS)
    if note:
        r["note"] = note
    r["speedup_over_torch_chain"] = r["torch_chain"]["median_us"] / r["epsilon_greedy"]["median_us"]
    if parent_files:
        runs = []
        for f in parent_files:
            with open(f) as fh:
                runs += [json.loads(l) for l in fh if l.startswith("{")]
        med = [x["greedy"]["median_us"] for x in runs]
        lo, hi = min(x["greedy"]["min_us"] for x in runs), max(x["greedy"]["max_us"] for x in runs)
        r["parent_greedy"] = {"runs": len(runs), "median_us": statistics.median(med), "min_us": lo, "max_us": hi, "spread_us": hi - lo}
        r["goal_met"] = all(lo - (hi - lo) <= r[k]["median_us"] <= hi + (hi - lo) for k in ("greedy", "epsilon_greedy"))
    else:
        r["parent_greedy"], r["goal_met"] = "not measured (no --parent-loop file given)", None
    return r


def head(env, M, mix, K, reps):
    from multiagent_particle_envs_amd.learner import RowsLayout, q_loss_tensors
    from multiagent_particle_envs_amd.replay import NStepReplayBatch
    A, dev = env.n, torch.device("cuda")
    gen = torch.Generator(device="cuda").manual_seed(M)
    lay = RowsLayout(69, 0, [54, 59, 64], [True] * 3, [False] * 3)
    q_n = [torch.randn(M, 5, generator=gen, device=dev) for _ in range(A)]
    nt, no = torch.zeros(A, M, 16, device=dev), torch.zeros(A, M, 16, device=dev)
    nt[..., :5], no[..., :5] = torch.randn(A, M, 5, generator=gen, device=dev), torch.randn(A, M, 5, generator=gen, device=dev)
    b = NStepReplayBatch()
    b.act = F.one_hot(torch.randint(0, 5, (A, M), generator=gen, device=dev), 5).float().contiguous()
    b.utter, b.rew = None, torch.randn(A, M, generator=gen, device=dev)
    b.ret, b.discount = torch.randn(A, M, generator=gen, device=dev), torch.full((M,), 0.95 ** 3, device=dev)
    b._done_u8 = (torch.rand(A, M, generator=gen, device=dev) < 0.1).to(torch.uint8)
    w = torch.rand(M, generator=gen, device=dev) + 0.5
    live = 1.0 - b._done_u8.float()
    res = q_loss_tensors(lay, q_n, b, nt, no, mix=mix, weights=w)
    tz = [z.clone().requires_grad_() for z in q_n]
    idx = [b.act[i].argmax(dim=1, keepdim=True) for i in range(A)]

    def torch_loss():
        q = [tz[i].gather(1, idx[i])[:, 0] for i in range(A)]
        v = [nt[i, :, :5].gather(1, no[i, :, :5].argmax(dim=1, keepdim=True))[:, 0] for i in range(A)]
        if mix == "independent":
            return sum((w * (q[i] - (b.ret[i] + b.discount * live[i] * v[i])) ** 2).mean() for i in range(A))
        return (w * (sum(q) - (b.ret.sum(dim=0) / A + b.discount * live.min(dim=0).values * sum(v))) ** 2).mean()

    def torch_both(k):
        return torch.autograd.grad(torch_loss(), tz)
    want = torch_both(0)
    torch.cuda.synchronize()
    worst = max(float((a - b_).abs().max() / b_.abs().max()) for a, b_ in zip(res.dq_n, want))
    assert worst < 1e-5, worst
    one = torch.ones((), device=dev)

    def ours(k):
        q_loss_tensors(lay, q_n, b, nt, no, mix=mix, weights=w, out=res)
        return one * res.grads      # (the autograd backward's one multiply)
    # compulsory bytes: q, act, dq [A, M, 5]; nt, no [A, M, 16]; ret, q_taken, y [A, M] floats and done bytes; discount, w, td_abs [M]
    nbytes = 4 * A * M * (3 * 5 + 2 * 16 + 3) + A * M + 4 * 3 * M
    src, dst = torch.zeros(nbytes // 2, dtype=torch.uint8, device=dev), torch.zeros(nbytes // 2, dtype=torch.uint8, device=dev)
    r = rounds({"ours": graph_of(ours, K), "torch_graph": graph_of(torch_both, K), "copy_floor": graph_of(lambda k: dst.copy_(src), K),
                "torch_eager": lambda: [torch_both(0) for _ in range(K)]}, K, reps)
    r["equal_before_timing"] = {"dq_max_relative_difference": worst}
    r["compulsory_bytes"] = nbytes
    r["fraction_of_copy_floor"] = r["copy_floor"]["median_us"] / r["ours"]["median_us"]
    r["speedup_over_torch_graph"] = r["torch_graph"]["median_us"] / r["ours"]["median_us"]
    r["speedup_over_torch_eager"] = r["torch_eager"]["median_us"] / r["ours"]["median_us"]
    r["goal_met"] = r["ours"]["max_us"] < r["torch_graph"]["min_us"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--greedy-loop-only", action="store_true")
    ap.add_argument("--parent-loop", nargs="*", default=[])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "q_loss_rate.py measures on a GPU: there is no CPU path"
    if a.greedy_loop_only:
        env = mpe.make_env("simple_spread", batch_size=WORLDS, seed=1)
        torch.manual_seed(0)
        r = rounds({"greedy": greedy_loop(env, [mlp(18, 5) for _ in range(env.n)])}, T_LOOP, a.reps)
        r["tree"] = os.path.dirname(os.path.abspath(mpe.__file__))
        print(json.dumps(r))
        return
    env = mpe.make_env("simple_spread", batch_size=64, seed=1)
    res = {"device": torch.cuda.get_device_name(0), "scenario": "simple_spread", "agents": env.n, "target": "double-Q, weights, 3-step discounts",
           "passes_per_graph": a.steps, "graph_replays_per_timing": a.reps, "unit": "us per pass (head) / per step (loop)", "head": {}}
    for M in (1024, 65536):
        res["head"]["M%d" % M] = {mix: head(env, M, mix, a.steps, a.reps) for mix in ("independent", "vdn")}
    res["head_goal_met"] = all(r["goal_met"] for p in res["head"].values() for r in p.values())
    res["loop"] = loops(a.reps, a.parent_loop)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
