"""Independent Q-learning / VDN on simple_spread, wired from the device-side pieces.

    python examples/vdn_spread.py [--worlds 1024] [--batch 1024] [--updates 200] [--mix independent|vdn] [--double]
                                  [--n-step 3] [--prioritized] [--device-update]

A Q-network per agent is an actor whose 5 logits are action values.  The closed loop plays epsilon-greedy inside the actor launch
(Actors(mode="greedy", epsilon=...): one assignment per update moves a linear schedule) and fills a device replay ring with one
launch per step; a minibatch (one-step or n-step, uniform or prioritized) is one or two launches.  The update itself is plain
torch: Q_i(s)[a_i] by gather, the bootstrap Q'_i(s')[argmax Q'_i(s')] (or, with --double, at the online net's argmax), the per-agent
or (--mix vdn) summed target, the (weighted) squared error, torch Adam, and a hard target update every --target-every updates.
One JSON line per update.  A readable wiring, not a benchmark.

--device-update: the same update as a straight line of device launches.  QTargets runs the target (and online) networks on the next
observations, Trainable(actors) gives the logits and their backward, QLoss (mpe_q_loss) goes from the logits to dL/dlogits in two
launches, DeviceAdam holds the packed weights as the master copy (the exploring Actors joins it through share()), and
PolyakTargets(tau=1) is the hard target update.  The modules' own parameters are stale until write_back().
"""
import argparse
import copy
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multiagent_particle_envs_amd import (Actors, DeviceAdam, PolicyLoop, PolyakTargets, PrioritizedReplayBuffer, QLoss, QTargets,  # noqa: E402
                                          ReplayBuffer, Trainable, make_env)

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", type=int, default=1024)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--updates", type=int, default=200)
ap.add_argument("--steps-per-update", type=int, default=5)
ap.add_argument("--mix", choices=("independent", "vdn"), default="vdn")
ap.add_argument("--double", action="store_true", help="double-Q: the bootstrap is the target net's value at the online net's argmax")
ap.add_argument("--n-step", type=int, default=1)
ap.add_argument("--prioritized", action="store_true", help="a PrioritizedReplayBuffer: importance weights in, |td| back")
ap.add_argument("--gamma", type=float, default=0.95)
ap.add_argument("--lr", type=float, default=1e-3)
ap.add_argument("--target-every", type=int, default=10, help="updates between two hard target updates")
ap.add_argument("--eps-start", type=float, default=1.0)
ap.add_argument("--eps-end", type=float, default=0.05)
ap.add_argument("--beta", type=float, default=0.4)
ap.add_argument("--device-update", action="store_true", help="the loss head, the networks' passes, Adam and the target update on the device")
args = ap.parse_args()
EPISODE = 25


def mlp(n_in, n_out):
    return nn.Sequential(nn.Linear(n_in, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, n_out)).cuda()


torch.manual_seed(0)
env = make_env("simple_spread", batch_size=args.worlds)
A = env.n
buf = (PrioritizedReplayBuffer if args.prioritized else ReplayBuffer)(env, steps=4 * EPISODE)
nets = [mlp(D, 5) for D in buf.obs_widths]                # online Q-networks: a value per move
nets_targ = copy.deepcopy(nets)
behaviour = Actors(env, nets, mode="greedy", epsilon=args.eps_start)      # epsilon-greedy inside the actor launch
loop = PolicyLoop(env, behaviour, episode_len=EPISODE)
if args.device_update:
    online = Actors(env, nets, mode="greedy", logits=True)
    target = Actors(env, nets_targ, mode="greedy", logits=True)
    q_train = Trainable(online)
    opt = DeviceAdam([q_train], lr=args.lr)               # the packed buffer is the master copy from here on
    opt.share(q_train, behaviour)                         # the closed loop explores around the live networks
    hard = PolyakTargets([(q_train, target)], 1.0)        # tau = 1: the online bits
    targets = QTargets(target, online if args.double else None)
    head = QLoss(online, mix=args.mix, double=args.double)
else:
    opt = torch.optim.Adam([p for m in nets for p in m.parameters()], lr=args.lr)


def sample():
    kw = dict(n_step=args.n_step, gamma=args.gamma, episode_len=EPISODE) if args.n_step > 1 else {}
    batch = buf.sample(args.batch, **kw)
    ret, discount = (batch.ret, batch.discount) if args.n_step > 1 else (batch.rew, args.gamma)
    return batch, ret, discount, (batch.weights(args.beta).contiguous() if args.prioritized else None)


def device_update(batch, weights):
    next_target, next_online = targets.compute(batch)
    loss = head(q_train(batch.obs_n), batch, next_target, next_online, gamma=None if args.n_step > 1 else args.gamma, weights=weights)
    loss.backward()
    opt.step()
    for p in q_train.parameters():                        # (.grad of the stale module parameters is not used)
        p.grad = None
    return loss, head.last.td_abs


def torch_update(batch, ret, discount, weights):
    q, v = [], []
    for i in range(A):
        q.append(nets[i](batch.obs_n[i]).gather(1, batch.act[i].argmax(dim=1, keepdim=True))[:, 0])
        with torch.no_grad():
            zt = nets_targ[i](batch.next_obs_n[i])
            v.append(zt.gather(1, nets[i](batch.next_obs_n[i]).argmax(dim=1, keepdim=True))[:, 0] if args.double else zt.max(dim=1).values)
    live = (~batch.done).float()
    w = 1.0 if weights is None else weights
    if args.mix == "independent":
        deltas = [q[i] - (ret[i] + discount * live[i] * v[i]) for i in range(A)]
        loss = sum((w * d * d).mean() for d in deltas)
        td_abs = torch.stack(deltas).abs().max(dim=0).values
    else:
        delta = sum(q) - (ret.sum(dim=0) / A + discount * live.min(dim=0).values * sum(v))
        loss, td_abs = (w * delta * delta).mean(), delta.abs()
    opt.zero_grad()
    loss.backward()
    opt.step()
    return loss, td_abs.detach()


loop.run(EPISODE, record=False, replay=buf)               # something to sample from
for update in range(args.updates):
    frac = update / max(args.updates - 1, 1)
    behaviour.epsilon = args.eps_start + (args.eps_end - args.eps_start) * frac      # the linear schedule: one assignment
    loop.run(args.steps_per_update, record=False, replay=buf)
    batch, ret, discount, weights = sample()
    if args.device_update:
        loss, td_abs = device_update(batch, weights)
    else:
        loss, td_abs = torch_update(batch, ret, discount, weights)
    if args.prioritized:
        buf.update_td(batch.idx, td_abs)
    if (update + 1) % args.target_every == 0:
        if args.device_update:
            hard.step()
        else:
            for online_net, targ in zip(nets, nets_targ):
                targ.load_state_dict(online_net.state_dict())
    print(json.dumps({"update": update, "loss": float(loss), "epsilon": behaviour.epsilon, "mean_reward": float(batch.rew.mean()),
                      "mean_td": float(td_abs.mean())}), flush=True)
