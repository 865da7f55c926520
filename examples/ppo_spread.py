"""An IPPO learner on simple_spread, wired from the device-side pieces.

    python examples/ppo_spread.py [--worlds 1024] [--updates 50] [--epochs 4] [--minibatch M [--fused-loss [--fused-nets [--device-adam]]]]

The closed loop (PolicyLoop) plays one 25-step episode in every world and records, beside the rows played and their log
probabilities, the observation every step was decided on and each agent's own critic along it (run(25, values=V): one more launch
per step, and one for the bootstrap value of the episode's last output observation).  Advantages and returns are ONE launch (gae:
the episodes are cut by the time limit, so the last step bootstraps from V of its output observation).  Advantage normalisation,
the clipped surrogate, the value loss and the optimiser are plain torch autograd over traj.obs_in, traj.act and traj.logp.  With
--minibatch M every epoch is a shuffled pass over minibatches of M (step, world) pairs instead (Minibatches: the advantage
statistics once per rollout, then ONE launch per minibatch that draws its rows from a keyed permutation and gathers every agent's
observation, move, log probability, normalised advantage and return).  With --fused-loss the clipped surrogate, the value loss and
their gradients with respect to the logits and the values are the device's loss head instead (PpoLoss: two launches per minibatch
for all agents; the networks' forward and backward passes stay in torch autograd), and with --fused-nets those passes leave torch
too (Trainable: the actors' and the critics' forward are one launch each, their backward two launches each -- the hidden
activations recomputed, every weight's and bias's gradient written; the optimiser stays torch's).  With --device-adam the optimiser
leaves torch as well (DeviceAdam: the packed weights are the master copy, updated in place by two launches per minibatch for both
sets; every forward reads them, nothing is packed again).  One JSON line per update.  A readable wiring,
not a benchmark.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multiagent_particle_envs_amd import Actors, DeviceAdam, Minibatches, PolicyLoop, PpoLoss, Trainable, Values, gae, make_env  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", type=int, default=1024)
ap.add_argument("--updates", type=int, default=50)
ap.add_argument("--epochs", type=int, default=4)
ap.add_argument("--gamma", type=float, default=0.95)
ap.add_argument("--lam", type=float, default=0.95)
ap.add_argument("--clip", type=float, default=0.2)
ap.add_argument("--minibatch", type=int, default=0, help="rows per shuffled minibatch; 0: one full-batch step per epoch")
ap.add_argument("--fused-loss", action="store_true", help="the loss head on the device (PpoLoss); needs --minibatch")
ap.add_argument("--fused-nets", action="store_true", help="the networks' forward and backward on the device (Trainable); needs --fused-loss")
ap.add_argument("--device-adam", action="store_true", help="the optimiser step on the device (DeviceAdam); needs --fused-nets")
args = ap.parse_args()
if args.device_adam and not args.fused_nets:
    ap.error("--device-adam needs --fused-nets (the step reads the packed gradients of the backward kernel)")
if args.fused_nets and not args.fused_loss:
    ap.error("--fused-nets needs --fused-loss (the backward kernel starts from the loss head's dL/dlogits and dL/dvalues)")
if args.fused_loss and not args.minibatch:
    ap.error("--fused-loss needs --minibatch M (the loss head reads a minibatch's own tensors)")
EPISODE = 25


def mlp(n_in, n_out):
    return nn.Sequential(nn.Linear(n_in, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, n_out)).cuda()


torch.manual_seed(0)
env = make_env("simple_spread", batch_size=args.worlds)
A = env.n
widths = [int(env._obs_off[i + 1] - env._obs_off[i]) for i in range(A)]
pi = [mlp(D, 5) for D in widths]                          # independent actors: logits over the 5 moves
vf = [mlp(D, 1) for D in widths]                          # independent critics on the agent's own observation
behaviour = Actors(env, pi, mode="sample", logp=True)     # re-reads its modules at every act: each rollout plays the new policy
V = Values(env, vf)
loop = PolicyLoop(env, behaviour, episode_len=EPISODE)
opt = torch.optim.Adam([p for m in pi + vf for p in m.parameters()], lr=3e-4)
fused = PpoLoss(env, clip=args.clip, vf_coef=0.5) if args.fused_loss else None
if args.fused_nets:      # the same modules behind autograd Functions: logits [M, 5] and values [M] per agent, one launch per set
    pi_rows, v_rows = Trainable(Actors(env, pi, mode="sample", logits=True)), Trainable(V)
if args.device_adam:     # the packed weights become the master copy; the sampling set reads the same live buffer
    dev_opt = DeviceAdam([pi_rows, v_rows], lr=3e-4)
    dev_opt.share(pi_rows, behaviour)


def losses(i, obs, act, old_logp, adv, ret):
    """agent i's clipped surrogate and value loss over rows of any leading shape"""
    logp = (F.log_softmax(pi[i](obs), dim=-1) * act).sum(dim=-1)      # the move rows played are one-hot
    ratio = torch.exp(logp - old_logp)
    return -torch.min(ratio * adv, ratio.clamp(1 - args.clip, 1 + args.clip) * adv).mean(), F.mse_loss(vf[i](obs)[..., 0], ret)


for update in range(args.updates):
    traj = loop.run(EPISODE, values=V)                    # obs_in, act, logp, rew, done, val [T,A,B], boot [1,A,B]
    g = gae(traj, args.gamma, args.lam)                   # adv, ret [T,A,B]: one launch, no gradient
    mbs = Minibatches(traj, g, args.minibatch, seed=update) if args.minibatch else None      # + the advantage statistics, once
    for epoch in range(args.epochs):
        if mbs is not None:
            for batch in mbs.epoch(epoch):                # one launch each: rows of a keyed shuffle, adv already normalised
                if fused is not None:                     # every agent's loss and dL/dlogits, dL/dvalues: two launches
                    if args.fused_nets:
                        loss = fused(pi_rows(batch.obs_n), v_rows(batch.obs_n), batch)
                    else:
                        loss = fused([pi[i](batch.obs_n[i]) for i in range(A)], [vf[i](batch.obs_n[i]) for i in range(A)], batch)
                    if args.device_adam:
                        opt.zero_grad()               # host only (.grad = None): autograd's views of the packed gradient are set, not
                        loss.backward()               # accumulated; nothing reads them -- the step takes the packed gradient itself
                        dev_opt.step()
                        policy_loss, value_loss = -loss.stats[:, 0].sum(), loss.stats[:, 1].sum()
                        continue
                    opt.zero_grad()
                    loss.backward()
                    opt.step()
                    policy_loss, value_loss = -loss.stats[:, 0].sum(), loss.stats[:, 1].sum()
                    continue
                policy_loss = value_loss = 0.0
                for i in range(A):
                    pl, vl = losses(i, batch.obs_n[i], batch.act[i], batch.logp[i], batch.adv[i], batch.ret[i])
                    policy_loss, value_loss = policy_loss + pl, value_loss + vl
                opt.zero_grad()
                (policy_loss + 0.5 * value_loss).backward()
                opt.step()
            continue
        policy_loss = value_loss = 0.0
        for i in range(A):
            obs = torch.stack([traj.obs_in[t][i] for t in range(EPISODE)])      # [T, B, D_i]: what step t was decided on
            adv = g.adv[:, i]
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            logp = (F.log_softmax(pi[i](obs), dim=2) * traj.act[:, i]).sum(dim=2)      # the move rows played are one-hot
            ratio = torch.exp(logp - traj.logp[:, i])
            policy_loss = policy_loss - torch.min(ratio * adv, ratio.clamp(1 - args.clip, 1 + args.clip) * adv).mean()
            value_loss = value_loss + F.mse_loss(vf[i](obs)[:, :, 0], g.ret[:, i])
        opt.zero_grad()
        (policy_loss + 0.5 * value_loss).backward()
        opt.step()
    print(json.dumps({"update": update, "policy_loss": float(policy_loss), "value_loss": float(value_loss),
                      "mean_reward": float(traj.rew.mean()), "mean_advantage": float(g.adv.mean()), "mean_return": float(g.ret.mean())}),
          flush=True)
