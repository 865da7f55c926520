"""A MADDPG-style learner on simple_spread, wired from the device-side pieces.

    python examples/maddpg_spread.py [--worlds 1024] [--batch 1024] [--updates 200] [--fused-nets | --device-update]

The closed loop (PolicyLoop) fills a device replay ring with one launch per step; a minibatch with 3-step returns is one launch
(ReplayBuffer.sample); the no-grad half of the update -- target actors on the next observations, target critics on the joint rows,
the TD target y -- is two launches (TdTargets.compute).  The critic loss, the actor loss and the soft updates are plain torch
autograd.  One JSON line per update.  A readable wiring, not a benchmark.

--fused-nets: the networks' forward and backward passes run on the device kernels too (Trainable).  The critic loss goes through
Trainable(Critics); the actor loss -Q_i(joint row with agent i's action columns replaced by softmax(mu_i(obs_i))) through
Trainable(Actors, logits=True), torch's softmax and column write, and Trainable(Critics, input_grad=True, weight_grad=False, cols=...):
the critics are a constant of it, and what it needs of them is their gradient with respect to those 5 input columns (one launch).
The optimisers, the soft updates and the softmax Jacobian (a [M, 5] op) stay in torch.

--device-update (implies --fused-nets): the rest of the update leaves torch too.  The critic loss is TdLoss
(mpe_td_loss), the actor loss ActorLoss (mpe_policy_rows, the critics, their input gradient, mpe_policy_rows_grad); two DeviceAdam
hold the critics' and the actors' packed weights as the master copies, the sampling Actors joins the actors' buffer through share(),
and the soft updates are one launch on the packed buffers (PolyakTargets).  The modules' own parameters are stale until
write_back().
"""
import argparse
import copy
import json
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from multiagent_particle_envs_amd import (ActorLoss, Actors, Critics, DeviceAdam, PolicyLoop, PolyakTargets, ReplayBuffer, TdLoss,  # noqa: E402
                                          TdTargets, Trainable, make_env)

ap = argparse.ArgumentParser()
ap.add_argument("--worlds", type=int, default=1024)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--updates", type=int, default=200)
ap.add_argument("--steps-per-update", type=int, default=5)
ap.add_argument("--gamma", type=float, default=0.95)
ap.add_argument("--tau", type=float, default=0.01)
ap.add_argument("--fused-nets", action="store_true", help="forward and backward passes of the actors and critics on the device kernels")
ap.add_argument("--device-update", action="store_true", help="--fused-nets, and the losses, the optimisers and the soft updates on the device too")
args = ap.parse_args()
args.fused_nets = args.fused_nets or args.device_update
EPISODE, N_STEP = 25, 3


def mlp(n_in, n_out):
    return nn.Sequential(nn.Linear(n_in, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, n_out)).cuda()


torch.manual_seed(0)
env = make_env("simple_spread", batch_size=args.worlds)
A = env.n
buf = ReplayBuffer(env, steps=4 * EPISODE)
mu = [mlp(D, 5) for D in buf.obs_widths]                  # online actors: logits over the 5 moves
qs = [mlp(buf.joint_width, 1) for _ in range(A)]          # online centralised critics
mu_targ, q_targ = copy.deepcopy(mu), copy.deepcopy(qs)
behaviour = Actors(env, mu, mode="sample")                # explores by sampling its softmax
loop = PolicyLoop(env, behaviour, episode_len=EPISODE)
target_actors = Actors(env, mu_targ, mode="softmax")      # MADDPG's relaxed one-hot actions
target_critics = Critics(env, q_targ)
td = TdTargets(target_actors, target_critics)             # both re-read their modules at every call: soft updates are seen
if not args.device_update:
    opt_q = torch.optim.Adam([p for m in qs for p in m.parameters()], lr=1e-3)
    opt_mu = torch.optim.Adam([p for m in mu for p in m.parameters()], lr=1e-3)
col = target_actors.col_move                              # agent i's action columns of a joint row
if args.fused_nets:
    q_train = Trainable(Critics(env, qs))                 # critic loss: the weights' gradients
    pi_train = Trainable(Actors(env, mu, mode="softmax", logits=True))
    q_const = Trainable(Critics(env, qs), input_grad=True, weight_grad=False, cols=[(c, 5) for c in col])      # actor loss: dQ_i / d(action columns)
if args.device_update:
    opt_q = DeviceAdam([q_train], lr=1e-3)                # the packed buffers are the master copies from here on
    opt_mu = DeviceAdam([pi_train], lr=1e-3)
    opt_mu.share(pi_train, behaviour)                     # the closed loop samples from the live actors
    polyak = PolyakTargets([(pi_train, target_actors), (q_train, target_critics)], args.tau)
    critic_head, actor_head = TdLoss(), ActorLoss(pi_train.net, q_train.net)      # the critics are a constant of the actor loss


def device_update(batch, y):
    """The whole update as a straight line of device launches: the two losses behind autograd, Adam and the soft updates in place"""
    critic_loss = critic_head(q_train(batch.joint), y)
    critic_loss.backward()
    opt_q.step()
    actor_loss = actor_head(pi_train(batch.obs_n), batch.joint)      # reads the critics the step above just updated
    actor_loss.backward()
    opt_mu.step()
    polyak.step()
    for p in q_train.parameters() + pi_train.parameters():          # (.grad of the stale module parameters is not used)
        p.grad = None
    return critic_loss, actor_loss


def critic_values(joint):
    """Q_i of every agent on the batch's joint rows -> A tensors [M]"""
    return q_train(joint) if args.fused_nets else [qs[i](joint)[:, 0] for i in range(A)]


def actor_values(batch):
    """Q_i(joint with agent i's own action columns replaced by its current policy's, the others' as played) -> A tensors [M]"""
    logits = pi_train(batch.obs_n) if args.fused_nets else [mu[i](batch.obs_n[i]) for i in range(A)]
    joints = []
    for i in range(A):
        joint = batch.joint.clone()
        joint[:, col[i]:col[i] + 5] = F.softmax(logits[i], dim=1)
        joints.append(joint)
    return q_const(joints) if args.fused_nets else [qs[i](joints[i])[:, 0] for i in range(A)]


loop.run(EPISODE, record=False, replay=buf)               # something to sample from
for update in range(args.updates):
    loop.run(args.steps_per_update, record=False, replay=buf)
    batch = buf.sample(args.batch, joint=True, n_step=N_STEP, gamma=args.gamma, episode_len=EPISODE)
    y = td.compute(batch)                                 # [A, M], two launches, no gradient
    if args.device_update:
        critic_loss, actor_loss = device_update(batch, y)
        print(json.dumps({"update": update, "critic_loss": float(critic_loss), "actor_loss": float(actor_loss),
                          "mean_reward": float(batch.rew.mean()), "mean_y": float(y.mean())}), flush=True)
        continue
    # critics: Q_i(obs, actions) -> y_i
    q = critic_values(batch.joint)
    critic_loss = sum(F.mse_loss(q[i], y[i]) for i in range(A))
    opt_q.zero_grad()
    critic_loss.backward()
    opt_q.step()
    # actors: agent i's own action columns replaced by its current policy's, the others' as played
    actor_loss = 0.0
    for q_i in actor_values(batch):
        actor_loss = actor_loss - q_i.mean()
    opt_mu.zero_grad()
    actor_loss.backward()
    opt_mu.step()
    with torch.no_grad():                                 # soft updates, in place: the next compute() packs the new weights
        for online, targ in zip(mu + qs, mu_targ + q_targ):
            for p, pt in zip(online.parameters(), targ.parameters()):
                pt.lerp_(p, args.tau)
    print(json.dumps({"update": update, "critic_loss": float(critic_loss), "actor_loss": float(actor_loss),
                      "mean_reward": float(batch.rew.mean()), "mean_y": float(y.mean())}), flush=True)
