"""SHA-256 of everything a tiny seeded learner computes on the device, through the public Python API only: a tool for before / after
a change to the host layer over the learner kernels (policy.py, learner.py, onpolicy.py, train.py, optim.py, netset.py).

    python tools/learner_bits.py [--out FILE]          one JSON object {name: digest}; two trees on one machine compare bit for bit

Three on-policy runs -- simple_spread with decentralised and with centralised Values (3 agents, agents 0 and 1 sharing ONE actor
module object), and simple_speaker_listener (an utterance head) -- each B = 64 worlds, T = 5 steps with episode_len = 3 (so K > 1
segments): the recorded trajectory (act, utter, logp, val, boot), gae's adv and ret, one minibatch's fields at M = 80 and the short last
minibatch at M = 96 (T * B = 320 = 4 * 80 = 3 * 96 + 32), then two updates {PpoLoss on Trainable nets, backward, DeviceAdam.step}: the loss,
its stats and gradients and each net's packed gradient of both, and afterwards each net's weights, m and v and the modules'
parameters behind write_back().  One off-policy pass: Critics + TdTargets on 96 sampled joint rows (n-step and one-step): y,
joint_next_act, q_next.  The digests depend on the compiler version and the torch build: not a test."""
import argparse
import hashlib
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import multiagent_particle_envs_amd as mpe  # noqa: E402

B, T, EPISODE_LEN = 64, 5, 3


def digest(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def mlp(n_in, n_out, hidden=(64, 32)):
    mods, k = [], n_in
    for h in hidden:
        mods += [nn.Linear(k, h), nn.Tanh()]
        k = h
    return nn.Sequential(*(mods + [nn.Linear(k, n_out)])).cuda()


def batch_fields(out, label, b):
    for name in ("idx", "obs", "act", "utter", "logp", "adv", "ret", "val", "joint_obs"):
        if getattr(b, name) is not None:
            out["%s.%s" % (label, name)] = digest(getattr(b, name))


def on_policy(out, label, scenario, centralised):
    torch.manual_seed(7)
    env = mpe.make_env(scenario, batch_size=B, seed=1)
    agents, A = env.world.agents, env.n
    widths = [int(env._obs_off[i + 1] - env._obs_off[i]) for i in range(A)]
    dim_c = int(env.world.dim_c) if any(not a.silent for a in agents) else 0
    n_out = [5 * bool(a.movable) + dim_c * (not a.silent) for a in agents]
    pm = [mlp(widths[i], n_out[i]) for i in range(A)]
    if A > 2 and (widths[0], n_out[0]) == (widths[1], n_out[1]):
        pm[1] = pm[0]      # two agents, ONE module object: one packed copy
    vm = [mlp(sum(widths) if centralised else widths[i], 1, hidden=(20,)) for i in range(A)]
    behaviour = mpe.Actors(env, pm, mode="sample", seed=2, logp=True)
    V = mpe.Values(env, vm, centralised=centralised)
    loop = mpe.PolicyLoop(env, behaviour, episode_len=EPISODE_LEN, seed=5)
    traj = loop.run(T, values=V)
    for name in ("act", "utter", "logp", "val", "boot", "rew"):
        if getattr(traj, name) is not None:
            out["%s.traj.%s" % (label, name)] = digest(getattr(traj, name))
    g = mpe.gae(traj, 0.95, 0.9)
    out[label + ".g.adv"], out[label + ".g.ret"] = digest(g.adv), digest(g.ret)
    mb = mpe.Minibatches(traj, g, 80, seed=6, joint=centralised)
    out[label + ".adv_stats"] = digest(mb.stats)
    batch_fields(out, label + ".batch80_e1_k2", mb.batch(1, 2))
    batch_fields(out, label + ".batch96_e0_k3_short", mpe.Minibatches(traj, g, 96, seed=6).batch(0, 3))
    pi_t, V_t = mpe.Trainable(mpe.Actors(env, pm, mode="sample", logits=True)), mpe.Trainable(V)
    out[label + ".pack.actors"], out[label + ".pack.values"] = digest(pi_t.net.pack()[0]), digest(V.pack()[0])
    head = mpe.PpoLoss(env, clip=0.2, vf_coef=0.5, ent_coef=0.01)
    opt = mpe.DeviceAdam([pi_t, V_t], lr=1e-2, max_grad_norm=0.5, weight_decay=0.01)
    opt.share(pi_t, behaviour)
    params = [p for m in dict.fromkeys(pm + vm) for p in m.parameters()]
    for k in range(2):
        b = mb.batch(0, k)
        for p in params:
            p.grad = None
        loss = head(pi_t(b.obs_n), V_t(b.obs_n), b)
        loss.backward()
        step = "%s.update%d" % (label, k)
        out[step + ".loss"], out[step + ".stats"], out[step + ".grads"] = digest(loss), digest(loss.stats), digest(head.last.grads)
        out[step + ".packed_grad.actors"], out[step + ".packed_grad.values"] = digest(pi_t.last_grad.packed), digest(V_t.last_grad.packed)
        out[step + ".param_grads"] = digest(torch.cat([p.grad.reshape(-1) for p in params]))
        opt.step()
    for name, k in (("actors", 0), ("values", 1)):
        for what, ts in (("weights", opt.weights), ("m", opt.m), ("v", opt.v)):
            out["%s.adam.%s.%s" % (label, name, what)] = digest(ts[k])
    out[label + ".adam.state"] = digest(opt.state)
    action = behaviour.act(loop.obs_n, 11)      # the sampling set reads the optimiser's live buffer
    out[label + ".act_after_updates"] = digest(action[0] if isinstance(action, tuple) else action)
    opt.write_back()
    out[label + ".params_after_write_back"] = digest(torch.cat([p.reshape(-1) for p in params]))


def off_policy(out, label):
    torch.manual_seed(3)
    env = mpe.make_env("simple_spread", batch_size=B, seed=1)
    pi = mpe.Actors(env, [mlp(18, 5) for _ in range(3)], mode="sample", seed=2)
    buf = mpe.ReplayBuffer(env, 8, seed=4)
    mpe.PolicyLoop(env, pi, episode_len=5).run(12, record=False, replay=buf)
    shared = mlp(18, 5)
    mu_t = mpe.Actors(env, [shared, shared, mlp(18, 5)], mode="softmax")
    q_t = mpe.Critics(env, [mlp(69, 1) for _ in range(3)])
    td = mpe.TdTargets(mu_t, q_t)
    for kind, kw, ckw in (("nstep", dict(n_step=3, gamma=0.95, episode_len=5), {}), ("one_step", {}, dict(gamma=0.95))):
        batch = buf.sample(96, joint=True, **kw)
        y = td.compute(batch, **ckw)
        out["%s.%s.y" % (label, kind)], out["%s.%s.joint_next_act" % (label, kind)] = digest(y), digest(td.joint_next_act)
        out["%s.%s.q_next" % (label, kind)] = digest(td.q_next)
    out[label + ".q_of_joint"] = digest(q_t.q(batch.joint))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "learner_bits needs a GPU"
    out = {}
    on_policy(out, "spread_decentralised", "simple_spread", False)
    on_policy(out, "spread_centralised", "simple_spread", True)
    on_policy(out, "speaker_listener", "simple_speaker_listener", False)
    off_policy(out, "td_spread")
    line = json.dumps(out, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
