"""SHA-256 of everything the fused step kernels (csrc/mpe_split.hip: k_split, k_split_policy) write, for every shape of their
tables and every role they are built in.

    python tools/split_bits.py > listing.txt          (MPE_HIP_LIB=<another build> for the other column)

Per kSplitTable shape, from a seeded device reset (a third of the worlds shrunk so that agents touch), one line per tensor:
  steps     3 launched steps with every info buffer attached (benchmark=True), then the state: B = 70 (two workgroups, a ragged last
            wave of 6 live lanes)
  rollout   a 7-step fused rollout, episode_len = 3 from global step 2, moves (and words) drawn in the kernel: at B = 70 (the
            dual-role kernel where the kind has one) and at B = 64 * floor(1.5 * CUs) + 37 (the single-role kernel)
  served    the same two batch sizes through StepServer, every step commanded ahead (run): 7 steps, episode_len = 3, the caller's
            moves and -- the communication scenarios -- utterance rings
Per kPolicyTable shape: the policy rollout at B = 70, 7 steps, episode_len = 3, sample mode, with act, logp and the recorded inputs.
The nontemporal instantiations: simple_spread N = 3 at 65 536 worlds (one launched step) and simple_world_comm at 65 536 worlds (a
2-step rollout).  The tests compare these kernels with each other and with the oracle at 1e-5; two listings from two builds on one
machine compare them bit for bit.  The digests depend on the compiler version: a tool for before / after a change to that file,
not a test."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import multiagent_particle_envs_amd as mpe                                                             # noqa: E402
from multiagent_particle_envs_amd import _abi                                                          # noqa: E402
from multiagent_particle_envs_amd.rollout import MlpPolicy, PolicyRollout, RandomRollout, StepServer, Trajectory  # noqa: E402

SEED, T, EPISODE_LEN, STEP0, B_SMALL = 0x5EED, 7, 3, 2, 70


def tag(nadv, ngood, nl):
    return {"num_adversaries": nadv, "num_good_agents": ngood, "num_landmarks": nl}


# kSplitTable, in its order
SHAPES = [("simple", {})] + [("simple_spread", {"num_agents": n}) for n in range(1, 7)] + \
         [("simple_tag", tag(3, 1, 2)), ("simple_tag", tag(1, 1, 1)), ("simple_tag", tag(4, 2, 3)),
          ("simple_adversary", {}), ("simple_push", {}), ("simple_speaker_listener", {}), ("simple_reference", {}),
          ("simple_crypto", {}), ("simple_world_comm", {})]
# kPolicyTable
POLICY_SHAPES = [("simple", {})] + [("simple_spread", {"num_agents": n}) for n in range(1, 4)] + [("simple_adversary", {}), ("simple_push", {})]


def digest(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def show(label, what, t):
    print("%-40s %-26s %s" % (label, what, digest(t)), flush=True)


def label_of(name, kw, B):
    return "%s %s B=%d" % (name, ",".join(str(v) for v in kw.values()) or "-", B)


def fresh(name, kw, B, benchmark=False):
    env = mpe.make_env(name, benchmark=benchmark, batch_size=B, seed=SEED, **kw)
    env.reset()
    env._ensure_buffers()
    env.world.pos[..., ::3] *= 0.35
    assert env.fused, "%s %s: not a shape of the wave-per-agent kernels" % (name, kw)
    return env


def one_hot(rs, shape, n):
    return torch.as_tensor(np.eye(n, dtype=np.float32)[rs.randint(0, n, size=shape)]).cuda().contiguous()


def state(label, what, env):
    w = env.world
    show(label, what + " pos", w.pos)
    show(label, what + " vel", w.vel)
    if w.choice_i32 is not None:
        show(label, what + " choice", w.choice_i32)
    if env._comm is not None:
        show(label, what + " comm", env._comm)


def steps(name, kw, B, n=3):
    label = label_of(name, kw, B)
    rs = np.random.RandomState(1)
    env = fresh(name, kw, B, benchmark=True)
    A = len(env.world.agents)
    for t in range(n):
        act = one_hot(rs, (A, B), 5)
        if env._comm is not None:      # agent i's row: [move if movable] + [utterance if it speaks] (environment._stage_comm_actions)
            act = [torch.cat(([act[i]] if a.movable else []) + ([] if a.silent else [one_hot(rs, (B,), int(env.world.dim_c))]), dim=-1)
                   for i, a in enumerate(env.world.agents)]
        obs_n, rew_n, done_n, info = env.step(act)
        show(label, "step %d obs" % t, torch.cat([o.reshape(-1) for o in obs_n]))
        show(label, "step %d rew" % t, torch.stack(list(rew_n)))
        show(label, "step %d done" % t, torch.stack(list(done_n)))
        for k, s in enumerate(env._sets):
            for key, v in sorted(s.info.items()):
                show(label, "step %d set %d info_%s" % (t, k, key), v)
    state(label, "steps", env)


def rollout(name, kw, B, n=T):
    label = label_of(name, kw, B)
    env = fresh(name, kw, B)
    traj = Trajectory(env, n)
    roll = RandomRollout(env, episode_len=EPISODE_LEN, pool=2, seed=SEED)
    roll.t = STEP0
    roll.fused(n, traj)
    show(label, "rollout obs", traj.obs_flat)
    show(label, "rollout rew", traj.rew)
    show(label, "rollout done", traj.done)
    state(label, "rollout", env)


def served(name, kw, B):
    label = label_of(name, kw, B)
    env = fresh(name, kw, B)
    if _abi.lib().mpe_step_server_supported(C.byref(env._desc), B) != 1:
        print("%-40s %-26s %s" % (label, "served", "(not served)"), flush=True)
        return
    rs = np.random.RandomState(3)
    A = len(env.world.agents)
    moves = one_hot(rs, (T, A, B), 5)
    comm = one_hot(rs, (T, A, B), int(env.world.dim_c)) if env._comm is not None else None
    srv = StepServer(env, moves, slots=T, episode_len=EPISODE_LEN, seed=SEED, timeout_s=5.0, probe=False, ahead=True, comm=comm)
    srv.run(T)
    torch.cuda.synchronize()
    srv.check()
    show(label, "served obs", srv.blocks.obs_flat)
    show(label, "served rew", srv.blocks.rew)
    show(label, "served done", srv.blocks.done)
    show(label, "served flag", srv.flag)
    state(label, "served", env)


def policy(name, kw, B):
    label = label_of(name, kw, B)
    env = fresh(name, kw, B)
    torch.manual_seed(7)
    mods = []
    for i in range(env.n):
        D = int(env._obs_off[i + 1] - env._obs_off[i])
        act = torch.nn.Tanh if i & 1 else torch.nn.ReLU      # (one activation per actor)
        mods.append(torch.nn.Sequential(torch.nn.Linear(D, 64), act(), torch.nn.Linear(64, 64), act(), torch.nn.Linear(64, 5)))
    mods = [m.cuda() for m in mods]
    roll = PolicyRollout(env, MlpPolicy(mods), mode="sample", episode_len=EPISODE_LEN, seed=SEED, policy_seed=11)
    roll.t = STEP0
    traj = roll.run(T, record_inputs=True)
    for what in ("obs_flat", "rew", "done", "act", "logp", "obs_in_flat"):
        show(label, "policy " + what, getattr(traj, what))
    state(label, "policy", env)


def main():
    assert torch.cuda.is_available(), "split_bits needs a GPU"
    # the dual-role kernels take a launch up to floor(1.5 * CUs) workgroups of 64 worlds (launch_split, launch_split_serve)
    b_single = 64 * (torch.cuda.get_device_properties(0).multi_processor_count * 3 // 2) + 37
    for name, kw in SHAPES:
        steps(name, kw, B_SMALL)
        for B in (B_SMALL, b_single):
            rollout(name, kw, B)
            served(name, kw, B)
    for name, kw in POLICY_SHAPES:
        policy(name, kw, B_SMALL)
    steps("simple_spread", {"num_agents": 3}, 65536, n=1)      # rows stored nontemporal
    rollout("simple_world_comm", {}, 65536, n=2)


if __name__ == "__main__":
    main()
