"""SHA-256 of everything the wide kernels (csrc/mpe_wide.hip) write, on the smallest shapes that reach each of their paths.

    python tools/wide_bits.py > profiles/wide_bits.txt          (MPE_HIP_LIB=<another build> for the other column)

Per shape, from a seeded device reset (a third of the worlds shrunk so that agents touch): 3 launched steps, then a 7-step
fused rollout with episode_len = 3 from global step 2 -- once with moves drawn in the kernel (mpe_rollout_random), once with the
caller's moves -- and one line per output tensor.  The caller's moves go to mpe_rollout_actions directly, not through
env.step_many: step_many launches the same entry point for these shapes but always counts its steps from 0, and the reset
schedule is wanted off the start of an episode.  Plus one observe-only call (mpe_observe) at N = 40 and one physics-only call
(mpe_world_step) at N = 40 (k_wave) and at N = 16 (k_multi).  The tests compare the wide kernels with
each other, or with the oracle at 1e-5; two listings from two builds on one machine compare them bit for bit.  The digests
depend on the compiler version: a tool for before / after a change to that file, not a test."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import multiagent_particle_envs_amd as mpe                                  # noqa: E402
from multiagent_particle_envs_amd import _abi                               # noqa: E402
from multiagent_particle_envs_amd.rollout import RandomRollout, Trajectory  # noqa: E402

SEED, T, EPISODE_LEN, STEP0 = 0x5EED, 7, 3, 2
TAG = {"num_adversaries": 40, "num_good_agents": 30, "num_landmarks": 20}
SHAPES = [("simple_spread", {"num_agents": 7}, 70), ("simple_spread", {"num_agents": 12}, 70),
          ("simple_spread", {"num_agents": 20}, 70), ("simple_spread", {"num_agents": 28}, 70),
          ("simple_spread", {"num_agents": 33}, 5), ("simple_spread", {"num_agents": 34}, 258),
          ("simple_spread", {"num_agents": 64}, 256), ("simple_spread", {"num_agents": 70}, 33), ("simple_tag", TAG, 64)]


def digest(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def show(label, what, t):
    print("%-34s %-22s %s" % (label, what, digest(t)))


def fresh(name, kw, B):
    env = mpe.make_env(name, benchmark=True, batch_size=B, seed=SEED, **kw)
    env.reset()
    env.world.pos[..., ::3] *= 0.35
    return env


def moves(rs, shape):
    return torch.as_tensor(np.eye(5, dtype=np.float32)[rs.randint(0, 5, size=shape)]).cuda().contiguous()


def state(label, what, env):
    show(label, what + " pos", env.world.pos)
    show(label, what + " vel", env.world.vel)


def run(name, kw, B):
    label = "%s %s B=%d" % (name, ",".join(str(v) for v in kw.values()), B)
    rs = np.random.RandomState(1)
    env = fresh(name, kw, B)
    A = len(env.world.agents)
    for t in range(3):
        obs_n, rew_n, done_n, info = env.step(moves(rs, (A, B)))
        show(label, "step %d obs" % t, torch.cat([o.reshape(-1) for o in obs_n]))
        show(label, "step %d rew" % t, torch.stack(list(rew_n)))
        show(label, "step %d done" % t, torch.stack(list(done_n)))
        for k, s in enumerate(env._sets):
            for key, v in sorted(s.info.items()):
                show(label, "step %d set %d info_%s" % (t, k, key), v)
    state(label, "steps", env)
    for how in ("drawn", "act_seq"):
        env = fresh(name, kw, B)
        traj = Trajectory(env, T)
        if how == "drawn":
            roll = RandomRollout(env, episode_len=EPISODE_LEN, pool=2, seed=SEED)
            roll.t = STEP0
            roll.fused(T, traj)
        else:
            seq = moves(rs, (T, A, B))
            b = traj.bufs
            b.act = b.ids = b.u = None
            _abi.check(_abi.lib().mpe_rollout_actions(C.byref(env._desc), C.byref(b), B, T, EPISODE_LEN, float(getattr(env._scenario, "landmark_range", 1.0)),
                                                      SEED, STEP0, int(env.world.world_offset), 1, seq.data_ptr(),
                                                      _abi.raw_stream(env.world.device)), "mpe_rollout_actions")
        show(label, "rollout %s obs" % how, traj.obs_flat)
        show(label, "rollout %s rew" % how, traj.rew)
        show(label, "rollout %s done" % how, traj.done)
        state(label, "rollout " + how, env)


def main():
    assert torch.cuda.is_available(), "wide_bits needs a GPU"
    for name, kw, B in SHAPES:
        run(name, kw, B)
    # physics only (mpe_world_step) and observe only (mpe_observe, inside env.reset) at N = 40
    env = fresh("simple_spread", {"num_agents": 40}, 70)
    show("simple_spread 40 B=70", "observe-only obs", torch.cat([o.reshape(-1) for o in env._sets[0].obs_n] +
                                                                 [o.reshape(-1) for s in env._sets[1:] for o in s.obs_n]))
    for n in (40, 16):
        env = fresh("simple_spread", {"num_agents": n}, 70)
        rs = np.random.RandomState(2)
        for agent in env.world.agents:
            agent.action.u = torch.as_tensor(rs.uniform(-1, 1, size=(70, 2)).astype(np.float32)).cuda()
        env.world.step()
        state("simple_spread %d B=70" % n, "physics-only", env)


if __name__ == "__main__":
    main()
