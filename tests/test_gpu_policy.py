"""GPU: policy rollouts (mpe_rollout_policy / PolicyRollout) -- an MLP actor per agent evaluated inside the fused rollout.

The rows the kernel chose are replayed through step_many (the step server: the golden-checked step path) and must give the
same outputs bit for bit; the decisions are checked against an fp64 torch forward pass on the recorded decision inputs; the
decision inputs themselves against the env's own observations."""
import os

import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.rollout import MlpPolicy, PolicyRollout, step_many
from oracle import philox
from oracle import spec as ospec
from oracle.mpe_batched import BatchedOracle, seeded_initial_state
from oracle.mpe_f3 import F3Oracle

from _parity_util import close, np_

pytestmark = pytest.mark.gpu

# (name, kwargs, worlds, world_offset): 4000 leaves a ragged last wave (the live-lane guards of the act / obs_in / logp stores);
# a world_offset != 0 moves the sample draws, which are keyed by the global world
SHAPES = [("simple", {}, 4096, 0), ("simple_spread", {}, 4096, 0), ("simple_spread", {}, 65536, 0), ("simple_spread", {}, 4000, 777),
          ("simple_adversary", {}, 4096, 0), ("simple_push", {}, 4000, 123)]
SPECS = {"simple": lambda: ospec.simple(), "simple_spread": lambda: ospec.simple_spread(3),
         "simple_adversary": lambda: ospec.by_name("simple_adversary"), "simple_push": lambda: ospec.by_name("simple_push")}
F3 = ("simple_adversary", "simple_push")


def actors(env, seed, hidden=(64, 64), act=torch.nn.ReLU):
    torch.manual_seed(seed)
    mods = []
    for i in range(env.n):
        D = int(env._obs_off[i + 1] - env._obs_off[i])
        widths = [D] + list(hidden) + [5]
        layers = []
        for k in range(len(widths) - 1):
            layers.append(torch.nn.Linear(widths[k], widths[k + 1]))
            if k + 2 < len(widths):
                layers.append(act())
        mods.append(torch.nn.Sequential(*layers).cuda())
    return mods


def fresh(name, kw, B):
    env = mpe.make_env(name, batch_size=B, seed=7, **kw)
    env.reset()
    return env


STREAM_POLICY = 0x504F4C49   # "POLI"


def policy_bits(seed, B, step, A, world_offset=0):
    """[A, B] uint32: the SAMPLE draw's bits, restated from oracle.philox under action_ids' counter layout: key = policy seed,
    counter = (world lo, world hi ^ step hi, agent >> 2, STREAM_POLICY ^ step lo), word agent & 3."""
    b = np.arange(B, dtype=np.uint64) + np.uint64(world_offset)
    out = np.zeros((A, B), np.uint32)
    for q in range((A + 3) // 4):
        o = philox.philox4x32_10(b & philox.MASK, ((b >> np.uint64(32)) ^ np.uint64(step >> 32)) & philox.MASK,
                                 np.full(B, q, np.uint64), np.full(B, (STREAM_POLICY ^ (step & 0xFFFFFFFF)) & 0xFFFFFFFF, np.uint64),
                                 seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        for k in range(4):
            if 4 * q + k < A:
                out[4 * q + k] = o[k]
    return out


def z64(mods, i, x):
    import copy
    m = copy.deepcopy(mods[i]).double()
    with torch.no_grad():
        return m(x.double())


@pytest.mark.parametrize("mode", ["greedy", "softmax", "sample"])
@pytest.mark.parametrize("name,kw,B,off", SHAPES)
def test_replay_identity_and_decisions(name, kw, B, off, mode):
    env = fresh(name, kw, B)
    env2 = fresh(name, kw, B)
    env2.world.set_state(*env.world.get_state())
    env.world.world_offset = env2.world.world_offset = off
    mods = actors(env, 1)
    roll = PolicyRollout(env, MlpPolicy(mods), mode=mode, episode_len=25, policy_seed=9)
    T = 60
    traj = roll.run(T, record_inputs=True)
    torch.cuda.synchronize()
    # 1. replay through the golden-checked step path, bit for bit
    outs = step_many(env2, traj.act.contiguous(), episode_len=25, seed=env.world.seed)
    torch.cuda.synchronize()
    for t in range(T):
        o, r, d = outs[t]
        for i in range(env.n):
            assert torch.equal(traj.obs[t][i], o[i]), (t, i)
        assert torch.equal(traj.rew[t], r), t
        assert torch.equal(traj.done[t], d), t
    p1, v1 = env.world.get_state()
    p2, v2 = env2.world.get_state()
    assert np.array_equal(p1, p2) and np.array_equal(v1, v2)
    # 3. decision inputs: obs_in[t] is step t-1's output unless t is an episode start
    for t in range(1, T):
        if t % 25:
            for i in range(env.n):
                assert torch.equal(traj.obs_in[t][i], traj.obs[t - 1][i]), (t, i)
    # 2. decisions against fp64
    bad = n = 0
    for t in (0, 1, 24, 25, 26, 59):
        for i in range(env.n):
            z = z64(mods, i, traj.obs_in[t][i])
            a = traj.act[t, i].double()
            p = torch.softmax(z, dim=-1)
            if mode == "softmax":
                assert float((a - p).abs().max()) < 1e-5, (t, i)
                continue
            idx = a.argmax(dim=-1)
            assert torch.equal(a.sum(dim=-1), torch.ones_like(a[:, 0])), (t, i)
            if mode == "greedy":
                top = torch.topk(z, 2, dim=-1).values
                margin = (top[:, 0] - top[:, 1]) > 1e-5 * torch.clamp(z.abs().max(dim=-1).values, min=1.0)
                want = z.argmax(dim=-1)
            else:
                bits = policy_bits(roll.policy_seed, B, t, env.n, int(env.world.world_offset))[i]
                u = torch.as_tensor((bits >> 8).astype(np.float64) * 2.0 ** -24, device=z.device)
                cum = torch.cumsum(p, dim=-1)[:, :4]
                want = (cum <= u[:, None]).sum(dim=-1).clamp(max=4)
                margin = ((cum - u[:, None]).abs() > 1e-5).all(dim=-1)
                lp = torch.log(p.gather(1, idx[:, None]))[:, 0]
                assert float((traj.logp[t, i].double() - lp).abs().max()) < 1e-5, (t, i)
            bad += int((margin & (idx != want)).sum())
            n += int((~margin).sum())
    assert bad == 0
    assert n <= 0.001 * 6 * env.n * B + 1


@pytest.mark.parametrize("name,kw,B,off", [s for s in SHAPES if s[2] != 65536])
def test_episode_start_inputs_against_the_oracle(name, kw, B, off):
    """episode_len = 25: steps 0, 25 and 50 are episode starts, and the actor acts on the RESET state -- its observation is
    assembled in the kernel from registers, not stored by any step.  obs_in there is the fp64 oracle's observation of the state
    mpe_reset draws (oracle.philox.reset_positions / reset_choices for episodes 0, 1, 2), within 1e-5."""
    spec = SPECS[name]()
    env = fresh(name, kw, B)
    env.world.world_offset = off
    roll = PolicyRollout(env, MlpPolicy(actors(env, 8)), mode="sample", episode_len=25, seed=4242, policy_seed=1)
    traj = roll.run(51, record_inputs=True)
    torch.cuda.synchronize()
    A, L = spec.n_agents, spec.n_entities - spec.n_agents
    pops = list(spec.choice_pops) if name in F3 else []
    for ep, t in enumerate((0, 25, 50)):
        orc = (F3Oracle if name in F3 else BatchedOracle)(spec, B, np.float64)
        orc.set_state(philox.reset_positions(4242, B, ep, A, L, spec.landmark_range, off).astype(np.float64), np.zeros((B, A, 2)))
        if pops:
            orc.set_choice(philox.reset_choices(4242, B, ep, pops, off).T.astype(np.int64))
        want = orc.observe()
        for i in range(A):
            close(np_(traj.obs_in[t][i]), want[i], what="t=%d obs_in%d" % (t, i))


@pytest.mark.parametrize("name,B", [("simple_spread", 4096), ("simple", 4096)])
def test_free_running_against_the_oracle(name, B):
    """The rollout's own rows fed to the fp64 oracle from the same start state, free-running for one episode (no teacher forcing):
    the GPU's drift from fp64 stays within test_free_running_episode_drift's bound -- 2x the drift of the same arithmetic in
    NumPy float32 (+ 1e-7) at the median, p90 and p99, median < 1e-5, max < 2e-3."""
    spec = SPECS[name]()
    pos, vel = seeded_initial_state(spec, np.arange(B) + 5000)
    p32 = pos.astype(np.float32)
    o64, o32 = BatchedOracle(spec, B, np.float64), BatchedOracle(spec, B, np.float32)
    o64.set_state(p32, vel)
    o32.set_state(p32, vel)
    env = mpe.make_env(name, batch_size=B, seed=3)
    env.reset()
    env.world.set_state(p32, vel)
    roll = PolicyRollout(env, MlpPolicy(actors(env, 12)), mode="sample", episode_len=0, policy_seed=5)
    t = 0
    for n in (5, 5, 15):            # three launches: steps 1-5, 6-10, 11-25 (the state in HBM after each)
        traj = roll.run(n)
        for k in range(n):
            act = np_(traj.act[k])
            assert np.array_equal(act.sum(-1), np.ones(act.shape[:2], np.float32))
            o64.step(act)
            o32.step(act)
        t += n
        gpos, _ = env.world.get_state()
        err = np.abs(gpos - o64.pos).max(axis=(1, 2))
        err32 = np.abs(o32.pos.astype(np.float64) - o64.pos).max(axis=(1, 2))
        for q in (50, 90, 99):
            assert np.percentile(err, q) <= 2.0 * np.percentile(err32, q) + 1e-7, (t, q)
    assert np.median(err) < 1e-5 and err.max() < 2e-3


def test_launches_are_bounded_by_work():
    """One launch holds at most MPE_POLICY_MAX_LAUNCH_WORK agent-world-steps: the ABI refuses more, run() splits by work and
    gives the same rollout as short runs."""
    import ctypes as C
    B = 65536
    env = fresh("simple_spread", {}, B)
    env2 = fresh("simple_spread", {}, B)
    env2.world.set_state(*env.world.get_state())
    mods = actors(env, 13)
    roll = PolicyRollout(env, MlpPolicy(mods), mode="sample", episode_len=25, policy_seed=2)
    T = _abi.MPE_POLICY_MAX_LAUNCH_WORK // (env.n * B) + 5        # two launches inside one run()
    traj = roll.run(T)
    _, pol = MlpPolicy(mods).pack(roll.obs_widths, env.world.device, "greedy", 0)
    rc = _abi.lib().mpe_rollout_policy(C.byref(roll._desc), C.byref(traj.bufs), C.byref(pol), B, T, 25, 1.0, 0, 0, 0, 1,
                                       traj.act.data_ptr(), None, None, _abi.raw_stream(env.world.device))
    assert rc == -1 and b"T * B * A" in _abi.lib().mpe_last_error()
    r2 = PolicyRollout(env2, MlpPolicy(mods), mode="sample", episode_len=25, policy_seed=2)
    a = r2.run(100)                                             # (other launch boundaries than the long run's)
    b = r2.run(T - 100)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([a.act, b.act]), traj.act) and torch.equal(env.world.pos, env2.world.pos)


def test_decision_inputs_match_env_observation():
    """episode_len = 0: the first decision acts on the env's current observation (env.step's last obs_n)."""
    B = 4096
    env = fresh("simple_spread", {}, B)
    mv = torch.nn.functional.one_hot(torch.randint(0, 5, (env.n, B), device="cuda"), 5).float()
    obs_n, _, _, _ = env.step(mv)
    obs_n = [o.clone() for o in obs_n]
    roll = PolicyRollout(env, MlpPolicy(actors(env, 2)), episode_len=0)
    traj = roll.run(3, record_inputs=True)
    torch.cuda.synchronize()
    for i in range(env.n):
        assert torch.equal(traj.obs_in[0][i], obs_n[i]), i


def test_users_torch_loop_agrees():
    """episode_len = 0, T = 25: the eager torch greedy loop over env.step takes the same decisions (>= 99.9 %)."""
    B, T = 4096, 25
    env = fresh("simple_spread", {}, B)
    env2 = fresh("simple_spread", {}, B)
    mv = torch.zeros((env.n, B, 5), device="cuda")
    mv[..., 0] = 1
    obs_n = [o.clone() for o in env2.step(mv)[0]]
    env.world.set_state(*env2.world.get_state())
    mods = actors(env, 3)
    pol = MlpPolicy(mods)
    traj = PolicyRollout(env, pol, episode_len=0).run(T)
    agree = 0
    same = torch.ones(B, dtype=torch.bool, device="cuda")       # worlds whose decisions all agree
    for t in range(T):
        rows = pol.action(obs_n, mode="greedy")
        for i in range(env.n):
            eq = rows[i].argmax(-1) == traj.act[t, i].argmax(-1)
            agree += int(eq.sum())
            same &= eq
        obs_n = [o.clone() for o in env2.step(torch.stack(rows))[0]]
    assert agree >= 0.999 * T * env.n * B
    for i in range(env.n):
        assert float((traj.obs[T - 1][i][same] - obs_n[i][same]).abs().max()) <= 1e-6, i
    assert float((env.world.pos[..., same] - env2.world.pos[..., same]).abs().max()) <= 1e-6


def test_continuity_and_freshness():
    B = 4096
    a, b = fresh("simple_spread", {}, B), fresh("simple_spread", {}, B)
    b.world.set_state(*a.world.get_state())
    mods = actors(a, 4)
    ra = PolicyRollout(a, MlpPolicy(mods), mode="sample", policy_seed=3)
    import copy
    rb = PolicyRollout(b, MlpPolicy(copy.deepcopy(mods)), mode="sample", policy_seed=3)      # (its own copy: not edited below)
    t1 = ra.run(30)
    t2 = ra.run(30)
    tb = rb.run(60)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([t1.act, t2.act]), tb.act) and torch.equal(torch.cat([t1.rew, t2.rew]), tb.rew)
    assert torch.equal(a.world.pos, b.world.pos)
    with torch.no_grad():
        mods[0][0].weight.mul_(-3.0)
    t3 = ra.run(30)
    t4 = rb.run(30)
    torch.cuda.synchronize()
    assert not torch.equal(t3.act[:, 0], t4.act[:, 0])


def test_refusals_leave_the_env_untouched():
    cases = [("simple_speaker_listener", {}), ("simple_spread", {"num_agents": 20}), ("simple_spread", {"num_agents": 4}), ("simple_spread", {}), ("simple_tag", {})]
    for k, (name, kw) in enumerate(cases):
        env = fresh(name, kw, 256)
        pos = env.world.pos.clone()
        if k == 3:
            mods = actors(env, 5)
            mods[0] = torch.nn.Sequential(torch.nn.Linear(7, 5)).cuda()
        else:
            mods = torch.nn.Sequential(torch.nn.Linear(int(env._obs_off[1]), 5)).cuda()
        with pytest.raises(_abi.MpeError):
            PolicyRollout(env, mods).run(3)
        assert torch.equal(env.world.pos, pos)
    env = mpe.make_env(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "corral.py"),
                       batch_size=256)                                           # a row-program env
    env.reset()
    pos = env.world.pos.clone()
    with pytest.raises(_abi.MpeError):
        PolicyRollout(env, torch.nn.Sequential(torch.nn.Linear(int(env._obs_off[1]), 5)).cuda()).run(3)
    assert torch.equal(env.world.pos, pos)
    env = mpe.make_env("simple_spread", batch_size=256, max_episode_steps=25)
    env.reset()
    pos = env.world.pos.clone()
    with pytest.raises(_abi.MpeError):
        PolicyRollout(env, MlpPolicy(actors(env, 6))).run(3)
    assert torch.equal(env.world.pos, pos)
