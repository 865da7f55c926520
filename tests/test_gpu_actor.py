"""GPU: the standalone actor kernel (mpe_actor_act / policy.Actors) and the closed loop over it (policy.PolicyLoop).

Decisions are checked against Actors.reference (an fp64 torch forward pass) under the bands of tests/test_gpu_policy.py: logits and
softmax rows within 1e-5 * max(1, max|z|); one-hot rows equal to the fp64 choice wherever the fp64 margin is outside that band;
logp within 1e-5; rows inside the band are left out and may be at most 0.1 % of the rows checked."""
import os

import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop
from multiagent_particle_envs_amd.rollout import MlpPolicy, PolicyRollout, step_many
from oracle import philox

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINE = ["simple", "simple_spread", "simple_tag", "simple_adversary", "simple_push", "simple_speaker_listener", "simple_reference",
        "simple_crypto", "simple_world_comm"]
ENVS = [(n, {}) for n in NINE] + [("simple_spread", {"num_agents": 10}), (os.path.join(ROOT, "examples", "corral.py"), {}),
                                  (os.path.join(ROOT, "tests", "refstyle", "convoy.py"), {}),
                                  ("simple_spread", {"num_agents": 16})]      # 96 columns: three passes of the first layer's k loop
# (activation, hidden widths): 3, 2 and 1 Linear layers, a hidden width that is not a multiple of 16
CONFIGS = [(torch.nn.ReLU, (64, 64)), (torch.nn.Tanh, (64,)), (torch.nn.ReLU, ()), (torch.nn.Tanh, (20, 64)), (torch.nn.ReLU, (20,))]
STREAMS = (_abi.MPE_STREAM_POLICY, _abi.MPE_STREAM_POLICY_COMM)


def fresh(name, kw, B, off=0):
    env = mpe.make_env(name, batch_size=B, seed=7, **kw)
    env.reset()
    env.world.world_offset = off
    return env


def widths(env):
    return [int(env._obs_off[i + 1] - env._obs_off[i]) for i in range(len(env.world.agents))]


def actors(env, seed, hidden=(64, 64), act=torch.nn.ReLU):
    """torch's default init, one module per agent: D_i -> hidden -> 5 * movable + dim_c * speaks"""
    torch.manual_seed(seed)
    speaks = any(not a.silent for a in env.world.agents)
    mods = []
    for i, D in enumerate(widths(env)):
        a = env.world.agents[i]
        sizes = [D] + list(hidden) + [5 * bool(a.movable) + (env.world.dim_c if speaks and not a.silent else 0)]
        layers = []
        for k in range(len(sizes) - 1):
            layers.append(torch.nn.Linear(sizes[k], sizes[k + 1]))
            if k + 2 < len(sizes):
                layers.append(act())
        mods.append(torch.nn.Sequential(*layers).cuda())
    return mods


def draw_bits(stream, seed, B, step, A, world_offset):
    """[A, B] uint32: key = seed, counter = (world lo, world hi ^ step hi, agent >> 2, stream ^ step lo), word agent & 3."""
    b = np.arange(B, dtype=np.uint64) + np.uint64(world_offset)
    out = np.zeros((A, B), np.uint32)
    for q in range((A + 3) // 4):
        o = philox.philox4x32_10(b & philox.MASK, ((b >> np.uint64(32)) ^ np.uint64(step >> 32)) & philox.MASK,
                                 np.full(B, q, np.uint64), np.full(B, (stream ^ (step & 0xFFFFFFFF)) & 0xFFFFFFFF, np.uint64),
                                 seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        for k in range(4):
            if 4 * q + k < A:
                out[4 * q + k] = o[k]
    return out


def check_decisions(pi, obs_n, t, moves=None, logp=None):
    """pi's outputs of act(obs_n, t) against the fp64 reference -> (rows checked, rows left out as inside the band)."""
    ref = pi.reference(obs_n)
    B, A, mode = pi.B, pi.A, pi.mode
    moves = pi.moves if moves is None else moves
    logp = pi.logp if logp is None else logp
    checked = inband = 0
    for i in range(A):
        heads = [(ref[i][0], moves[i], 0), (ref[i][1], pi.utter[i] if pi.utter is not None else None, 1)]
        zall = torch.cat([z for z, _, _ in heads if z is not None], dim=1)
        scale = torch.clamp(zall.abs().max(dim=-1).values, min=1.0)
        if pi.logits is not None:
            got = pi.logits[i].double()
            assert float(((got[:, :zall.shape[1]] - zall).abs().max(dim=-1).values / scale).max()) < 1e-5, ("logits", i)
            assert float(got[:, zall.shape[1]:].abs().max()) == 0.0 if zall.shape[1] < 16 else True
        lp = torch.zeros(B, dtype=torch.float64, device=zall.device)
        for z, rows, h in heads:
            if z is None:
                if rows is not None:
                    assert float(rows.abs().max()) == 0.0, ("a head the agent does not have", i, h)
                if pi.ids is not None:
                    assert bool((pi.ids[h, i] == -1).all())
                continue
            a, n = rows.double(), z.shape[1]
            p = torch.softmax(z, dim=-1)
            hs = torch.clamp(z.abs().max(dim=-1).values, min=1.0)
            if mode == "softmax":
                assert float((a - p).abs().max()) < 1e-5, (i, h)
                checked += B
                continue
            idx = a.argmax(dim=-1)
            assert torch.equal(a.sum(dim=-1), torch.ones_like(a[:, 0])) and float(a.max()) == 1.0, (i, h)
            if pi.ids is not None:
                assert torch.equal(pi.ids[h, i].long(), idx), (i, h)
            if mode == "greedy":
                if n > 1:
                    top = torch.topk(z, 2, dim=-1).values
                    margin = (top[:, 0] - top[:, 1]) > 1e-5 * hs
                else:
                    margin = torch.ones(B, dtype=torch.bool, device=z.device)
                want = z.argmax(dim=-1)
            else:
                bits = draw_bits(STREAMS[h], pi.seed, B, t, A, int(pi.world.world_offset))[i]
                u = torch.as_tensor((bits >> 8).astype(np.float64) * 2.0 ** -24, device=z.device)
                cum = torch.cumsum(p, dim=-1)[:, :n - 1]
                want = (cum <= u[:, None]).sum(dim=-1).clamp(max=n - 1)
                margin = ((cum - u[:, None]).abs() > 1e-5).all(dim=-1)
            lp += torch.log(p.gather(1, idx[:, None]))[:, 0]
            assert int((margin & (idx != want)).sum()) == 0, (i, h, mode)
            checked += B
            inband += int((~margin).sum())
        if logp is not None and mode != "softmax":
            assert float((logp[i].double() - lp).abs().max()) < 1e-5, ("logp", i)
    return checked, inband


@pytest.mark.parametrize("mode", ["greedy", "softmax", "sample"])
@pytest.mark.parametrize("k", range(len(ENVS)))
def test_decisions_against_fp64(k, mode):
    name, kw = ENVS[k]
    B, off = 4000, 777      # a ragged last wave; a world_offset that moves the draw keys
    env = fresh(name, kw, B, off)
    checked = inband = 0
    for c in (k, k + 2):
        act, hidden = CONFIGS[c % len(CONFIGS)]
        pi = Actors(env, actors(env, 1 + c, hidden, act), mode=mode, seed=9, logp=True, ids=True, logits=True)
        gen = torch.Generator(device="cuda").manual_seed(100 + k)
        obs_n = [torch.rand((B, D), generator=gen, device="cuda") * 2 - 1 for D in widths(env)]
        for t in (3, (5 << 32) + 11):
            pi.act(obs_n, t)
            torch.cuda.synchronize()
            n, m = check_decisions(pi, obs_n, t)
            checked += n
            inband += m
    print("%s %s: %d rows checked, %d inside the band" % (os.path.basename(name), mode, checked, inband))
    assert inband <= 0.001 * checked + 1


ROLLOUT_SHAPES = [("simple", {}, 4096, 0), ("simple_spread", {}, 4000, 777), ("simple_adversary", {}, 4096, 0), ("simple_push", {}, 4000, 123)]


@pytest.mark.parametrize("mode", ["greedy", "softmax", "sample"])
@pytest.mark.parametrize("name,kw,B,off", ROLLOUT_SHAPES)
def test_same_decisions_as_policy_rollout(name, kw, B, off, mode):
    """PolicyRollout's recorded decision inputs through the standalone kernel, same policy seed: the same rows.  This pins the sample
    draw's key layout.  Both kernels are the same fmaf chain: the number of rows that differ at all is printed (expected 0)."""
    env = fresh(name, kw, B, off)
    mods = actors(env, 1)
    traj = PolicyRollout(env, MlpPolicy(mods), mode=mode, episode_len=25, policy_seed=9).run(30, record_inputs=True)
    pi = Actors(env, mods, mode=mode, seed=9, logp=mode != "softmax", logits=True)
    differ = checked = inband = 0
    for t in (0, 1, 24, 25, 29):
        a = pi.act(traj.obs_in[t], t)
        torch.cuda.synchronize()
        n, m = check_decisions(pi, traj.obs_in[t], t)
        checked += n
        inband += m
        rows = (a != traj.act[t]).any(dim=-1)
        differ += int(rows.sum())
        if mode == "softmax":
            assert float((a - traj.act[t]).abs().max()) < 2e-5, t
        else:
            # a row the two kernels choose differently must be one the fp64 reference leaves out (inside the band)
            n2, m2 = check_decisions(pi, traj.obs_in[t], t, moves=traj.act[t], logp=traj.logp[t] if traj.logp is not None else None)
            inband = max(inband, m2)
            if traj.logp is not None and pi.logp is not None:
                same = ~rows
                assert float(((pi.logp - traj.logp[t]).abs() * same).max()) < 2e-5, t
    print("%s %s: rows that differ at all between mpe_actor_act and mpe_rollout_policy: %d of %d" % (name, mode, differ, checked))
    assert differ <= 0.001 * checked + 1 and inband <= 0.001 * checked + 1


@pytest.mark.parametrize("name", ["simple_tag", "simple_reference"])
def test_action_is_what_env_step_takes(name):
    B = 4000
    env, twin = fresh(name, {}, B), fresh(name, {}, B)
    twin.world.set_state(*env.world.get_state())
    assert torch.equal(env.world.pos, twin.world.pos)
    pi = Actors(env, actors(env, 2), mode="sample", seed=4)
    obs = env.reset()
    twin.reset()
    assert all(torch.equal(a, b) for a, b in zip(obs, twin._sets[twin._flip].obs_n))
    for t in range(3):
        action = pi.act(obs, t)
        pair = isinstance(action, tuple)
        assert pair == (name == "simple_reference")
        moves = (action[0] if pair else action).clone()[None].contiguous()
        comm = action[1].clone()[None].contiguous() if pair else None
        obs, rew, done, _ = env.step(action)
        o2, r2, d2 = step_many(twin, moves, comm=comm)[0]
        torch.cuda.synchronize()
        for i in range(env.n):
            assert torch.equal(obs[i], o2[i]), (t, i)
            assert torch.equal(rew[i], r2[i]) and torch.equal(done[i], d2[i]), (t, i)
    assert torch.equal(env.world.pos, twin.world.pos) and torch.equal(env.world.vel, twin.world.vel)


@pytest.mark.parametrize("name", ["simple_tag", "simple_speaker_listener"])
def test_policy_loop_is_the_hand_written_loop(name):
    B, T = 4000, 60
    envs = [fresh(name, {}, B) for _ in range(3)]
    mods = actors(envs[0], 3)
    pis = [Actors(e, mods, mode="sample", seed=5, logp=True) for e in envs]
    loops = [PolicyLoop(e, p, episode_len=25) for e, p in zip(envs, pis)]
    traj = loops[0].run(T)
    assert loops[0].t == T
    # the hand-written loop: the device reset at steps 0, 25 and 50, then act / step
    env, pi = envs[1], pis[1]

    def hand(t0, n, check):
        obs = hand.obs
        for t in range(t0, t0 + n):
            if t % 25 == 0:
                obs = loops[1].device_reset(t // 25)
            action = pi.act(obs, t)
            mv = action[0] if isinstance(action, tuple) else action
            if check is not None:
                assert torch.equal(mv, check.act[t - t0]), t
                assert torch.equal(pi.logp, check.logp[t - t0]), t
                if check.utter is not None:
                    assert torch.equal(action[1], check.utter[t - t0]), t
            obs, rew, done, _ = env.step(action)
            if check is not None:
                for i in range(env.n):
                    assert torch.equal(obs[i], check.obs[t - t0][i]), (t, i)
                    assert torch.equal(rew[i], check.rew[t - t0, i]) and torch.equal(done[i], check.done[t - t0, i]), (t, i)
        hand.obs = obs
    hand.obs = None
    hand(0, T, traj)
    assert torch.equal(envs[0].world.pos, env.world.pos)
    # the same T steps as one graph, from the same (fresh) state
    g = loops[2].capture(T)
    g.replay()
    torch.cuda.synchronize()
    assert loops[2].t == T
    assert torch.equal(envs[2].world.pos, envs[0].world.pos) and torch.equal(envs[2].world.vel, envs[0].world.vel)
    for i in range(env.n):
        assert torch.equal(loops[2].obs_n[i], loops[0].obs_n[i]), i
    # a second run continues the step count (draw keys, episode clock)
    traj2 = loops[0].run(15)
    assert loops[0].t == T + 15
    hand(T, 15, traj2)
    assert torch.equal(envs[0].world.pos, env.world.pos)


def test_refusals_leave_the_world_untouched():
    from multiagent_particle_envs_amd import scenarios
    B = 256
    # noise, max_episode_steps, a Python callback: what step_many refuses, by the same names
    env = fresh("simple_spread", {}, B)
    pi = Actors(env, actors(env, 1))
    env.world.agents[0].u_noise = 0.1
    pos = env.world.pos.clone()
    with pytest.raises(_abi.MpeError, match="fused"):
        PolicyLoop(env, pi)
    assert torch.equal(env.world.pos, pos)
    env = mpe.make_env("simple_spread", batch_size=B, max_episode_steps=25)
    env.reset()
    pos = env.world.pos.clone()
    with pytest.raises(_abi.MpeError, match="max_episode_steps"):
        PolicyLoop(env, Actors(env, actors(env, 1))).run(3)
    assert torch.equal(env.world.pos, pos)
    sc = scenarios.load("simple_spread.py").Scenario()
    w = sc.make_world(batch_size=B)
    env = mpe.MultiAgentEnv(w, sc.reset_world, lambda agent, world: sc.reward(agent, world), sc.observation)
    env.reset()
    pos = env.world.pos.clone()
    with pytest.raises(_abi.MpeError):
        PolicyLoop(env, Actors(env, actors(env, 1))).run(3)
    assert torch.equal(env.world.pos, pos)
    # 65-wide hidden layers; an input wider than the cap (refused by the C entry point too, by name)
    env = fresh("simple_spread", {}, B)
    pos = env.world.pos.clone()
    with pytest.raises(_abi.MpeError, match="hidden width 65 > 64"):
        Actors(env, actors(env, 1, hidden=(65,)))
    aset = _abi.MpeActorSet()
    aset.n_agents, aset.mode = 1, _abi.MPE_POLICY_GREEDY
    aset.n_layers[0], aset.movable[0] = 1, 1
    aset.width[0][0], aset.width[0][1] = _abi.MPE_ACTOR_MAX_INPUT + 1, 5
    import ctypes as C
    assert _abi.lib().mpe_actor_supported(C.byref(aset), B) == 0
    assert b"MPE_ACTOR_MAX_INPUT" in _abi.lib().mpe_last_error()
    aset.width[0][0] = 18
    assert _abi.lib().mpe_actor_supported(C.byref(aset), B) == 1
    aset.n_agents = _abi.MPE_ACTOR_MAX_AGENTS + 1
    assert _abi.lib().mpe_actor_supported(C.byref(aset), B) == 0
    assert b"MPE_ACTOR_MAX_AGENTS" in _abi.lib().mpe_last_error()
    assert torch.equal(env.world.pos, pos)
