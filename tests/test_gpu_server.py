"""The step server (include/mpe_hip.h: mpe_step_server_*; rollout.StepServer): per-step COMMANDS to one resident launch.

The served steps must be the per-step kernel's, bit for bit -- T x {mpe_reset at the episode boundaries; mpe_step} through
RandomRollout.enqueue on a second env with the same seed and the same move tensors -- in every commanding pattern: all doorbells
rung ahead (the pipelined regime the server exists for), one at a time with the host in between (the closed loop: the server is
AHEAD of its commander and must publish a step's completion without waiting for the next command), in bursts; on ragged batches,
with per-world picks (simple_adversary) and an immovable-free / adversary mix (simple_tag).  A server whose doorbell never rings
gives up after its timeout and says so; shapes it cannot serve are refused with the reason."""
import time

import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.rollout import RandomRollout, StepServer

pytestmark = pytest.mark.gpu


def reference_steps(name, kw, B, T, EP, ring):
    """T steps through the per-step launches: -> (the move ring, per step: obs rows of every agent, rew, done, pos, vel)."""
    env = mpe.make_env(name, batch_size=B, seed=3, **kw)
    rr = RandomRollout(env, episode_len=EP, pool=ring, regenerate=False)
    out = []
    for _ in range(T):
        o = rr.enqueue(1)
        torch.cuda.synchronize()
        pos, vel = env.world.pos.clone(), env.world.vel.clone()
        ch = env.world.choice_i32.clone() if env.world.choice_i32 is not None else None
        out.append(([x.clone() for x in o.obs_n], o.rew.clone(), o.done.clone(), pos, vel, ch))
    comm = rr.pool_c.clone() if rr.pool_c is not None else None
    return (rr.pool_t.clone(), comm, env._comm.clone() if env._comm is not None else None), out


def same(step, srv, env, g, what):
    obs, rew, done, pos, vel, ch = step
    o_s, r_s, d_s = srv.outputs(g)
    for i, (a, b) in enumerate(zip(o_s, obs)):
        assert torch.equal(a, b), "%s: obs of agent %d at step %d" % (what, i, g)
    assert torch.equal(r_s, rew) and torch.equal(d_s, done), "%s: rew / done at step %d" % (what, g)


# (up to 1.5 workgroups per CU -- 24 576 worlds on 256 CUs -- the server is the DUAL-role kernel, a physics and a rows wave per
#  agent; beyond, the single-role one: the 32 768- and 40 000-world cases)
CASES = [("simple_spread", {}, 4096, 25), ("simple_spread", {}, 1000, 7), ("simple_tag", {}, 1000, 25),
         ("simple_adversary", {}, 777, 10), ("simple_push", {}, 640, 25), ("simple", {}, 130, 5),
         ("simple_spread", {"num_agents": 5}, 900, 25), ("simple_spread", {}, 32768, 25), ("simple_tag", {}, 40000, 9),
         # the communication scenarios: the speakers' words come from an utterance ring as the moves from the move ring
         ("simple_speaker_listener", {}, 1000, 25), ("simple_reference", {}, 700, 6), ("simple_crypto", {}, 1500, 25),
         ("simple_world_comm", {}, 600, 10)]


@pytest.mark.parametrize("name,kw,B,EP", CASES)
def test_served_steps_are_the_launched_steps_bit_for_bit(name, kw, B, EP):
    T, ring = (60, 16) if B < 20000 else (28, 8)
    (moves, comm, comm_after), ref = reference_steps(name, kw, B, T, EP, ring)
    env = mpe.make_env(name, batch_size=B, seed=3, **kw)
    srv = StepServer(env, moves, slots=T, episode_len=EP, timeout_s=5.0, comm=comm)
    srv.start(T)
    srv.ring(T)                      # every step commanded ahead: the server runs them back to back
    srv.join()
    torch.cuda.synchronize()
    srv.check()
    assert int(srv.flag.min()) == T and int(srv.door.item()) == T
    for g in range(T):
        same(ref[g], srv, env, g, "all rung ahead")
    assert torch.equal(env.world.pos, ref[-1][3]) and torch.equal(env.world.vel, ref[-1][4])      # the state after the last step, in HBM
    if ref[-1][5] is not None:
        assert torch.equal(env.world.choice_i32, ref[-1][5])
    if comm_after is not None:       # the agents' comm state afterwards = their last words
        assert torch.equal(env._comm, comm_after)


@pytest.mark.parametrize("name,kw,B,EP", [CASES[1], CASES[3], CASES[7], CASES[11]])
def test_closed_loop_commands_one_step_at_a_time(name, kw, B, EP):
    """ring -> wait -> read -> ring ...: the server is ahead of its commander at every step (the idle path: a step's completion is
    published without the next command), state visible in HBM after each step, host pauses in between."""
    T, ring = 12, 4
    (moves, comm, _), ref = reference_steps(name, kw, B, T, EP, ring)
    env = mpe.make_env(name, batch_size=B, seed=3, **kw)
    srv = StepServer(env, moves, slots=2, episode_len=EP, timeout_s=20.0, comm=comm)
    srv.start(T)
    for g in range(T):
        srv.ring()
        srv.wait()
        torch.cuda.current_stream().synchronize()         # (only this stream: the server launch is still running on its own)
        assert int(srv.status.item()) == 0
        same(ref[g], srv, env, g, "closed loop")
        assert torch.equal(env.world.pos, ref[g][3]) and torch.equal(env.world.vel, ref[g][4]), "state in HBM after step %d" % g
        if g in (2, 7):
            time.sleep(0.05)
    srv.join()
    torch.cuda.synchronize()
    srv.check()


def test_bursts_and_two_launches():
    """Doorbells in bursts with the host asleep in between, over two consecutive server launches (the second starts from the
    state the first left in HBM; doorbell and flags count on)."""
    name, kw, B, EP = "simple_spread", {}, 2048, 25
    T, ring = 50, 8
    (moves, _, _), ref = reference_steps(name, kw, B, T, EP, ring)
    env = mpe.make_env(name, batch_size=B, seed=3, **kw)
    srv = StepServer(env, moves, slots=T, episode_len=EP, timeout_s=20.0)
    srv.start(30)
    for n in (1, 3, 9, 17):
        srv.ring(n)
        srv.wait()
        torch.cuda.current_stream().synchronize()
        time.sleep(0.01)
    srv.start(20)
    srv.ring(20)
    srv.join()
    torch.cuda.synchronize()
    srv.check()
    for g in range(T):
        same(ref[g], srv, env, g, "bursts")
    assert torch.equal(env.world.pos, ref[-1][3])


def dual_max_workgroups():
    """launch_split_serve takes the dual-role server up to n_cu * 3 / 2 workgroups of 64 worlds."""
    return torch.cuda.get_device_properties(0).multi_processor_count * 3 // 2


@pytest.mark.parametrize("role", ["dual", "single"])
def test_a_server_nobody_commands_gives_up(role):
    """A launch of 4 steps, 2 of them commanded: after the timeout the server says so (status 1, every workgroup's flag at 2) and
    has touched nothing of the 2 steps nobody commanded -- their output blocks are still what the caller left there (NaN rows,
    True dones) and the state in HBM is the state after 2 steps, as 2 env.step calls leave it.  The dual-role server's rows waves
    never wait for a doorbell themselves: they leave with the others (the workgroup's abort word)."""
    B = 512 if role == "dual" else 64 * dual_max_workgroups() + 37
    assert ((B + 63) // 64 <= dual_max_workgroups()) == (role == "dual")
    T = 4
    ref = mpe.make_env("simple_spread", batch_size=B, seed=3)
    env = mpe.make_env("simple_spread", batch_size=B, seed=3)
    ref.reset()
    env.world.set_state(*ref.world.get_state())
    g = torch.Generator(device="cpu").manual_seed(8)
    moves = torch.nn.functional.one_hot(torch.randint(0, 5, (T, 3, B), generator=g), 5).float().cuda()
    srv = StepServer(env, moves, slots=T, timeout_s=0.2)
    srv.blocks.obs_flat.fill_(float("nan"))
    srv.blocks.rew.fill_(float("nan"))
    srv.blocks.done.fill_(True)
    torch.cuda.synchronize()
    srv.start(T)
    srv.ring(2)
    t0 = time.time()
    srv.join()
    torch.cuda.synchronize()
    assert time.time() - t0 < 5.0
    assert int(srv.status.item()) == 1 and int(srv.flag.min()) == 2 and int(srv.flag.max()) == 2    # two steps served, then the timeout
    for t in range(2):
        obs_n, rew_n, done_n, _ = ref.step(moves[t])
        o_s, r_s, d_s = srv.outputs(t)
        for i in range(3):
            assert torch.equal(o_s[i], obs_n[i]) and torch.equal(r_s[i], rew_n[i]) and torch.equal(d_s[i], done_n[i]), (t, i)
    for t in (2, 3):
        o_s, r_s, d_s = srv.outputs(t)
        assert all(bool(torch.isnan(o).all()) for o in o_s), "block %d: rows written for a step nobody commanded" % t
        assert bool(torch.isnan(r_s).all()) and bool(d_s.all()), "block %d: rewards / dones written" % t
    assert torch.equal(env.world.pos, ref.world.pos) and torch.equal(env.world.vel, ref.world.vel)
    with pytest.raises(_abi.MpeError, match="timed out"):
        srv.check()
    with pytest.raises(_abi.MpeError, match="start"):
        srv.ring(5)


def test_what_the_server_refuses():
    env = mpe.make_env("simple_speaker_listener", batch_size=256)
    with pytest.raises(_abi.MpeError, match="utterances"):      # a scenario whose agents speak needs the utterance ring
        StepServer(env, torch.zeros((2, 2, 256, _abi.MPE_ACTION_DIM), device="cuda"))
    env = mpe.make_env("simple_spread", batch_size=256, num_agents=10)      # 20 entities: no wave-per-agent kernel
    with pytest.raises(_abi.MpeError, match="step server"):
        StepServer(env, torch.zeros((2, 10, 256, _abi.MPE_ACTION_DIM), device="cuda"))
    env = mpe.make_env("simple_spread", batch_size=256)
    with pytest.raises(_abi.MpeError, match="moves"):
        StepServer(env, torch.zeros((2, 3, 255, _abi.MPE_ACTION_DIM), device="cuda"))
    B = 1 << 20                                        # 16 384 workgroups cannot all be resident
    env = mpe.make_env("simple_spread", batch_size=B)
    srv = StepServer(env, torch.zeros((1, 3, B, _abi.MPE_ACTION_DIM), device="cuda"), slots=1)
    with pytest.raises(_abi.MpeError, match="resident"):
        srv.start(1)


@pytest.mark.parametrize("name", ["simple_spread", "simple_reference"])
@pytest.mark.parametrize("graphs", [False, True])
def test_served_rollout_is_the_fresh_moves_rollout(graphs, name):
    """rollout.ServedRollout (bench.py's step-server leg): block draws into the halves of a 2-episode move ring, 25 doorbells per
    episode, one server launch per enqueue -- the state and the last step's outputs equal RandomRollout(regenerate=True)'s
    launches.  With graphs=True the caller-side half of an episode is a HIP graph per ring half (its draw repeats the moves of
    episodes 0 / 1): compared over the first two episodes, then run on for the protocol's sake."""
    from multiagent_particle_envs_amd.rollout import ServedRollout
    B, EP = 4096, 25
    K = 2 * EP if graphs else 4 * EP
    ref_env = mpe.make_env(name, batch_size=B, seed=5)
    rr = RandomRollout(ref_env, episode_len=EP, pool=EP, regenerate=True)
    o = rr.enqueue(K)
    torch.cuda.synchronize()
    env = mpe.make_env(name, batch_size=B, seed=5)
    roll = ServedRollout(env, episode_len=EP, slots=2, graphs=graphs)
    roll.enqueue(K)
    torch.cuda.synchronize()
    roll.srv.check()
    assert torch.equal(env.world.pos, ref_env.world.pos) and torch.equal(env.world.vel, ref_env.world.vel)
    obs, rew, done = roll.srv.outputs(K - 1)
    for a, b in zip(obs, o.obs_n):
        assert torch.equal(a, b)
    assert torch.equal(rew, o.rew) and int(roll.srv.flag.min()) == K and int(roll.srv.door.item()) == K
    if graphs:
        roll.enqueue(6 * EP)
        torch.cuda.synchronize()
        roll.srv.check()
        assert int(roll.srv.flag.min()) == K + 6 * EP and bool(torch.isfinite(env.world.pos).all())


@pytest.mark.parametrize("name,kw,B", [("simple_spread", {}, 3000), ("simple_tag", {}, 4096), ("simple_spread", {}, 40000)])
def test_step_many_is_the_env_step_loop(name, kw, B):
    """rollout.step_many(env, moves[T]): the caller's `for t: env.step(moves[t])` loop as ONE launch on the caller's own stream (the
    doorbell rung T ahead, then the server launch: no second stream) -- bit-identical to the T env.step calls, twice in a row."""
    from multiagent_particle_envs_amd.rollout import step_many
    T = 9
    ref = mpe.make_env(name, batch_size=B, seed=11, **kw)
    env = mpe.make_env(name, batch_size=B, seed=11, **kw)
    ref.reset()
    env.world.set_state(*ref.world.get_state())
    A = ref.n
    g = torch.Generator(device="cpu").manual_seed(5)
    moves = torch.empty((T, A, B, _abi.MPE_ACTION_DIM), device="cuda")
    for rnd in range(2):
        moves.copy_(torch.nn.functional.one_hot(torch.randint(0, 5, (T, A, B), generator=g), 5).float())
        outs = step_many(env, moves)
        torch.cuda.synchronize()
        for t in range(T):
            obs_n, rew_n, done_n, _ = ref.step(moves[t])
            o_s, r_s, d_s = outs[t]
            for i in range(A):
                assert torch.equal(o_s[i], obs_n[i]), (rnd, t, i)
                assert torch.equal(r_s[i], rew_n[i]) and torch.equal(d_s[i], done_n[i])
        assert torch.equal(env.world.pos, ref.world.pos) and torch.equal(env.world.vel, ref.world.vel)


def test_launches_whose_commands_precede_them_need_no_residency():
    """`ahead`: every step of a launch is commanded before the launch starts (ring, then start, in stream order) -- nothing in it
    ever waits, so its 16 384 workgroups need not be resident: step_many and ServedRollout(launch_per_episode=True) at 1 048 576
    worlds, bit-identical to the launched steps."""
    from multiagent_particle_envs_amd.rollout import ServedRollout, step_many
    B, EP = 1 << 20, 5
    ref_env = mpe.make_env("simple_spread", batch_size=B, seed=5)
    rr = RandomRollout(ref_env, episode_len=EP, pool=EP, regenerate=True)
    o = rr.enqueue(3 * EP)
    torch.cuda.synchronize()
    env = mpe.make_env("simple_spread", batch_size=B, seed=5)
    roll = ServedRollout(env, episode_len=EP, slots=2, graphs=False, launch_per_episode=True)
    roll.enqueue(3 * EP)
    torch.cuda.synchronize()
    roll.srv.check()
    assert torch.equal(env.world.pos, ref_env.world.pos) and torch.equal(env.world.vel, ref_env.world.vel)
    obs, rew, done = roll.srv.outputs(3 * EP - 1)
    assert all(torch.equal(a, b) for a, b in zip(obs, o.obs_n)) and torch.equal(rew, o.rew)
    del roll, rr
    moves = torch.nn.functional.one_hot(torch.randint(0, 5, (3, 3, B)), 5).float().cuda()
    outs = step_many(env, moves)
    for t in range(3):
        obs_n, rew_n, _, _ = ref_env.step(moves[t])
        assert all(torch.equal(a, b) for a, b in zip(outs[t][0], obs_n)) and torch.equal(outs[t][1][0], rew_n[0])


@pytest.mark.parametrize("what", ["spread10", "spread40", "tag12", "corral", "convoy"])
def test_step_many_beyond_the_server(what):
    """env.step_many where the step server does not serve: simple_spread / simple_tag beyond 16 entities (the wave-per-world
    rollouts with the caller's moves: mpe_rollout_actions) and row-program envs -- a user scenario (examples/corral.py) and a
    traced reference-style file (tests/refstyle/convoy.py): mpe_rollout_rows_actions -- bit-identical to the env.step loop."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name, kw, B = {"spread10": ("simple_spread", {"num_agents": 10}, 3000), "spread40": ("simple_spread", {"num_agents": 40}, 700),
                   "tag12": ("simple_tag", {"num_good_agents": 4, "num_adversaries": 8, "num_landmarks": 3}, 1500),
                   "corral": (os.path.join(root, "examples", "corral.py"), {}, 4096),
                   "convoy": (os.path.join(root, "tests", "refstyle", "convoy.py"), {}, 2000)}[what]
    T = 7
    ref = mpe.make_env(name, batch_size=B, seed=11, **kw)
    env = mpe.make_env(name, batch_size=B, seed=11, **kw)
    ref.reset()
    env.reset()
    assert torch.equal(env.world.pos, ref.world.pos)
    A = ref.n
    g = torch.Generator(device="cpu").manual_seed(6)
    moves = torch.empty((T, A, B, _abi.MPE_ACTION_DIM), device="cuda")
    for rnd in range(2):
        moves.copy_(torch.nn.functional.one_hot(torch.randint(0, 5, (T, A, B), generator=g), 5).float())
        outs = env.step_many(moves)
        torch.cuda.synchronize()
        for t in range(T):
            obs_n, rew_n, done_n, _ = ref.step(moves[t])
            o_s, r_s, d_s = outs[t]
            for i in range(A):
                assert torch.equal(o_s[i], obs_n[i]), (rnd, t, i)
                assert torch.equal(r_s[i], rew_n[i]) and torch.equal(d_s[i], done_n[i])
        assert torch.equal(env.world.pos, ref.world.pos) and torch.equal(env.world.vel, ref.world.vel)


# ---- step_many keeps env.step's contract: constants, flags, seeds, streams (tests/test_gpu_server_oracle.py: against the reference)
PATHS = {"spread3": ("simple_spread", {}, 3000),                       # the step server
         "spread10": ("simple_spread", {"num_agents": 10}, 1500),      # mpe_rollout_actions
         "corral": ("corral", {}, 2048)}                                # a row program: mpe_rollout_rows_actions


def twin_envs(what, **kw):
    import os
    name, skw, B = PATHS[what]
    if name == "corral":
        name = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "corral.py")
    ref = mpe.make_env(name, batch_size=B, seed=11, **dict(skw, **kw))
    env = mpe.make_env(name, batch_size=B, seed=11, **dict(skw, **kw))
    ref.reset()
    env.reset()
    assert torch.equal(env.world.pos, ref.world.pos)
    return ref, env


def random_moves(moves, seed):
    T, A, B, _ = moves.shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    moves.copy_(torch.nn.functional.one_hot(torch.randint(0, 5, (T, A, B), generator=g), 5).float())
    return moves


def same_as_env_step(outs, ref, moves, what):
    torch.cuda.synchronize()
    for t in range(moves.shape[0]):
        obs_n, rew_n, done_n, _ = ref.step(moves[t])
        o_s, r_s, d_s = outs[t]
        for i in range(ref.n):
            assert torch.equal(o_s[i], obs_n[i]), (what, t, i)
            assert torch.equal(r_s[i], rew_n[i]) and torch.equal(d_s[i], done_n[i]), (what, t, i)


CONSTANTS = {"max_speed": lambda w: [setattr(a, "max_speed", 0.35) for a in w.agents],
             "size": lambda w: [setattr(e, "size", e.size * 1.8) for e in w.entities],
             "damping": lambda w: setattr(w, "damping", 0.6),
             "contact_margin": lambda w: setattr(w, "contact_margin", 0.02)}


@pytest.mark.parametrize("const", list(CONSTANTS))
@pytest.mark.parametrize("what", list(PATHS))
def test_step_many_rereads_constants_assigned_between_calls(what, const):
    """A constant assigned between two step_many calls with the SAME move tensor (a cached server / rollout state) is honoured
    as env.step honours it (the descriptor and the entity table re-read)."""
    ref, env = twin_envs(what)
    moves = torch.empty((6, ref.n, ref.batch_size, _abi.MPE_ACTION_DIM), device="cuda")
    same_as_env_step(env.step_many(random_moves(moves, 1)), ref, moves, "before")
    for e in (ref, env):
        CONSTANTS[const](e.world)
    same_as_env_step(env.step_many(random_moves(moves, 2)), ref, moves, "after " + const)
    assert torch.equal(env.world.pos, ref.world.pos) and torch.equal(env.world.vel, ref.world.vel)


@pytest.mark.parametrize("what", list(PATHS))
def test_step_many_refuses_noise_set_after_a_cached_call(what):
    ref, env = twin_envs(what)
    moves = random_moves(torch.empty((4, env.n, env.batch_size, _abi.MPE_ACTION_DIM), device="cuda"), 3)
    env.step_many(moves)
    env.world.agents[0].u_noise = 0.1          # env.step: the generic path, which draws the noise
    with pytest.raises(_abi.MpeError, match="fused"):
        env.step_many(moves)


FLAGS = {"force_discrete_action": lambda e: setattr(e, "force_discrete_action", True),
         "discrete_action_space": lambda e: setattr(e, "discrete_action_space", False),
         "discrete_action_input": lambda e: setattr(e, "discrete_action_input", True)}


@pytest.mark.parametrize("flag", list(FLAGS) + ["max_episode_steps", "max_episode_steps+auto_reset"])
@pytest.mark.parametrize("what", list(PATHS))
def test_step_many_refuses_what_env_step_does_differently(what, flag):
    """Each flag env.step honours and step_many does not is refused by name: set on a live env after a cached call, or (the
    episode horizon) given to make_env."""
    if flag.startswith("max_episode_steps"):
        _, env = twin_envs(what, max_episode_steps=10, auto_reset=flag.endswith("auto_reset"))
    else:
        _, env = twin_envs(what)
    moves = random_moves(torch.empty((4, env.n, env.batch_size, _abi.MPE_ACTION_DIM), device="cuda"), 4)
    if flag in FLAGS:
        env.step_many(moves)
        FLAGS[flag](env)
    with pytest.raises(_abi.MpeError, match=flag.split("+")[0]):
        env.step_many(moves)


@pytest.mark.parametrize("what", ["spread3", "spread10"])
def test_step_many_restarts_with_the_seed_it_is_given(what):
    """episode_len = T = 5: every call is one episode that starts with mpe_reset's draws of its seed, counted per seed -- seed 1
    (episode 0), seed 2 (episode 0), seed 1 again (episode 1).  The landmarks never move: their positions are the draws."""
    from oracle import philox
    _, env = twin_envs(what)
    w = env.world
    A, L, B = len(w.agents), len(w.landmarks), w.batch_size
    moves = random_moves(torch.empty((5, A, B, _abi.MPE_ACTION_DIM), device="cuda"), 5)
    for seed, episode in ((1, 0), (2, 0), (1, 1)):
        env.step_many(moves, episode_len=5, seed=seed)
        torch.cuda.synchronize()
        pos, _ = w.get_state()
        want = philox.reset_positions(seed, B, episode, A, L, float(env._scenario.landmark_range), int(w.world_offset))
        assert np.array_equal(pos[:, A:], want[:, A:]), (seed, episode)


@pytest.mark.parametrize("what", list(PATHS))
def test_step_many_on_another_stream(what):
    """A call under another torch.cuda.Stream than the cached server's first call: stepped there, the env.step loop's result."""
    ref, env = twin_envs(what)
    moves = torch.empty((5, ref.n, ref.batch_size, _abi.MPE_ACTION_DIM), device="cuda")
    same_as_env_step(env.step_many(random_moves(moves, 6)), ref, moves, "current stream")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        outs = env.step_many(random_moves(moves, 7))
    torch.cuda.current_stream().wait_stream(s)
    same_as_env_step(outs, ref, moves, "side stream")
    assert torch.equal(env.world.pos, ref.world.pos) and torch.equal(env.world.vel, ref.world.vel)


def test_refused_commands_change_no_count():
    """A refused ring() -- from a stream the server was not probed against, or beyond the launches -- and a refused run() leave
    `commanded` and `served_to` as they were; the server then serves on as commanded."""
    env = mpe.make_env("simple_spread", batch_size=512, seed=3)
    moves = torch.zeros((4, 3, 512, _abi.MPE_ACTION_DIM), device="cuda")
    srv = StepServer(env, moves, slots=4, timeout_s=5.0)
    srv.start(2)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with pytest.raises(_abi.MpeError, match="stream"):
            srv.ring()
    assert (srv.commanded, srv.served_to) == (0, 2)
    with pytest.raises(_abi.MpeError, match="start"):
        srv.ring(3)
    assert (srv.commanded, srv.served_to) == (0, 2)
    srv.ring(2)
    srv.join()
    torch.cuda.synchronize()
    srv.check()
    assert int(srv.flag.min()) == 2
    srv.commanded += 1          # (a count the commands cannot have reached: run()'s doorbell is refused)
    with pytest.raises(_abi.MpeError, match="start"):
        srv.run(2)
    assert (srv.commanded, srv.served_to) == (3, 2)
