"""The host ABI's refusals, pinned: return code, full text of mpe_last_error() and the ORDER of the checks of every
environment entry point of csrc/mpe_abi.hip (steps, phases, resets, rollouts, the policy rollout, the step server, row programs;
of the actor kernel's, mpe_actor_supported alone).

Each ladder starts from arguments that are wrong in every way its entry point checks and repairs one thing per call, so the
chain of checks is walked in order; after every call the return code and the whole message are compared with what is written
here.  The strings were recorded from the library as it stood before the entry points' shared rules were factored into
helpers, and the file has not been edited since: it holds for the library before and after.

No device is needed and none is touched: a library call that fails a check returns before anything reaches the HIP runtime,
and so does a call with B == 0 (or T == 0 where that returns first).  NO CALL HERE PASSES EVERY CHECK WITH B > 0 AND T > 0 --
that call would launch a kernel on the host addresses below.  Every rung is a refusal, or a return of 0 with B == 0 / T == 0
(which leaves mpe_last_error() as the refusal before it left it); run_ladder() enforces the second half before it calls.
The *_supported queries launch nothing whatever they answer."""
import ctypes as C
import types

import pytest

from multiagent_particle_envs_amd import _abi

# what a pointer field holds: the address of a small host array (the host checks never dereference it)
_HOST = (C.c_float * 16)()
PTR = C.addressof(_HOST)
BIG = 1 << 20      # a batch at which T * B * A passes MPE_POLICY_MAX_LAUNCH_WORK (mpe_rollout_policy's last refusal)


def _desc(kind, A, L, dim_c=2, nadv=0, collaborative=0, picks=()):
    d = _abi.MpeScenarioDesc()
    d.kind, d.n_agents, d.n_landmarks, d.dim_c, d.n_adversaries, d.collaborative = kind, A, L, dim_c, nadv, collaborative
    d.dt, d.damping, d.contact_force, d.contact_margin = 0.1, 0.25, 100.0, 1e-3
    for e in range(A + L):
        d.size[e], d.mass[e], d.accel[e], d.max_speed[e] = (0.15 if e < A else 0.05), 1.0, 5.0, -1.0
        d.movable[e] = d.collide[e] = 1 if e < A else 0
    d.n_choices = len(picks)
    for k, n in enumerate(picks):
        d.choice_pop[k] = n
    if kind != _abi.MPE_SCN_GENERIC:
        assert _abi.lib().mpe_fill_obs_layout(C.byref(d)) > 0
    else:
        for i in range(A + 1):
            d.obs_off[i] = 4 * i
    return d


def spread(A=3, L=3):
    return _desc(_abi.MPE_SCN_SPREAD, A, L, collaborative=1)


def adversary(A=3, L=2, nadv=1):
    return _desc(_abi.MPE_SCN_ADVERSARY, A, L, nadv=nadv, picks=(L,))


def speaker_listener():
    return _desc(_abi.MPE_SCN_SPEAKER_LISTENER, 2, 3, dim_c=3, collaborative=1, picks=(3,))


def generic(A=2, L=2, movable_landmark=True, picks=()):
    """kind GENERIC (World.step only, or a row program's descriptor); its last landmark movable unless told otherwise"""
    d = _desc(_abi.MPE_SCN_GENERIC, A, L, picks=picks)
    d.movable[A + L - 1] = 1 if movable_landmark else 0
    return d


def buffers(*names):
    b = _abi.MpeBuffers()
    for n in names:
        setattr(b, n, PTR)
    return b


def server(*names, ring=0, slots=0):
    s = _abi.MpeStepServer()
    for n in names:
        setattr(s, n, PTR)
    s.ring, s.slots = ring, slots
    return s


def actors(d, n_layers=2, hidden=8, out=_abi.MPE_ACTION_DIM, mode=_abi.MPE_POLICY_GREEDY):
    """a valid actor per agent of d: obs width -> hidden -> 5, ReLU, offsets multiples of 16 floats"""
    p = _abi.MpePolicy()
    p.mode = mode
    for i in range(d.n_agents):
        p.n_layers[i] = n_layers
        p.width[i][0] = d.obs_off[i + 1] - d.obs_off[i]
        for l in range(1, n_layers):
            p.width[i][l] = hidden
        p.width[i][n_layers] = out
        p.offset[i] = 1024 * i
    return p


def fill(array, n, value):
    """array[0 .. n) = value (one repair for every agent at once)"""
    for i in range(n):
        array[i] = value


def fill2(array, n, col, value):
    for i in range(n):
        array[i][col] = value


HELPERS = dict(spread=spread, adversary=adversary, speaker_listener=speaker_listener, generic=generic, buffers=buffers, server=server,
               actors=actors, fill=fill, fill2=fill2, PTR=PTR, BIG=BIG, RowProgram=_abi.MpeRowProgram, ActorSet=_abi.MpeActorSet,
               **{k: getattr(_abi, k) for k in dir(_abi) if k.startswith(("MPE_SCN_", "MPE_POLICY_"))})


def _ref(x):
    return None if x is None else C.byref(x)


def _new_state():
    """Every argument of every entry point, at its WRONG value: pointers NULL, counts negative."""
    return types.SimpleNamespace(
        desc=None, bufs=None, prog=None, policy=None, srv=None, mask=None, act=None, ids=None, act_seq=None, act_out=None, obs_in_out=None,
        logp_out=None, episode_step=None, actor_set=None, B=-1, T=-1, episode_len=-1, max_episode_steps=-1, landmark_range=1.0, seed=1, step0=0,
        episode=0, world_offset=0, trajectory=0, speakers=0)


def _simple(name):
    return lambda L, s: getattr(L, name)(_ref(s.desc), _ref(s.bufs), s.B, None)


def _rows(name):
    return lambda L, s: getattr(L, name)(_ref(s.desc), _ref(s.bufs), _ref(s.prog), s.B, None)


def _rows_episode(name):
    return lambda L, s: getattr(L, name)(_ref(s.desc), _ref(s.bufs), _ref(s.prog), s.B, s.episode_step, s.max_episode_steps,
                                         s.landmark_range, s.seed, s.episode, s.world_offset, None)


CALLS = {name: _simple(name) for name in ("mpe_step", "mpe_step_thread", "mpe_observe", "mpe_world_step", "mpe_apply_action_force",
                                          "mpe_collision_force", "mpe_integrate_state")}
CALLS.update({name: _rows(name) for name in ("mpe_rows", "mpe_step_rows")})
CALLS.update({name: _rows_episode(name) for name in ("mpe_step_rows_episode", "mpe_episode_finish")})
CALLS.update({
    "mpe_reset": lambda L, s: L.mpe_reset(_ref(s.desc), _ref(s.bufs), s.B, s.mask, s.landmark_range, s.seed, s.episode, s.world_offset, None),
    "mpe_reset_rows": lambda L, s: L.mpe_reset_rows(_ref(s.desc), _ref(s.bufs), _ref(s.prog), s.B, s.mask, s.landmark_range, s.seed,
                                                    s.episode, s.world_offset, None),
    "mpe_reset_random_actions_block": lambda L, s: L.mpe_reset_random_actions_block(
        _ref(s.desc), _ref(s.bufs), s.B, s.landmark_range, s.episode, s.act, s.ids, s.seed, s.step0, s.T, s.world_offset, None),
    "mpe_rollout_random": lambda L, s: L.mpe_rollout_random(_ref(s.desc), _ref(s.bufs), s.B, s.T, s.episode_len, s.landmark_range, s.seed,
                                                            s.step0, s.world_offset, s.trajectory, None),
    "mpe_rollout_actions": lambda L, s: L.mpe_rollout_actions(_ref(s.desc), _ref(s.bufs), s.B, s.T, s.episode_len, s.landmark_range, s.seed,
                                                              s.step0, s.world_offset, s.trajectory, s.act_seq, None),
    "mpe_rollout_policy_supported": lambda L, s: L.mpe_rollout_policy_supported(_ref(s.desc), _ref(s.policy), s.B),
    "mpe_rollout_policy": lambda L, s: L.mpe_rollout_policy(_ref(s.desc), _ref(s.bufs), _ref(s.policy), s.B, s.T, s.episode_len,
                                                            s.landmark_range, s.seed, s.step0, s.world_offset, s.trajectory, s.act_out,
                                                            s.obs_in_out, s.logp_out, None),
    "mpe_step_server_supported": lambda L, s: L.mpe_step_server_supported(_ref(s.desc), s.B),
    "mpe_actor_supported": lambda L, s: L.mpe_actor_supported(_ref(s.actor_set), s.B),
    "mpe_step_server_start": lambda L, s: L.mpe_step_server_start(_ref(s.desc), _ref(s.bufs), s.B, s.T, s.episode_len, s.landmark_range,
                                                                  s.seed, s.step0, s.world_offset, _ref(s.srv), None),
    "mpe_rollout_rows": lambda L, s: L.mpe_rollout_rows(_ref(s.desc), _ref(s.bufs), _ref(s.prog), s.B, s.T, s.episode_len, s.landmark_range,
                                                        s.seed, s.step0, s.world_offset, s.trajectory, s.speakers, None),
    "mpe_rollout_rows_actions": lambda L, s: L.mpe_rollout_rows_actions(_ref(s.desc), _ref(s.bufs), _ref(s.prog), s.B, s.T, s.episode_len,
                                                                        s.landmark_range, s.seed, s.step0, s.world_offset, s.trajectory,
                                                                        s.act_seq, None),
    "mpe_rollout_rows_episode": lambda L, s: L.mpe_rollout_rows_episode(_ref(s.desc), _ref(s.bufs), _ref(s.prog), s.B, s.T, s.episode_step,
                                                                        s.max_episode_steps, s.landmark_range, s.seed, s.step0, s.episode,
                                                                        s.world_offset, s.trajectory, s.speakers, None),
})
QUERIES = ("mpe_rollout_policy_supported", "mpe_step_server_supported", "mpe_actor_supported")      # answer 0 / 1, launch nothing
HAS_T = ("mpe_rollout_random", "mpe_rollout_actions", "mpe_step_server_start", "mpe_rollout_rows", "mpe_rollout_rows_actions",
         "mpe_rollout_rows_episode")      # return 0 for T == 0 as they do for B == 0


def run_ladder(entry, start, rungs):
    """Walk one ladder.  `start` and every rung's repair are statements over the call's arguments (_new_state) and HELPERS."""
    L = _abi.lib()
    s = _new_state()
    exec(start, HELPERS, s.__dict__)
    last = None
    for n, (repair, rc_want, msg_want) in enumerate(rungs):
        exec(repair, HELPERS, s.__dict__)
        if entry not in QUERIES and rc_want == 0:      # the hard condition: a call that is let through does no work
            assert s.B == 0 or (entry in HAS_T and s.T == 0), (entry, n, repair)
        rc = CALLS[entry](L, s)
        msg = L.mpe_last_error().decode()
        assert (rc, msg) == (rc_want, msg_want), "%s, rung %d (%r)" % (entry, n, repair)
        if entry not in QUERIES and rc == 0:
            assert msg == last, "%s, rung %d: a call that returns 0 leaves the last error alone" % (entry, n)
        last = msg


# (entry point, what the ladder shows, the arguments it starts from, [(repair, return code, mpe_last_error()), ...])
LADDERS = [
    ('mpe_step', 'simple_spread: every check of the descriptor, then state, actions, obs, info',
     'd = spread(); d.n_agents = 0; d.kind = 99; d.movable[4] = 1; d.mass[1] = 0; d.dim_c = 3; d.n_choices = 5; b = '
     "buffers('act', 'ids', 'info_rew')",
     [
      ('', -1,
       'mpe_step: desc is NULL'),
      ('desc = d', -1,
       'mpe_step: need 1 <= A, 0 <= L, A+L <= 512 (got A=0 L=3)'),
      ('d.n_agents = 3', -1,
       'mpe_step: bad kind 99'),
      ('d.kind = MPE_SCN_SPREAD', -2,
       'mpe_step: a movable landmark (entity 4) is stepped by mpe_world_step (kind GENERIC) only'),
      ('d.movable[4] = 0', -1,
       'mpe_step: mass[1] must be > 0'),
      ('d.mass[1] = 1.0', -2,
       'mpe_step: built-in spread/tag kernels assume dim_c == 2 (got 3)'),
      ('d.dim_c = 2', -1,
       'mpe_step: bad n_choices 5'),
      ('d.n_choices = 1', -1,
       'mpe_step: choice_pop[0] must be >= 1'),
      ('d.n_choices = 0', -1,
       'mpe_step: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_step: B < 0'),
      ('B = 4', -1,
       'mpe_step: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_step: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_step: exactly one of bufs->act / bufs->ids / bufs->u must be set'),
      ('b.ids = None', -1,
       'mpe_step: bufs->obs is NULL'),
      ('b.obs = PTR', -1,
       'mpe_step: spread benchmark_data needs all four info_* buffers'),
      ('B = 0', -1,
       'mpe_step: spread benchmark_data needs all four info_* buffers'),
      ('b.info_collisions = b.info_min_dists = b.info_occupied = PTR', 0,
       'mpe_step: spread benchmark_data needs all four info_* buffers'),
     ]),
    ('mpe_step', 'simple_adversary: the team and goal rules of the descriptor, then choice',
     "d = adversary(); d.n_adversaries = 0; d.n_choices = 0; d.choice_pop[0] = 3; b = buffers('pos', 'vel', 'act', 'obs'); "
     'desc = d; bufs = b; B = 4',
     [
      ('', -1,
       'mpe_step: this scenario needs 1 <= n_adversaries < A'),
      ('d.n_adversaries = 1', -1,
       'mpe_step: adversary/push pick one goal among the landmarks (n_choices = 1, choice_pop[0] = L)'),
      ('d.n_choices = 1', -1,
       'mpe_step: adversary/push pick one goal among the landmarks (n_choices = 1, choice_pop[0] = L)'),
      ('d.choice_pop[0] = 2', -1,
       'mpe_step: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('B = 0', -1,
       'mpe_step: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('b.choice = PTR', 0,
       'mpe_step: bufs->choice (the per-world picks of reset_world) is NULL'),
     ]),
    ('mpe_step', 'simple_speaker_listener: the one shape it is built for, then choice, then comm',
     "d = speaker_listener(); d.n_landmarks = 2; b = buffers('pos', 'vel', 'act', 'obs'); desc = d; bufs = b; B = 4",
     [
      ('', -2,
       'mpe_step: kind 6 is built for A=2 L=3 dim_c=3 n_choices=1 (got A=2 L=2 dim_c=3 n_choices=1)'),
      ('d.n_landmarks = 3', -1,
       'mpe_step: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('b.choice = PTR', -1,
       'mpe_step: bufs->comm (communication action rows / current comm state) is NULL'),
      ('B = 0', -1,
       'mpe_step: bufs->comm (communication action rows / current comm state) is NULL'),
      ('b.comm = PTR', 0,
       'mpe_step: bufs->comm (communication action rows / current comm state) is NULL'),
     ]),
    ('mpe_step', 'kind GENERIC has no output stage; a built-in kind refuses a movable landmark',
     "d = generic(); b = buffers('pos', 'vel', 'act', 'obs'); desc = d; bufs = b; B = 4",
     [
      ('', -1,
       'mpe_step: kind GENERIC has no output stage'),
      ('d.kind = MPE_SCN_SPREAD', -2,
       'mpe_step: a movable landmark (entity 3) is stepped by mpe_world_step (kind GENERIC) only'),
      ('B = 0', -2,
       'mpe_step: a movable landmark (entity 3) is stepped by mpe_world_step (kind GENERIC) only'),
      ('d.movable[3] = 0', 0,
       'mpe_step: a movable landmark (entity 3) is stepped by mpe_world_step (kind GENERIC) only'),
     ]),
    ('mpe_step', 'past the wave-per-agent shapes simple_spread needs the entity table -- asked for after the B == 0 return',
     "d = spread(20, 3); b = buffers('pos', 'vel', 'act', 'obs'); desc = d; bufs = b; B = 4",
     [
      ('', -1,
       'mpe_step: bufs->entity_table (required by the wave-per-world kernel) is NULL'),
      ('B = 0', 0,
       'mpe_step: bufs->entity_table (required by the wave-per-world kernel) is NULL'),
     ]),
    ('mpe_step', 'no kernel for a shape -- said after the B == 0 return',
     "d = adversary(20, 19); b = buffers('pos', 'vel', 'act', 'obs', 'choice'); desc = d; bufs = b; B = 4",
     [
      ('', -2,
       'mpe_step: no kernel for kind=4 A=20 L=19 n_adv=1'),
      ('B = 0', 0,
       'mpe_step: no kernel for kind=4 A=20 L=19 n_adv=1'),
     ]),
    ('mpe_step_thread', 'simple_spread: descriptor, state, actions, obs, info',
     "d = spread(); d.n_agents = 0; b = buffers('act', 'u', 'info_rew')",
     [
      ('', -1,
       'mpe_step_thread: desc is NULL'),
      ('desc = d', -1,
       'mpe_step_thread: need 1 <= A, 0 <= L, A+L <= 512 (got A=0 L=3)'),
      ('d.n_agents = 3', -1,
       'mpe_step_thread: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_step_thread: B < 0'),
      ('B = 4', -1,
       'mpe_step_thread: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_step_thread: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_step_thread: exactly one of bufs->act / bufs->ids / bufs->u must be set'),
      ('b.u = None', -1,
       'mpe_step_thread: bufs->obs is NULL'),
      ('b.obs = PTR', -1,
       'mpe_step_thread: spread benchmark_data needs all four info_* buffers'),
      ('B = 0', -1,
       'mpe_step_thread: spread benchmark_data needs all four info_* buffers'),
      ('b.info_collisions = b.info_min_dists = b.info_occupied = PTR', 0,
       'mpe_step_thread: spread benchmark_data needs all four info_* buffers'),
     ]),
    ('mpe_observe', 'simple_spread: no action check',
     "d = spread(); d.n_agents = 0; b = buffers('info_rew')",
     [
      ('', -1,
       'mpe_observe: desc is NULL'),
      ('desc = d', -1,
       'mpe_observe: need 1 <= A, 0 <= L, A+L <= 512 (got A=0 L=3)'),
      ('d.n_agents = 3', -1,
       'mpe_observe: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_observe: B < 0'),
      ('B = 4', -1,
       'mpe_observe: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_observe: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_observe: bufs->obs is NULL'),
      ('b.obs = PTR', -1,
       'mpe_observe: spread benchmark_data needs all four info_* buffers'),
      ('B = 0', -1,
       'mpe_observe: spread benchmark_data needs all four info_* buffers'),
      ('b.info_collisions = b.info_min_dists = b.info_occupied = PTR', 0,
       'mpe_observe: spread benchmark_data needs all four info_* buffers'),
     ]),
    ('mpe_observe', 'simple_speaker_listener: choice, then comm',
     "d = speaker_listener(); b = buffers('pos', 'vel', 'obs'); desc = d; bufs = b; B = 4",
     [
      ('', -1,
       'mpe_observe: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('b.choice = PTR', -1,
       'mpe_observe: bufs->comm (communication action rows / current comm state) is NULL'),
      ('B = 0', -1,
       'mpe_observe: bufs->comm (communication action rows / current comm state) is NULL'),
      ('b.comm = PTR', 0,
       'mpe_observe: bufs->comm (communication action rows / current comm state) is NULL'),
     ]),
    ('mpe_observe', 'no kernel for a shape',
     "d = adversary(20, 19); b = buffers('pos', 'vel', 'obs', 'choice'); desc = d; bufs = b; B = 4",
     [
      ('', -2,
       'mpe_observe: no kernel for kind=4 A=20 L=19 n_adv=1'),
      ('B = 0', 0,
       'mpe_observe: no kernel for kind=4 A=20 L=19 n_adv=1'),
     ]),
    ('mpe_world_step', 'GENERIC with movable landmarks 2 and 3 of 2..4: their mass, then bufs->u for n_dyn = last movable + 1',
     'd = generic(2, 3, False); d.movable[2] = d.movable[3] = 1; d.mass[3] = 0; b = buffers()',
     [
      ('', -1,
       'mpe_world_step: desc is NULL'),
      ('desc = d', -1,
       'mpe_world_step: mass[3] must be > 0'),
      ('d.mass[3] = 1.0', -1,
       'mpe_world_step: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_world_step: B < 0'),
      ('B = 4', -1,
       'mpe_world_step: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_world_step: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_world_step: exactly one of bufs->act / bufs->ids / bufs->u must be set'),
      ('b.act = PTR', -1,
       'mpe_world_step: movable landmarks need bufs->u ([n_dyn][2][B], n_dyn = 4: zero rows for the landmarks)'),
      ('B = 0', 0,
       'mpe_world_step: movable landmarks need bufs->u ([n_dyn][2][B], n_dyn = 4: zero rows for the landmarks)'),
     ]),
    ('mpe_world_step', 'a built-in descriptor steps its world without obs',
     "d = spread(); b = buffers('pos', 'vel'); desc = d; bufs = b; B = 4",
     [
      ('', -1,
       'mpe_world_step: exactly one of bufs->act / bufs->ids / bufs->u must be set'),
      ('B = 0', -1,
       'mpe_world_step: exactly one of bufs->act / bufs->ids / bufs->u must be set'),
      ('b.ids = PTR', 0,
       'mpe_world_step: exactly one of bufs->act / bufs->ids / bufs->u must be set'),
     ]),
    ('mpe_apply_action_force', 'the phase calls: state, force, the action triple, then A + L <= 16',
     'd = spread(3, 14); b = buffers()',
     [
      ('', -1,
       'mpe_apply_action_force: desc is NULL'),
      ('desc = d', -1,
       'mpe_apply_action_force: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_apply_action_force: B < 0'),
      ('B = 4', -1,
       'mpe_apply_action_force: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_apply_action_force: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_apply_action_force: bufs->force is NULL'),
      ('b.force = PTR', -1,
       'mpe_apply_action_force: exactly one of bufs->act / bufs->ids / bufs->u must be set'),
      ('b.act = PTR', -2,
       'mpe_apply_action_force: phase-level entry points cover A+L <= 16'),
      ('B = 0', -2,
       'mpe_apply_action_force: phase-level entry points cover A+L <= 16'),
      ('d.n_landmarks = 3', 0,
       'mpe_apply_action_force: phase-level entry points cover A+L <= 16'),
     ]),
    ('mpe_collision_force', 'the phase calls: state, force, then A + L <= 16',
     'd = spread(3, 14); b = buffers()',
     [
      ('', -1,
       'mpe_collision_force: desc is NULL'),
      ('desc = d', -1,
       'mpe_collision_force: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_collision_force: B < 0'),
      ('B = 4', -1,
       'mpe_collision_force: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_collision_force: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_collision_force: bufs->force is NULL'),
      ('b.force = PTR', -2,
       'mpe_collision_force: phase-level entry points cover A+L <= 16'),
      ('B = 0', -2,
       'mpe_collision_force: phase-level entry points cover A+L <= 16'),
      ('d.n_landmarks = 3', 0,
       'mpe_collision_force: phase-level entry points cover A+L <= 16'),
     ]),
    ('mpe_integrate_state', 'the phase calls: state, force, then A + L <= 16',
     'd = spread(3, 14); b = buffers()',
     [
      ('', -1,
       'mpe_integrate_state: desc is NULL'),
      ('desc = d', -1,
       'mpe_integrate_state: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_integrate_state: B < 0'),
      ('B = 4', -1,
       'mpe_integrate_state: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_integrate_state: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_integrate_state: bufs->force is NULL'),
      ('b.force = PTR', -2,
       'mpe_integrate_state: phase-level entry points cover A+L <= 16'),
      ('B = 0', -2,
       'mpe_integrate_state: phase-level entry points cover A+L <= 16'),
      ('d.n_landmarks = 3', 0,
       'mpe_integrate_state: phase-level entry points cover A+L <= 16'),
     ]),
    ('mpe_reset', 'simple_adversary: descriptor, state, choice',
     'd = adversary(); d.n_landmarks = -1; b = buffers()',
     [
      ('', -1,
       'mpe_reset: desc is NULL'),
      ('desc = d', -1,
       'mpe_reset: need 1 <= A, 0 <= L, A+L <= 512 (got A=3 L=-1)'),
      ('d.n_landmarks = 2', -1,
       'mpe_reset: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_reset: B < 0'),
      ('B = 4', -1,
       'mpe_reset: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_reset: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_reset: desc->n_choices = 1 but bufs->choice is NULL'),
      ('B = 0', -1,
       'mpe_reset: desc->n_choices = 1 but bufs->choice is NULL'),
      ('b.choice = PTR', 0,
       'mpe_reset: desc->n_choices = 1 but bufs->choice is NULL'),
     ]),
    ('mpe_reset_rows', 'prog first; without boxes it IS mpe_reset; with boxes: descriptor, state, 64 entities, choice',
     'd = generic(3, 70, False, picks=(2,)); b = buffers(); p = RowProgram()',
     [
      ('', -1,
       'mpe_reset_rows: prog is NULL'),
      ('prog = p', -1,
       'mpe_reset: desc is NULL'),
      ('p.reset_boxes = 1', -1,
       'mpe_reset_rows: desc is NULL'),
      ('desc = d', -1,
       'mpe_reset_rows: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_reset_rows: B < 0'),
      ('B = 4', -1,
       'mpe_reset_rows: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_reset_rows: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_reset_rows: more than 64 entities'),
      ('d.n_landmarks = 2', -1,
       'mpe_reset_rows: desc->n_choices = 1 but bufs->choice is NULL'),
      ('B = 0', -1,
       'mpe_reset_rows: desc->n_choices = 1 but bufs->choice is NULL'),
      ('b.choice = PTR', 0,
       'mpe_reset_rows: desc->n_choices = 1 but bufs->choice is NULL'),
     ]),
    ('mpe_reset_random_actions_block', 'descriptor, state, choice, act / ids, T',
     'd = adversary(); b = buffers()',
     [
      ('', -1,
       'mpe_reset_random_actions_block: desc is NULL'),
      ('desc = d', -1,
       'mpe_reset_random_actions_block: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_reset_random_actions_block: B < 0'),
      ('B = 4', -1,
       'mpe_reset_random_actions_block: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_reset_random_actions_block: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_reset_random_actions_block: desc->n_choices = 1 but bufs->choice is NULL'),
      ('b.choice = PTR', -1,
       'mpe_reset_random_actions_block: act and ids are both NULL'),
      ('ids = PTR', -1,
       "mpe_reset_random_actions_block: T = -1 (the reset rides on the block's first step: 1..65535)"),
      ('T = 0', -1,
       "mpe_reset_random_actions_block: T = 0 (the reset rides on the block's first step: 1..65535)"),
      ('T = 65536', -1,
       "mpe_reset_random_actions_block: T = 65536 (the reset rides on the block's first step: 1..65535)"),
      ('B = 0', -1,
       "mpe_reset_random_actions_block: T = 65536 (the reset rides on the block's first step: 1..65535)"),
      ('T = 65535', 0,
       "mpe_reset_random_actions_block: T = 65536 (the reset rides on the block's first step: 1..65535)"),
     ]),
    ('mpe_rollout_random', 'simple_spread: descriptor, state, obs, info, T / episode_len',
     "d = spread(); d.n_agents = 0; b = buffers('info_rew')",
     [
      ('', -1,
       'mpe_rollout_random: desc is NULL'),
      ('desc = d', -1,
       'mpe_rollout_random: need 1 <= A, 0 <= L, A+L <= 512 (got A=0 L=3)'),
      ('d.n_agents = 3', -1,
       'mpe_rollout_random: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_rollout_random: B < 0'),
      ('B = 4', -1,
       'mpe_rollout_random: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_rollout_random: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_rollout_random: bufs->obs is NULL'),
      ('b.obs = PTR', -1,
       'mpe_rollout_random: spread benchmark_data needs all four info_* buffers'),
      ('b.info_collisions = b.info_min_dists = b.info_occupied = PTR', -1,
       'mpe_rollout_random: T, episode_len must be >= 0'),
      ('T = 5', -1,
       'mpe_rollout_random: T, episode_len must be >= 0'),
      ('B = 0', -1,
       'mpe_rollout_random: T, episode_len must be >= 0'),
      ('episode_len = 0', 0,
       'mpe_rollout_random: T, episode_len must be >= 0'),
     ]),
    ('mpe_rollout_random', 'choice; T == 0 and B == 0 return 0 BEFORE the no-kernel-for-this-shape refusal',
     "d = adversary(20, 19); b = buffers('pos', 'vel', 'obs'); desc = d; bufs = b; B = 4; T = 5; episode_len = 0",
     [
      ('', -1,
       'mpe_rollout_random: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('b.choice = PTR', -2,
       'mpe_rollout_random: the fused rollout exists for the wave-per-agent shapes and for simple_spread / simple_tag of any size'),
      ('T = 0', 0,
       'mpe_rollout_random: the fused rollout exists for the wave-per-agent shapes and for simple_spread / simple_tag of any size'),
      ('T = 5', -2,
       'mpe_rollout_random: the fused rollout exists for the wave-per-agent shapes and for simple_spread / simple_tag of any size'),
      ('B = 0', 0,
       'mpe_rollout_random: the fused rollout exists for the wave-per-agent shapes and for simple_spread / simple_tag of any size'),
     ]),
    ('mpe_rollout_random', 'simple_speaker_listener: choice, then comm (its own words for it)',
     "d = speaker_listener(); b = buffers('pos', 'vel', 'obs'); desc = d; bufs = b; B = 4; T = 5; episode_len = 0",
     [
      ('', -1,
       'mpe_rollout_random: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('b.choice = PTR', -1,
       "mpe_rollout_random: bufs->comm (receives the agents' comm state after the last step) is NULL"),
      ('B = 0', -1,
       "mpe_rollout_random: bufs->comm (receives the agents' comm state after the last step) is NULL"),
      ('b.comm = PTR', 0,
       "mpe_rollout_random: bufs->comm (receives the agents' comm state after the last step) is NULL"),
     ]),
    ('mpe_rollout_random', 'past the wave-per-agent shapes simple_spread needs the entity table',
     "d = spread(20, 3); b = buffers('pos', 'vel', 'obs'); desc = d; bufs = b; B = 4; T = 5; episode_len = 0",
     [
      ('', -1,
       'mpe_rollout_random: bufs->entity_table (required by the wave-per-world kernel) is NULL'),
      ('T = 0', 0,
       'mpe_rollout_random: bufs->entity_table (required by the wave-per-world kernel) is NULL'),
     ]),
    ('mpe_rollout_actions', "act_seq first; a wave-per-agent shape is refused after the B == 0 return (the step server's job)",
     'd = spread(); b = buffers(); B = 4',
     [
      ('', -1,
       'mpe_rollout_actions: act_seq is NULL'),
      ('act_seq = PTR', -1,
       'mpe_rollout_actions: desc is NULL'),
      ('desc = d', -1,
       'mpe_rollout_actions: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_rollout_actions: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_rollout_actions: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_rollout_actions: bufs->obs is NULL'),
      ('b.obs = PTR', -1,
       'mpe_rollout_actions: T, episode_len must be >= 0'),
      ('T = 5', -1,
       'mpe_rollout_actions: T, episode_len must be >= 0'),
      ('episode_len = 0', -2,
       "mpe_rollout_actions: this shape has a wave-per-agent kernel -- its T-step launch with the caller's moves is the step server's (mpe_step_server_ring, then mpe_step_server_start with srv->ahead = 1)"),
      ('B = 0', 0,
       "mpe_rollout_actions: this shape has a wave-per-agent kernel -- its T-step launch with the caller's moves is the step server's (mpe_step_server_ring, then mpe_step_server_start with srv->ahead = 1)"),
     ]),
    ('mpe_rollout_actions', 'no kernel for a shape',
     "d = adversary(20, 19); b = buffers('pos', 'vel', 'obs', 'choice'); desc = d; bufs = b; B = 4; T = 5; episode_len = 0; "
     'act_seq = PTR',
     [
      ('', -2,
       'mpe_rollout_actions: the fused rollout exists for the wave-per-agent shapes and for simple_spread / simple_tag of any size'),
      ('T = 0', 0,
       'mpe_rollout_actions: the fused rollout exists for the wave-per-agent shapes and for simple_spread / simple_tag of any size'),
     ]),
    ('mpe_rollout_policy_supported', 'EINVAL passes through, EUNSUPPORTED becomes 0 (and leaves its message), then the shape answer',
     'd = spread(17, 3); pol = actors(spread()); pol.mode = 7; fill(pol.n_layers, 3, 0); fill2(pol.width, 3, 0, 1); '
     'fill2(pol.width, 3, 1, 65); fill2(pol.width, 3, 2, 4); fill(pol.activation, 3, 9); fill(pol.offset, 3, 8)',
     [
      ('', -1,
       'mpe_rollout_policy_supported: desc is NULL'),
      ('desc = d', -1,
       'mpe_rollout_policy_supported: policy is NULL'),
      ('policy = pol', -1,
       'mpe_rollout_policy_supported: bad policy mode 7'),
      ('pol.mode = MPE_POLICY_SAMPLE', 0,
       'mpe_rollout_policy_supported: more than 16 agents'),
      ('d = spread(); desc = d', -1,
       'mpe_rollout_policy_supported: agent 0: 0 Linear layers (1..3)'),
      ('fill(pol.n_layers, 3, 2)', -1,
       'mpe_rollout_policy_supported: agent 0: actor input width 1, observation width 18'),
      ('fill2(pol.width, 3, 0, 18)', -1,
       'mpe_rollout_policy_supported: agent 0: hidden width 65 (1..64)'),
      ('fill2(pol.width, 3, 1, 8)', -1,
       'mpe_rollout_policy_supported: agent 0: actor output width 4 (need 5)'),
      ('fill2(pol.width, 3, 2, 5)', -1,
       'mpe_rollout_policy_supported: agent 0: bad activation 9'),
      ('fill(pol.activation, 3, MPE_POLICY_TANH)', -1,
       'mpe_rollout_policy_supported: agent 0: offset 8 (a multiple of 16 floats)'),
      ('fill(pol.offset, 3, 0)', 0,
       'mpe_rollout_policy_supported: agent 0: offset 8 (a multiple of 16 floats)'),
      ('B = 4', 1,
       'mpe_rollout_policy_supported: agent 0: offset 8 (a multiple of 16 floats)'),
      ('d.n_landmarks = 4', 0,
       'mpe_rollout_policy_supported: agent 0: offset 8 (a multiple of 16 floats)'),
      ('d.n_landmarks = 3', 1,
       'mpe_rollout_policy_supported: agent 0: offset 8 (a multiple of 16 floats)'),
      ('B = 0', 0,
       'mpe_rollout_policy_supported: agent 0: offset 8 (a multiple of 16 floats)'),
     ]),
    ('mpe_rollout_policy', 'simple_adversary: the policy is checked before choice; weights, act_out, logp_out, T; the work bound after B == 0',
     'd = adversary(); b = buffers(); pol = actors(d, mode=MPE_POLICY_SOFTMAX); fill(pol.n_layers, 3, 0); logp_out = PTR',
     [
      ('', -1,
       'mpe_rollout_policy: desc is NULL'),
      ('desc = d', -1,
       'mpe_rollout_policy: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_rollout_policy: B < 0'),
      ('B = BIG', -1,
       'mpe_rollout_policy: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_rollout_policy: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_rollout_policy: bufs->obs is NULL'),
      ('b.obs = PTR', -1,
       'mpe_rollout_policy: policy is NULL'),
      ('policy = pol', -1,
       'mpe_rollout_policy: agent 0: 0 Linear layers (1..3)'),
      ('fill(pol.n_layers, 3, 2)', -1,
       'mpe_rollout_policy: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('b.choice = PTR', -1,
       'mpe_rollout_policy: policy->weights is NULL'),
      ('pol.weights = PTR', -1,
       'mpe_rollout_policy: act_out is NULL'),
      ('act_out = PTR', -1,
       'mpe_rollout_policy: logp_out needs a chosen index (GREEDY / SAMPLE)'),
      ('logp_out = None', -1,
       'mpe_rollout_policy: 1 <= T <= 65535 and episode_len >= 0 (got T=-1)'),
      ('T = 65535', -1,
       'mpe_rollout_policy: 1 <= T <= 65535 and episode_len >= 0 (got T=65535)'),
      ('episode_len = 0', -1,
       'mpe_rollout_policy: T * B * A = 206155284480 agent-world-steps in one launch (at most 33554432: split the rollout into launches with step0 advanced)'),
      ('B = 0', 0,
       'mpe_rollout_policy: T * B * A = 206155284480 agent-world-steps in one launch (at most 33554432: split the rollout into launches with step0 advanced)'),
     ]),
    ('mpe_rollout_policy', 'simple_spread: info before the policy; the shape is refused BEFORE the B == 0 return',
     "d = spread(); d.n_landmarks = 4; b = buffers('pos', 'vel', 'obs', 'info_rew'); pol = actors(d); pol.weights = PTR; "
     'act_out = PTR; T = 1; episode_len = 0; B = 0; desc = d; bufs = b',
     [
      ('', -1,
       'mpe_rollout_policy: spread benchmark_data needs all four info_* buffers'),
      ('b.info_collisions = b.info_min_dists = b.info_occupied = PTR', -1,
       'mpe_rollout_policy: policy is NULL'),
      ('policy = pol', -2,
       'mpe_rollout_policy: policy rollouts exist for simple, simple_spread with up to 3 agents, simple_adversary (3 agents, 1 adversary) and simple_push (kind=2 A=3 L=4 n_adv=0)'),
      ('d.n_landmarks = 3', 0,
       'mpe_rollout_policy: policy rollouts exist for simple, simple_spread with up to 3 agents, simple_adversary (3 agents, 1 adversary) and simple_push (kind=2 A=3 L=4 n_adv=0)'),
     ]),
    ('mpe_actor_supported', 'as mpe_rollout_policy_supported: EINVAL passes through, EUNSUPPORTED becomes 0 (and leaves its message)',
     'a = ActorSet(); a.n_agents = 17; a.mode = 7',
     [
      ('', -1,
       'mpe_actor_supported: set is NULL'),
      ('actor_set = a', 0,
       'mpe_actor_supported: 17 agents in one actor set (at most MPE_ACTOR_MAX_AGENTS = 16: split the agents over several sets)'),
      ('a.n_agents = 1', -1,
       'mpe_actor_supported: mode 7 (MPE_POLICY_GREEDY / SAMPLE / SOFTMAX)'),
      ('a.mode = MPE_POLICY_GREEDY', -1,
       'mpe_actor_supported: agent 0 has 0 Linear layers (1..3)'),
      ('a.n_layers[0] = 1', -1,
       'mpe_actor_supported: agent 0: input width 0'),
      ('a.width[0][0] = 300', 0,
       'mpe_actor_supported: agent 0: input width 300 > MPE_ACTOR_MAX_INPUT = 256'),
      ('a.width[0][0] = 8', -1,
       'mpe_actor_supported: agent 0 neither moves nor speaks: it has no head'),
      ('a.movable[0] = 1', -1,
       'mpe_actor_supported: agent 0: the last layer gives 0 outputs, its heads need 5 (5 * movable + dim_c * speaks)'),
      ('a.width[0][1] = 5', 0,
       'mpe_actor_supported: agent 0: the last layer gives 0 outputs, its heads need 5 (5 * movable + dim_c * speaks)'),
      ('B = 4', 1,
       'mpe_actor_supported: agent 0: the last layer gives 0 outputs, its heads need 5 (5 * movable + dim_c * speaks)'),
     ]),
    ('mpe_step_server_supported', "the descriptor's refusals pass through; the answer is 0 for B <= 0 and for shapes without a server",
     'd = spread(); d.n_agents = 0',
     [
      ('', -1,
       'mpe_step_server_supported: desc is NULL'),
      ('desc = d', -1,
       'mpe_step_server_supported: need 1 <= A, 0 <= L, A+L <= 512 (got A=0 L=3)'),
      ('d.n_agents = 3', 0,
       'mpe_step_server_supported: need 1 <= A, 0 <= L, A+L <= 512 (got A=0 L=3)'),
      ('B = 4', 1,
       'mpe_step_server_supported: need 1 <= A, 0 <= L, A+L <= 512 (got A=0 L=3)'),
      ('d = spread(20, 3); desc = d', 0,
       'mpe_step_server_supported: need 1 <= A, 0 <= L, A+L <= 512 (got A=0 L=3)'),
      ('d = adversary(20, 19); desc = d', 0,
       'mpe_step_server_supported: need 1 <= A, 0 <= L, A+L <= 512 (got A=0 L=3)'),
     ]),
    ('mpe_step_server_start', 'simple_spread: descriptor, state, obs, info, then srv, its ring, T / episode_len',
     "d = spread(); b = buffers('info_rew'); sv = server('door', 'flag')",
     [
      ('', -1,
       'mpe_step_server_start: desc is NULL'),
      ('desc = d', -1,
       'mpe_step_server_start: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_step_server_start: B < 0'),
      ('B = 4', -1,
       'mpe_step_server_start: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_step_server_start: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_step_server_start: bufs->obs is NULL'),
      ('b.obs = PTR', -1,
       'mpe_step_server_start: spread benchmark_data needs all four info_* buffers'),
      ('b.info_collisions = b.info_min_dists = b.info_occupied = PTR', -1,
       'mpe_step_server_start: srv is NULL'),
      ('srv = sv', -1,
       'mpe_step_server_start: srv->door / flag / status must be device words'),
      ('sv.status = PTR', -1,
       'mpe_step_server_start: srv->act_ring, ring >= 1, slots >= 1'),
      ('sv.act_ring = PTR', -1,
       'mpe_step_server_start: srv->act_ring, ring >= 1, slots >= 1'),
      ('sv.ring = 2', -1,
       'mpe_step_server_start: srv->act_ring, ring >= 1, slots >= 1'),
      ('sv.slots = 1', -1,
       'mpe_step_server_start: T, episode_len must be >= 0'),
      ('T = 5', -1,
       'mpe_step_server_start: T, episode_len must be >= 0'),
      ('B = 0', -1,
       'mpe_step_server_start: T, episode_len must be >= 0'),
      ('episode_len = 0', 0,
       'mpe_step_server_start: T, episode_len must be >= 0'),
     ]),
    ('mpe_step_server_start', 'simple_adversary: srv is checked before choice',
     "d = adversary(); b = buffers('pos', 'vel', 'obs'); desc = d; bufs = b; B = 4; episode_len = 0",
     [
      ('', -1,
       'mpe_step_server_start: srv is NULL'),
      ("srv = server('door', 'flag', 'status', 'act_ring', ring=2, slots=1)", -1,
       'mpe_step_server_start: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('b.choice = PTR', -1,
       'mpe_step_server_start: T, episode_len must be >= 0'),
      ('B = 0', -1,
       'mpe_step_server_start: T, episode_len must be >= 0'),
      ('T = 5', 0,
       'mpe_step_server_start: T, episode_len must be >= 0'),
     ]),
    ('mpe_step_server_start', 'B == 0 and T == 0 return 0 BEFORE the no-server-for-this-shape refusal',
     "d = spread(20, 3); b = buffers('pos', 'vel', 'obs'); srv = server('door', 'flag', 'status', 'act_ring', ring=2, "
     'slots=1); desc = d; bufs = b; B = 4; T = 5; episode_len = 0',
     [
      ('', -2,
       'mpe_step_server_start: the step server exists for the shapes with a wave-per-agent kernel'),
      ('B = 0', 0,
       'mpe_step_server_start: the step server exists for the shapes with a wave-per-agent kernel'),
      ('B = 4', -2,
       'mpe_step_server_start: the step server exists for the shapes with a wave-per-agent kernel'),
      ('T = 0', 0,
       'mpe_step_server_start: the step server exists for the shapes with a wave-per-agent kernel'),
     ]),
    ('mpe_step_server_start', 'simple_speaker_listener: bufs->comm is not asked for, srv->comm_ring is -- after the B == 0 return',
     "d = speaker_listener(); b = buffers('pos', 'vel', 'obs', 'choice'); srv = server('door', 'flag', 'status', 'act_ring', "
     'ring=2, slots=1); desc = d; bufs = b; B = 4; T = 5; episode_len = 0',
     [
      ('', -1,
       'mpe_step_server_start: srv->comm_ring (the utterance tensors of the communication scenarios) is NULL'),
      ('T = 0', 0,
       'mpe_step_server_start: srv->comm_ring (the utterance tensors of the communication scenarios) is NULL'),
     ]),
    ('mpe_rows', "every check of the program's header, then header_device, state, obs, choice (asked of ANY kind with picks)",
     'd = generic(70, 2, False, picks=(2,)); d.obs_off[2] = 1; p = RowProgram(); p.n_ops = 2; p.n_vel = -1; p.n_regions = 3; '
     'p.region_entity[0] = 99; p.obs_begin[1] = 5; p.rew_begin[0] = 1; p.done_begin[2] = 9; p.n_shared = 1; b = buffers()',
     [
      ('', -1,
       'mpe_rows: desc is NULL'),
      ('desc = d', -1,
       'mpe_rows: prog is NULL'),
      ('prog = p', -2,
       'mpe_rows: row programs cover A + L <= 64 (got 72)'),
      ('d.n_agents = 3', -1,
       'mpe_rows: prog->ops_device is NULL'),
      ('p.ops_device = PTR', -1,
       'mpe_rows: prog->n_vel = -1, need 0 .. A + L'),
      ('p.n_vel = 3', -1,
       'mpe_rows: prog->n_regions = 3, need 0 .. 2'),
      ('p.n_regions = 1', -1,
       'mpe_rows: region 0 names entity 99'),
      ('p.region_entity[0] = 4', -1,
       'mpe_rows: obs_begin[1] = 5 out of order / range'),
      ('p.obs_begin[1] = 0', -1,
       'mpe_rows: rew_begin[1] = 0 out of order / range'),
      ('p.rew_begin[0] = 0', -1,
       'mpe_rows: done_begin[2] = 9 out of order / range'),
      ('p.done_begin[2] = 0', -1,
       'mpe_rows: desc->obs_off is not a prefix sum'),
      ('d.obs_off[2] = 8', -1,
       'mpe_rows: prog->n_shared = 1 (0..64, traced programs only)'),
      ('p.n_shared = 0', -1,
       'mpe_rows: prog->header_device is NULL (MPE_ROWS_HEADER_BYTES of device memory)'),
      ('p.header_device = PTR', -1,
       'mpe_rows: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_rows: B < 0'),
      ('B = 4', -1,
       'mpe_rows: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_rows: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_rows: bufs->obs is NULL'),
      ('b.obs = PTR', -1,
       'mpe_rows: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('B = 0', -1,
       'mpe_rows: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('b.choice = PTR', 0,
       'mpe_rows: bufs->choice (the per-world picks of reset_world) is NULL'),
     ]),
    ('mpe_rows', 'a traced program without its image is refused after the B == 0 return',
     "d = generic(2, 2, False); p = RowProgram(); p.header_device = PTR; p.traced = 1; b = buffers('pos', 'vel', 'obs'); "
     'desc = d; bufs = b; prog = p; B = 4',
     [
      ('', -2,
       'mpe_rows: a traced program runs compiled in only -- no image is attached, or the descriptor is not the one it was compiled for (mpe_rows_static_source + the traced source -> hipcc --genco -> mpe_rows_load_image)'),
      ('B = 0', 0,
       'mpe_rows: a traced program runs compiled in only -- no image is attached, or the descriptor is not the one it was compiled for (mpe_rows_static_source + the traced source -> hipcc --genco -> mpe_rows_load_image)'),
     ]),
    ('mpe_step_rows', 'a zeroed program passes the header: header_device, state, obs, choice, actions, the movable landmark',
     'd = generic(2, 2, picks=(2,)); p = RowProgram(); b = buffers()',
     [
      ('', -1,
       'mpe_step_rows: desc is NULL'),
      ('desc = d', -1,
       'mpe_step_rows: prog is NULL'),
      ('prog = p', -1,
       'mpe_step_rows: prog->header_device is NULL (MPE_ROWS_HEADER_BYTES of device memory)'),
      ('p.header_device = PTR', -1,
       'mpe_step_rows: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_step_rows: B < 0'),
      ('B = 4', -1,
       'mpe_step_rows: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_step_rows: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_step_rows: bufs->obs is NULL'),
      ('b.obs = PTR', -1,
       'mpe_step_rows: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('b.choice = PTR', -1,
       'mpe_step_rows: exactly one of bufs->act / bufs->ids / bufs->u must be set'),
      ('b.u = PTR', -2,
       'mpe_step_rows: a movable landmark (entity 3) is stepped by mpe_world_step only'),
      ('B = 0', -2,
       'mpe_step_rows: a movable landmark (entity 3) is stepped by mpe_world_step only'),
      ('d.movable[3] = 0', 0,
       'mpe_step_rows: a movable landmark (entity 3) is stepped by mpe_world_step only'),
     ]),
    ('mpe_step_rows', 'a traced program without its image',
     "d = generic(2, 2, False); p = RowProgram(); p.header_device = PTR; p.traced = 1; b = buffers('pos', 'vel', 'obs', "
     "'act'); desc = d; bufs = b; prog = p; B = 4",
     [
      ('', -2,
       'mpe_step_rows: a traced program runs compiled in only -- no image is attached, or the descriptor is not the one it was compiled for (mpe_rows_static_source + the traced source -> hipcc --genco -> mpe_rows_load_image)'),
      ('B = 0', 0,
       'mpe_step_rows: a traced program runs compiled in only -- no image is attached, or the descriptor is not the one it was compiled for (mpe_rows_static_source + the traced source -> hipcc --genco -> mpe_rows_load_image)'),
     ]),
    ('mpe_rollout_rows', 'T / episode_len BEFORE desc; the speakers mask; T == 0 returns 0 with a NULL program and an unchecked descriptor; then the row call without an action check',
     'd = generic(3, 2, picks=(2,)); d.dim_c = 0; d.mass[0] = 0; p = RowProgram(); b = buffers(); speakers = 0xff',
     [
      ('', -1,
       'mpe_rollout_rows: T, episode_len must be >= 0'),
      ('T = 0', -1,
       'mpe_rollout_rows: T, episode_len must be >= 0'),
      ('episode_len = 0', -1,
       'mpe_rollout_rows: desc is NULL'),
      ('desc = d', -1,
       'mpe_rollout_rows: speakers 0xff but desc->dim_c = 0'),
      ('d.dim_c = 2', -1,
       'mpe_rollout_rows: speakers 0xff names agents beyond 3'),
      ('speakers = 0x5', -1,
       "mpe_rollout_rows: bufs->comm (receives the speaking agents' last words) is NULL"),
      ('bufs = b', -1,
       "mpe_rollout_rows: bufs->comm (receives the speaking agents' last words) is NULL"),
      ('b.comm = PTR', 0,
       "mpe_rollout_rows: bufs->comm (receives the speaking agents' last words) is NULL"),
      ('T = 5', -1,
       'mpe_rollout_rows: mass[0] must be > 0'),
      ('d.mass[0] = 1.0', -1,
       'mpe_rollout_rows: prog is NULL'),
      ('prog = p', -1,
       'mpe_rollout_rows: prog->header_device is NULL (MPE_ROWS_HEADER_BYTES of device memory)'),
      ('p.header_device = PTR', -1,
       'mpe_rollout_rows: B < 0'),
      ('B = 4', -1,
       'mpe_rollout_rows: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_rollout_rows: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_rollout_rows: bufs->obs is NULL'),
      ('b.obs = PTR', -1,
       'mpe_rollout_rows: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('b.choice = PTR', -2,
       'mpe_rollout_rows: a movable landmark (entity 4) is stepped by mpe_world_step only'),
      ('B = 0', -2,
       'mpe_rollout_rows: a movable landmark (entity 4) is stepped by mpe_world_step only'),
      ('d.movable[4] = 0', 0,
       'mpe_rollout_rows: a movable landmark (entity 4) is stepped by mpe_world_step only'),
     ]),
    ('mpe_rollout_rows_actions', 'act_seq first, then as mpe_rollout_rows without speakers',
     'd = generic(3, 2); p = RowProgram(); b = buffers()',
     [
      ('', -1,
       'mpe_rollout_rows_actions: act_seq is NULL'),
      ('act_seq = PTR', -1,
       'mpe_rollout_rows_actions: T, episode_len must be >= 0'),
      ('T = 5', -1,
       'mpe_rollout_rows_actions: T, episode_len must be >= 0'),
      ('episode_len = 0', -1,
       'mpe_rollout_rows_actions: desc is NULL'),
      ('desc = d', -1,
       'mpe_rollout_rows_actions: prog is NULL'),
      ('prog = p', -1,
       'mpe_rollout_rows_actions: prog->header_device is NULL (MPE_ROWS_HEADER_BYTES of device memory)'),
      ('p.header_device = PTR', -1,
       'mpe_rollout_rows_actions: bufs is NULL'),
      ('bufs = b', -1,
       'mpe_rollout_rows_actions: B < 0'),
      ('B = 4', -1,
       'mpe_rollout_rows_actions: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_rollout_rows_actions: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_rollout_rows_actions: bufs->obs is NULL'),
      ('b.obs = PTR', -2,
       'mpe_rollout_rows_actions: a movable landmark (entity 4) is stepped by mpe_world_step only'),
      ('B = 0', -2,
       'mpe_rollout_rows_actions: a movable landmark (entity 4) is stepped by mpe_world_step only'),
      ('d.movable[4] = 0', 0,
       'mpe_rollout_rows_actions: a movable landmark (entity 4) is stepped by mpe_world_step only'),
     ]),
    ('mpe_rollout_rows_episode', 'T, the episode arguments, desc; a speakers mask naming agents beyond A is NOT refused here; T == 0 returns 0; then the row call',
     'd = generic(3, 2, picks=(2,)); d.dim_c = 0; d.mass[0] = 0; p = RowProgram(); b = buffers(); speakers = 0xff',
     [
      ('', -1,
       'mpe_rollout_rows_episode: T must be >= 0'),
      ('T = 0', -1,
       'mpe_rollout_rows_episode: episode_step is NULL'),
      ('episode_step = PTR', -1,
       "mpe_rollout_rows_episode: bufs->done (the agents' done rows) is NULL"),
      ('bufs = b', -1,
       "mpe_rollout_rows_episode: bufs->done (the agents' done rows) is NULL"),
      ('b.done = PTR', -1,
       'mpe_rollout_rows_episode: max_episode_steps < 0'),
      ('max_episode_steps = 25', -1,
       'mpe_rollout_rows_episode: desc is NULL'),
      ('desc = d', -1,
       'mpe_rollout_rows_episode: speakers 0xff but desc->dim_c = 0'),
      ('d.dim_c = 2', -1,
       "mpe_rollout_rows_episode: bufs->comm (receives the speaking agents' last words) is NULL"),
      ('b.comm = PTR', 0,
       "mpe_rollout_rows_episode: bufs->comm (receives the speaking agents' last words) is NULL"),
      ('T = 5', -1,
       'mpe_rollout_rows_episode: mass[0] must be > 0'),
      ('d.mass[0] = 1.0', -1,
       'mpe_rollout_rows_episode: prog is NULL'),
      ('prog = p', -1,
       'mpe_rollout_rows_episode: prog->header_device is NULL (MPE_ROWS_HEADER_BYTES of device memory)'),
      ('p.header_device = PTR', -1,
       'mpe_rollout_rows_episode: B < 0'),
      ('B = 4', -1,
       'mpe_rollout_rows_episode: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_rollout_rows_episode: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_rollout_rows_episode: bufs->obs is NULL'),
      ('b.obs = PTR', -1,
       'mpe_rollout_rows_episode: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('b.choice = PTR', -2,
       'mpe_rollout_rows_episode: a movable landmark (entity 4) is stepped by mpe_world_step only'),
      ('B = 0', -2,
       'mpe_rollout_rows_episode: a movable landmark (entity 4) is stepped by mpe_world_step only'),
      ('d.movable[4] = 0', 0,
       'mpe_rollout_rows_episode: a movable landmark (entity 4) is stepped by mpe_world_step only'),
     ]),
    ('mpe_step_rows_episode', 'the episode arguments, then the row call with its action check',
     'd = generic(2, 2, picks=(2,)); p = RowProgram(); b = buffers()',
     [
      ('', -1,
       'mpe_step_rows_episode: episode_step is NULL'),
      ('episode_step = PTR', -1,
       "mpe_step_rows_episode: bufs->done (the agents' done rows) is NULL"),
      ('bufs = b', -1,
       "mpe_step_rows_episode: bufs->done (the agents' done rows) is NULL"),
      ('b.done = PTR', -1,
       'mpe_step_rows_episode: max_episode_steps < 0'),
      ('max_episode_steps = 25', -1,
       'mpe_step_rows_episode: desc is NULL'),
      ('desc = d', -1,
       'mpe_step_rows_episode: prog is NULL'),
      ('prog = p', -1,
       'mpe_step_rows_episode: prog->header_device is NULL (MPE_ROWS_HEADER_BYTES of device memory)'),
      ('p.header_device = PTR', -1,
       'mpe_step_rows_episode: B < 0'),
      ('B = 4', -1,
       'mpe_step_rows_episode: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_step_rows_episode: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_step_rows_episode: bufs->obs is NULL'),
      ('b.obs = PTR', -1,
       'mpe_step_rows_episode: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('b.choice = PTR', -1,
       'mpe_step_rows_episode: exactly one of bufs->act / bufs->ids / bufs->u must be set'),
      ('b.ids = PTR', -2,
       'mpe_step_rows_episode: a movable landmark (entity 3) is stepped by mpe_world_step only'),
      ('B = 0', -2,
       'mpe_step_rows_episode: a movable landmark (entity 3) is stepped by mpe_world_step only'),
      ('d.movable[3] = 0', 0,
       'mpe_step_rows_episode: a movable landmark (entity 3) is stepped by mpe_world_step only'),
     ]),
    ('mpe_episode_finish', 'the episode arguments, then the row call that steps nothing (a movable landmark is no obstacle)',
     'd = generic(2, 2, picks=(2,)); p = RowProgram(); b = buffers()',
     [
      ('', -1,
       'mpe_episode_finish: episode_step is NULL'),
      ('episode_step = PTR', -1,
       "mpe_episode_finish: bufs->done (the agents' done rows) is NULL"),
      ('bufs = b', -1,
       "mpe_episode_finish: bufs->done (the agents' done rows) is NULL"),
      ('b.done = PTR', -1,
       'mpe_episode_finish: max_episode_steps < 0'),
      ('max_episode_steps = 25', -1,
       'mpe_episode_finish: desc is NULL'),
      ('desc = d', -1,
       'mpe_episode_finish: prog is NULL'),
      ('prog = p', -1,
       'mpe_episode_finish: prog->header_device is NULL (MPE_ROWS_HEADER_BYTES of device memory)'),
      ('p.header_device = PTR', -1,
       'mpe_episode_finish: B < 0'),
      ('B = 4', -1,
       'mpe_episode_finish: bufs->pos is NULL'),
      ('b.pos = PTR', -1,
       'mpe_episode_finish: bufs->vel is NULL'),
      ('b.vel = PTR', -1,
       'mpe_episode_finish: bufs->obs is NULL'),
      ('b.obs = PTR', -1,
       'mpe_episode_finish: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('B = 0', -1,
       'mpe_episode_finish: bufs->choice (the per-world picks of reset_world) is NULL'),
      ('b.choice = PTR', 0,
       'mpe_episode_finish: bufs->choice (the per-world picks of reset_world) is NULL'),
     ]),
]


@pytest.mark.parametrize("n", range(len(LADDERS)), ids=["%02d-%s" % (n, l[0]) for n, l in enumerate(LADDERS)])
def test_refusal_ladder(n):
    entry, _, start, rungs = LADDERS[n]
    run_ladder(entry, start, rungs)


def test_every_entry_point_has_a_ladder_and_every_ladder_ends_let_through():
    assert {l[0] for l in LADDERS} == set(CALLS)
    assert sum(len(l[3]) for l in LADDERS) == 369
    for entry, _, _, rungs in LADDERS:
        if entry not in QUERIES:
            assert rungs[-1][1] == 0 and all(rc in (0, -1, -2) for _, rc, _ in rungs), entry
