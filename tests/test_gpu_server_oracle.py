"""The step server (k_split<..., SERVE=true>: StepServer, env.step_many) against the REFERENCE -- the recorded goldens and the fp64
oracle -- rather than against the launched steps (tests/test_gpu_server.py compares the two bit for bit, which a mistake both
share would pass).  What only a served step runs: the system-scope move / utterance loads from the caller's rings, the output
block of step g, the state carried in registers from step to step with write-through stores of world.pos / vel, the in-launch
resets, and the dual-role variant (a physics and a rows wave per agent) below 1.5 workgroups per CU.

Bars (tests/test_gpu_parity.py): per element |gpu - fp64| <= 1e-5 * max(1, |ref|); the outputs that count strict-< events
(collisions, caught prey, forests, food) exact outside the 1e-6 guard band, which may mask at most 1 % of the worlds; `done`
always False."""
import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from _parity_util import close, golden_moves_and_words, guard_ok, np_, set_choices
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.rollout import StepServer
from oracle import philox
from oracle import spec as ospec
from oracle.mpe_batched import BatchedOracle, seeded_initial_state
from oracle.mpe_f3 import F3Oracle, knife_edge

pytestmark = pytest.mark.gpu


def dual_max_workgroups():
    """launch_split_serve takes the dual-role kernel up to n_cu * 3 / 2 workgroups of 64 worlds (where the kind has one)."""
    return torch.cuda.get_device_properties(0).multi_processor_count * 3 // 2


def single_role_batch():
    """A ragged batch one workgroup above the dual-role limit: the single-role kernel."""
    return 64 * dual_max_workgroups() + 37


def speaks(env):
    return any(not a.silent for a in env.world.agents)


def is_dual(env):
    kind = env._kind
    return kind in (_abi.MPE_SCN_SIMPLE, _abi.MPE_SCN_SPREAD, _abi.MPE_SCN_TAG, _abi.MPE_SCN_ADVERSARY, _abi.MPE_SCN_PUSH) and \
        (env.batch_size + 63) // 64 <= dual_max_workgroups()


# ---- a. teacher-forced through the served kernel against the reference's goldens ----------------------------------------------
BASE = {"simple": ("simple", {}), "simple_spread": ("simple_spread", {}), "simple_tag": ("simple_tag", {}),
        "simple_spread_n5": ("simple_spread", {"num_agents": 5})}
F3 = ["simple_adversary", "simple_push", "simple_speaker_listener", "simple_reference", "simple_crypto", "simple_world_comm"]
GOLDENS = list(BASE) + ["f3_" + n for n in F3] + ["custom_simple_spread", "custom_simple_tag"] + ["f3c_" + n for n in F3]


def _custom_env(name, B, custom_golden):
    """A world with the scenario's DEFAULT constants, an env on it, and one step_many call -- a server is cached with the default
    descriptor -- then the golden's constants assigned on the live world (as the reference's caller would: plain attributes)."""
    sc = mpe.scenarios.load(name + ".py").Scenario()
    w = sc.make_world(batch_size=B)
    w.rng_mode = "device"
    sc.reset_world(w)
    env = mpe.MultiAgentEnv(w, sc.reset_world, sc.reward, sc.observation)
    env.scenario = sc
    assert env.fused
    A = len(w.agents)
    mv = torch.zeros((1, A, B, _abi.MPE_ACTION_DIM), device="cuda")
    comm = torch.zeros((1, A, B, int(w.dim_c)), device="cuda") if speaks(env) else None
    env.step_many(mv, comm=comm)
    torch.cuda.synchronize()
    assert env._step_many_servers, "no server cached by the first call"
    g = custom_golden
    for k, e in enumerate(w.entities):
        e.size, e.initial_mass, e.collide = float(g["c_size"][k]), float(g["c_mass"][k]), bool(g["c_collide"][k])
    for k, a in enumerate(w.agents):
        a.max_speed = None if g["c_max_speed"][k] < 0 else float(g["c_max_speed"][k])
        a.accel = None if g["c_accel"][k] < 0 else float(g["c_accel"][k])
    w.dt, w.damping, w.contact_force, w.contact_margin = [float(x) for x in g["c_world"]]
    return env, mv, comm


@pytest.mark.parametrize("width", ["own", "single_role"])
@pytest.mark.parametrize("gname", GOLDENS)
def test_served_step_teacher_forced_against_reference_golden(gname, width, golden, record_parity):
    """Every recorded step as ONE served step (env.step_many(moves[None])) from the reference's own pre-step state, at the golden's
    width (the dual-role kernel for the kinds that have one) and tiled to a ragged batch above the dual-role limit (single-role).
    The custom_* / f3c_* goldens are stepped by a server cached BEFORE their constants were assigned."""
    g = golden(gname)
    W, T = g["rew"].shape[1], g["rew"].shape[0]
    B = W if width == "own" else single_role_batch()
    idx = np.arange(B) % W
    custom = gname.startswith(("custom_", "f3c_"))
    name = gname.split("_", 1)[1] if gname.startswith(("f3_", "f3c_", "custom_")) else gname
    if custom:
        env, mv, comm = _custom_env(name, B, g)
    else:
        scn, kw = BASE.get(name, (name, {}))
        env = mpe.make_env(scn, batch_size=B, **kw)
        A = len(env.world.agents)
        mv = torch.zeros((1, A, B, _abi.MPE_ACTION_DIM), device="cuda")
        comm = torch.zeros((1, A, B, int(env.world.dim_c)), device="cuda") if speaks(env) else None
    w = env.world
    A = len(w.agents)
    assert is_dual(env) == (width == "own" and env._kind in (_abi.MPE_SCN_SIMPLE, _abi.MPE_SCN_SPREAD, _abi.MPE_SCN_TAG,
                                                             _abi.MPE_SCN_ADVERSARY, _abi.MPE_SCN_PUSH))
    if width == "single_role":
        assert (B + 63) // 64 > dual_max_workgroups()
    moves, words = golden_moves_and_words(g, w)
    assert (words is None) == (comm is None)
    if "choice" in g:
        set_choices(env, g["choice"][idx])
    if gname.startswith("custom_"):
        from test_oracle_golden import custom_spec
        spec = custom_spec(name, g)
    sizes = np.array([e.size for e in w.entities])
    worst = {"pos": 0.0, "vel": 0.0, "obs": 0.0, "rew": 0.0, "c": 0.0}
    masked = 0
    for t in range(T):
        w.set_state((g["pos0"] if t == 0 else g["pos"][t - 1])[idx], (g["vel0"] if t == 0 else g["vel"][t - 1])[idx])
        mv[0].copy_(torch.from_numpy(np.ascontiguousarray(moves[t][:, idx])))
        if comm is not None:
            comm[0].copy_(torch.from_numpy(np.ascontiguousarray(words[t][:, idx])))
        (obs_n, rew, done), = env.step_many(mv, comm=comm)
        torch.cuda.synchronize()
        pos, vel = w.get_state()
        worst["pos"] = max(worst["pos"], close(pos, g["pos"][t][idx], what="t=%d pos" % t))
        worst["vel"] = max(worst["vel"], close(vel, g["vel"][t][idx], what="t=%d vel" % t))
        ok = np.ones(B, bool)
        if gname.startswith("custom_"):
            ok = guard_ok(spec, g["pos"][t][idx])
        elif gname.startswith("f3c_"):        # (as test_f3_scenarios: a pair within 1e-6 of touching)
            d = np.linalg.norm(g["pos"][t][idx][:, :, None, :] - g["pos"][t][idx][:, None, :, :], axis=-1)
            ok = ~(np.abs(d - (sizes[:, None] + sizes[None, :])[None]) < 1e-6).any(axis=(1, 2))
            assert (~ok).sum() <= max(1, 0.01 * B)
        masked = max(masked, int((~ok).sum()))
        for i in range(A):
            worst["obs"] = max(worst["obs"], close(np_(obs_n[i]), g["obs%d" % i][t][idx], what="t=%d obs%d" % (t, i)))
            worst["rew"] = max(worst["rew"], close(np_(rew[i])[ok], g["rew"][t][idx, i][ok], what="t=%d rew%d" % (t, i)))
            if comm is not None:      # the comm state after the step: what the agent said (silent: zeros)
                worst["c"] = max(worst["c"], close(np_(env._comm[i]), g["c%d" % i][t][idx], what="t=%d c%d" % (t, i)))
        assert not np_(done).any()
    record_parity("served_golden_%s_%s" % (gname, width), {"worlds": B, "steps": T, "dual_role": is_dual(env),
                                                            "max_scaled_err": worst, "worlds_masked_guard_band": masked,
                                                            "against": "tests/golden/%s.npz, teacher-forced, one served step each" % gname})


# ---- b. closed loop inside ONE launch against the fp64 oracle ---------------------------------------------------------------------
# every served instantiation of kSplitTable (mpe_split.hip): (name, make_env kwargs, oracle spec)
SERVED = [("simple", {}, lambda: ospec.simple())] + \
    [("simple_spread", {"num_agents": n}, (lambda n=n: ospec.simple_spread(n))) for n in range(1, 7)] + \
    [("simple_tag", {"num_good_agents": gd, "num_adversaries": ad, "num_landmarks": lm},
      (lambda gd=gd, ad=ad, lm=lm: ospec.simple_tag(n_adversaries=ad, n_good=gd, n_landmarks=lm))) for gd, ad, lm in
     ((1, 3, 2), (1, 1, 1), (2, 4, 3))] + \
    [(n, {}, (lambda n=n: ospec.by_name(n))) for n in F3]
CLOSED = [c + (997,) for c in SERVED] + [c + (None,) for c in SERVED if (c[0], c[1]) in (
    ("simple_spread", {"num_agents": 3}), ("simple_tag", {"num_good_agents": 1, "num_adversaries": 3, "num_landmarks": 2}),
    ("simple_adversary", {}), ("simple_crypto", {}))]
CLOSED_IDS = ["%s%s-%s" % (c[0], "-".join(map(str, c[1].values())), "single" if c[3] is None else c[3]) for c in CLOSED]


@pytest.mark.parametrize("name,kw,mk,B", CLOSED, ids=CLOSED_IDS)
def test_served_closed_loop_against_the_fp64_oracle(name, kw, mk, B, record_parity):
    """ONE StepServer launch of 3 * EP + 2 steps with in-launch resets every EP steps, world_offset != 0, commanded a step at a
    time (ring, wait, read).  Step g is checked against the fp64 oracle stepped once from the GPU's OWN state after step g - 1 as
    world.pos / vel / choice_i32 hold it -- or, at an episode boundary, from mpe_reset's draws (oracle/philox.py) with zero
    velocity.  The kernel computes step g from its registers, not from HBM: this checks the arithmetic AND that what it stores is
    what it carries.  An in-launch reset redraws every entity's position and the per-world picks (simple_crypto's goal, which the
    reward wave tracks on its own, among them; simple_world_comm's food are landmarks and redrawn with them); the comm state is not
    reset -- a served step's observations hold the utterances of the step itself, taken from the caller's ring."""
    EP, SEED, OFF = 5, 4242, 12345
    T = 3 * EP + 2
    B = single_role_batch() if B is None else B
    spec = mk()
    f3 = name in F3
    env = mpe.make_env(name, batch_size=B, seed=SEED, **kw)
    w = env.world
    w.world_offset = OFF
    A, L, dc = spec.n_agents, spec.n_landmarks, int(w.dim_c)
    assert (A, L) == (len(w.agents), len(w.landmarks))
    assert float(getattr(env._scenario, "landmark_range", 1.0)) == spec.landmark_range
    assert is_dual(env) == (B <= 64 * dual_max_workgroups() and name in ("simple", "simple_spread", "simple_tag", "simple_adversary",
                                                                          "simple_push"))
    rs = np.random.RandomState(31)
    hard = np.eye(5, dtype=np.float32)[rs.randint(0, 5, size=(T, A, B))]
    moves = np.where((rs.rand(T, A, B) < 0.25)[..., None], rs.uniform(-1, 1, (T, A, B, 5)).astype(np.float32), hard)
    words = None
    if speaks(env):
        words = np.where((rs.rand(T, A, B) < 0.25)[..., None], rs.uniform(0, 1, (T, A, B, dc)),
                         np.eye(dc)[rs.randint(0, dc, size=(T, A, B))]).astype(np.float32)
        words[rs.rand(T, A, B) < 0.05] = 0.0
        for i in range(A):
            if spec.silent_of(i):
                words[:, i] = 0.0
    moves_t = torch.as_tensor(moves).cuda().contiguous()
    words_t = torch.as_tensor(words).cuda().contiguous() if words is not None else None
    srv = StepServer(env, moves_t, slots=2, episode_len=EP, seed=SEED, timeout_s=20.0, comm=words_t)
    srv.start(T)
    orc = (F3Oracle if f3 else BatchedOracle)(spec, B, np.float64)
    pops = list(spec.choice_pops) if f3 else []
    prev = None
    worst = {"pos": 0.0, "vel": 0.0, "obs": 0.0, "rew": 0.0}
    masked = 0
    try:
        for g in range(T):
            srv.ring()
            srv.wait()
            torch.cuda.current_stream().synchronize()
            assert int(srv.status.item()) == 0
            pos, vel = w.get_state()
            choice = np_(w.choice_i32).reshape(len(pops), B).T.copy() if pops else None
            obs_n, rew, done = srv.outputs(g)
            if g % EP == 0:      # the episode's first step starts from mpe_reset's draws
                p0 = philox.reset_positions(SEED, B, g // EP, A, L, spec.landmark_range, OFF).astype(np.float64)
                v0 = np.zeros((B, A, 2))
                c0 = philox.reset_choices(SEED, B, g // EP, pops, OFF).T.astype(np.int64) if pops else None
            else:
                p0, v0, c0 = prev
            orc.set_state(p0, v0)
            if f3:
                orc.set_choice(c0 if pops else np.zeros((B, 0), np.int64))
                acts = []
                for i in range(A):
                    parts = ([moves[g, i]] if spec.movable[i] else []) + ([words[g, i]] if not spec.silent_of(i) else [])
                    acts.append(np.concatenate(parts, axis=1).astype(np.float64))
                obs64, rew64, _, _ = orc.step(acts)
                edge = knife_edge(spec, orc.pos, 1e-6)
                assert edge.sum() <= max(1, 0.01 * B), "knife edge masks %d of %d worlds" % (edge.sum(), B)
                ok = ~edge
            else:
                obs64, rew64, _, _ = orc.step(moves[g])
                ok = guard_ok(spec, orc.pos)
            masked = max(masked, int((~ok).sum()))
            worst["pos"] = max(worst["pos"], close(pos, orc.pos, what="g=%d pos" % g))
            worst["vel"] = max(worst["vel"], close(vel, orc.vel, what="g=%d vel" % g))
            if pops:
                assert np.array_equal(choice, c0), "g=%d: the picks in HBM" % g
            for i in range(A):
                o = np_(obs_n[i])
                worst["obs"] = max(worst["obs"], close(o[ok] if f3 else o, obs64[i][ok] if f3 else obs64[i], what="g=%d obs%d" % (g, i)))
                worst["rew"] = max(worst["rew"], close(np_(rew[i])[ok], (rew64[i] * np.ones(B))[ok], what="g=%d rew%d" % (g, i)))
            assert not np_(done).any()
            prev = (pos.astype(np.float64), vel.astype(np.float64), choice)
    finally:      # (a failed check: the remaining steps commanded, so that the launch ends now and not at its timeout)
        if srv.commanded < T:
            srv.ring(T - srv.commanded)
    srv.join()
    torch.cuda.synchronize()
    srv.check()
    record_parity("served_closed_loop_%s" % "_".join([name] + ["%s" % v for v in kw.values()] + [str(B)]),
                  {"worlds": B, "steps": T, "episode_len": EP, "world_offset": OFF, "dual_role": is_dual(env), "max_scaled_err": worst,
                   "worlds_masked_guard_band": masked, "against": "oracle fp64, one step from the GPU's state (or mpe_reset's draws)"})


# ---- c. back-to-back `ahead` launches, free-running -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mk,B", [("simple_spread", lambda: ospec.simple_spread(3), 4096),
                                        ("simple_tag", lambda: ospec.simple_tag(), 16384),
                                        ("simple_spread", lambda: ospec.simple_spread(3), 65536)], ids=["C2", "C3", "C5"])
def test_step_many_free_running_against_the_fp64_oracle(name, mk, B, record_parity):
    """env.step_many of 25 steps (one launch, every command ahead of it) from seeded worlds, no teacher forcing: step 0 per element
    at 1e-5; at steps 5 / 10 / 25 the drift of the agents' positions (read from their observation rows: vel, pos first) stays
    within 2x the same arithmetic's drift in NumPy float32 + 1e-7 -- test_free_running_episode_drift's comparator."""
    spec = mk()
    A, T = spec.n_agents, 25
    rs = np.random.RandomState(3)
    pos, vel = seeded_initial_state(spec, np.arange(B) + 5000)
    p32 = pos.astype(np.float32)
    o64, o32 = BatchedOracle(spec, B, np.float64), BatchedOracle(spec, B, np.float32)
    o64.set_state(p32, vel)
    o32.set_state(p32, vel)
    env = mpe.make_env(name, batch_size=B)
    env.world.set_state(p32, vel)
    moves = np.eye(5, dtype=np.float32)[rs.randint(0, 5, size=(T, A, B))]
    outs = env.step_many(torch.as_tensor(moves).cuda().contiguous())
    torch.cuda.synchronize()
    drift, drift32, step0 = {}, {}, {"obs": 0.0, "rew": 0.0}

    def pcts(err):
        return {"median": float(np.median(err)), "p90": float(np.percentile(err, 90)), "p99": float(np.percentile(err, 99)),
                "max": float(err.max())}
    for t in range(T):
        obs64, rew64, _, _ = o64.step(moves[t])
        o32.step(moves[t])
        obs_n, rew, done = outs[t]
        assert not np_(done).any()
        if t == 0:
            ok = guard_ok(spec, o64.pos)
            for i in range(A):
                step0["obs"] = max(step0["obs"], close(np_(obs_n[i]), obs64[i], what="t=0 obs%d" % i))
                step0["rew"] = max(step0["rew"], close(np_(rew[i])[ok], rew64[i][ok], what="t=0 rew%d" % i))
        if t + 1 in (5, 10, 25):
            gpos = np.stack([np_(obs_n[i])[:, 2:4] for i in range(A)], axis=1).astype(np.float64)
            err = np.abs(gpos - o64.pos[:, :A]).max(axis=(1, 2))
            err32 = np.abs(o32.pos[:, :A].astype(np.float64) - o64.pos[:, :A]).max(axis=(1, 2))
            drift["t=%d" % (t + 1)], drift32["t=%d" % (t + 1)] = pcts(err), pcts(err32)
    gpos, _ = env.world.get_state()
    assert np.array_equal(gpos[:, :A], np.stack([np_(outs[T - 1][0][i])[:, 2:4] for i in range(A)], axis=1))
    record_parity("served_drift_%s_A%d_B%d" % (name, A, B), {"worlds": B, "step0_max_scaled_err": step0, "steps": drift,
                                                              "steps_numpy_fp32_same_order": drift32,
                                                              "what": "max |agent pos - fp64| per world, env.step_many free-running"})
    for k in drift:
        for q in ("median", "p90", "p99"):
            assert drift[k][q] <= 2.0 * drift32[k][q] + 1e-7, (k, q, drift[k][q], drift32[k][q])
