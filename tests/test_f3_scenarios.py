"""the six scenarios outside BASELINE.json's configs, on the generic path (torch
callbacks over the SoA views + `mpe_world_step`).  Golden vectors: tests/golden/f3_*.npz, recorded from
the unmodified reference by tests/golden/gen_golden_scenarios.py.

CPU part (no GPU needed: resets, observation() and reward() are host/torch code):
  * `env.reset(seeds=...)` reproduces the reference's `np.random.seed(s); env.reset()` per world --
    including the np.random.choice draws that precede the positions (goal / key landmarks);
  * observation() and reward() evaluated on the golden states equal the reference's outputs.
GPU part: env.step() -- _set_action in all its modes (move, speak, MultiDiscrete), World.step on the
GPU, callbacks, shared-reward sum -- teacher-forced against the golden trajectories.
"""
import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe

NAMES = ["simple_adversary", "simple_push", "simple_speaker_listener", "simple_reference", "simple_crypto",
         "simple_world_comm"]
from _parity_util import TOL, close, np_, set_choices, set_comm  # noqa: E402,F401  (shared with the served-step tests)


def get_choices(env):
    sc = env.scenario
    for attr in ("choice_index", "goal_index"):
        if hasattr(sc, attr):
            v = np_(getattr(sc, attr))
            return v.reshape(v.shape[0], -1)
    return np.zeros((env.batch_size, 0), np.int64)


def rewards(env):
    r = [np_(env._get_reward(a)).astype(np.float64) * np.ones(env.batch_size) for a in env.agents]
    if env.shared_reward:
        r = [np.sum(r, axis=0)] * env.n
    return np.stack(r, axis=1)


@pytest.mark.parametrize("name", NAMES)
def test_reset_and_callbacks_match_reference_on_cpu(name, golden):
    g = golden("f3_" + name)
    W = len(g["seeds"])
    env = mpe.make_env(name, batch_size=W, device="cpu", fused=False)   # the torch callbacks (generic path)
    A = env.n
    # --- seeded reset: choices, positions, observations ---------------------------------------------
    obs = env.reset(seeds=[int(s) for s in g["seeds"]])
    assert np.array_equal(get_choices(env), g["choice"])
    plain = ~g["staged"]      # staged worlds (tests/golden/gen_golden_scenarios.py) were moved after their reset
    pos, vel = env.world.get_state()
    close(pos[plain], g["pos0"][plain], what="reset pos")
    assert not vel.any()
    for i in range(A):
        close(np_(obs[i])[plain], g["obs_reset%d" % i][plain], what="reset obs%d" % i)
    # --- observation() on the (squeezed) initial states ---------------------------------------------------
    env.world.set_state(g["pos0"], g["vel0"])
    set_comm(env, g, -1)
    for i, agent in enumerate(env.agents):
        close(np_(env._get_obs(agent)), g["obs_reset%d" % i], what="obs0 %d" % i)
    # --- observation() / reward() on every golden state ----------------------------------------------------------
    for t in range(g["rew"].shape[0]):
        env.world.set_state(g["pos"][t], g["vel"][t])
        set_comm(env, g, t)
        for i, agent in enumerate(env.agents):
            close(np_(env._get_obs(agent)), g["obs%d" % i][t], what="t=%d obs%d" % (t, i))
        close(rewards(env), g["rew"][t], what="t=%d rew" % t)


@pytest.mark.parametrize("name", NAMES)
def test_compat_mode_reset_consumes_the_numpy_stream_like_the_reference(name, golden):
    g = golden("f3_" + name)
    env = mpe.make_env(name, device="cpu", fused=False)      # batch_size=None: one world, global np.random, NumPy I/O
    for w in [int(x) for x in np.flatnonzero(~g["staged"])[:3]]:
        np.random.seed(int(g["seeds"][w]))
        env.reset_callback(env.world)            # reset_world only (the observation gather needs no GPU either)
        assert np.array_equal(get_choices(env)[0], g["choice"][w])
        pos, _ = env.world.get_state()
        close(pos[0], g["pos0"][w])
        for i, agent in enumerate(env.agents):
            close(np_(env._get_obs(agent))[0], g["obs_reset%d" % i][w])


def test_f3_spaces_match_the_reference():
    want = {"simple_adversary": ([8, 10, 10], [5, 5, 5]), "simple_push": ([8, 19], [5, 5]),
            "simple_speaker_listener": ([3, 11], [3, 5]), "simple_reference": ([21, 21], [(5, 10), (5, 10)]),
            "simple_crypto": ([4, 8, 8], [4, 4, 4]),
            "simple_world_comm": ([34, 34, 34, 34, 28, 28], [(5, 4), 5, 5, 5, 5, 5])}
    for name, (obs_dims, acts) in want.items():
        env = mpe.make_env(name, batch_size=2, device="cpu")
        assert env.fused
        assert [sp.shape[0] for sp in env.observation_space] == obs_dims
        for sp, a in zip(env.action_space, acts):
            if isinstance(a, tuple):       # environment.py:58-61 MultiDiscrete([[0, n-1], ...])
                assert list(sp.high - sp.low + 1) == list(a)
            else:
                assert sp.n == a


FUSED = list(NAMES)            # every one of them has a fused kernel (KIND specialisations of k_split)
FUSED_ROLLOUT = ["simple_adversary", "simple_push"]


@pytest.mark.gpu
@pytest.mark.parametrize("name,fused", [(n, False) for n in NAMES] + [(n, True) for n in FUSED],
                         ids=[n + "-generic" for n in NAMES] + [n + "-fused" for n in FUSED])
def test_step_teacher_forced_against_reference_golden(name, fused, golden):
    g = golden("f3_" + name)
    env = mpe.make_env(name, batch_size=len(g["seeds"]), fused=fused)
    assert env.fused == fused
    print("max scaled err %s: %.3e" % (name, teacher_forced_against_golden(env, g)))


def teacher_forced_against_golden(env, g):
    """Every recorded step from the reference's own pre-step state: pos / vel / obs / reward / comm state at 1e-5."""
    W, T = len(g["seeds"]), g["rew"].shape[0]
    A = env.n
    set_choices(env, g["choice"])
    worst = 0.0
    for t in range(T):
        if t == 0:
            env.world.set_state(g["pos0"], g["vel0"])
            set_comm(env, g, -1)
        else:
            env.world.set_state(g["pos"][t - 1], g["vel"][t - 1])
            set_comm(env, g, t - 1)
        act = [torch.as_tensor(g["act%d" % i][t], dtype=torch.float32).cuda() for i in range(A)]
        obs_n, rew_n, done_n, _ = env.step(act)
        pos, vel = env.world.get_state()
        worst = max(worst, close(pos, g["pos"][t], what="t=%d pos" % t), close(vel, g["vel"][t], what="t=%d vel" % t))
        for i in range(A):
            worst = max(worst, close(np_(obs_n[i]), g["obs%d" % i][t], what="t=%d obs%d" % (t, i)))
            worst = max(worst, close(np_(rew_n[i]) * np.ones(W), g["rew"][t][:, i], what="t=%d rew%d" % (t, i)))
            worst = max(worst, close(np_(env.world.agents[i].state.c), g["c%d" % i][t], what="t=%d c%d" % (t, i)))
            assert not np_(done_n[i]).any()
    return worst


def random_actions(env, rs, B):
    acts = []
    for agent in env.agents:
        parts = []
        if agent.movable:
            parts.append(np.eye(5, dtype=np.float32)[rs.randint(0, 5, size=B)])
        if not agent.silent:
            parts.append(rs.uniform(0, 1, size=(B, env.world.dim_c)).astype(np.float32))
        acts.append(torch.as_tensor(np.concatenate(parts, axis=1)).cuda())
    return acts


@pytest.mark.gpu
@pytest.mark.parametrize("name", FUSED)
def test_fused_kernel_equals_generic_path_at_size(name):
    """65 536 random worlds: the fused kernel (KIND specialisation of k_split) against the generic path
    (torch callbacks written from the reference + mpe_world_step), same states, goals and actions."""
    B = 65536
    rs = np.random.RandomState(9)
    ef = mpe.make_env(name, batch_size=B)
    eg = mpe.make_env(name, batch_size=B, fused=False)
    assert ef.fused and not eg.fused
    A, E = len(ef.world.agents), len(ef.world.entities)
    pos = rs.uniform(-1, 1, (B, E, 2)).astype(np.float32)
    pos[::3] *= 0.3
    vel = rs.uniform(-0.5, 0.5, (B, A, 2)).astype(np.float32)
    pops = ef.world.choice_pops
    choice = np.stack([rs.randint(0, n, size=B) for n in pops], axis=1) if pops else np.zeros((B, 0), np.int64)
    for env in (ef, eg):
        env.world.set_state(pos, vel)
        set_choices(env, choice)
    act = random_actions(ef, rs, B)
    of, rf, df, _ = ef.step(act)
    og, rg, dg, _ = eg.step(act)
    pf, vf = ef.world.get_state()
    pg, vg = eg.world.get_state()
    close(pf, pg, what="pos")
    close(vf, vg, what="vel")
    for i in range(A):
        close(np_(of[i]), np_(og[i]), what="obs%d" % i)
        close(np_(rf[i]) * np.ones(B), np_(rg[i]) * np.ones(B), what="rew%d" % i)
        close(np_(ef.world.agents[i].state.c), np_(eg.world.agents[i].state.c), what="c%d" % i)
        assert not np_(df[i]).any()
    # reset(): the fused kernel's observe half against the torch observation()
    seeds = list(range(1000, 1000 + B))[:256]
    ef2 = mpe.make_env(name, batch_size=256)
    eg2 = mpe.make_env(name, batch_size=256, fused=False)
    o_f, o_g = ef2.reset(seeds=seeds), eg2.reset(seeds=seeds)
    for i in range(A):
        close(np_(o_f[i]), np_(o_g[i]), what="reset obs%d" % i)


def staged_batch(spec, B, rs):
    """B random worlds with the rare branches well populated (vectorised twin of tests/golden/gen_golden_scenarios.py's
    staging): a third squeezed into contact; for simple_world_comm also prey in the boundary band, next to an adversary,
    on a food item, agents around the forests, and fast agents (speed limits)."""
    A, E = spec.n_agents, spec.n_entities
    pos = rs.uniform(-1, 1, (B, E, 2))
    pos[:, A:] *= spec.landmark_range
    vel = rs.uniform(-0.5, 0.5, (B, A, 2))
    k = np.arange(B) % 8
    pos[k == 1] *= 0.3

    def disk(n, r):
        th, rr = rs.uniform(0, 2 * np.pi, n), r * np.sqrt(rs.uniform(0, 1, n))
        return np.stack([rr * np.cos(th), rr * np.sin(th)], axis=1)
    if spec.name == "simple_push":      # a contact lasts a step or two: most worlds start in (or at the edge of) one
        w = np.flatnonzero(k >= 2)
        pos[w, 1] = pos[w, 0] + disk(len(w), 0.11)
    if spec.name == "simple_world_comm":
        nadv = sum(spec.adversary)
        for g in range(nadv, A):        # the good agents
            w = np.flatnonzero(k == 2)
            pos[w, g, rs.randint(0, 2, len(w))] = rs.choice([-1, 1], len(w)) * rs.uniform(0.88, 1.15, len(w))
            w = np.flatnonzero((k == 3) | (k == 7))
            pos[w, g] = pos[w, rs.randint(0, nadv, len(w))] + disk(len(w), 0.13)
            w = np.flatnonzero(k == 4)
            pos[w, g] = pos[w, A + 1 + (g - nadv) % 2] + disk(len(w), 0.07)
        w = np.flatnonzero((k == 5) | (k == 7))
        vel[w] = rs.uniform(-1.5, 1.5, (len(w), A, 2))
        w = np.flatnonzero(k == 6)
        for i in range(A):
            pos[w, i] = pos[w, A + 3 + rs.randint(0, 2, len(w))] + disk(len(w), 0.45)
    return pos.astype(np.float32), vel.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_fused_step_teacher_forced_against_the_fp64_oracle_at_size(name, record_parity):
    against_the_fp64_oracle(name, {}, {}, 65536, record_parity, "f3_" + name)


def against_the_fp64_oracle(name, spec_kw, env_kw, B, record_parity, key, min_cov=0.05):
    """65 536 worlds, three teacher-forced steps: the fused kernels (KIND specialisations of k_split) against
    oracle/mpe_f3.py -- the fp64 restatement that tests/test_oracle_golden.py pins to the reference at 1e-12 -- instead
    of against the package's own torch callbacks.  Per-element 1e-5 for obs / reward / pos / vel / comm state; worlds in
    which a strict `<` test of the scenario (forest membership, caught prey, food) sits within 1e-6 of its threshold are
    masked, counted, and must stay below 1 %; branch coverage of the batch is printed and must be >= 5 % everywhere."""
    from oracle import spec as ospec
    from oracle.mpe_f3 import F3Oracle, branch_coverage, knife_edge
    T = 3
    spec = ospec.by_name(name, **spec_kw)
    rs = np.random.RandomState(77)
    env = mpe.make_env(name, batch_size=B, **env_kw)
    assert env.fused
    A, E = spec.n_agents, spec.n_entities
    pos, vel = staged_batch(spec, B, rs)
    pops = spec.choice_pops
    choice = np.stack([rs.randint(0, n, size=B) for n in pops], axis=1) if pops else np.zeros((B, 0), np.int64)
    set_choices(env, choice)
    orc = F3Oracle(spec, B, np.float64)
    orc.set_choice(choice)
    comm = np.zeros((A, B, spec.dim_c))
    worst = {"pos": 0.0, "vel": 0.0, "obs": 0.0, "rew": 0.0, "c": 0.0}
    masked = 0
    rec = {"pos": [], "c": [[] for _ in range(A)], "vel": []}
    for t in range(T):
        env.world.set_state(pos, vel)
        for i, agent in enumerate(env.world.agents):
            agent.state.c = torch.as_tensor(comm[i], dtype=torch.float32, device=env.world.device)
        orc.set_state(pos, vel)
        orc.set_comm(comm)
        acts = []
        for i in range(A):
            parts = []
            if spec.movable[i]:
                hard = np.eye(5)[rs.randint(0, 5, size=B)]
                parts.append(np.where((rs.rand(B) < 0.25)[:, None], rs.uniform(-1, 1, (B, 5)), hard))
            if not spec.silent_of(i):
                hard = np.eye(spec.dim_c)[rs.randint(0, spec.dim_c, size=B)]
                soft = rs.uniform(0, 1, (B, spec.dim_c))
                word = np.where((rs.rand(B) < 0.25)[:, None], soft, hard)
                word[rs.rand(B) < 0.05] = 0.0              # the all-zero utterance (simple_crypto.py:107: skipped)
                parts.append(word)
            acts.append(np.concatenate(parts, axis=1).astype(np.float32))
        obs64, rew64, _, _ = orc.step([a.astype(np.float64) for a in acts])
        obs_n, rew_n, done_n, _ = env.step([torch.as_tensor(a).cuda() for a in acts])
        p, v = env.world.get_state()
        edge = knife_edge(spec, orc.pos, 1e-6)
        masked = max(masked, int(edge.sum()))
        ok = ~edge
        worst["pos"] = max(worst["pos"], close(p, orc.pos, what="t=%d pos" % t))
        worst["vel"] = max(worst["vel"], close(v, orc.vel, what="t=%d vel" % t))
        for i in range(A):
            worst["obs"] = max(worst["obs"], close(np_(obs_n[i])[ok], obs64[i][ok], what="t=%d obs%d" % (t, i)))
            worst["rew"] = max(worst["rew"], close((np_(rew_n[i]) * np.ones(B))[ok], rew64[i][ok], what="t=%d rew%d" % (t, i)))
            worst["c"] = max(worst["c"], close(np_(env.world.agents[i].state.c), orc.c[i], what="t=%d c%d" % (t, i)))
            assert not np_(done_n[i]).any()
            rec["c"][i].append(orc.c[i].copy())
        rec["pos"].append(orc.pos.copy())
        rec["vel"].append(orc.vel.copy())
        # teacher forcing: both sides continue from the fp64 trajectory rounded to fp32
        pos, vel, comm = orc.pos.astype(np.float32), orc.vel.astype(np.float32), orc.c.astype(np.float32).astype(np.float64)
    g = {"pos": np.stack(rec["pos"]), "vel": np.stack(rec["vel"]), "choice": choice}
    for i in range(A):
        g["c%d" % i] = np.stack(rec["c"][i])
    cov = branch_coverage(spec, g)
    print("%s: max scaled err %s; %d of %d worlds masked (knife edge); coverage %s"
          % (key, {k: "%.2e" % x for k, x in worst.items()}, masked, B, {k: "%.1f%%" % (100 * x) for k, x in cov.items()}))
    assert masked <= 0.01 * B
    assert all(x >= min_cov for x in cov.values()), cov
    record_parity(key, {"worlds": B, "steps": T, "max_scaled_err": worst, "worlds_masked_knife_edge": masked,
                                 "branch_coverage": cov, "against": "oracle/mpe_f3.py fp64, teacher-forced"})


# ---- team sizes other than the reference's make_world (its callbacks are written for any: simple_adversary.py:69-139,
# simple_world_comm.py:126-289); goldens: tests/golden/gen_golden_shapes.py --------------------------------------------------
from oracle.spec import TEAM_SIZE_VARIANTS as SHAPES  # noqa: E402  (2..6 agents x 1..2 adversaries; 1..3 prey x 2..5 predators)
SHAPE_IDS = ["%s-%d-%d" % s for s in SHAPES]


def shape_kw(name, A, nadv):
    """(oracle spec kwargs, make_env kwargs) of a team-size variant."""
    if name == "simple_world_comm":
        return {"n_good": A - nadv, "n_adversaries": nadv}, {"num_good_agents": A - nadv, "num_adversaries": nadv}
    return {"n_agents": A, "n_adversaries": nadv}, {"num_agents": A, "num_adversaries": nadv}


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
@pytest.mark.parametrize("name,A,nadv", SHAPES, ids=SHAPE_IDS)
def test_other_team_sizes_against_reference_golden(name, A, nadv, fused, golden):
    """The reference's callbacks on worlds of other team sizes (recorded by gen_golden_shapes.py), teacher-forced: the
    fused kernels built for these shapes (mpe_split.hip's table) and the generic path, both at 1e-5; with
    benchmark=True the fused launch also delivers the reference's benchmark_data."""
    from oracle import spec as ospec
    from oracle.mpe_f3 import knife_edge
    g = golden("shape_%s_%d_%d" % (name, A, nadv))
    spec_kw, env_kw = shape_kw(name, A, nadv)
    env = mpe.make_env(name, batch_size=len(g["seeds"]), fused=fused, **env_kw)
    assert env.fused == fused and env.n == A
    print("max scaled err %s %d/%d: %.3e" % (name, A, nadv, teacher_forced_against_golden(env, g)))
    if not fused:
        return
    env = mpe.make_env(name, batch_size=len(g["seeds"]), benchmark=True, **env_kw)
    # (a shape with a kernel of its own gets its benchmark_data from the same launch; a row-program shape evaluates the
    #  scenario's benchmark_data callback on the post-step world)
    assert env.fused and env._py_info == (env._prog is not None)
    set_choices(env, g["choice"])
    for t in range(g["rew"].shape[0]):
        env.world.set_state(g["pos0"] if t == 0 else g["pos"][t - 1], g["vel0"] if t == 0 else g["vel"][t - 1])
        set_comm(env, g, t - 1)
        _, _, _, info = env.step([torch.as_tensor(g["act%d" % i][t], dtype=torch.float32).cuda() for i in range(A)])
        inf = info["n"]
        if name == "simple_adversary":      # simple_adversary.py:57-67
            for k in range(A):
                if k < nadv:
                    close(np_(inf[k]), g["info_adv"][t][:, k], what="t=%d adversary %d" % (t, k))
                else:
                    assert isinstance(inf[k], tuple) and len(inf[k]) == g["info_good"].shape[-1]
                    for j, x in enumerate(inf[k]):
                        close(np_(x), g["info_good"][t][:, k - nadv, j], what="t=%d good %d datum %d" % (t, k, j))
        else:                               # simple_world_comm.py:115-124: exact outside the knife edge
            ok = ~knife_edge(ospec.by_name(name, **spec_kw), g["pos"][t], 1e-6)
            got = np.stack([np_(x) for x in inf], axis=1)
            assert got.dtype == np.int32 and np.array_equal(got[ok], g["info_collisions"][t][ok]) and ok.mean() > 0.98


@pytest.mark.gpu
@pytest.mark.parametrize("name,A,nadv", SHAPES, ids=SHAPE_IDS)
def test_other_team_sizes_against_the_fp64_oracle_at_size(name, A, nadv, record_parity):
    """16 384 staged worlds per team-size variant against oracle/mpe_f3.py (pinned to the reference at these very shapes
    by tests/test_oracle_golden.py), same protocol and bars as the reference shapes above."""
    spec_kw, env_kw = shape_kw(name, A, nadv)
    against_the_fp64_oracle(name, spec_kw, env_kw, 16384, record_parity, "shape_%s_%d_%d" % (name, A, nadv))


@pytest.mark.gpu
@pytest.mark.parametrize("name,A,nadv", SHAPES, ids=SHAPE_IDS)
def test_other_team_sizes_reset_and_auto_reset(name, A, nadv):
    """env.reset() (mpe_observe: the kernels' observe half) and the device-side auto-reset at the horizon, fused against the
    generic path's torch observation() on the same seeded worlds."""
    _, env_kw = shape_kw(name, A, nadv)
    B = 300
    ef = mpe.make_env(name, batch_size=B, max_episode_steps=2, auto_reset=True, seed=9, **env_kw)
    eg = mpe.make_env(name, batch_size=B, fused=False, **env_kw)
    assert ef.fused and not eg.fused
    seeds = list(range(500, 500 + B))
    of, og = ef.reset(seeds=seeds), eg.reset(seeds=seeds)
    for i in range(A):
        close(np_(of[i]), np_(og[i]), what="reset obs%d" % i)
    rs = np.random.RandomState(3)
    ef.step(random_actions(ef, rs, B))
    o, _, d, _ = ef.step(random_actions(ef, rs, B))          # the horizon: every world restarts, rows of the new episode
    assert all(np_(x).all() for x in d)
    eg.world.set_state(*ef.world.get_state())
    set_choices(eg, get_choices(ef))
    for i, agent in enumerate(eg.world.agents):
        agent.state.c = torch.zeros_like(agent.state.c)
    for i in range(A):
        close(np_(o[i]), np_(eg._get_obs(eg.agents[i])), what="auto-reset obs%d" % i)


@pytest.mark.gpu
def test_a_team_size_without_a_kernel_steps_through_its_row_program():
    """11 agents (5 prey, 6 predators): no k_split entry -- World.step + the scenario's row program in one launch, held to the
    torch callbacks of the generic path on the same worlds (and past 64 entities: the generic path itself)."""
    B = 512
    env = mpe.make_env("simple_world_comm", batch_size=B, num_good_agents=5, num_adversaries=6, seed=2)
    gen = mpe.make_env("simple_world_comm", batch_size=B, num_good_agents=5, num_adversaries=6, seed=2, fused=False)
    assert env.fused and env._prog is not None and not gen.fused
    rs = np.random.RandomState(0)
    o1, o2 = env.reset(), gen.reset()
    for t in range(4):
        if t == 1:
            for e in (env, gen):
                e.world.pos.mul_(0.4)
        act = random_actions(env, rs, B)
        o1, r1, _, _ = env.step(act)
        o2, r2, _, _ = gen.step(act)
        assert torch.equal(env.world.pos, gen.world.pos) and torch.equal(env.world.vel, gen.world.vel)
        for i in range(11):
            assert o1[i].shape == o2[i].shape and torch.allclose(o1[i], o2[i], atol=1e-6, rtol=0), (t, i)
            err = ((r1[i] - r2[i]).abs() / r2[i].abs().clamp(min=1.0))
            assert float(err.quantile(0.999)) <= 1e-5, (t, i, float(err.max()))      # (a knife-edge contact may flip in one path)
    big = mpe.make_env("simple_adversary", batch_size=16, num_agents=40, num_adversaries=3)     # 79 entities
    assert not big.fused
    with pytest.raises(RuntimeError):      # _abi.MpeError
        mpe.make_env("simple_adversary", batch_size=16, num_agents=40, num_adversaries=3, fused=True)


@pytest.mark.gpu
def test_device_reset_draws_goal_landmarks_bit_exact():
    from oracle import philox
    B, seed, offset = 5000, 0x1234567890ABCDEF, 77
    env = mpe.make_env("simple_adversary", batch_size=B, seed=seed)
    env.world.world_offset = offset
    for ep in range(3):
        env.world._episode = ep
        env.scenario.reset_world(env.world)
        want = philox.reset_choices(seed, B, ep, [2], world_offset=offset)
        assert np.array_equal(np_(env.world.choice_i32), want)
        assert np.array_equal(np_(env.scenario.goal_index), want[0])
    frac = float(np_(env.world.choice_i32).mean())
    assert 0.45 < frac < 0.55


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_compat_mode_episode_like_a_reference_caller(name, golden):
    """The drop-in usage, verbatim: make_env(name) -> one world, NumPy in / NumPy out, np.random-seeded reset,
    per-agent action rows as the reference takes them; a free-running episode against the golden one
    (free-running fp32 vs fp64: looser bound than the teacher-forced tests)."""
    g = golden("f3_" + name)
    env = mpe.make_env(name)
    assert env.fused and env.batch_size == 1
    w = 0
    np.random.seed(int(g["seeds"][w]))
    obs = env.reset()
    for i in range(env.n):
        assert isinstance(obs[i], np.ndarray) and obs[i].ndim == 1
        close(obs[i], g["obs_reset%d" % i][w], what="reset obs%d" % i)
    for t in range(g["rew"].shape[0]):
        act = [g["act%d" % i][t, w] for i in range(env.n)]
        obs, rew, done, info = env.step(act)
        for i in range(env.n):
            close(obs[i], g["obs%d" % i][t, w], tol=1e-4, what="t=%d obs%d" % (t, i))
        close(np.array(rew), g["rew"][t, w], tol=1e-4, what="t=%d rew" % t)
        assert done == [False] * env.n
    # the same episode teacher-forced (state put back on the reference's fp64 trajectory before every step): the
    # per-step bar of 1e-5 through the same NumPy-in / NumPy-out calls
    np.random.seed(int(g["seeds"][w]))
    env.reset()
    for t in range(g["rew"].shape[0]):
        env.world.set_state((g["pos0"] if t == 0 else g["pos"][t - 1])[w][None], (g["vel0"] if t == 0 else g["vel"][t - 1])[w][None])
        obs, rew, done, info = env.step([g["act%d" % i][t, w] for i in range(env.n)])
        for i in range(env.n):
            close(obs[i], g["obs%d" % i][t, w], what="teacher-forced t=%d obs%d" % (t, i))
        close(np.array(rew), g["rew"][t, w], what="teacher-forced t=%d rew" % t)


@pytest.mark.gpu
def test_discrete_action_input_on_a_comm_scenario_matches_one_hot_rows():
    """environment.py:161-167 / :183-186: integer actions (note the opposite x/y sign convention of the integer
    form).  For the scenarios that speak the env routes this mode through the generic path; it
    must agree with the fused kernel fed the equivalent one-hot rows."""
    B = 512
    rs = np.random.RandomState(4)
    ef = mpe.make_env("simple_reference", batch_size=B)
    ei = mpe.make_env("simple_reference", batch_size=B)
    ei.discrete_action_input = True
    E, A = len(ef.world.entities), 2
    pos = rs.uniform(-1, 1, (B, E, 2)).astype(np.float32)
    vel = rs.uniform(-0.5, 0.5, (B, A, 2)).astype(np.float32)
    choice = np.stack([rs.randint(0, 3, size=B) for _ in range(2)], axis=1)
    for env in (ef, ei):
        env.world.set_state(pos, vel)
        set_choices(env, choice)
    move = rs.randint(0, 5, size=(A, B))
    say = rs.randint(0, 10, size=(A, B))
    # integer id 1 means -x, one-hot index 1 means +x (and likewise 3/4 for y): swap to get the same force
    swap = np.array([0, 2, 1, 4, 3])
    rows = [torch.as_tensor(np.concatenate([np.eye(5, dtype=np.float32)[swap[move[i]]],
                                            np.eye(10, dtype=np.float32)[say[i]]], axis=1)).cuda() for i in range(A)]
    ids = [torch.as_tensor(np.stack([move[i], say[i]], axis=1)).cuda() for i in range(A)]
    of, rf, _, _ = ef.step(rows)
    oi, ri, _, _ = ei.step(ids)
    for i in range(A):
        close(np_(oi[i]), np_(of[i]), what="obs%d" % i)
        close(np_(ri[i]) * np.ones(B), np_(rf[i]) * np.ones(B), what="rew%d" % i)


@pytest.mark.gpu
def test_action_noise_and_scripted_agents_on_the_generic_path():
    """core.py:119-120,138,176 (u_noise / c_noise: Gaussian noise on the applied force and the emitted word) and
    core.py:112-114,119-120 (agents with an action_callback are scripted: not policy agents, stepped by the world).
    No shipped scenario sets them; they force the generic path.  In device mode the noise is counter-based
    -- a hash of (world.seed, global world index, draw number, column), not torch's global generator -- so a second
    world with the same seed re-draws the same normals draw by draw, torch.manual_seed does not move them, and another
    shard (world_offset) draws different ones (shard invariance itself: tests/test_host_cpu.py)."""
    B = 257
    Base = mpe.scenarios.load("simple_speaker_listener.py").Scenario
    sc = Base()
    w = sc.make_world(batch_size=B)
    w.agents[1].u_noise = 0.5                  # the listener moves
    w.agents[0].c_noise = 0.25                 # the speaker speaks
    env = mpe.MultiAgentEnv(w, sc.reset_world, sc.reward, sc.observation)
    assert not env.fused
    env.reset(seeds=np.arange(B) + 3)
    pos0, vel0 = w.get_state()
    rs = np.random.RandomState(0)
    word = np.eye(3, dtype=np.float32)[rs.randint(0, 3, B)]
    move = np.eye(5, dtype=np.float32)[rs.randint(0, 5, B)]
    w.seed = 77
    torch.manual_seed(11)
    obs, _, _, _ = env.step([torch.as_tensor(word).cuda(), torch.as_tensor(move).cuda()])
    torch.manual_seed(12345)                                         # irrelevant by construction
    twin = Base().make_world(batch_size=B)
    twin.seed = 77
    nu = twin._randn((B, 2)).cpu().numpy() * 0.5                     # World.step draws u noise first (agents in order)
    nc = twin._randn((B, 3)).cpu().numpy() * 0.25                    # then update_agent_state draws c noise
    other = Base().make_world(batch_size=B)
    other.seed, other.world_offset = 77, B                           # another shard of the same job: another stream
    assert not torch.equal(other._randn((B, 2)), torch.as_tensor(nu / 0.5).cuda())
    u = np.stack([move[:, 1] - move[:, 2], move[:, 3] - move[:, 4]], 1) * 5.0 + nu
    v = vel0[:, 1] * 0.75 + u * 0.1            # no contacts in this scenario (nothing collides)
    p = pos0[:, 1] + v * 0.1
    pos1, vel1 = w.get_state()
    close(vel1[:, 1], v, what="noisy velocity")
    close(pos1[:, 1], p, what="noisy position")
    close(np_(w.agents[0].state.c), word + nc, what="noisy word")
    close(np_(obs[1])[:, -3:], word + nc, what="listener hears the noisy word")

    # scripted agent: the prey of simple_tag runs away along +x by itself
    sc = mpe.scenarios.load("simple_tag.py").Scenario()
    w = sc.make_world(batch_size=B)

    def flee(agent, world):
        act = mpe.core.Action()
        act.u = torch.zeros((world.batch_size, 2), device=world.device)
        act.u[:, 0] = agent.accel
        act.c = torch.zeros((world.batch_size, world.dim_c), device=world.device)
        return act
    w.agents[3].action_callback = flee
    env = mpe.MultiAgentEnv(w, sc.reset_world, sc.reward, sc.observation)
    assert env.n == 3 and not env.fused and len(w.scripted_agents) == 1
    env.reset(seeds=np.arange(B) + 5)
    ref = mpe.make_env("simple_tag", batch_size=B)
    ref.reset(seeds=np.arange(B) + 5)
    assert np.array_equal(ref.world.get_state()[0], w.get_state()[0])
    acts = rs.randint(0, 5, (3, B))
    rows = [torch.as_tensor(np.eye(5, dtype=np.float32)[acts[i]]).cuda() for i in range(3)]
    plus_x = torch.zeros(B, 5, device="cuda"); plus_x[:, 1] = 1.0
    o_s, r_s, _, _ = env.step(rows)
    o_r, r_r, _, _ = ref.step(rows + [plus_x])
    assert np.array_equal(ref.world.get_state()[0], w.get_state()[0])
    assert len(o_s) == 3
    for i in range(3):
        close(np_(o_s[i]), np_(o_r[i]))
        close(np_(r_s[i]), np_(r_r[i]))


def _mirror_case(name, B, kw):
    rs = np.random.RandomState(B % 9973)
    env = mpe.make_env(name, batch_size=B, **kw)
    assert env.fused
    A, E = len(env.world.agents), len(env.world.entities)
    pos = rs.uniform(-1, 1, (B, E, 2)).astype(np.float32)
    pos[::3] *= 0.3
    vel = rs.uniform(-0.7, 0.7, (B, A, 2)).astype(np.float32)
    pops = env.world.choice_pops
    choice = np.stack([rs.randint(0, n, size=B) for n in pops], axis=1) if pops else np.zeros((B, 0), np.int64)
    act = random_actions(env, rs, B)

    def run(p, v, a):
        env.world.set_state(p, v)
        set_choices(env, choice)
        o, r, _, _ = env.step(a)
        ps, vs = env.world.get_state()
        return [np_(x).copy() for x in o], [np_(x).copy() * np.ones(B, np.float32) for x in r], ps, vs
    o0, r0, p0, v0 = run(pos, vel, act)
    return env, (pos, vel, act), (o0, r0, p0, v0), run


MIRROR_CASES = [(n, 16384, {}) for n in ("simple", "simple_tag", "simple_adversary", "simple_push",
                                         "simple_speaker_listener", "simple_reference", "simple_crypto",
                                         "simple_world_comm")] + \
               [("simple_spread", 524288, {}), ("simple_spread", 8192, {"num_agents": 16}),
                ("simple_spread", 4096, {"num_agents": 64})]


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,kw", MIRROR_CASES, ids=["%s-%d" % (c[0], c[1]) for c in MIRROR_CASES])
def test_mirror_and_transpose_symmetry_at_full_size(name, B, kw):
    """Size-independent, bit-exact properties of the step (every kernel family, BASELINE sizes and the 8-GPU total
    of 524 288 worlds on one device): reflecting the world in the y axis (x -> -x, moves +x <-> -x) negates the
    x components of the state and of every geometric observation column and leaves every other output bit-identical
    (IEEE negation commutes with every operation on the path; distances use dx*dx + dy*dy).  Swapping the axes
    (x <-> y, moves accordingly) swaps the state components bit-exactly as well (fp addition commutes); rewards then
    agree to rounding only where a scenario sums per-axis terms in a fixed order (simple_tag's boundary penalty)."""
    env, (pos, vel, act), (o0, r0, p0, v0), run = _mirror_case(name, B, kw)
    sx = np.array([-1.0, 1.0], np.float32)

    def swap_moves(a, perm):
        out = []
        for agent, x in zip(env.agents, a):
            x = x.clone()
            if agent.movable:
                x[:, :5] = x[:, perm]
            out.append(x)
        return out
    om, rm, pm, vm = run(pos * sx, vel * sx, swap_moves(act, [0, 2, 1, 3, 4]))
    assert np.array_equal(pm, p0 * sx) and np.array_equal(vm, v0 * sx)
    n_geo = 0
    for i in range(len(o0)):
        assert np.array_equal(rm[i], r0[i]), "reward of agent %d changed under reflection" % i
        same = (om[i] == o0[i]).all(axis=0)
        neg = (om[i] == -o0[i]).all(axis=0)
        assert (same | neg).all(), "agent %d: columns %s neither kept nor negated" % (i, np.nonzero(~(same | neg))[0])
        n_geo += int((neg & ~same).sum())
    movers = sum(1 for a in env.agents if a.movable)
    assert n_geo >= movers                                # at least the x velocity column of every mover flips
    ot, rt, pt, vt = run(pos[..., ::-1].copy(), vel[..., ::-1].copy(), swap_moves(act, [0, 3, 4, 1, 2]))
    assert np.array_equal(pt, p0[..., ::-1]) and np.array_equal(vt, v0[..., ::-1])
    for i in range(len(o0)):
        close(rt[i], r0[i], what="reward under axis swap")
        assert np.array_equal(np.sort(np.abs(ot[i]), axis=1), np.sort(np.abs(o0[i]), axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize("name,fused", [("simple_tag", True), ("simple_tag", False), ("simple_adversary", True),
                                        ("simple_adversary", False), ("simple_reference", True)])
def test_episode_horizon_and_device_side_auto_reset(name, fused):
    """New API (the reference never ends an episode, environment.py:132-135): with max_episode_steps the
    env counts steps per world on the device and reports done at the horizon; with auto_reset the finished worlds
    start their next episode inside step() (masked `mpe_reset`, no host synchronisation) and the returned
    observation rows are the new episode's first.  Mirrored here by a plain env that is reset by hand with the same
    masks at the same moments: states, goals, observations and rewards must stay bit-identical throughout."""
    B, H = 300, 5
    env = mpe.make_env(name, batch_size=B, seed=3, fused=fused, max_episode_steps=H, auto_reset=True)
    ref = mpe.make_env(name, batch_size=B, seed=3, fused=fused)
    assert env.fused == fused
    A = env.n
    rs = np.random.RandomState(1)
    half = torch.as_tensor(rs.rand(B) < 0.5).cuda()
    o_e, o_r = env.reset(), ref.reset()
    finishing = {5: None, 10: ~half, 12: half, 15: ~half}      # step -> worlds that reach the horizon (None = all)
    for t in range(1, 17):
        act = random_actions(env, rs, B)
        o_e, r_e, d_e, _ = env.step(act)
        o_r, r_r, d_r, _ = ref.step(act)
        m = finishing.get(t, False)
        want_done = torch.zeros(B, dtype=torch.bool, device="cuda") if m is False else \
            (torch.ones(B, dtype=torch.bool, device="cuda") if m is None else m)
        for i in range(A):
            assert torch.equal(d_e[i].bool(), want_done), (t, i)
            assert not d_r[i].any()
            assert torch.equal(r_e[i] * torch.ones(B, device="cuda"), r_r[i] * torch.ones(B, device="cuda")), (t, i)
        if m is not False:
            o_r = ref.reset(mask=m) if m is not None else ref.reset()
        if t == 7:                                                # a manual masked reset in the middle of an episode
            o_e, o_r = env.reset(mask=half), ref.reset(mask=half)
        assert np.array_equal(env.world.get_state()[0], ref.world.get_state()[0]), t
        assert np.array_equal(env.world.get_state()[1], ref.world.get_state()[1]), t
        if env.world.choice_i32 is not None:
            assert torch.equal(env.world.choice_i32, ref.world.choice_i32), t
        for i in range(A):
            assert torch.equal(o_e[i], o_r[i]), (t, i)
    want = torch.where(half, torch.tensor(4, device="cuda"), torch.tensor(1, device="cuda")).int()
    assert torch.equal(env.episode_step, want)                   # half finished at 12, the rest at 15; now t = 16

    # without auto_reset: done stays up until the caller resets
    env2 = mpe.make_env(name, batch_size=B, seed=3, fused=fused, max_episode_steps=3)
    env2.reset()
    seen = []
    for t in range(1, 8):
        _, _, d, _ = env2.step(random_actions(env2, rs, B))
        seen.append(bool(d[0].all()) if d[0].any() else False)
        if t == 5:
            env2.reset()
    assert seen == [False, False, True, True, True, False, False]


@pytest.mark.gpu
@pytest.mark.parametrize("name,fused", [("simple_adversary", False), ("simple_reference", False),
                                        ("simple_world_comm", False), ("simple_tag", True)])
def test_graphed_step_replays_the_eager_step(name, fused):
    """GraphedStep: env.step captured once into a HIP graph (the generic path's ~100 launches become one replay).
    Same kernels on the same buffers, so a replay must reproduce the eager step bit-for-bit, across resets too."""
    B = 513
    rs = np.random.RandomState(4)
    env_g = mpe.make_env(name, batch_size=B, seed=8, fused=fused)
    env_e = mpe.make_env(name, batch_size=B, seed=8, fused=fused)
    o_g, o_e = env_g.reset(), env_e.reset()
    gs = mpe.GraphedStep(env_g, random_actions(env_g, rs, B))
    assert np.array_equal(env_g.world.get_state()[0], env_e.world.get_state()[0])     # capture left the state alone
    for t in range(7):
        act = random_actions(env_e, rs, B)
        o_g, r_g, d_g, _ = gs.step(act)
        o_e, r_e, d_e, _ = env_e.step(act)
        for i in range(env_e.n):
            assert torch.equal(o_g[i], o_e[i]), (t, i)
            assert torch.equal(r_g[i] * torch.ones(B, device="cuda"), r_e[i] * torch.ones(B, device="cuda")), (t, i)
            assert torch.equal(d_g[i].bool(), d_e[i].bool())
            c_g, c_e = env_g.world.agents[i].state.c, env_e.world.agents[i].state.c
            assert torch.equal(c_g, c_e), (t, i)
        assert np.array_equal(env_g.world.get_state()[0], env_e.world.get_state()[0]), t
        if t == 3:
            env_g.reset()
            env_e.reset()


@pytest.mark.gpu
def test_graphed_step_and_state_round_trip_with_a_movable_landmark():
    """A movable landmark's velocity is state (core.py:158-169): GraphedStep's warm-up steps must not leave a trace in it,
    and set_state(*get_state()) must restore it (round-3 ADVICE)."""
    B = 256
    rs = np.random.RandomState(9)
    envs = []
    for _ in range(2):
        sc = mpe.scenarios.load("simple_tag.py").Scenario()
        w = sc.make_world(batch_size=B)
        w.seed = 4
        w.landmarks[0].movable, w.landmarks[0].initial_mass = True, 2.0
        env = mpe.MultiAgentEnv(w, sc.reset_world, sc.reward, sc.observation)
        env.reset()
        w.pos.mul_(0.3)                       # crowded: the landmark gets pushed
        envs.append(env)
    env_g, env_e = envs
    assert not env_g.fused
    for e in envs:
        for _ in range(3):
            e.step(random_actions(e, np.random.RandomState(1), B))
    p0, v0 = env_g.world.get_state()
    assert v0.shape[1] == len(env_g.world.entities) and np.abs(v0[:, len(env_g.world.agents)]).max() > 0    # the landmark moves
    gs = mpe.GraphedStep(env_g, random_actions(env_g, rs, B))
    p1, v1 = env_g.world.get_state()
    assert np.array_equal(p0, p1) and np.array_equal(v0, v1)            # the warm-up steps did not happen, landmark rows included
    for t in range(4):
        act = random_actions(env_e, rs, B)
        gs.step(act)
        env_e.step(act)
        assert torch.equal(env_g.world.pos, env_e.world.pos) and torch.equal(env_g.world._vel_all, env_e.world._vel_all), t
    p, v = env_e.world.get_state()
    env_e.world.set_state(np.zeros_like(p), None)
    env_e.world.set_state(p, v)
    assert torch.equal(env_g.world.pos, env_e.world.pos) and torch.equal(env_g.world._vel_all, env_e.world._vel_all)


CUSTOM = [("simple_spread", {}), ("simple_spread", {"num_agents": 8}), ("simple_spread", {"num_agents": 40, "num_landmarks": 7}),
          ("simple_tag", {}), ("simple_adversary", {}), ("simple_push", {}), ("simple_world_comm", {}), ("simple", {})]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", CUSTOM, ids=["%s%s" % (n, "-".join(map(str, k.values()))) for n, k in CUSTOM])
@pytest.mark.parametrize("trial", [0, 1])
def test_customised_entity_constants_fused_equals_generic(name, kw, trial):
    """The kernels read sizes, masses, collide flags, speed limits and action gains from the descriptor at run time
    (the reference keeps them as plain attributes anyone may change after make_world, core.py:27-51).  Randomise
    them on a built-in scenario and hold the fused kernel to the generic path (torch callbacks written from the
    reference + mpe_world_step) on crowded random worlds."""
    B = 2048
    rs = np.random.RandomState(100 * trial + len(name))

    def build(fused):
        sc = mpe.scenarios.load(name + ".py").Scenario()
        w = sc.make_world(batch_size=B, **kw)
        r = np.random.RandomState(7 + trial)                    # the same customisation for both envs
        for e in w.entities:
            e.size = float(r.uniform(0.03, 0.2))
            e.initial_mass = float(r.uniform(0.5, 2.0))
            if r.rand() < 0.3:
                e.collide = not e.collide
        for a in w.agents:
            a.max_speed = None if r.rand() < 0.4 else float(r.uniform(0.4, 1.5))
            a.accel = None if r.rand() < 0.4 else float(r.uniform(2.0, 6.0))
        if trial == 1:                                           # World constants too (core.py:94-99)
            w.dt, w.damping = 0.05, 0.4
            w.contact_force, w.contact_margin = 250.0, 4e-3
        w.seed = 5
        w.rng_mode = "device"
        sc.reset_world(w)
        env = mpe.MultiAgentEnv(w, sc.reset_world, sc.reward, sc.observation, fused=fused)
        env.scenario = sc
        return env
    ef, eg = build(True), build(False)
    A, E = len(ef.world.agents), len(ef.world.entities)
    pos = rs.uniform(-1, 1, (B, E, 2)).astype(np.float32)
    pos[::2] *= 0.35
    vel = rs.uniform(-0.8, 0.8, (B, A, 2)).astype(np.float32)
    pops = ef.world.choice_pops
    choice = np.stack([rs.randint(0, n, size=B) for n in pops], axis=1) if pops else np.zeros((B, 0), np.int64)
    for env in (ef, eg):
        env.world.set_state(pos, vel)
        set_choices(env, choice)
    act = random_actions(ef, rs, B)
    of, rf, _, _ = ef.step(act)
    og, rg, _, _ = eg.step(act)
    pf, vf = ef.world.get_state()
    pg, vg = eg.world.get_state()
    close(pf, pg, what="pos")
    close(vf, vg, what="vel")
    near = np.zeros(B, bool)                                     # worlds with a pair within 1e-5 of touching: the strict
    for a_ in range(E):                                          # `<` of the collision counts may flip between fp32 paths
        for b_ in range(a_ + 1, E):
            dist = np.linalg.norm(pf[:, a_] - pf[:, b_], axis=1)
            near |= np.abs(dist - (ef.world.entities[a_].size + ef.world.entities[b_].size)) < 1e-5
    for i in range(A):
        close(np_(of[i]), np_(og[i]), what="obs%d" % i)
        close((np_(rf[i]) * np.ones(B))[~near], (np_(rg[i]) * np.ones(B))[~near], what="rew%d" % i)


@pytest.mark.gpu
def test_shared_reward_can_be_flipped_on_a_live_env():
    """environment.py:100-102 reads self.shared_reward at every step: flipping it changes what step() returns.  The
    fused kernels implement the scenario's own setting; the other one is served by the generic path."""
    B = 500
    rs = np.random.RandomState(0)
    tag, twin = mpe.make_env("simple_tag", batch_size=B, seed=1), mpe.make_env("simple_tag", batch_size=B, seed=1)
    tag.reset(), twin.reset()
    pos, vel = twin.world.get_state()
    pos[::2] *= 0.2
    tag.world.set_state(pos, vel), twin.world.set_state(pos, vel)
    tag.shared_reward = True
    assert not tag.fused and twin.fused
    act = random_actions(twin, rs, B)
    _, r_sum, _, _ = tag.step(act)
    _, r_own, _, _ = twin.step(act)
    total = sum(np_(r).astype(np.float64) for r in r_own)
    assert np.abs(total).max() > 0
    for r in r_sum:
        close(np_(r), total)
    spread = mpe.make_env("simple_spread", batch_size=B, seed=1)
    twin = mpe.make_env("simple_spread", batch_size=B, seed=1)
    spread.shared_reward = False
    _, r_ind, _, _ = spread.step(random_actions(twin, np.random.RandomState(3), B))
    _, r_sh, _, _ = twin.step(random_actions(twin, np.random.RandomState(3), B))
    close(sum(np_(r).astype(np.float64) for r in r_ind), np_(r_sh[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [{}, {"num_agents": 20}], ids=["n3", "n20"])
def test_refresh_constants_on_a_live_env(kw):
    """Constants are snapshotted into the kernel descriptor when the env is built; refresh_constants() re-reads them."""
    B = 300
    rs = np.random.RandomState(0)
    env = mpe.make_env("simple_spread", batch_size=B, seed=2, **kw)
    gen = mpe.make_env("simple_spread", batch_size=B, seed=2, fused=False, **kw)
    act = random_actions(env, rs, B)
    env.step(act), gen.step(act)                      # buffers exist, descriptor in use
    for e in (env, gen):
        for k, a in enumerate(e.world.agents):
            a.size = 0.05 + 0.01 * (k % 5)
            a.max_speed = 0.7
        e.world.damping = 0.5
        e.refresh_constants()
        e.world.set_state(*env.world.get_state())
    o1, r1, _, _ = env.step(act)
    o2, r2, _, _ = gen.step(act)
    assert np.abs(env.world.get_state()[1]).max() <= 0.7 * (1 + 1e-5)
    close(env.world.get_state()[0], gen.world.get_state()[0])
    close(np_(o1[0]), np_(o2[0]))
    close(np_(r1[0]), np_(r2[0]) * np.ones(B))


@pytest.mark.gpu
@pytest.mark.parametrize("name,fused", [(n, False) for n in NAMES] + [(n, True) for n in FUSED],
                         ids=[n + "-generic" for n in NAMES] + [n + "-fused" for n in FUSED])
def test_customised_constants_against_reference_golden(name, fused, golden):
    """tests/golden/f3c_*.npz: the reference stepped after its sizes, masses, collide flags, speed limits, action gains
    and dt / damping / contact constants were changed (gen_golden_custom.py --f3).  Same assignments here, both paths."""
    g = golden("f3c_" + name)
    W, T = len(g["seeds"]), g["rew"].shape[0]
    sc = mpe.scenarios.load(name + ".py").Scenario()
    w = sc.make_world(batch_size=W)
    for k, e in enumerate(w.entities):
        e.size, e.initial_mass, e.collide = float(g["c_size"][k]), float(g["c_mass"][k]), bool(g["c_collide"][k])
    for k, a in enumerate(w.agents):
        a.max_speed = None if g["c_max_speed"][k] < 0 else float(g["c_max_speed"][k])
        a.accel = None if g["c_accel"][k] < 0 else float(g["c_accel"][k])
    w.dt, w.damping, w.contact_force, w.contact_margin = [float(x) for x in g["c_world"]]
    w.rng_mode = "device"
    sc.reset_world(w)
    env = mpe.MultiAgentEnv(w, sc.reset_world, sc.reward, sc.observation, fused=fused)
    env.scenario = sc
    assert env.fused == fused
    A = env.n
    set_choices(env, g["choice"])
    # worlds where a pair sits within 1e-6 of touching: collision-count rewards may flip between fp32 and fp64
    sizes = np.array([e.size for e in w.entities])
    for t in range(T):
        if t == 0:
            w.set_state(g["pos0"], g["vel0"])
            set_comm(env, g, -1)
        else:
            w.set_state(g["pos"][t - 1], g["vel"][t - 1])
            set_comm(env, g, t - 1)
        act = [torch.as_tensor(g["act%d" % i][t], dtype=torch.float32).cuda() for i in range(A)]
        obs_n, rew_n, _, _ = env.step(act)
        pos, vel = w.get_state()
        close(pos, g["pos"][t], what="t=%d pos" % t)
        close(vel, g["vel"][t], what="t=%d vel" % t)
        d = np.linalg.norm(g["pos"][t][:, :, None, :] - g["pos"][t][:, None, :, :], axis=-1)
        ok = ~(np.abs(d - (sizes[:, None] + sizes[None, :])[None]) < 1e-6).any(axis=(1, 2))
        for i in range(A):
            close(np_(obs_n[i]), g["obs%d" % i][t], what="t=%d obs%d" % (t, i))
            close((np_(rew_n[i]) * np.ones(W))[ok], g["rew"][t][:, i][ok], what="t=%d rew%d" % (t, i))
            close(np_(w.agents[i].state.c), g["c%d" % i][t], what="t=%d c%d" % (t, i))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["simple_spread", "simple_reference"])
def test_action_and_comm_noise_follow_the_reference_numpy_stream(name, golden):
    """Agent.u_noise / c_noise (core.py:138,176) are drawn from the process-global np.random inside World.step.  In
    reference-compatibility mode `np.random.seed(s); env.reset(); env.step(...)` must reproduce the reference's noisy
    trajectory (tests/golden/noise_*.npz, recorded from the reference) -- and leave the stream where the reference
    leaves it: every world's reset below comes out of the same stream the previous episode's noise came from."""
    g = golden("noise_" + name)
    env = mpe.make_env(name)
    assert env.fused
    for a, un, cn in zip(env.world.agents, g["u_noise"], g["c_noise"]):   # set after make_env, as a reference user would
        a.u_noise = float(un) if un else None
        a.c_noise = float(cn) if cn else None
    T, W, A = g["rew"].shape
    for w in range(W):
        np.random.seed(int(g["seeds"][w]))
        env.reset()
        assert not env.fused or w == 0       # the first step notices the noise and leaves the fused path
        pos, vel = env.world.get_state()
        close(pos[0], g["pos0"][w], what="reset pos")
        for t in range(T):
            if t:   # teacher-forced; the noise stream runs on
                env.world.set_state(g["pos"][t - 1, w][None], g["vel"][t - 1, w][None])
            obs, rew, done, info = env.step([g["act%d" % i][t, w] for i in range(A)])
            assert not env.fused
            pos, vel = env.world.get_state()
            close(pos[0], g["pos"][t, w], what="w=%d t=%d pos" % (w, t))
            close(vel[0], g["vel"][t, w], what="w=%d t=%d vel" % (w, t))
            for i in range(A):
                close(obs[i], g["obs%d" % i][t, w], what="w=%d t=%d obs%d" % (w, t, i))
                close(np_(env.world.agents[i].state.c)[0], g["c%d" % i][t, w], what="w=%d t=%d c%d" % (w, t, i))
            close(np.array(rew), g["rew"][t, w], what="w=%d t=%d rew" % (w, t))


@pytest.mark.gpu
def test_constants_assigned_on_a_live_env_are_honoured_without_a_refresh_call():
    """The reference reads sizes, masses, speed limits, dt ... on every step (core.py:117-196), so assigning one on a
    live env takes effect at the next step.  Here the kernels' descriptor is a snapshot; assignments bump a version the
    step compares, so the same holds -- fused and generic paths."""
    B = 512
    rs = np.random.RandomState(4)
    pos = (rs.uniform(-1, 1, (B, 6, 2)) * 0.3).astype(np.float32)
    vel = rs.uniform(-1, 1, (B, 3, 2)).astype(np.float32)
    act = torch.as_tensor(np.eye(5, dtype=np.float32)[rs.randint(0, 5, size=(3, B))]).cuda()

    def edit(env):
        env.world.agents[1].size = 0.21
        env.world.agents[2].max_speed = 0.3
        env.world.agents[0].initial_mass = 2.5
        env.world.damping = 0.4
    for fused in (True, False):
        live = mpe.make_env("simple_spread", batch_size=B, fused=fused)
        live.world.set_state(pos, vel)
        live.step(act if fused else [act[i] for i in range(3)])      # descriptor snapshotted with the default constants
        edit(live)
        live.world.set_state(pos, vel)
        o1, r1, _, _ = live.step(act if fused else [act[i] for i in range(3)])
        fresh = mpe.make_env("simple_spread", batch_size=B, fused=fused)
        edit(fresh)
        fresh.world.set_state(pos, vel)
        o2, r2, _, _ = fresh.step(act if fused else [act[i] for i in range(3)])
        assert torch.equal(live.world.pos, fresh.world.pos) and torch.equal(live.world.vel, fresh.world.vel)
        for i in range(3):
            assert torch.equal(o1[i], o2[i]) and torch.equal(r1[i], r2[i])
        untouched = mpe.make_env("simple_spread", batch_size=B, fused=fused)
        untouched.world.set_state(pos, vel)
        untouched.step(act if fused else [act[i] for i in range(3)])
        assert not torch.equal(untouched.world.vel, fresh.world.vel)     # the edits do change the physics


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["simple_adversary", "simple_crypto", "simple_world_comm"])
def test_benchmark_data_of_the_f3_scenarios_rides_on_the_fused_step(name):
    """make_env(name, benchmark=True): simple_adversary's squared distances and simple_world_comm's contact counts come out
    of the SAME launch as the step (round 3: agent waves / reward wave write them; no Python evaluation); simple_crypto's
    benchmark_data is (agent.state.c, goal colour) -- views of what the env holds, evaluated in Python without a launch.
    Same info as the all-Python generic path."""
    B = 500
    ef = mpe.make_env(name, benchmark=True, batch_size=B, seed=2)
    eg = mpe.make_env(name, benchmark=True, batch_size=B, seed=2, fused=False)
    if not hasattr(ef.scenario, "benchmark_data"):
        pytest.skip("no benchmark_data in this scenario")
    assert ef.fused and not ef._py_reward and not eg.fused
    assert ef._py_info == (name == "simple_crypto")      # the others: written by the step's own launch
    eg.world.pos.copy_(ef.world.pos)
    eg.world.vel.copy_(ef.world.vel)
    if ef.world.choice_i32 is not None:
        eg.world.choice_i32.copy_(ef.world.choice_i32)
        eg.scenario._apply(eg.world)
    rs = np.random.RandomState(0)
    for t in range(3):
        acts = random_actions(ef, rs, B)
        of, rf, _, inf_f = ef.step(acts)
        og, rg, _, inf_g = eg.step(acts)
        for i in range(ef.n):
            close(np_(of[i]), np_(og[i]), what="obs%d" % i)
            close(np_(rf[i]) * np.ones(B), np_(rg[i]) * np.ones(B), what="rew%d" % i)
            a, b = inf_f["n"][i], inf_g["n"][i]
            a = a if isinstance(a, (tuple, list)) else (a,)
            b = b if isinstance(b, (tuple, list)) else (b,)
            assert len(a) == len(b)
            for x, y in zip(a, b):
                x, y = np_(x).astype(np.float64), np_(y).astype(np.float64)
                close(np.broadcast_to(x, np.broadcast(x, y).shape), np.broadcast_to(y, np.broadcast(x, y).shape), what="info%d" % i)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["simple_adversary", "simple_world_comm"])
def test_fused_benchmark_data_against_reference_golden(name, golden):
    """benchmark_data of simple_adversary (squared distances: simple_adversary.py:57-67) and simple_world_comm (an
    adversary's contacts with good agents: simple_world_comm.py:115-124) as the reference returned them
    (tests/golden/f3_*.npz, info_* arrays), from the fused step's own launch, teacher-forced: floats at 1e-5, the counts
    exact outside a 1e-6 band around the contact threshold."""
    from oracle import spec as ospec
    from oracle.mpe_f3 import knife_edge
    g = golden("f3_" + name)
    W, T = len(g["seeds"]), g["rew"].shape[0]
    env = mpe.make_env(name, batch_size=W, benchmark=True)
    assert env.fused and not env._py_info
    A = env.n
    set_choices(env, g["choice"])
    for t in range(T):
        env.world.set_state(g["pos0"] if t == 0 else g["pos"][t - 1], g["vel0"] if t == 0 else g["vel"][t - 1])
        set_comm(env, g, t - 1)
        act = [torch.as_tensor(g["act%d" % i][t], dtype=torch.float32).cuda() for i in range(A)]
        _, _, _, info = env.step(act)
        inf = info["n"]
        if name == "simple_adversary":
            close(np_(inf[0]), g["info_adv"][t][:, 0], what="t=%d adversary" % t)
            for k in range(1, A):
                assert isinstance(inf[k], tuple) and len(inf[k]) == g["info_good"].shape[-1]
                for j, x in enumerate(inf[k]):
                    close(np_(x), g["info_good"][t][:, k - 1, j], what="t=%d good %d datum %d" % (t, k, j))
        else:
            ok = ~knife_edge(ospec.by_name(name), g["pos"][t], 1e-6)
            got = np.stack([np_(x) for x in inf], axis=1)
            assert got.dtype == np.int32 and np.array_equal(got[ok], g["info_collisions"][t][ok]) and ok.mean() > 0.99
            assert g["info_collisions"][t].sum() > 0 or t > 0
