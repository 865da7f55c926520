"""The oracle against the reference on worlds the other fixtures do not hold.

tests/golden/*.npz pin the oracle to recordings; this test closes the remaining gap ("the oracle fits the fixtures") with worlds
recorded from the unmodified reference on seeds of their own (tests/golden/live_*.npz, written by tests/golden/gen_golden_live.py
with the recorders that made the other fixtures and the shape-only gym stub), replayed through the fp64 batched oracle, the C
restatement, the per-object loop port and the host callbacks of the six other scenarios.
"""
import os

import numpy as np
import pytest

from oracle import spec as ospec
from oracle.mpe_batched import BatchedOracle, seeded_initial_state
from oracle.mpe_loop import LoopEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = 1e-12


def _live(name):
    return dict(np.load(os.path.join(GOLDEN, "live_" + name + ".npz")))


def _base_seed():
    """The day stamp the recorded worlds were drawn for (tests/golden/gen_golden_live.py)."""
    return int(_live("simple")["live_seed"])


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    scale = np.maximum(1.0, np.abs(b))
    assert np.all(np.abs(a - b) <= TOL * scale), "max scaled err %.3e (worlds of day stamp %d)" % (
        float(np.max(np.abs(a - b) / scale)), _base_seed())


@pytest.fixture(scope="module")
def fresh():
    return _live


CASES = [("simple", ospec.simple(), False), ("simple_spread", ospec.simple_spread(3), True), ("simple_tag", ospec.simple_tag(), True),
         ("simple_spread_n7", ospec.simple_spread(7), True)]


@pytest.mark.parametrize("name,spec,bench", CASES, ids=[c[0] for c in CASES])
def test_batched_oracle_replays_fresh_reference_worlds(name, spec, bench, fresh):
    g = fresh(name)
    T, W, A = g["rew"].shape
    orc = BatchedOracle(spec, W, np.float64, benchmark=bench)
    orc.set_state(g["pos0"], g["vel0"])
    for i, o in enumerate(orc.observe()):
        _close(o, g["obs_reset%d" % i])
    for t in range(T):
        obs, rew, done, info = orc.step(np.transpose(g["act"][t], (1, 0, 2)))
        _close(orc.pos, g["pos"][t])
        _close(orc.vel, g["vel"][t])
        for i in range(A):
            _close(obs[i], g["obs%d" % i][t])
        _close(rew.T, g["rew"][t])
        assert not done.any() and not g["done"][t].any()
        if "info_collisions" in g:
            assert np.array_equal(info["collisions"].T, g["info_collisions"][t])
        if "info_occupied" in g:
            assert np.array_equal(info["occupied_landmarks"].T, g["info_occupied"][t])
            _close(info["min_dists"].T, g["info_min_dists"][t])


@pytest.mark.parametrize("name,spec,bench", CASES, ids=[c[0] for c in CASES])
def test_c_restatement_replays_fresh_reference_worlds(name, spec, bench, fresh):
    """oracle/mpe_oracle.c (bench.py's `c_port`), teacher-forced from the reference's own states."""
    from oracle import build_c
    g = fresh(name)
    T, W, A = g["rew"].shape
    for t in range(T):
        p0 = g["pos0"] if t == 0 else g["pos"][t - 1]
        v0 = g["vel0"] if t == 0 else g["vel"][t - 1]
        pos, vel, obs, rew, col = build_c.step_batch(spec, p0, v0, g["act"][t], threads=2)
        _close(pos, g["pos"][t])
        _close(vel, g["vel"][t])
        for i in range(A):
            _close(obs[i], g["obs%d" % i][t])
        _close(rew, g["rew"][t])
        if "info_collisions" in g:
            assert np.array_equal(col, g["info_collisions"][t])


def test_seeded_resets_of_fresh_worlds(fresh):
    """reset_world consumes the global MT19937 stream in the reference's order: the un-squeezed worlds' initial
    states follow from their seeds alone."""
    for name, spec, every in (("simple", ospec.simple(), 0), ("simple_spread", ospec.simple_spread(3), 3), ("simple_tag", ospec.simple_tag(), 3)):
        g = fresh(name)
        plain = [w for w in range(len(g["seeds"])) if not every or w % every != every - 1]
        pos, vel = seeded_initial_state(spec, g["seeds"][plain])
        assert np.array_equal(pos, g["pos0"][plain]) and np.array_equal(vel, g["vel0"][plain])


def test_loop_port_replays_fresh_reference_worlds(fresh):
    """oracle/mpe_loop.py (bench.py's CPU baseline, kind "port") on the same fresh worlds, one world at a time."""
    for name, spec in (("simple_spread", ospec.simple_spread(3)), ("simple_tag", ospec.simple_tag())):
        g = fresh(name)
        T, W, A = g["rew"].shape
        for w in range(0, W, 2):
            env = LoopEnv(spec)
            env.set_state(g["pos0"][w], g["vel0"][w])
            for t in range(T):
                obs, rew, done, _ = env.step([g["act"][t, w, i] for i in range(A)])
                for i in range(A):
                    _close(obs[i], g["obs%d" % i][t, w])
                _close(np.array(rew, dtype=np.float64), g["rew"][t, w])


# ---- the six other scenarios: the product's own reset_world / observation / reward (torch, on the CPU) against the
#      reference on the recorded worlds -- the check tests/test_f3_scenarios.py makes against the committed f3_*.npz, on other seeds ---
@pytest.fixture(scope="module")
def fresh_f3():
    return _live


def test_host_callbacks_of_the_other_six_scenarios_on_fresh_reference_worlds(fresh_f3):
    import test_f3_scenarios as f3
    for name in f3.NAMES:
        f3.test_reset_and_callbacks_match_reference_on_cpu(name, fresh_f3)


def test_f3_oracle_replays_fresh_reference_worlds(fresh_f3):
    """oracle/mpe_f3.py (the fp64 restatement the GPU tests compare the six other scenarios' fused kernels with) against
    the reference on 64 recorded worlds per scenario, staged like the fixtures, whole trajectories at 1e-12, and
    the seeded resets (np.random.choice picks, then agents, then landmarks)."""
    import test_oracle_golden as tg
    from oracle.mpe_f3 import seeded_initial_state_f3
    for name in tg.F3:
        g = fresh_f3("f3_" + name)
        spec = ospec.by_name(name)
        tg._replay_f3(spec, g)
        plain = np.flatnonzero(~g["staged"])
        pos, vel, choice = seeded_initial_state_f3(spec, g["seeds"])
        assert np.array_equal(choice, g["choice"]), "day stamp %d" % _base_seed()
        assert np.array_equal(pos[plain], g["pos0"][plain]), "day stamp %d" % _base_seed()


def test_f3_oracle_at_other_team_sizes_replays_fresh_reference_worlds(fresh_f3):
    """The team-size variants of simple_adversary / simple_world_comm (tests/golden/gen_golden_shapes.py) on fresh seeds."""
    import test_oracle_golden as tg
    from oracle.mpe_f3 import seeded_initial_state_f3
    for name, A, nadv in tg.SHAPES:
        g = fresh_f3("shape_%s_%d_%d" % (name, A, nadv))
        spec = tg.shape_spec(name, A, nadv)
        tg._replay_f3(spec, g)
        plain = np.flatnonzero(~g["staged"])
        pos, vel, choice = seeded_initial_state_f3(spec, g["seeds"])
        assert np.array_equal(choice, g["choice"]), "day stamp %d" % _base_seed()
        assert np.array_equal(pos[plain], g["pos0"][plain]), "day stamp %d" % _base_seed()
