"""CPU-only checks (no GPU, no compute calls): the C-ABI library loads and exports every symbol
include/mpe_hip.h declares, struct layouts agree, argument validation works, and the host-side
mirror of the reference API (spaces, observation widths, scenario constants, state views, the
NumPy-order reset) behaves like the reference."""
import ctypes as C
import os
import sys
import re

import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi, core, spaces
from oracle import spec as ospec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "mpe_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|size_t|const char \*)\s*\**\s*(mpe_\w+)\s*\(", hdr, flags=re.M))
    assert len(declared) >= 15
    assert declared == set(_abi.EXPORTS), declared ^ set(_abi.EXPORTS)
    raw = C.CDLL(_abi.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    L = _abi.lib()
    assert L.mpe_abi_version() == _abi.MPE_ABI_VERSION
    assert L.mpe_sizeof_desc() == C.sizeof(_abi.MpeScenarioDesc)
    assert L.mpe_sizeof_buffers() == C.sizeof(_abi.MpeBuffers)


def test_header_constants_match_binding():
    hdr = open(os.path.join(ROOT, "include", "mpe_hip.h")).read()
    assert int(re.search(r"#define MPE_MAX_ENTITIES (\d+)", hdr).group(1)) == _abi.MPE_MAX_ENTITIES
    assert int(re.search(r"#define MPE_ABI_VERSION (\d+)", hdr).group(1)) == _abi.MPE_ABI_VERSION
    assert int(re.search(r"#define MPE_ACTION_DIM (\d+)", hdr).group(1)) == _abi.MPE_ACTION_DIM


def test_argument_validation_without_a_gpu():
    L = _abi.lib()
    b = _abi.MpeBuffers()
    d = _abi.MpeScenarioDesc()
    assert L.mpe_step(None, C.byref(b), 4, None) == -1
    assert b"desc is NULL" in L.mpe_last_error()
    d.kind, d.n_agents, d.n_landmarks = _abi.MPE_SCN_SPREAD, 0, 3
    assert L.mpe_step(C.byref(d), C.byref(b), 4, None) == -1
    d.n_agents = 3
    for e in range(3):
        d.mass[e] = 1.0
    d.dim_c = 2
    assert L.mpe_step(C.byref(d), None, 4, None) == -1
    assert L.mpe_step(C.byref(d), C.byref(b), 4, None) == -1 and b"pos" in L.mpe_last_error()
    d.movable[4] = 1                                  # a movable landmark
    assert L.mpe_fill_obs_layout(C.byref(d)) == -2
    d.movable[4] = 0
    d.kind = 99
    assert L.mpe_fill_obs_layout(C.byref(d)) == -1
    assert L.mpe_random_actions(None, None, 3, 8, 0, 0, 0, None) == -1


@pytest.mark.parametrize("name,kw,mk", [
    ("simple", {}, lambda: ospec.simple()),
    ("simple_spread", {}, lambda: ospec.simple_spread(3)),
    ("simple_spread", {"num_agents": 64}, lambda: ospec.simple_spread(64)),
    ("simple_spread", {"num_agents": 5, "num_landmarks": 2}, lambda: ospec.simple_spread(5, 2)),
    ("simple_tag", {}, lambda: ospec.simple_tag()),
    ("simple_tag", {"num_adversaries": 4, "num_good_agents": 2, "num_landmarks": 3}, lambda: ospec.simple_tag(4, 2, 3)),
])
def test_env_construction_matches_oracle_constants(name, kw, mk):
    """The product's scenario constants (read off its own make_world) agree with the oracle's
    independent transcription of the reference's make_world, and the C side's obs layout agrees
    with the oracle's obs widths."""
    spec = mk()
    env = mpe.make_env(name, batch_size=4, device="cpu", **kw)
    assert env.n == spec.n_agents and env.fused
    assert [s.shape[0] for s in env.observation_space] == spec.obs_dims()
    assert all(isinstance(a, spaces.Discrete) and a.n == 5 for a in env.action_space)
    assert env.shared_reward == spec.collaborative
    d = env._desc
    E = spec.n_entities
    assert (d.n_agents, d.n_landmarks, d.dim_c) == (spec.n_agents, spec.n_landmarks, spec.dim_c)
    assert np.allclose(list(d.size)[:E], spec.size)
    assert list(d.movable)[:E] == [int(x) for x in spec.movable]
    assert list(d.collide)[:E] == [int(x) for x in spec.collide]
    assert np.allclose(list(d.accel)[:spec.n_agents], [5.0 if a is None else a for a in spec.accel])
    assert np.allclose(list(d.max_speed)[:spec.n_agents], [-1.0 if m is None else m for m in spec.max_speed])
    assert (d.dt, d.damping, d.contact_force) == (np.float32(0.1), 0.25, 100.0)
    assert abs(d.contact_margin - 1e-3) < 1e-9
    n = _abi.lib().mpe_fill_entity_table(C.byref(d), None)
    assert n == 6 * E


def test_no_cpu_fallback():
    env = mpe.make_env("simple_spread", batch_size=4, device="cpu")
    with pytest.raises(_abi.MpeError, match="no CPU fallback"):
        env.reset()
    with pytest.raises(_abi.MpeError, match="no CPU fallback"):
        env.step(torch.zeros(3, 4, 5))
    with pytest.raises(_abi.MpeError, match="no CPU fallback"):
        env.world.step()


def test_state_views_are_live():
    sc = mpe.scenarios.load("simple_tag.py").Scenario()
    w = sc.make_world(batch_size=5, device="cpu")
    a0 = w.agents[0]
    assert a0.state.p_pos.shape == (5, 2)
    a0.state.p_pos = torch.arange(10.0).reshape(5, 2)
    assert torch.equal(w.pos[0, 0], torch.tensor([0.0, 2, 4, 6, 8]))       # SoA storage, batch innermost
    w.pos[0, 1, 3] = -7.0
    assert a0.state.p_pos[3, 1] == -7.0                                      # a view, not a copy
    a0.state.p_vel = np.array([1.0, 2.0])                                    # broadcast over the batch
    assert torch.equal(w.vel[0, :, 2], torch.tensor([1.0, 2.0]))
    assert w.landmarks[0].state.p_vel.abs().sum() == 0
    pos, vel = w.get_state()
    w.set_state(pos * 2, vel)
    assert torch.allclose(w.agents[0].state.p_pos, torch.as_tensor(pos[:, 0] * 2))
    assert len(w.entities) == 6 and len(w.policy_agents) == 4 and w.scripted_agents == []


def test_numpy_order_reset_matches_reference(golden):
    """Reference-compatibility mode draws from the global np.random in the reference's order, so
    seeding right before reset gives the reference's own initial state (golden pos0)."""
    for name in ("simple", "simple_tag"):
        g = golden(name)
        env = mpe.make_env(name, device="cpu")           # compat mode: B=1, rng_mode numpy
        assert env.world.rng_mode == "numpy" and env.numpy_io
        for w in (0, 1, 3):
            np.random.seed(int(g["seeds"][w]))
            env.scenario.reset_world(env.world)
            pos, vel = env.world.get_state()
            assert np.array_equal(pos[0], g["pos0"][w].astype(np.float32))
            assert not vel.any()
    # batched per-world seeds
    g = golden("simple_spread")
    env = mpe.make_env("simple_spread", batch_size=4, device="cpu")
    env.world.reset_from_numpy_seeds([int(g["seeds"][w]) for w in (0, 1, 3, 4)])
    pos, _ = env.world.get_state()
    assert np.array_equal(pos, g["pos0"][[0, 1, 3, 4]].astype(np.float32))


def test_scenario_loader_and_generic_detection(tmp_path):
    assert mpe.scenarios.load("simple.py").Scenario.kind == _abi.MPE_SCN_SIMPLE
    with pytest.raises(FileNotFoundError):
        mpe.scenarios.load("simple_no_such_scenario.py")
    assert mpe.scenarios.load("simple_crypto.py").Scenario.kind == _abi.MPE_SCN_CRYPTO
    # a subclass that overrides REWARD keeps the kernel for action decode + World.step + observation rows and gets its
    # own reward evaluated in Python on the post-step world (partial fusion); one that overrides OBSERVATION keeps it for
    # action decode + World.step + reward and gets its own rows evaluated in Python; overriding both leaves the kernel
    Base = mpe.scenarios.load("simple_spread.py").Scenario

    class MyReward(Base):
        def reward(self, agent, world):
            return -agent.state.p_pos.abs().sum(dim=1)

    class MyObs(Base):
        def observation(self, agent, world):
            return Base.observation(self, agent, world)[:, :7]

    class Both(MyReward, MyObs):
        pass
    sc = MyReward()
    w = sc.make_world(batch_size=3, device="cpu")
    env = mpe.MultiAgentEnv(w, sc.reset_world, sc.reward, sc.observation)
    assert env.fused and env._py_reward and not env._py_obs and not env._py_done and not env._py_info
    assert env.observation_space[0].shape == (18,)
    env = mpe.MultiAgentEnv(w, sc.reset_world, sc.reward, sc.observation, done_callback=lambda agent, world: False)
    assert env.fused and env._py_done
    sc = MyObs()
    w = sc.make_world(batch_size=3, device="cpu")
    env = mpe.MultiAgentEnv(w, sc.reset_world, sc.reward, sc.observation)
    assert env.fused and env._py_obs and not env._py_reward and env.observation_space[0].shape == (7,)
    sc = Both()
    w = sc.make_world(batch_size=3, device="cpu")
    env = mpe.MultiAgentEnv(w, sc.reset_world, sc.reward, sc.observation)
    assert not env.fused and not env._py_reward and not env._py_obs and env.observation_space[0].shape == (7,)
    with pytest.raises(_abi.MpeError):
        mpe.MultiAgentEnv(w, sc.reset_world, sc.reward, sc.observation, fused=True)
    env = mpe.MultiAgentEnv(w, sc.reset_world, sc.reward, lambda agent, world: agent.state.p_pos)   # not the scenario's method
    assert not env.fused and env.observation_space[0].shape == (2,)


def test_fused_kernels_cover_the_reference_shapes_and_other_shapes_fall_back():
    """mpe_step_supported: the nine scenarios at the reference's team sizes and simple_spread at every size have a fused
    kernel; other shapes of the f3 scenarios keep their torch callbacks around mpe_world_step (the env says so up
    front instead of failing at the first step)."""
    def env_of(name, **kw):
        sc = mpe.scenarios.load(name + ".py").Scenario()
        w = sc.make_world(batch_size=2, device="cpu", **kw)
        return mpe.MultiAgentEnv(w, sc.reset_world, sc.reward, sc.observation)
    for name in ("simple", "simple_spread", "simple_tag", "simple_adversary", "simple_push", "simple_speaker_listener",
                 "simple_reference", "simple_crypto", "simple_world_comm"):
        assert env_of(name).fused, name
    for n in (2, 6, 7, 16, 33, 64, 100, 256):
        assert env_of("simple_spread", num_agents=n).fused, n
    big = env_of("simple_tag", num_adversaries=40, num_good_agents=30, num_landmarks=20)   # any team sizes: wave-per-world kernel
    assert big.fused and big.observation_space[0].shape == (4 + 40 + 138 + 60,)
    assert big.observation_space[69].shape == (4 + 40 + 138 + 58,)
    assert env_of("simple_tag", num_adversaries=2).fused
    # simple_adversary / simple_world_comm (callbacks written for any team size): the reference's team sizes have a kernel of
    # their own, every other -- round 3's grid of 19 and beyond, up to 64 entities -- steps as World.step + the scenario's row
    # program (rowspec.builtin_program): two launches, no instantiation per shape
    from oracle.spec import TEAM_SIZE_VARIANTS
    for name, A, nadv in TEAM_SIZE_VARIANTS:
        if name == "simple_adversary":
            e = env_of(name, num_agents=A, num_adversaries=nadv)
            assert e.fused and e.n == A and e._prog is not None, (name, A, nadv)
        else:
            good, adv = A - nadv, nadv
            e = env_of(name, num_good_agents=good, num_adversaries=adv)
            assert e.fused and e.n == A and e._prog is not None, (good, adv)
            assert e.observation_space[0].shape == (4 + 10 + 2 * (A - 1) + 2 * good + 2 + 4,)
            assert e.observation_space[adv].shape == (4 + 10 + 2 * (A - 1) + 2 + 2 * (good - 1),)
    assert env_of("simple_adversary").fused and env_of("simple_adversary")._prog is None          # the reference's shape: its own kernel
    for e in (env_of("simple_adversary", num_agents=7, num_adversaries=3), env_of("simple_world_comm", num_good_agents=5, num_adversaries=6),
              env_of("simple_adversary", num_agents=30, num_adversaries=9), env_of("simple_world_comm", num_good_agents=20, num_adversaries=12)):
        assert e.fused and e._prog is not None and e._kind == _abi.MPE_SCN_GENERIC
    assert not env_of("simple_adversary", num_agents=40, num_adversaries=3).fused            # 79 entities: past the row programs' 64
    d = big.world.scenario_desc(_abi.MPE_SCN_GENERIC)
    assert _abi.lib().mpe_step_supported(C.byref(d)) == 0
    d = _abi.MpeScenarioDesc()
    d.kind, d.n_agents = 99, 1
    assert _abi.lib().mpe_step_supported(C.byref(d)) < 0


def test_header_is_plain_c_and_a_c_program_can_call_the_library(tmp_path):
    """include/mpe_hip.h compiles as C (gcc -std=c99 -pedantic) and a C program links and calls libmpe_hip.so."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib_dir = os.path.dirname(_abi.LIB_PATH)
    exe = str(tmp_path / "abi_smoke")
    cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
           os.path.join(root, "tests", "c", "abi_smoke.c"), "-o", exe, "-L", lib_dir, "-lmpe_hip",
           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout, r.stderr)


def test_device_mode_noise_is_a_function_of_the_global_world_index():
    """u_noise / c_noise in batched mode (core.py:138,176 draw Gaussian noise inside World.step): counter-based, keyed by
    (seed, global world, draw number, column) -- shards of any sizes draw exactly the rows of one big batch, successive
    draws differ, and the numbers are standard normal."""
    import torch
    from multiagent_particle_envs_amd.core import counter_randn
    full = counter_randn(9, 0, 2, (1000, 2), "cpu")
    for off, cnt in ((0, 300), (300, 500), (800, 200)):
        assert torch.equal(counter_randn(9, off, 2, (cnt, 2), "cpu"), full[off:off + cnt])
    other = counter_randn(9, 0, 3, (1000, 2), "cpu")
    assert not torch.equal(other, full) and not torch.equal(counter_randn(10, 0, 2, (1000, 2), "cpu"), full)
    x = counter_randn(1, 0, 0, (200000, 4), "cpu")
    assert abs(float(x.mean())) < 0.01 and abs(float(x.std()) - 1.0) < 0.01
    assert abs(float((x[:, 0] * x[:, 1]).mean())) < 0.01 and abs(float((x[:-1, 0] * x[1:, 0]).mean())) < 0.01
    assert abs(float((x.abs() > 1.959964).float().mean()) - 0.05) < 0.003


def test_no_kernel_uses_scratch_memory():
    """Every kernel keeps its per-lane state in registers: the build leaves the device assembly in
    multiagent_particle_envs_amd/build/ (-save-temps=obj) and none of its kernels may declare private (scratch) memory.
    Round 3 shipped, for a few hours, communication kernels whose position arrays had gone to scratch (a chain of selects
    over three landmarks turned into a phi of pointers): 48 bytes per lane and a dozen scratch loads per step, unnoticed
    because nothing looked."""
    import glob
    import re
    from multiagent_particle_envs_amd import _build
    files = sorted(glob.glob(os.path.join(_build.OBJ, "mpe_*-hip-amdgcn-amd-amdhsa-gfx950.s")))
    files = [f for f in files if "_stress" not in os.path.basename(f)]
    if len(files) < len(_build.SOURCES):
        pytest.skip("device assembly not present (built elsewhere): run python -m multiagent_particle_envs_amd._build --force")
    bad, n = [], 0
    for f in files:
        text = open(f).read()
        for m in re.finditer(r"\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+)", text, re.S):
            n += 1
            if int(m.group(2)) > 0:
                bad.append((os.path.basename(f), m.group(1)[:90], int(m.group(2))))
    assert n > 100, n          # the library has a few hundred kernels
    assert not bad, bad


def test_bench_two_point_slope_rejects_a_bad_point():
    """bench.py times a kernel as the slope between a body of n and one of 2n launches.  One slow body must not pass as a
    fast kernel (seen once: 2.76 ms / 4.17 ms for n = 400 / 800 read as 3.5 us for a 5.2 us kernel): the implied fixed
    cost of a replay is checked, and the 2n body's average -- an upper bound -- is reported when it is implausible."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    us, fixed, ok = bench.two_point_slope_us(2.2034, 4.3679, 400)            # the headline's own raw times: sound
    assert ok and abs(us - 5.411) < 0.01 and 0.0 < fixed < 0.06
    us, fixed, ok = bench.two_point_slope_us(2.7603, 4.1715, 400)            # the int-ids leg's bad pair
    assert not ok and fixed > 1.0 and abs(us - 4.1715e3 / 800) < 1e-9
    us, fixed, ok = bench.two_point_slope_us(6.8078, 13.5060, 100)           # C4: a long kernel, fixed cost inside 2 % of the body
    assert ok and abs(us - 66.98) < 0.01
    us, fixed, ok = bench.two_point_slope_us(2.0683, 4.1764, 400)            # slightly negative fixed cost: measurement noise
    assert ok and -0.05 < fixed < 0.0


def test_bench_dump_outputs_is_capped_by_a_fixed_sample_of_worlds(tmp_path):
    """--dump-outputs writes every array whole while they fit in 64 MB, else the SAME seeded sample of worlds from each (their
    numbers in world_index) -- float32 / float64 files only; --full is off by default."""
    import bench
    assert not bench.parse_args([]).full and bench.parse_args(["--full"]).full
    assert bench.parse_args(["--dump-outputs", str(tmp_path)]).dump_outputs == str(tmp_path)
    rs = np.random.RandomState(0)
    small = {"obs0": rs.rand(64, 18).astype(np.float32), "rew": rs.rand(3, 64).astype(np.float32),
             "pos": rs.rand(6, 2, 64).astype(np.float32)}
    assert bench.sample_outputs(small) is small
    B = 1 << 20
    big = {"obs0": np.arange(B, dtype=np.float32)[:, None] * np.ones((1, 18), np.float32), "rew": np.tile(np.arange(B, dtype=np.float32), (3, 1)),
           "pos": np.tile(np.arange(B, dtype=np.float32), (6, 2, 1))}
    a, b = bench.sample_outputs(big), bench.sample_outputs(big)
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BYTES and a["world_index"].dtype == np.float64
    w = a["world_index"]
    assert np.array_equal(w, b["world_index"]) and np.all(np.diff(w) > 0) and 0 < len(w) < B
    assert np.array_equal(a["obs0"][:, 5], w) and np.array_equal(a["rew"][2], w) and np.array_equal(a["pos"][4, 1], w)
    bench.write_outputs(small, str(tmp_path / "d"))
    assert sorted(os.listdir(str(tmp_path / "d"))) == ["obs0.npy", "pos.npy", "rew.npy"]
    assert np.array_equal(np.load(str(tmp_path / "d" / "rew.npy")), small["rew"])


def test_bench_refuses_ranks_that_share_a_gpu():
    """bench.py --gpus N checks, before measuring, that the N ranks drive N different GPUs (UUID, else PCI address): a
    mis-mapped job must not print n_gpus = N for fewer GPUs."""
    import bench
    ok = [{"rank": r, "uuid": "GPU-%04d" % r, "pci": None} for r in range(8)]
    assert bench.duplicate_gpus(ok) == ""
    two = [dict(x) for x in ok]
    two[5]["uuid"] = two[2]["uuid"]
    assert "ranks 2 and 5" in bench.duplicate_gpus(two)
    pci = [{"rank": r, "uuid": None, "pci": "0000:%02x:00" % (r // 2)} for r in range(4)]      # no UUIDs: the PCI address decides
    msg = bench.duplicate_gpus(pci)
    assert "ranks 0 and 1" in msg and "ranks 2 and 3" in msg
    assert "no UUID" in bench.duplicate_gpus([{"rank": 0, "uuid": None, "pci": None}, {"rank": 1, "uuid": "a", "pci": None}])
    st = bench.per_gpu_stats([{"env_steps_per_s": {"median": v}} for v in (9.0, 10.0, 7.0, 8.0)])
    assert (st["min"], st["median"], st["max"], st["ranks"]) == (7.0, 9.0, 10.0, 4)


def test_pmc_traffic_json_is_what_the_cited_files_say():
    """bench.py's `roofline.traffic` comes from profiles/pmc_traffic.json; every entry there must equal the last line of the
    PMC summary it cites (profiles/make_pmc_traffic.py regenerates it; round-3 verdict: two entries were 0.5-2 % off)."""
    import importlib.util
    p = os.path.join(ROOT, "profiles", "make_pmc_traffic.py")
    spec = importlib.util.spec_from_file_location("make_pmc_traffic", p)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    import json
    assert json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json"))) == m.build()


def test_bench_line_is_compact_and_round_trips():
    """The driver parses ONE line from rank 0 (round 5's 20 KB line came back `parsed: null`): the printed line is the compact
    form of the full record -- under bench.LINE_BUDGET bytes whatever the record holds -- with the contract's keys, `roofline`
    (kernel-only and timed-region fractions, the rocprof durations, the HBM-resident fraction) and `cpu_baseline`."""
    import copy
    import json
    import bench
    rec = json.load(open(os.path.join(ROOT, "profiles", "r5_bench_default_steps20_box31.json")))      # a real 20 KB record
    assert len(json.dumps(rec)) > 15000
    line = bench.compact_line(rec, "gpurun_out/bench_full.json")
    assert len(line) < bench.LINE_BUDGET == 4096 and "\n" not in line
    out = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "timed_steps", "timed_region_s"):
        assert k in out, k
    assert out["steps"] == 20 and out["warmup"] == 5 and out["n_gpus"] == 1 and out["vs_baseline"] is None
    assert abs(out["value"] / rec["value"] - 1) < 1e-5 and abs(out["ms_per_step"] / rec["ms_per_step"] - 1) < 1e-5
    assert abs(out["timed_steps"] * out["ms_per_step"] * 1e-3 / out["timed_region_s"] - 1) < 1e-3      # what the driver can check
    assert "workload" in out["config"] and "model" not in out["config"] and out["config"]["batch_per_gpu"] == 65536
    roof = out["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "frac_timed_region", "kernel", "kernel_us_per_launch",
              "algorithmic_bytes_per_launch", "hbm_resident_frac", "l3_resident"):
        assert k in roof, k
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-5 and roof["frac_timed_region"] < roof["frac"]
    cpu = out["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["value"] > 0 and cpu["cores"] == 16 and cpu["sample"] and cpu["unit"] == "env-steps/s"
    assert cpu["reference_build_container"]["env_steps_per_s_all_cores"] > 0
    assert set(out["configs"]) == {"C2_spread_n3_B4096", "C3_tag_B16384", "C4_spread_n64_B4096"}
    assert out["full_record"] == "gpurun_out/bench_full.json"
    # an 8-rank record with long per-rank blocks and prose: still one line under the budget, the contract's objects kept
    big = copy.deepcopy(rec)
    big["n_gpus"] = 8
    big["config"]["ranks"] = [dict(rank=r, note="x" * 500) for r in range(8)]
    big["roofline"]["kernel_us_per_launch_by_rank"] = [5.4 + 0.01 * r for r in range(8)]
    big["roofline"]["per_gpu"] = True
    big["extra"]["configs"]["C9_" + "y" * 3000] = big["extra"]["configs"]["C2_spread_n3_B4096"]
    line8 = bench.compact_line(big, None)
    out8 = json.loads(line8)
    assert len(line8) < bench.LINE_BUDGET and len(out8["roofline"]["kernel_us_per_launch_by_rank"]) == 8
    assert "roofline" in out8 and "cpu_baseline" in out8 and "full_record" not in out8
    assert bench.sig(10358300123.4) == 10358300000.0 and bench.sig(0.00632694123) == 0.00632694 and bench.sig(7) == 7
    # a round-6 record (the line's value is the step server's; the launched steps' figures ride in roofline.launched), and the line
    # the GPU box printed from it
    rec6 = json.load(open(os.path.join(ROOT, "profiles", "r6_bench_default_steps20_box16.json")))
    line6 = bench.compact_line(rec6, rec6.get("full_record"))
    out6 = json.loads(line6)
    assert len(line6) < bench.LINE_BUDGET and out6["config"]["mode"] == "step-server"
    r6 = out6["roofline"]
    assert r6["launched"]["value"] < out6["value"] and r6["launched"]["frac_timed_region"] < r6["frac_timed_region"] < 1.0
    assert r6["kernel_us_rocprof"]["source"].startswith("profiles/") and r6["traffic"] > 0 and r6["hbm_resident_frac"] > 0.5
    assert abs(out6["timed_steps"] * out6["ms_per_step"] * 1e-3 / out6["timed_region_s"] - 1) < 1e-3 and out6["timed_region_s"] >= 2.0
    printed = json.loads(open(os.path.join(ROOT, "profiles", "r6_bench_line_box16.json")).read().strip().splitlines()[-1])
    assert printed["value"] == out6["value"] and printed["roofline"]["frac"] == r6["frac"]
