"""CPU: the case table of tests/_wide_custom.py is worth running on a GPU (tests/test_gpu_wide_custom.py).

  facts          every case reaches the kernel and the branches it names: mpe_wide_plan (the function launch_wide switches on) and a
                 plain restatement of homo / agents_only / one_csize / nC from the spec give what the table states;
  conditions     the reference alone stays inside the GPU tests' conditions: the 1e-6 guard band masks at most 1 % of a case's
                 worlds (at least one world is allowed), the fp32 oracle stays below a quarter of the bar against the fp64 one;
  discriminate   each mistake a branch invites, restated as a mutation of the spec, moves the fp64 oracle's post-step velocities
                 by at least 10 x the bar in at least 10 % of the worlds -- so a kernel that made it could not pass;
  cull band      with a customised margin, collidable pairs lie between the default cull distance and the customised one.

No device is touched: mpe_wide_plan is host arithmetic, its pointer arguments are never dereferenced."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _wide_custom as wc  # noqa: E402
from _parity_util import TOL, _guard_ok  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd import _abi  # noqa: E402
from oracle.mpe_batched import BatchedOracle  # noqa: E402

IDS = [c.id for c in wc.CASES]
FAKE = 1 << 20      # a 128-byte-aligned "device address" (torch's allocations are): the plan reads alignment, nothing else


def cpu_world(case):
    sc = mpe.scenarios.load(case.scenario + ".py").Scenario()
    w = sc.make_world(batch_size=case.B, device="cpu", **case.kw)
    wc.customise_world(case, w)
    return sc, w


def plan_of(case, phys=True, out=True, roll=False):
    sc, w = cpu_world(case)
    desc = w.scenario_desc(sc.kind, getattr(sc, "num_adversaries", 0))
    bufs = _abi.MpeBuffers()
    bufs.pos = bufs.vel = bufs.act = bufs.obs = bufs.rew = bufs.entity_table = FAKE
    return _abi.wide_plan(desc, bufs, case.B, phys, out, roll)


@pytest.mark.parametrize("cid", IDS)
def test_case_reaches_the_kernel_and_branches_it_names(cid):
    case = wc.BY_ID[cid]
    spec = wc.custom_spec(case)
    facts = wc.facts_of(spec)
    plan, homo = plan_of(case)
    got = dict(facts, plan=plan, homo=homo)
    want = dict(case.facts, plan=getattr(_abi, case.facts["plan"]))
    assert got == want and facts["homo"] == homo, cid
    if case.roll_plan:
        assert plan_of(case, roll=True) == (getattr(_abi, case.roll_plan), homo), cid
    # no case is served by another kernel family, whatever half of the step is asked for
    assert plan_of(case, out=False)[0] in (_abi.MPE_WIDE_WAVE, _abi.MPE_WIDE_MULTI8, _abi.MPE_WIDE_MULTI16, _abi.MPE_WIDE_MULTI32)
    assert plan_of(case, phys=False)[0] != _abi.MPE_WIDE_NONE


@pytest.mark.parametrize("cid", IDS)
def test_both_sides_get_the_same_constants(cid):
    """One description, two appliers: the descriptor built from the customised world holds the customised spec's numbers."""
    case = wc.BY_ID[cid]
    spec = wc.custom_spec(case)
    sc, w = cpu_world(case)
    d = w.scenario_desc(sc.kind, getattr(sc, "num_adversaries", 0))
    E, A = spec.n_entities, spec.n_agents
    assert (d.n_agents, d.n_landmarks) == (A, spec.n_landmarks)
    f = np.float32      # (the descriptor is float32; the customised values are float32-representable, the scenarios' own need not be)
    assert [d.size[e] for e in range(E)] == [f(x) for x in spec.size] and [d.mass[e] for e in range(E)] == [f(spec.mass_of(e)) for e in range(E)]
    assert [bool(d.collide[e]) for e in range(E)] == list(spec.collide) and [bool(d.movable[e]) for e in range(E)] == list(spec.movable)
    assert [d.accel[i] for i in range(A)] == [f(5.0 if x is None else x) for x in spec.accel]
    assert [d.max_speed[i] for i in range(A)] == [f(-1.0 if x is None else x) for x in spec.max_speed]
    base = wc.base_spec(case)      # every customised constant is stored as its float32 value
    for name in ("size", "accel", "max_speed"):
        assert all(x == y or x is None or f(x) == x for x, y in zip(getattr(spec, name), getattr(base, name))), name
    assert all(f(x) == x for x in spec.mass) and all(f(v) == v for v in (case.custom.get("world") or {}).values())
    assert (d.dt, d.damping, d.contact_force, d.contact_margin) == (f(spec.dt), f(spec.damping), f(spec.contact_force), f(spec.contact_margin))
    assert case.custom.get("immovable", ()) == tuple(i for i in range(A) if not spec.movable[i])


@pytest.mark.parametrize("cid", IDS)
def test_the_reference_alone_stays_inside_the_conditions(cid):
    spec, steps = wc.reference(cid)
    B = wc.BY_ID[cid].B
    worst = 0.0
    for st in steps:
        ok = _guard_ok(spec, st["pos"], 1e-6)
        assert int((~ok).sum()) <= max(1, 0.01 * B), "the guard band masks %d of %d worlds" % (int((~ok).sum()), B)
        o32 = BatchedOracle(spec, B, np.float32, benchmark=True)
        o32.set_state(*st["start"])
        obs32, rew32, _, _ = o32.step(st["act"])
        errs = [wc.scaled(o32.pos, st["pos"]).max(), wc.scaled(o32.vel, st["vel"]).max(), wc.scaled(rew32[:, ok], st["rew"][:, ok]).max()]
        errs += [wc.scaled(a, b).max() for a, b in zip(obs32, st["obs"])]
        worst = max(worst, float(max(errs)))
    print("%s: fp32 oracle vs fp64, worst scaled error %.2e" % (cid, worst))
    assert worst < 0.25 * TOL, worst


def test_the_table_names_exactly_the_mutations_that_apply():
    for case in wc.CASES:
        spec = wc.custom_spec(case)
        applies = tuple(m for m, fn in wc.MUTATIONS.items() if not wc.is_identity(spec, fn(spec)))
        assert applies == case.catches, case.id


@pytest.mark.parametrize("cid,mutation", [(c.id, m) for c in wc.CASES for m in c.catches])
def test_the_inputs_expose_the_mistake(cid, mutation):
    spec, steps = wc.reference(cid)
    B = wc.BY_ID[cid].B
    st = steps[0]
    wrong = BatchedOracle(wc.MUTATIONS[mutation](spec), B, np.float64)
    wrong.set_state(*st["start"])
    wrong.integrate(wrong.forces(wrong.decode(st["act"])))
    moved = wc.scaled(wrong.vel, st["vel"]).reshape(B, -1).max(axis=1) >= 10 * TOL
    print("%s %s: %.0f %% of the worlds move by 10 x the bar" % (cid, mutation, 100 * moved.mean()))
    assert moved.mean() >= 0.10, (cid, mutation, float(moved.mean()))


@pytest.mark.parametrize("cid", [c.id for c in wc.CASES if "contact_margin" in (c.custom.get("world") or {})])
def test_the_cull_band_is_populated(cid):
    """Collidable pairs between dist_min + 20 * 1e-3 (where a cull at the default margin drops them) and dist_min + 20 * margin."""
    case = wc.BY_ID[cid]
    spec = wc.custom_spec(case)
    p32, _, _ = wc.inputs(case)
    E = spec.n_entities
    p = p32.astype(np.float64)
    d = np.sqrt(((p[:, :, None, :] - p[:, None, :, :]) ** 2).sum(-1))
    size, coll = np.asarray(spec.size), np.asarray(spec.collide)
    dmin = size[:, None] + size[None, :]
    pairs = np.triu(coll[:, None] & coll[None, :], 1)
    n = int(((d >= dmin + 20e-3) & (d < dmin + 20 * spec.contact_margin) & pairs[None]).sum())
    print("%s: %d collidable pairs in the cull band" % (cid, n))
    assert spec.contact_margin > 1e-3 and n >= 100, n
