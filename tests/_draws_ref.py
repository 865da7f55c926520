"""Helpers of tests/test_oracle_philox.py and tests/test_gpu_draws.py (no tests in here): the edge tables of the device draws and
what the restatements expect at each row.  Nothing is restated here: every expectation is a call into oracle/philox.py (reset,
box, choice, action and comm draws), tests/_actor_ref.py (the policy streams), tests/_replay_ref.py, tests/_replay_prio_ref.py
(the replay streams) or tests/_onpolicy_batch_ref.py (the minibatch round keys).

Every row names the counter WORDS it is in the table for, and `expect(case, zero=word)` is the same restatement with that word
zeroed: a row whose expectation does not change under it could not tell a kernel that drops the word from one that keeps it.
    world high    bits 32.. of the global world index         (counter word 1, xor-ed with the step's / episode's high word)
    step high     bits 32.. of the global step (or draw number, or epoch)
    episode high  bits 32.. of the episode number
    quad          counter word 2: the agent quad, the pick quad or the entity pair
    pair half     which words of the Philox block the draw reads (entity & 1, agent & 3, pick & 3)
    seed high     key word 1
    stream        the stream constant in counter word 3
"""
import contextlib

import numpy as np

import _actor_ref
import _onpolicy_batch_ref
import _replay_prio_ref
import _replay_ref
from oracle import philox

M32, M64 = 0xFFFFFFFF, 2 ** 64 - 1
WORDS = ("world high", "step high", "episode high", "quad", "pair half", "seed high", "stream")
W = 8          # worlds (or samples) per CPU case: consecutive, so a case placed 4 below a carry straddles it

# the edge values of the sweep (the GPU table below and the CPU table share them)
OFF_CARRY, OFF_HIGH = 2 ** 32 - 40, 2 ** 40 + 3
STEP_CARRY, STEP_HIGH = 2 ** 32 - 2, 2 ** 40 + 1
SEEDS = (0, 0xFFFFFFFF, 2 ** 32, 2 ** 64 - 1)


def off_top(B):
    """the last world_offset an int64 argument can carry for a batch of B"""
    return 2 ** 63 - 1 - B


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


# ---- "the restatement with that word zeroed" -------------------------------------------------------------------------------------
def pieces(offset, B):
    """[(first local world, global world of it, count)]: the batch cut where the world index's high word changes"""
    out, w = [], 0
    while w < B:
        g = offset + w
        n = min(B - w, ((g >> 32) + 1 << 32) - g)
        out.append((w, g, n))
        w += n
    return out


def over_worlds(fn, offset, B, zero_high, axis):
    """fn(offset, B) -> array with the world axis at `axis`; with zero_high every world is drawn at (world & 0xFFFFFFFF)"""
    if not zero_high:
        return fn(offset, B)
    return np.concatenate([fn(g & M32, n) for _, g, n in pieces(offset, B)], axis=axis)


@contextlib.contextmanager
def stream_zeroed(module, name, on):
    keep = getattr(module, name)
    if on:
        setattr(module, name, 0)
    try:
        yield
    finally:
        setattr(module, name, keep)


def _t(case, zero):
    t = case["t"]
    return t & M32 if zero in ("step high", "episode high") else t


def _seed(case, zero):
    return case["seed"] & M32 if zero == "seed high" else case["seed"]


def _idx(case, zero, per_block):
    i = case["idx"]
    if zero == "quad":
        return i % per_block
    if zero == "pair half":
        return i - i % per_block
    return i


# ---- the CPU table: one entity / agent / pick of W consecutive worlds per case ---------------------------------------------------
def expect(case, zero=None):
    """What the restatements give for `case` -> an integer array [W] (floats as their bit patterns, [W, 2])."""
    kind, seed, t, world = case["kind"], _seed(case, zero), _t(case, zero), case.get("world", 0)
    zw = zero == "world high"
    if kind == "reset":
        e, r = _idx(case, zero, 2), case["r"]
        A, L = (e + 1, 0) if r == 1.0 else (e, 1)
        with stream_zeroed(philox, "STREAM_RESET", zero == "stream"):
            return over_worlds(lambda o, n: philox.reset_positions(seed, n, t, A, L, r, world_offset=o)[:, e], world, W, zw, 0).view(np.uint32)
    if kind == "box":
        e = _idx(case, zero, 2)
        with stream_zeroed(philox, "STREAM_RESET", zero == "stream"):
            return over_worlds(lambda o, n: philox.reset_positions_box(seed, n, t, [case["box"]] * (e + 1), world_offset=o)[:, e],
                               world, W, zw, 0).view(np.uint32)
    if kind == "choice":
        k = _idx(case, zero, 4)
        with stream_zeroed(philox, "STREAM_CHOICE", zero == "stream"):
            return over_worlds(lambda o, n: philox.reset_choices(seed, n, t, [case["n"]] * (k + 1), world_offset=o)[k], world, W, zw, 0)
    if kind == "action":
        i = _idx(case, zero, 4)
        with stream_zeroed(philox, "STREAM_ACTION", zero == "stream"):
            return over_worlds(lambda o, n: philox.action_ids(seed, n, t, i + 1, world_offset=o)[i], world, W, zw, 0)
    if kind == "comm":
        i = _idx(case, zero, 4)
        with stream_zeroed(philox, "STREAM_COMM", zero == "stream"):
            return over_worlds(lambda o, n: philox.comm_ids(seed, n, t, i + 1, case["n"], world_offset=o)[i], world, W, zw, 0)
    if kind in ("policy", "policycomm"):      # tests/_actor_ref.py: the 24 bits the head rule reads, as u = bits * 2^-24 in fp64
        i = _idx(case, zero, 4)
        stream = 0 if zero == "stream" else (_actor_ref.STREAM_POLICY if kind == "policy" else _actor_ref.STREAM_POLICY_COMM)
        u = over_worlds(lambda o, n: _actor_ref.draw_u(stream, seed, n, t, i, o), world, W, zw, 0)
        return (u * 2.0 ** 24).astype(np.int64)
    if kind == "replay":                      # tests/_replay_ref.py: samples 0 .. W-1 of draw number t, 64 bits each
        with stream_zeroed(_replay_ref, "STREAM_REPLAY", zero == "stream"):
            hi, lo = _replay_ref.draw_words(seed, t, W)
        return (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    if kind == "replayprio":                  # tests/_replay_prio_ref.py: the 24 bits of the stratified draw
        with stream_zeroed(_replay_prio_ref, "STREAM_REPLAY_PRIO", zero == "stream"):
            return _replay_prio_ref.prio_bits(seed, t, W).astype(np.int64)
    if kind == "minibatch":                   # tests/_onpolicy_batch_ref.py: the four round keys of (seed, epoch)
        with stream_zeroed(_onpolicy_batch_ref, "STREAM_MINIBATCH", zero == "stream"):
            return np.array(_onpolicy_batch_ref.round_keys(seed, t), np.int64)
    raise KeyError(kind)


def walk_lines(case):
    """the lines tests/c/draws_host_walk.cpp reads for `case` (one per world / sample; one for the minibatch keys)"""
    kind, seed, t, i = case["kind"], case["seed"], case["t"], case.get("idx", 0)
    worlds = [case.get("world", 0) + w for w in range(W)]
    if kind == "reset":
        return ["reset %d %d %d %d %d" % (seed, g, t, i, f32_bits(case["r"])) for g in worlds]
    if kind == "box":
        return ["box %d %d %d %d %d %d %d %d" % ((seed, g, t, i) + tuple(f32_bits(v) for v in case["box"])) for g in worlds]
    if kind in ("choice", "comm"):
        return ["%s %d %d %d %d %d" % (kind, seed, g, t, i, case["n"]) for g in worlds]
    if kind in ("action", "policy", "policycomm"):
        return ["%s %d %d %d %d" % (kind, seed, g, t, i) for g in worlds]
    if kind in ("replay", "replayprio"):
        return ["replay %d %d %d %d" % (seed, k, t, kind == "replayprio") for k in range(W)]
    if kind == "minibatch":
        return ["minibatch 1000 %d %d" % (seed, t)]
    raise KeyError(kind)


def parse_walk(case, lines):
    """the walk's answers for `case` in expect()'s form"""
    kind = case["kind"]
    if kind in ("reset", "box"):
        return np.array([[float.fromhex(v) for v in ln.split()] for ln in lines], np.float32).view(np.uint32)
    if kind in ("choice", "action", "comm"):
        return np.array([int(ln) for ln in lines], np.int32)
    if kind in ("policy", "policycomm"):
        return np.array([int(ln, 16) >> 8 for ln in lines], np.int64)
    if kind == "replay":
        return np.array([int(ln, 16) for ln in lines], np.uint64)
    if kind == "replayprio":
        return np.array([int(ln, 16) >> 40 for ln in lines], np.int64)
    if kind == "minibatch":
        return np.array([int(v, 16) for v in lines[0].split()], np.int64)
    raise KeyError(kind)


def _case(kind, name, words, seed=0, world=0, t=0, idx=0, **kw):
    c = dict(kind=kind, name="%s-%s" % (kind, name), words=tuple(words), seed=seed, world=world, t=t, idx=idx)
    c.update(kw)
    return c


def _cpu_cases():
    """Per draw function the edge values of the sweep, one at a time and then together.  (the reason for each row is its words:
    a row that only moves LOW words -- all zeros, seed 0xFFFFFFFF, the two steps below the carry -- is told apart by the stream)"""
    out = []
    time_high = {"reset": "episode high", "box": "episode high", "choice": "episode high"}
    for kind, kw, hi_idx, half_idx in (("reset", dict(r=1.0), 510, 1), ("reset", dict(r=0.9), 3, 1),
                                       ("box", dict(box=(0.2, 0.7, -0.9, 1.8)), 63, 1), ("choice", dict(n=7), 3, 2),
                                       ("action", {}, 32, 3), ("comm", dict(n=10), 31, 1),
                                       ("policy", {}, 15, 2), ("policycomm", {}, 9, 3)):
        th = time_high.get(kind, "step high")
        per = 2 if kind in ("reset", "box") else 4
        tag = "r%g-" % kw["r"] if kind == "reset" else ""
        add = lambda name, words, **a: out.append(_case(kind, tag + name, words, **dict(kw, **a)))     # noqa: E731
        add("zeros", ["stream"])
        add("world-straddles-carry", ["world high"], world=2 ** 32 - 4)
        add("world-2^40+3", ["world high"], world=OFF_HIGH)
        add("world-top", ["world high"], world=off_top(W))
        for s in range(5):      # the T = 5 block at step0 = 2^32 - 2: two steps below the carry, three above
            add("t-carry%+d" % (s - 2), [th] if s >= 2 else ["stream"], t=STEP_CARRY + s, world=5)
        add("t-2^40+1", [th], t=STEP_HIGH)
        add("seed-low-ones", ["stream"], seed=SEEDS[1])
        add("seed-2^32", ["seed high"], seed=SEEDS[2])
        add("seed-ones", ["seed high"], seed=SEEDS[3])
        add("half", ["pair half"], idx=half_idx)
        if hi_idx >= per:       # (choice has MPE_MAX_CHOICES = 4 picks: one quad)
            add("quad", ["quad"] + (["pair half"] if hi_idx % per else []), idx=hi_idx)
        add("together", ["world high", th, "seed high"] + (["quad"] if hi_idx >= per else []), seed=0xFEDCBA9876543210,
            world=2 ** 32 - 4, t=STEP_HIGH, idx=hi_idx)
    for kind in ("replay", "replayprio", "minibatch"):
        add = lambda name, words, **a: out.append(_case(kind, name, words, **a))     # noqa: E731
        add("zeros", ["stream"])
        for s in range(5):
            add("t-carry%+d" % (s - 2), ["step high"] if s >= 2 else ["stream"], t=STEP_CARRY + s)
        add("t-2^40+1", ["step high"], t=STEP_HIGH)
        add("seed-low-ones", ["stream"], seed=SEEDS[1])
        add("seed-2^32", ["seed high"], seed=SEEDS[2])
        add("seed-ones", ["seed high", "step high"], seed=SEEDS[3], t=STEP_HIGH)
    return out


CPU_CASES = _cpu_cases()

# ---- the ranges the range facts are stated for -----------------------------------------------------------------------------------
LANDMARK_RANGES = (1.0, 0.9)          # every landmark_range of the nine shipped scenarios (scenarios/*.py), and the agents' 1.0
# (lo, hi) per coordinate as the scenario states them; the device gets lo and span = hi - lo (float64 difference) as float32
# (rowspec.RowProgram / World.reset_boxes): tests/test_rowspec.py's Yard, tests/refstyle/herd.py (the traced file with boxes)
BOX_RANGES = {"yard agents": (-0.25, 0.25), "yard posts x": (0.2, 0.9), "yard posts y": (-0.9, 0.9),
              "herd agents": (-0.8, 0.8), "herd landmarks": (-1.0, 1.0)}


# ---- the GPU table ---------------------------------------------------------------------------------------------------------------
def _row(name, why, words, **kw):
    return dict(kw, name=name, why=why, words=tuple(words))


# mpe_random_actions / mpe_random_actions_block: B, A, T, seed, step0, world_offset
MOVES = [
    _row("one-lane", "B = 1: one lane of one wave, the clamp nvalid - 1 = 0; everything else zero (T = 4: one move could not tell)", ["stream"],
         B=1, A=1, T=4, seed=0, t=0, off=0),
    _row("partial-wave", "B = 63: a partial only wave; A = 3: a half-used block; world high word alone", ["world high", "pair half"],
         B=63, A=3, T=1, seed=SEEDS[1], t=0, off=OFF_HIGH),
    _row("both-carries", "B = 64 at offset 2^32 - 40 and T = 5 at step0 = 2^32 - 2: the batch and the block straddle their carries",
         ["world high", "step high", "seed high", "pair half"], B=64, A=4, T=5, seed=SEEDS[2], t=STEP_CARRY, off=OFF_CARRY),
    _row("second-wave-of-one", "B = 65: a second wave of one world; A = 5: quad 1 holds one agent; key and step high words",
         ["quad", "step high", "seed high"], B=65, A=5, T=2, seed=SEEDS[3], t=STEP_HIGH, off=0),
    _row("second-block-top-offset", "B = 257: a second workgroup of one world, at the last offset an int64 carries; two full quads",
         ["world high", "quad"], B=257, A=8, T=1, seed=0, t=0, off=off_top(257)),
    _row("tail-and-carries", "B = 700: two full workgroups and a tail of 188 (a partial wave of 60); A = 9: quad 2 holds one agent",
         ["world high", "step high", "quad", "seed high"], B=700, A=9, T=3, seed=0xFEDCBA9876543210, t=STEP_CARRY, off=OFF_CARRY),
    _row("nine-quads", "A = 33: quad index 8, one agent in it", ["quad", "step high"], B=65, A=33, T=1, seed=7, t=STEP_HIGH, off=0),
]

# mpe_reset: B, A, L, landmark_range, pops, seed, episode, world_offset
RESETS = [
    _row("odd-3+2", "A + L odd, agents and landmarks meet inside pair 1, landmark_range 0.9; no picks", ["pair half", "quad"],
         B=63, A=3, L=2, lr=0.9, pops=(), seed=0, t=0, off=0),
    _row("odd-2+3-carries", "pair 1 is two landmarks, pair 2 half used; batch and episode at their carries; one pick of 1",
         ["world high", "episode high", "seed high", "quad"], B=64, A=2, L=3, lr=0.9, pops=(1,), seed=SEEDS[2], t=STEP_CARRY + 2, off=OFF_CARRY),
    _row("lone-agent", "A = 1, L = 0: one half-used pair; B = 1; two picks", ["stream"], B=1, A=1, L=0, lr=1.0, pops=(1, 2), seed=SEEDS[1], t=0, off=0),
    _row("even-4+4", "full pairs; B = 257; three picks; world and episode high words", ["world high", "episode high", "quad"],
         B=257, A=4, L=4, lr=1.0, pops=(1, 2, 3), seed=0, t=STEP_HIGH, off=OFF_HIGH),
    _row("four-picks-top-offset", "MPE_MAX_CHOICES picks (1, 2, 3, 7); B = 700 at the last offset; all-ones key", ["world high", "seed high"],
         B=700, A=3, L=2, lr=0.9, pops=(1, 2, 3, 7), seed=SEEDS[3], t=STEP_CARRY, off=off_top(700)),
    _row("near-the-entity-cap", "A + L = 511 of MPE_MAX_ENTITIES = 512, B = 65: pair index 255, grid.y = 511", ["quad", "episode high"],
         B=65, A=300, L=211, lr=0.9, pops=(7,), seed=3, t=STEP_HIGH, off=0),
]

# mpe_reset_random_actions_block: the reset's row + T, step0
RESET_MOVES = [
    _row("B65-A5", "B = 65, A = 5: two waves, two quads, T = 3 across the step carry; episode != every step of the block",
         ["world high", "step high", "episode high", "quad"], B=65, A=5, L=2, lr=0.9, pops=(1, 2, 3, 7), seed=SEEDS[3], ep=STEP_HIGH,
         t=STEP_CARRY, T=3, off=OFF_CARRY),
    _row("B257-odd", "B = 257: two workgroups; A + L odd; no picks; T = 1", ["episode high"], B=257, A=3, L=2, lr=0.9, pops=(), seed=5,
         ep=STEP_CARRY + 3, t=0, T=1, off=0),
    _row("B700-ids", "B = 700 with a tail wave, A = 9 (three quads), T = 2, top offset", ["world high", "quad"], B=700, A=9, L=1, lr=1.0,
         pops=(3,), seed=SEEDS[2], ep=1, t=STEP_HIGH, T=2, off=off_top(700)),
]

# mpe_reset_rows with per-entity boxes (lo_x, span_x, lo_y, span_y): symmetric, off-centre, a span of 1e-6, lo = 100 with span 0.5,
# negative lo -- one entity each (A = 3, L = 2: an odd count, the last pair half used)
BOXES = [(-0.25, 0.5, -0.25, 0.5), (0.2, 0.7, -0.9, 1.8), (0.5, 1e-6, -0.5, 1e-6), (100.0, 0.5, 100.0, 0.5), (-3.0, 1.0, -7.5, 0.25)]
BOX_RESETS = [
    _row("boxes-plain", "every box kind once, B = 65, no picks", ["pair half", "quad"], B=65, A=3, L=2, pops=(), seed=0, t=0, off=0),
    _row("boxes-carries", "batch and episode at their carries, picks (2, 7)", ["world high", "episode high", "seed high"],
         B=257, A=3, L=2, pops=(2, 7), seed=SEEDS[3], t=STEP_CARRY + 2, off=OFF_CARRY),
    _row("boxes-top", "B = 700 at the last offset, episode high word, one pick", ["world high", "episode high"],
         B=700, A=3, L=2, pops=(3,), seed=SEEDS[1], t=STEP_HIGH, off=off_top(700)),
]

# mpe_random_comm: B, A, dim_c, speakers, T, seed, step0, world_offset
COMMS = [
    # (a SHAPE row: with one word to say no counter word can show -- it is here for rows of one float and the silent second agent)
    _row("one-word", "dim_c = 1: rows of one float, the only word; A = 2, speakers 0b1; B = 65", [], B=65, A=2, dim_c=1, speakers=0b1, T=1,
         seed=0, t=0, off=0),
    _row("two-of-three", "speakers 0b101 of A = 3 (agent 1 silent), dim_c = 3, T = 3 across the step carry", ["step high", "pair half"],
         B=257, A=3, dim_c=3, speakers=0b101, T=3, seed=SEEDS[1], t=STEP_CARRY, off=0),
    _row("agent-31", "only bit 31 of A = 32: quad 7, word 3; dim_c = 10; world high word", ["quad", "pair half", "world high"],
         B=63, A=32, dim_c=10, speakers=1 << 31, T=1, seed=SEEDS[2], t=5, off=OFF_HIGH),
    _row("tail-carries", "B = 700 across the world carry, A = 5 (agent 4 silent: quad 1 never drawn), dim_c = 4, all-ones key",
         ["world high", "seed high", "step high"], B=700, A=5, dim_c=4, speakers=0b101, T=2, seed=SEEDS[3], t=STEP_HIGH, off=OFF_CARRY),
]


def gpu_expect(table, row, zero=None):
    """The restatement's outputs for one row of a GPU table, in the device's layouts; zero: as in expect() (quad: every block is
    block 0; pair half: every draw reads its block's first words)."""
    seed = row["seed"] & M32 if zero == "seed high" else row["seed"]
    t = row["t"] & M32 if zero == "step high" or (zero == "episode high" and "ep" not in row) else row["t"]
    ep = row.get("ep", 0) & M32 if zero == "episode high" else row.get("ep", 0)
    B, off, zw = row["B"], row["off"], zero == "world high"

    def regroup(a, per, axis):      # the draws the device would make if it dropped the block index / the position in the block
        n = a.shape[axis]
        if zero == "quad":
            return np.take(a, [i % per for i in range(n)], axis=axis)
        if zero == "pair half":
            return np.take(a, [i - i % per for i in range(n)], axis=axis)
        return a
    out = {}
    if table in ("moves", "reset_moves"):
        T = row["T"]
        t_block = row["t"] if zero != "step high" else None
        with stream_zeroed(philox, "STREAM_ACTION", zero == "stream" and table == "moves"):
            if t_block is None:     # the high word dropped step by step (the block crosses the carry)
                ids = np.stack([over_worlds(lambda o, n: philox.action_ids(seed, n, (row["t"] + s) & M32, row["A"], world_offset=o), off, B, zw, 1)
                                for s in range(T)])
            else:
                ids = over_worlds(lambda o, n: philox.action_ids_block(seed, n, t_block, T, row["A"], world_offset=o), off, B, zw, 2)
        out["ids"] = regroup(ids, 4, 1)                                                   # [T, A, B]
    if table in ("resets", "reset_moves"):
        te = ep if table == "reset_moves" else t
        with stream_zeroed(philox, "STREAM_RESET", zero == "stream"):
            pos = over_worlds(lambda o, n: philox.reset_positions(seed, n, te, row["A"], row["L"], row["lr"], world_offset=o), off, B, zw, 0)
        out["pos"] = np.ascontiguousarray(regroup(pos, 2, 1).transpose(1, 2, 0))          # [E, 2, B]
        if row["pops"]:
            with stream_zeroed(philox, "STREAM_CHOICE", zero == "stream"):
                out["choice"] = over_worlds(lambda o, n: philox.reset_choices(seed, n, te, list(row["pops"]), world_offset=o), off, B, zw, 1)
    if table == "box_resets":
        with stream_zeroed(philox, "STREAM_RESET", zero == "stream"):
            pos = over_worlds(lambda o, n: philox.reset_positions_box(seed, n, t, BOXES, world_offset=o), off, B, zw, 0)
        out["pos"] = np.ascontiguousarray(regroup(pos, 2, 1).transpose(1, 2, 0))
        if row["pops"]:
            out["choice"] = over_worlds(lambda o, n: philox.reset_choices(seed, n, t, list(row["pops"]), world_offset=o), off, B, zw, 1)
    if table == "comms":
        T = row["T"]
        with stream_zeroed(philox, "STREAM_COMM", zero == "stream"):
            ids = np.stack([over_worlds(lambda o, n: philox.comm_ids(seed, n, ((row["t"] + s) & M32) if zero == "step high" else row["t"] + s,
                                                                      row["A"], row["dim_c"], world_offset=o), off, B, zw, 1) for s in range(T)])
        ids = regroup(ids, 4, 1)
        out["ids"] = ids[:, [i for i in range(row["A"]) if (row["speakers"] >> i) & 1]]  # the speaking agents' words [T, S, B]
    return out


GPU_TABLES = {"moves": MOVES, "resets": RESETS, "reset_moves": RESET_MOVES, "box_resets": BOX_RESETS, "comms": COMMS}


def ids(rows):
    return [r["name"] for r in rows]
