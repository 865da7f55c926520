"""CPU: the Philox restatement (oracle/philox.py) against the published known answers, and the device draws of csrc/mpe_device.h --
compiled for the HOST (tests/c/draws_host_walk.cpp: the very functions the kernels call) -- against the restatements at every
counter edge of tests/_draws_ref.py.  Integer work and fixed-sequence fp32, so every comparison is equality.

The minibatch round keys (csrc/mpe_internal.h onp_make_perm) ARE reachable from the host-only build and are walked too."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _draws_ref as D  # noqa: E402
from oracle import philox  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the philox4x32-10 rows of Random123's kat_vectors (Salmon et al., SC'11): counter, key -> output
KAT = [((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    from multiagent_particle_envs_amd import _build
    try:
        hipcc = shutil.which(_build._hipcc())          # the compiler the library itself is built with
    except RuntimeError:
        hipcc = None
    if hipcc is None:
        pytest.skip("no hipcc: the host walk includes csrc/mpe_device.h, which needs the HIP headers")
    exe = str(tmp_path_factory.mktemp("draws_walk") / "draws_host_walk")
    cmd = [hipcc, "--offload-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "multiagent_particle_envs_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "draws_host_walk.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-4000:]

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert p.returncode == 0, (p.stdout[-500:], p.stderr[-2000:])
        out = p.stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


@pytest.fixture(scope="module")
def walked(walk):
    """every case of the CPU table through the walk, in ONE run of the program: case name -> its answers"""
    lines, spans = [], {}
    for c in D.CPU_CASES:
        mine = D.walk_lines(c)
        spans[c["name"]] = (len(lines), len(mine))
        lines += mine
    out = walk(lines)
    return {name: out[a:a + n] for name, (a, n) in spans.items()}


def test_the_restatement_reproduces_the_known_answers():
    for ctr, key, want in KAT:
        got = philox.philox4x32_10(*[np.array([c], np.uint32) for c in ctr], key[0], key[1])
        assert tuple(int(g[0]) for g in got) == want, [hex(int(g[0])) for g in got]
    # ... vectorised: the three rows at once under one key each is the same function of the counters
    for k in range(3):
        cols = [np.array([KAT[j][0][w] for j in range(3)], np.uint32) for w in range(4)]
        got = philox.philox4x32_10(*cols, KAT[k][1][0], KAT[k][1][1])
        assert tuple(int(g[k]) for g in got) == KAT[k][2]


def test_the_device_generator_reproduces_the_known_answers(walk):
    out = walk(["philox %d %d %d %d %d %d" % (ctr + key) for ctr, key, _ in KAT])
    for line, (_, _, want) in zip(out, KAT):
        assert tuple(int(v, 16) for v in line.split()) == want, line


def test_the_case_names_are_unique_and_every_case_names_its_words():
    names = [c["name"] for c in D.CPU_CASES]
    assert len(set(names)) == len(names)
    for c in D.CPU_CASES:
        assert c["words"] and all(w in D.WORDS for w in c["words"]), c["name"]
    kinds = {c["kind"] for c in D.CPU_CASES}
    assert kinds == {"reset", "box", "choice", "action", "comm", "policy", "policycomm", "replay", "replayprio", "minibatch"}
    for table, rows in D.GPU_TABLES.items():
        assert len({r["name"] for r in rows}) == len(rows)
        for r in rows:
            assert all(w in D.WORDS for w in r["words"]) and r["why"], (table, r["name"])


@pytest.mark.parametrize("case", D.CPU_CASES, ids=[c["name"] for c in D.CPU_CASES])
def test_the_device_draw_equals_the_restatement(case, walked):
    got, want = D.parse_walk(case, walked[case["name"]]), D.expect(case)
    assert got.shape == want.shape and np.array_equal(got.astype(np.uint64), want.astype(np.uint64)), (case["name"], got, want)


@pytest.mark.parametrize("case", D.CPU_CASES, ids=[c["name"] for c in D.CPU_CASES])
def test_each_case_reaches_the_word_it_names(case):
    """The restatement with the named word zeroed expects something else for the case's own inputs: a device function that dropped
    that word would fail the case."""
    want = D.expect(case)
    for word in case["words"]:
        assert not np.array_equal(D.expect(case, zero=word), want), (case["name"], word)


@pytest.mark.parametrize("table", sorted(D.GPU_TABLES))
def test_each_row_of_the_gpu_sweep_reaches_the_words_it_names(table):
    """The same for tests/test_gpu_draws.py's tables (rows with no word are shape rows and say so in their reason)."""
    for row in D.GPU_TABLES[table]:
        want = D.gpu_expect(table, row)
        for word in row["words"]:
            other = D.gpu_expect(table, row, zero=word)
            assert any(not np.array_equal(other[k], want[k]) for k in want), (table, row["name"], word)


def test_the_block_forms_are_the_single_steps():
    a = philox.action_ids_block(9, 70, D.STEP_CARRY, 5, 6, world_offset=D.OFF_CARRY)
    c = philox.comm_ids_block(9, 70, D.STEP_CARRY, 5, 6, 10, world_offset=D.OFF_CARRY)
    assert a.shape == (5, 6, 70) and c.shape == (5, 6, 70)
    for s in range(5):
        assert np.array_equal(a[s], philox.action_ids(9, 70, D.STEP_CARRY + s, 6, world_offset=D.OFF_CARRY))
        assert np.array_equal(c[s], philox.comm_ids(9, 70, D.STEP_CARRY + s, 6, 10, world_offset=D.OFF_CARRY))


def test_a_box_of_the_symmetric_placement_draws_the_same_uniforms():
    """reset_positions_box shares reset_positions' counters: the box (-1, 2) reads the same 24 bits (x + 1) / 2 recovers exactly"""
    pos = philox.reset_positions(5, 33, 7, 2, 1, 1.0, world_offset=D.OFF_CARRY)
    box = philox.reset_positions_box(5, 33, 7, [(-1.0, 2.0, -1.0, 2.0)] * 3, world_offset=D.OFF_CARRY)
    assert np.array_equal(pos, box)          # u * 2 is exact, so both orders round once


# ---- the ranges, over all 2^24 inputs ---------------------------------------------------------------------------------------------
def _pair(line):
    return [np.float32(float.fromhex(v)) for v in line.split()]


def test_uniform_pm_is_half_open_for_every_shipped_range(walk):
    """u * (2 r) - r over all 2^24 values of bits >> 8: -r <= x < r for the agents' r = 1 and every shipped landmark_range."""
    import multiagent_particle_envs_amd.scenarios as S
    import importlib
    import pkgutil
    shipped = sorted({float(getattr(importlib.import_module(S.__name__ + "." + m.name).Scenario, "landmark_range"))
                      for m in pkgutil.iter_modules(S.__path__) if m.name.startswith("simple")})
    assert len([m for m in pkgutil.iter_modules(S.__path__) if m.name.startswith("simple")]) == 9
    assert set(shipped) <= set(D.LANDMARK_RANGES), shipped
    out = walk(["range_pm %d" % D.f32_bits(r) for r in D.LANDMARK_RANGES])
    for r, line in zip(D.LANDMARK_RANGES, out):
        lo, hi = _pair(line)
        r32 = np.float32(r)
        print("uniform_pm r = %r: min %s max %s" % (r, float(lo).hex(), float(hi).hex()))
        assert -r32 <= lo and hi < r32, (r, lo, hi)
        assert lo == -r32                  # the lower end IS reached (bits >> 8 == 0)


def test_box_placement_stays_in_its_box_and_where_the_upper_end_is_reached(walk):
    """lo + span * u over all 2^24 inputs.  u < 1, so fl(span * u) <= span and x <= fl(lo + span): that much always holds.  The
    upper end itself is NOT reached by any box the project ships or tests with (the Yard of tests/test_rowspec.py, the traced
    tests/refstyle/herd.py) -- their placement is half-open, as the docstrings say -- but it IS reached where |lo| is large next to
    the span (lo = 100, span = 0.5: 100 + 0.49999997 rounds to 100.5), which rowspec.RowProgram's docstring now states."""
    names = sorted(D.BOX_RANGES)
    cases = [(n, np.float32(D.BOX_RANGES[n][0]), np.float32(D.BOX_RANGES[n][1] - D.BOX_RANGES[n][0]), D.BOX_RANGES[n][1]) for n in names]
    cases.append(("lo 100 span 0.5", np.float32(100.0), np.float32(0.5), 100.5))
    out = walk(["range_box %d %d" % (D.f32_bits(lo), D.f32_bits(span)) for _, lo, span, _ in cases])
    reached = {}
    for (name, lo, span, hi), line in zip(cases, out):
        xmin, xmax = _pair(line)
        end = np.float32(lo + span)
        reached[name] = bool(xmax >= np.float32(hi))
        print("box %s: min %s max %s, upper end reached: %s" % (name, float(xmin).hex(), float(xmax).hex(), reached[name]))
        assert xmin == lo and xmax <= end, (name, xmin, xmax)
    assert reached.pop("lo 100 span 0.5")
    assert not any(reached.values()), reached
