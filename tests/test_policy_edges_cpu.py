"""CPU: the case table of the fused policy rollout's edge sweep (tests/_policy_edges.py) held to its own conditions before any GPU
time is spent on it -- it covers what it says it covers, the fp64 reference alone keeps the band count well inside the cap on the
case's own closed loop, every mistake the kernel invites is one the GPU comparison would notice, and fp32 itself stays under a
quarter of the bar on every case."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _actor_ref as R  # noqa: E402
import _policy_edges as PE  # noqa: E402
from oracle import philox  # noqa: E402


# ---- coverage -------------------------------------------------------------------------------------------------------------------------
def test_every_instantiation_path_and_activation_occurs():
    seen = set()
    for c in PE.CASES:
        assert c.aimed_at.strip(), c.id
        assert c.shape in PE.SHAPES and (c.shared or len(c.actors) == len(PE.obs_widths(c))), c.id
        for hidden, act in c.actors:
            seen.add((c.shape, len(hidden) + 1, act))
    for shape in PE.SHAPES:
        assert (shape, 1, PE.RELU) in seen, (shape, "nl = 1")
        for nl in (2, 3):
            for act in (PE.RELU, PE.TANH):
                assert (shape, nl, act) in seen, (shape, nl, PE.ACT_NAMES[act])


def test_every_hidden_width_occurs():
    used = {hidden for c in PE.CASES for hidden, _ in c.actors}
    want = {(1,), (20,), (63,), (64,), (1, 1), (20, 64), (64, 20), (33, 32), (64, 64)}
    assert want == set(PE.HIDDEN_WIDTHS) and want <= used, want - used


def test_the_edges_the_table_is_there_for():
    by = PE.BY_ID
    for shape in ("spread3", "push"):
        assert {by["batch_%s_B%d" % (shape, B)].B for B in (1, 63, 64, 65, 257)} == {1, 63, 64, 65, 257}
    assert {c.episode_len for c in PE.CASES if c.sweep == "episode" and c.shape == "spread3"} == {0, 1, 2, 7, 8}
    c = by["counters_step0"]
    assert c.step0 == 2 ** 32 - 3 and c.step0 + PE.T > 2 ** 32 and c.episode_len == 3 and c.modes == ("sample",)
    assert any(PE.is_restart(c, c.step0 + k) and c.step0 + k >= 2 ** 32 for k in range(PE.T)), "a restart behind the carry"
    c = by["counters_offset_B130"]
    assert c.world_offset == 2 ** 32 - 64 and c.B == 130 and c.world_offset + c.B > 2 ** 32
    c = by["counters_offset_B5"]
    assert c.world_offset == 2 ** 32 - 4 and c.B == 5
    assert {c.shape for c in PE.CASES if c.sweep == "constants"} == {"spread3", "adversary", "push"}
    for c in PE.CASES:
        if c.sweep != "constants":
            continue
        k = PE.constants(c)
        for name in ("accel", "max_speed"):
            assert any(v is None for v in k[name]) and any(v is not None for v in k[name]), (c.id, name)
        vals = k["size"] + k["mass"] + [v for v in k["accel"] + k["max_speed"] if v is not None] + list(k["world"].values())
        assert all(float(np.float32(v)) == v for v in vals if v != 250.0), (c.id, "a constant that is not its float32")
        assert k["world"] == PE.W1
    d = by["mixed_set"]
    assert d.actors == (((), PE.RELU), ((20,), PE.TANH), ((64, 33), PE.RELU)) and by["mixed_shared"].shared
    default = by["mixed_set"]
    assert (default.B, PE.T, default.episode_len, default.world_offset, default.policy_seed) == (130, 7, 3, 777, 9)
    assert [k for k in range(PE.T) if PE.is_restart(default, k)] == [0, 3, 6]


def test_shared_actors_are_one_object_and_scales_apply():
    lay, acts = PE.actor_layers([18] * 3, (((33, 32), PE.TANH),), 0, shared=True)
    assert lay[0] is lay[1] is lay[2] and acts == [PE.TANH] * 3
    a, _ = PE.actor_layers([18], (((20,), PE.RELU),), 5)
    b, _ = PE.actor_layers([18], (((20,), PE.RELU),), 5, scale=(2.0, 0.5))
    assert np.array_equal(b[0][0][0], 2 * a[0][0][0]) and np.array_equal(b[0][1][1], a[0][1][1] / 2)


# ---- the band condition, on the reference alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweep", PE.SWEEPS)
def test_reference_alone_keeps_the_band_half_empty(sweep):
    """Per sweep, over every case's closed loop in fp64 (greedy and sample): rows inside the band <= half of CAP * rows + 1."""
    for mode in ("greedy", "sample"):
        rows = inband = 0
        for c in PE.CASES:
            if c.sweep != sweep or mode not in c.modes:
                continue
            n = 0
            for st in PE.closed_loop(c.id, mode):
                for ref in st["refs"]:
                    rows += c.B
                    n += int((~ref["heads"][0]["ok"]).sum())
            if n:
                print("%s %s: %d rows inside the band" % (c.id, mode, n))
            inband += n
        print("%s %s: %d of %d rows inside the band" % (sweep, mode, inband, rows))
        assert rows > 0 or (mode == "greedy" and sweep == "counters"), "the counter edges run in sample mode only"
        assert inband <= 0.5 * (R.CAP * rows + 1), (sweep, mode, inband, rows)


@pytest.mark.parametrize("cid", PE.CASE_IDS)
def test_fp32_alone_stays_under_a_quarter_of_the_bar(cid):
    c = PE.BY_ID[cid]
    layers, acts = PE.case_layers(c)
    worst = 0.0
    for mode in c.modes:
        for st in PE.closed_loop(cid, mode):
            for i, ref in enumerate(st["refs"]):
                p, lp, z = PE.f32_cost(layers[i], acts[i], st["obs"][i], ref, mode)
                worst = max(worst, z, p, lp if mode == "sample" else 0.0)
    print("%s: fp32 alone costs %.3f of the bar" % (cid, worst))
    assert worst < 0.25, (cid, worst)


def test_closed_loop_restarts_where_the_kernel_does():
    """the countdown of k_split restated: resets on global steps that are multiples of episode_len, episode = gt / episode_len"""
    c = PE.BY_ID["counters_step0"]
    steps = PE.closed_loop(c.id, "sample")
    assert [s["gt"] for s in steps if s["restart"]] == [2 ** 32 - 1, 2 ** 32 + 2]
    ep = (2 ** 32 + 2) // 3
    want = philox.reset_positions(c.world_seed, c.B, ep, 3, 3, 1.0, c.world_offset)
    assert np.array_equal(steps[5]["start"][0], want.astype(np.float64))
    c = PE.BY_ID["episode_spread3_L1"]
    assert all(s["restart"] for s in PE.closed_loop(c.id, "greedy"))
    c = PE.BY_ID["episode_spread3_L0"]
    steps = PE.closed_loop(c.id, "greedy")
    assert not any(s["restart"] for s in steps)
    assert np.array_equal(steps[0]["start"][0], PE.initial_state(c)[0].astype(np.float64))


# ---- mutations: the GPU comparison would notice -----------------------------------------------------------------------------------------
def _as_kernel_output(ref, mode):
    d = ref["heads"][0]
    return PE.ref_rows(ref, mode).astype(np.float32), (ref["logp"].astype(np.float32) if mode == "sample" else None)


@pytest.mark.parametrize("name", sorted(PE.DECISION_MUTATIONS))
def test_a_wrong_decision_rule_misses_the_bars(name):
    """the wrong variant's rows, fed to the comparison the GPU test uses on the recorded decision inputs: >= 10 % of the rows
    checked miss a bar or stand for another index; the right variant's rows miss none"""
    cid, mode = PE.DECISION_MUTATIONS[name]
    c = PE.BY_ID[cid]
    layers, acts = PE.case_layers(c)
    rows = bad = moved = clean = 0
    for st in PE.closed_loop(cid, mode):
        for i, ref in enumerate(st["refs"]):
            lay, act, kw = PE.mutate_decision(name, layers[i], acts[i], dict(seed=c.policy_seed, t=st["gt"], world_offset=c.world_offset))
            wrong = R.ref_decide(lay, act, 1, 0, 0, st["obs"][i], mode, kw["seed"], kw["t"], i, kw["world_offset"])
            got = PE.compare(*_as_kernel_output(wrong, mode), ref, mode)
            rows += c.B
            bad += int(got["bad"].sum())
            moved += int((wrong["heads"][0]["chosen"] != ref["heads"][0]["chosen"]).sum())
            clean += int(PE.compare(*_as_kernel_output(ref, mode), ref, mode)["bad"].sum())
    print("%s on %s (%s): %d of %d rows miss a bar, %d indices moved" % (name, cid, mode, bad, rows, moved))
    assert clean == 0
    assert bad >= 0.1 * rows or moved >= 0.1 * rows, (name, bad, moved, rows)


def test_ties_to_the_highest_index_are_noticed():
    case, layers, acts = PE.known_equal_logits()
    obs = PE.known_obs(case)
    for i in range(3):
        ref = R.ref_decide(layers[i], acts[i], 1, 0, 0, obs[0][i], "greedy", case.policy_seed, 0, i, case.world_offset)
        assert (ref["z"] == 0.5).all() and (ref["heads"][0]["greedy"] == 0).all()
        assert (PE.ties_to_highest(ref) == 4).all()      # every index moves: the known-answer test asserts index 0


@pytest.mark.parametrize("cid", [c.id for c in PE.CASES if c.sweep == "constants"])
def test_accel_of_five_for_everyone_is_noticed(cid):
    """a step that decodes the row with the default sensitivity where the agent has an accel of its own: from each step's start
    state, with the reference's own rows, >= 10 % of the worlds end more than 10 bars (1e-4 scaled) away"""
    c = PE.BY_ID[cid]
    spec = PE.case_spec(c)
    wrong = dataclasses.replace(spec, accel=[None] * spec.n_agents)
    far = n = 0
    for st in PE.closed_loop(cid, "sample"):
        orc = PE.oracle_of(c, spec=wrong)
        PE.set_oracle(orc, *st["start"])
        orc.step(st["rows"])
        err = (np.abs(orc.pos - st["pos"]) / np.maximum(1.0, np.abs(st["pos"]))).max(axis=(1, 2))
        far += int((err > 1e-4).sum())
        n += c.B
    print("%s: %d of %d world-steps move under accel = 5" % (cid, far, n))
    assert far >= 0.1 * n


def test_an_episode_index_off_by_one_is_noticed():
    c = PE.BY_ID["mixed_set"]
    far = n = 0
    for st in PE.closed_loop(c.id, "greedy"):
        if not st["restart"]:
            continue
        orc = PE.oracle_of(c)
        PE.set_oracle(orc, *PE.restart_state(c, st["gt"] // c.episode_len + 1))
        for i, o in enumerate(orc.observe()):
            err = (np.abs(o - st["obs"][i]) / np.maximum(1.0, np.abs(st["obs"][i]))).max(axis=1)
            far += int((err > 1e-5).sum())
            n += c.B
    assert n == 3 * 3 * c.B and far >= 0.1 * n, (far, n)


# ---- the known-answer set-ups are what they say -------------------------------------------------------------------------------------------
def test_known_answer_actors():
    case, layers, acts, small = PE.known_saturated_tanh()
    assert min(small) > 50 and all(a == PE.TANH for a in acts), small
    case, layers, acts, margins = PE.known_large_logits()
    assert min(margins) > 200, margins
    obs = PE.known_obs(case)
    for i in range(3):
        ref = R.ref_decide(layers[i], acts[i], 1, 0, 0, obs[3][i], "sample", case.policy_seed, 3, i, case.world_offset)
        d = ref["heads"][0]
        assert (d["p"].max(axis=1) == 1.0).all() and np.array_equal(d["sample"], d["greedy"]) and (ref["logp"] == 0).all()
