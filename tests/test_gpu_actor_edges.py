"""GPU: mpe_actor_act at the level of its C entry point, on hand-built MpeActorSets -- the input widths, hidden widths, head kinds
and batch sizes no scenario has, large logits, known answers, neighbour isolation, the host contract and the refusals.

Every run goes through _actor_ref.run_abi (canary rows behind every output) and is compared with _actor_ref.ref_decide (NumPy
fp64, written from include/mpe_hip.h) under the project's bars: logits and softmax rows within 1e-5 * max(1, max|z|), indices and
one-hot rows exact outside the band, logp within three logit bars per head + 2e-6, rows inside the band counted and at most
0.1 % of the rows checked + 1.  tests/test_actor_ref_cpu.py holds the case table to those bars on the CPU first.

One set has one dim_c, so the head sweep's "all kinds in one 16-agent set" is three 16-agent sets (dim_c = 11, 1, 16), each with
every kind that dim_c admits."""
import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd.policy import Actors

import _actor_ref as R

pytestmark = pytest.mark.gpu

MODE_NAMES = ("greedy", "softmax", "sample")
_TALLY = {}


def tally(sweep, record_parity):
    t = _TALLY.setdefault(sweep, R.Tally())

    def done():
        rep = t.report()
        record_parity("actor_edges_" + sweep, rep)
        print("actor edges, %s so far: %s" % (sweep, rep))
        assert t.inband <= R.CAP * t.checked + 1
    return t, done


def run_and_check(agents, dim_c, obs, mode, t, world_offset, tl, tag, seed=9):
    out = R.run_abi(agents, dim_c, obs, mode, seed, t, world_offset)
    assert out["rc"] == 0, out["error"]
    tl.canary_ok = tl.canary_ok and out["canary_ok"]
    assert out["canary_ok"], (tag, "a store landed behind the last row")
    for name in ("moves", "utter", "logp", "logits"):      # every live element was written
        if out[name] is not None:
            assert not (out[name] == R.CANARY_F).any(), (tag, name, "rows the launch did not write")
    assert not (out["ids"] == R.CANARY_I).any(), (tag, "ids the launch did not write")
    before = (tl.checked, tl.inband)
    for i, a in enumerate(agents):
        ref = R.ref_decide(a["layers"], a["act"], a["movable"], a["speaks"], dim_c, obs[i], mode, seed, t, i, world_offset)
        R.check_agent(out, i, ref, mode, tl, tag)
    # the cap holds for this run alone too
    assert tl.inband - before[1] <= R.CAP * (tl.checked - before[0]) + 1, (tag, "rows inside the band")
    return out


@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_case_against_fp64(name, mode, record_parity):
    c = R.CASES[R.CASE_NAMES.index(name)]
    agents, obs = R.build_case(c)
    tl, done = tally(c["sweep"], record_parity)
    run_and_check(agents, c["dim_c"], obs, mode, c["t"], c["world_offset"], tl, "%s %s" % (name, mode), seed=c["draw_seed"])
    done()


# ---- known answers ------------------------------------------------------------------------------------------------------------
def one_agent(rs, D, hidden, act, movable, speaks, dim_c):
    return {"layers": R.make_layers(rs, D, hidden, 5 * movable + dim_c * speaks), "act": act, "movable": movable, "speaks": speaks}


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_zero_last_layer_equal_biases(mode, record_parity):
    """every logit is the same float: greedy picks index 0 (the tie rule), the softmax row is 1/n, logp = -log n, and the sample
    pick is the cell of u in the grid j/n.  The kernel's cumulative sums are at most 16 roundings of ulp(1)/2 off j/n (< 1e-6):
    rows whose u is that close to a grid point are counted and left out."""
    rs = np.random.RandomState(5)
    B, dim_c, seed, t, off = 1000, 11, 31, 7, 12345
    a = one_agent(rs, 18, (64, 64), R.RELU, 1, 1, dim_c)
    W, b = a["layers"][-1]
    a["layers"][-1] = (np.zeros_like(W), np.full_like(b, 0.5))
    obs = [rs.uniform(-1, 1, (B, 18)).astype(np.float32)]
    out = R.run_abi([a], dim_c, obs, mode, seed, t, off)
    assert out["rc"] == 0 and out["canary_ok"]
    assert (out["logits"][0].view(np.uint32) == np.float32(0.5).view(np.uint32)).all()
    assert (out["ids"][:, 0] == 0).all() if mode != "sample" else True
    want_lp = np.zeros(B)
    inband = 0
    for h, (rows, n, stream) in enumerate(((out["moves"][0], 5, R.STREAM_POLICY), (out["utter"][0], dim_c, R.STREAM_POLICY_COMM))):
        if mode == "softmax":
            assert float(np.abs(rows.astype(np.float64) - 1.0 / n).max()) <= 2.0 ** -23 / n, h
        elif mode == "greedy":
            assert (rows[:, 0] == 1).all() and (rows[:, 1:] == 0).all(), h
        else:
            u = R.draw_u(stream, seed, B, t, 0, off)
            grid = np.arange(1, n) / n
            want = np.minimum((grid[None, :] <= u[:, None]).sum(axis=1), n - 1)
            ok = (np.abs(grid[None, :] - u[:, None]) > 1e-6).all(axis=1)
            inband += int((~ok).sum())
            assert np.array_equal(out["ids"][h, 0][ok], want[ok]), h
            assert np.array_equal(rows.argmax(axis=1), out["ids"][h, 0]) and (rows.sum(axis=1) == 1).all() and (rows.max(axis=1) == 1).all()
            assert len(np.unique(out["ids"][h, 0])) == n, (h, "some index is never drawn in 1000 rows")
        want_lp -= np.log(n)
    assert float(np.abs(out["logp"][0] - want_lp).max()) <= 2e-6
    print("zero last layer %s: %d of %d sample rows within 1e-6 of a grid point" % (mode, inband, 2 * B))
    assert inband <= R.CAP * 2 * B + 1
    record_parity("actor_edges_known_equal_logits_" + mode, {"rows_checked": 2 * B, "rows_in_band": inband,
                                                             "worst_logp_error": float(np.abs(out["logp"][0] - want_lp).max())})


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_zero_observation_is_the_bias_only_pass(mode, record_parity):
    rs = np.random.RandomState(6)
    B, dim_c = 130, 4
    agents = [one_agent(rs, 18, (64, 20), R.TANH, 1, 1, dim_c), one_agent(rs, 65, (), R.RELU, 0, 1, dim_c)]
    obs = [np.zeros((B, 18), np.float32), np.zeros((B, 65), np.float32)]
    tl, done = tally("known_answers", record_parity)
    out = run_and_check(agents, dim_c, obs, mode, 3, 0, tl, "zero obs " + mode)
    for i, a in enumerate(agents):
        assert (out["logits"][i].view(np.uint32) == out["logits"][i][0].view(np.uint32)).all(), (i, "worlds differ on equal inputs")
    # the one-layer agent: its logits are its bias, exactly
    assert np.array_equal(out["logits"][1][:, :dim_c], np.broadcast_to(agents[1]["layers"][0][1], (B, dim_c)))
    done()


def test_tanh_saturates_to_one_without_nan(record_parity):
    """first-layer biases of +-100: exp2 overflows (or is 0) inside the Tanh; the activation is +-1 within 2e-7, read through a last
    layer that is the identity on units 0..4"""
    rs = np.random.RandomState(7)
    B = 200
    a = one_agent(rs, 18, (64,), R.TANH, 1, 0, 0)
    sign = np.where(np.arange(64) % 2 == 0, 1.0, -1.0).astype(np.float32)
    a["layers"][0] = (a["layers"][0][0], 100.0 * sign)
    eye = np.zeros((5, 64), np.float32)
    eye[np.arange(5), np.arange(5)] = 1.0
    a["layers"][1] = (eye, np.zeros(5, np.float32))
    obs = [rs.uniform(-1, 1, (B, 18)).astype(np.float32)]
    want = sign[:5].astype(np.float64)
    p = np.exp(want) / np.exp(want).sum()
    for mode in MODE_NAMES:      # (units 0, 2 and 4 tie at +1: every row is inside the greedy band, so no tally here)
        out = R.run_abi([a], 0, obs, mode, 9, 3, 0)
        assert out["rc"] == 0 and out["canary_ok"]
        z = out["logits"][0][:, :5].astype(np.float64)
        assert not np.isnan(out["logits"][0]).any() and not np.isnan(out["moves"][0]).any() and np.isfinite(out["logp"][0]).all()
        assert float(np.abs(z - want).max()) <= 2e-7
        if mode == "greedy":      # the tie rule again: the first of the three +1 units
            assert (out["ids"][0, 0] == 0).all() and (out["moves"][0][:, 0] == 1).all()
        if mode == "softmax":
            assert float(np.abs(out["moves"][0] - p).max()) < 1e-5
    record_parity("actor_edges_known_tanh_saturation", {"rows_checked": 3 * B, "worst_activation_error": float(np.abs(z - want).max())})


def test_duplicate_output_columns_go_to_the_lower_index(record_parity):
    """columns j < k of the last layer equal: z_j == z_k bit for bit, and greedy never answers k"""
    rs = np.random.RandomState(8)
    B, dim_c = 2000, 6
    a = one_agent(rs, 18, (33,), R.RELU, 1, 1, dim_c)
    W, b = a["layers"][-1]
    b[:] = 0      # (no column wins on its bias alone: every column is the maximum on some rows)
    for j, k in ((1, 3), (5 + 0, 5 + 4), (5 + 2, 5 + 5)):
        W[k], b[k] = W[j], b[j]
    obs = [rs.uniform(-1, 1, (B, 18)).astype(np.float32)]
    out = R.run_abi([a], dim_c, obs, "greedy", 9, 3, 0)
    assert out["rc"] == 0 and out["canary_ok"]
    z = out["logits"][0]
    assert np.array_equal(z[:, 1], z[:, 3]) and np.array_equal(z[:, 5], z[:, 9]) and np.array_equal(z[:, 7], z[:, 10])
    mv, ut = out["ids"][0, 0], out["ids"][1, 0]
    assert not (mv == 3).any() and not (ut == 4).any() and not (ut == 5).any()
    # ... although those columns do win: rows where the pair is the strict maximum of the head answer j
    top_m = (z[:, 1:2] > z[:, [0, 2, 4]]).all(axis=1)
    top_c = (z[:, 5:6] > z[:, [6, 7, 8]]).all(axis=1)
    assert top_m.sum() > 20 and top_c.sum() > 20
    assert (mv[top_m] == 1).all() and (ut[top_c] == 0).all()
    assert (out["moves"][0][top_m, 1] == 1).all() and (out["utter"][0][top_c, 0] == 1).all()
    record_parity("actor_edges_known_duplicate_columns", {"rows_checked": 2 * B, "rows_where_the_pair_wins": int(top_m.sum() + top_c.sum())})


# ---- isolation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODE_NAMES)
def test_a_poisoned_world_stays_alone(mode):
    """one world's rows NaN, another's +-inf: every other world's outputs are what a clean run gives, bit for bit.  (Odd input widths:
    the world in front of a poisoned one is the one whose masked last column sits on the poisoned row.)"""
    rs = np.random.RandomState(11)
    B, dim_c = 300, 3
    agents = [one_agent(rs, 33, (64, 64), R.RELU, 1, 1, dim_c), one_agent(rs, 7, (), R.RELU, 1, 0, dim_c),
              one_agent(rs, 1, (20,), R.TANH, 0, 1, dim_c)]
    clean = [rs.uniform(-1, 1, (B, a["layers"][0][0].shape[1])).astype(np.float32) for a in agents]
    bad = [o.copy() for o in clean]
    for o in bad:
        o[100] = np.nan
        o[200] = np.where(np.arange(o.shape[1]) % 2 == 0, np.inf, -np.inf)
    a = R.run_abi(agents, dim_c, clean, mode, 9, 3, 0)
    b = R.run_abi(agents, dim_c, bad, mode, 9, 3, 0)
    assert a["rc"] == 0 and b["rc"] == 0 and a["canary_ok"] and b["canary_ok"]
    keep = np.ones(B, bool)
    keep[[100, 200]] = False
    for name in ("moves", "utter", "logp", "logits"):
        x, y = a[name][:, keep], b[name][:, keep]
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (name, "a poisoned world reached its neighbours")
    assert np.array_equal(a["ids"][:, :, keep], b["ids"][:, :, keep])


# ---- the host contract, through Actors ----------------------------------------------------------------------------------------
def test_actors_see_in_place_updates_unless_frozen():
    B = 256
    env = mpe.make_env("simple_spread", batch_size=B, seed=7)
    env.reset()
    torch.manual_seed(3)
    mod = torch.nn.Sequential(torch.nn.Linear(18, 33), torch.nn.Tanh(), torch.nn.Linear(33, 5)).cuda()
    pi = Actors(env, mod, mode="softmax", logits=True)
    gen = torch.Generator(device="cuda").manual_seed(1)
    obs_n = [torch.rand((B, 18), generator=gen, device="cuda") * 2 - 1 for _ in range(3)]

    def logits():
        pi.act(obs_n, 0)
        torch.cuda.synchronize()
        return pi.logits.clone()

    def close_to_reference(z):
        ref = pi.reference(obs_n)
        for i in range(3):
            assert float((z[i, :, :5].double() - ref[i][0]).abs().max()) < 1e-5 * max(1.0, float(ref[i][0].abs().max()))

    def update(step):
        with torch.no_grad():
            mod[2].bias.add_(step)
            mod[0].weight.mul_(1.25)

    z0 = logits()
    close_to_reference(z0)
    update(0.5)
    z1 = logits()
    assert not torch.equal(z0, z1)
    close_to_reference(z1)                 # an in-place update is seen
    assert pi.freeze() is pi
    assert torch.equal(logits(), z1)
    update(-0.25)
    assert torch.equal(logits(), z1)       # frozen: not seen ...
    pi.freeze()
    z2 = logits()
    assert not torch.equal(z2, z1)         # ... until freeze() is called again
    close_to_reference(z2)
    update(0.125)
    assert torch.equal(logits(), z2)
    assert pi.unfreeze() is pi
    z3 = logits()
    assert not torch.equal(z3, z2)         # unfreeze(): seen again, at every act()
    close_to_reference(z3)
    update(0.0625)
    z4 = logits()
    assert not torch.equal(z4, z3)
    close_to_reference(z4)


# ---- refusals, through the C entry ----------------------------------------------------------------------------------------------
def test_refusals_by_name_leave_the_outputs_untouched():
    rs = np.random.RandomState(12)
    B = 70
    agents = [one_agent(rs, 18, (64,), R.RELU, 1, 1, 3), one_agent(rs, 18, (64,), R.RELU, 1, 0, 3)]
    obs = [rs.uniform(-1, 1, (B, 18)).astype(np.float32) for _ in agents]
    good = R.run_abi(agents, 3, obs, "greedy", 9, 3, 0)
    assert good["rc"] == 0 and not good["untouched"] and good["canary_ok"]
    size0 = R.pack(agents[0]["layers"]).size
    for kw, needle in (({"offsets": [0, size0 - 8]}, "offset"), ({"offsets": [4, size0]}, "offset"),
                       ({"misalign": "weights"}, "weights"), ({"misalign": "logits"}, "logits")):
        out = R.run_abi(agents, 3, obs, "greedy", 9, 3, 0, **kw)
        assert out["rc"] != 0, kw
        assert needle in out["error"] and "mpe_actor_act" in out["error"], (kw, out["error"])
        assert out["untouched"], (kw, "a refused call wrote")
    out = R.run_abi(agents, 3, [o[:0] for o in obs], "greedy", 9, 3, 0, B=0)
    assert out["rc"] == 0 and out["untouched"]
