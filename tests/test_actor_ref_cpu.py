"""CPU: the helpers of tests/_actor_ref.py before any device sees them -- ref_decide (NumPy fp64, written from include/mpe_hip.h)
against torch in fp64, the packed layout against policy.pack_actor16, and, for every case of the table the GPU file walks, the two
conditions that keep that file's bars honest: the fp64 reference itself leaves at most half the 0.1 % cap's share of a case's rows
inside the band, and a plain fp32 pass (ref_f32) stays inside the bars the kernel is held to."""
import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import policy
from multiagent_particle_envs_amd.policy import Actors

import _actor_ref as R


@pytest.fixture(scope="module")
def spread_env():
    return mpe.make_env("simple_spread", batch_size=8, device="cpu")


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_ref_decide_against_torch_fp64(name, spread_env):
    c = R.CASES[R.CASE_NAMES.index(name)]
    agents, obs = R.build_case(c)
    refs = R.case_refs(c, "sample", agents, obs)
    for i, (a, ref) in enumerate(zip(agents, refs)):
        x = torch.as_tensor(obs[i])
        if len(agents) == 1 and x.shape[1] == 18 and a["movable"] and not a["speaks"]:
            # simple_spread's shape: through Actors.reference (one module every agent shares)
            pi = Actors(spread_env, R.as_module(a["layers"], a["act"]))
            zm, zc = pi.reference([x] * 3)[0]
            assert zc is None
            heads = [zm, None]
        else:
            with torch.no_grad():
                z = R.as_module(a["layers"], a["act"], torch.float64)(x.double())
            heads = [z[:, :5] if a["movable"] else None, z[:, z.shape[1] - c["dim_c"]:] if a["speaks"] else None]
        for h, zt in enumerate(heads):
            d = ref["heads"][h]
            assert (zt is None) == (d is None)
            if zt is None:
                continue
            scale = max(1.0, float(zt.abs().max()))
            assert float(np.abs(zt.numpy() - d["z"]).max()) < 1e-12 * scale, (name, i, h)
            assert float(np.abs(torch.softmax(zt, dim=-1).numpy() - d["p"]).max()) < 1e-12
            assert float(np.abs(torch.log_softmax(zt, dim=-1).numpy() - d["logsm"]).max()) < 1e-12 * scale
            # argmax: equal wherever the top two differ at all (ties go to the lowest index in both)
            assert np.array_equal(zt.argmax(dim=-1).numpy(), d["greedy"])
            assert ((d["sample"] >= 0) & (d["sample"] < zt.shape[1])).all() and ((d["u"] >= 0) & (d["u"] < 1)).all()
            cum = torch.cumsum(torch.softmax(zt, dim=-1), dim=-1).numpy()
            lo = np.where(d["sample"] > 0, np.take_along_axis(cum, np.maximum(d["sample"] - 1, 0)[:, None], 1)[:, 0], 0.0)
            hi = np.where(d["sample"] < zt.shape[1] - 1, np.take_along_axis(cum, d["sample"][:, None], 1)[:, 0], 2.0)
            assert ((lo <= d["u"] + 1e-12) & (d["u"] < hi + 1e-12)).all(), (name, i, h, "the pick is not the inverse CDF of u")


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_case_cap_and_tolerance_conditions(name):
    c = R.CASES[R.CASE_NAMES.index(name)]
    agents, obs = R.build_case(c)
    for mode in ("greedy", "sample"):
        refs = R.case_refs(c, mode, agents, obs)
        checked = sum(ref["z"].shape[0] for ref in refs for d in ref["heads"] if d is not None)
        inband = sum(int((~d["ok"]).sum()) for ref in refs for d in ref["heads"] if d is not None)
        assert inband <= 0.5 * R.CAP * checked, "%s %s: %d of %d rows inside the band: move the case's seed" % (name, mode, inband, checked)
        for i, (a, ref) in enumerate(zip(agents, refs)):
            f32 = R.ref_f32(a["layers"], a["act"], a["movable"], a["speaks"], c["dim_c"], obs[i],
                            chosen=[d["chosen"] if d is not None else None for d in ref["heads"]])
            assert np.isfinite(f32["z"]).all()
            assert (np.abs(f32["z"] - ref["z"]).max(axis=1) < R.BAND * ref["scale"]).all(), (name, i, "fp32 logits")
            for h, d in enumerate(ref["heads"]):
                if d is not None:
                    assert (np.abs(f32["heads"][h]["p"] - d["p"]).max(axis=1) < R.BAND * d["scale"]).all(), (name, i, h, "fp32 softmax")
            assert (np.abs(f32["logp"] - ref["logp"]) < R.logp_bar(ref)).all(), (name, i, "fp32 logp")
    if c["zmax"] is not None:
        zs = [float(np.abs(ref["z"]).max()) for ref in refs]
        assert all(abs(z - c["zmax"]) < 0.01 * c["zmax"] for z in zs), zs


def test_large_logits_underflow_fp32_in_the_reference():
    """at max|z| = 80 the fp64 softmax has entries no normal float32 holds: the kernel's exp underflows there"""
    c = R.CASES[R.CASE_NAMES.index("large_logits_80")]
    ref = R.case_refs(c, "greedy")[0]
    tiny = float(np.finfo(np.float32).tiny)
    assert any(bool((d["p"] < tiny).any()) for d in ref["heads"])
    assert all(np.isfinite(d["logsm"]).all() for d in ref["heads"])
    assert np.isfinite(ref["logp"]).all() and float(ref["logp"].max()) <= 0


def test_case_table_covers_what_it_says():
    by = {}
    for c in R.CASES:
        by.setdefault(c["sweep"], []).append(c)
    assert sorted(by) == ["batch", "heads", "hidden_width", "input_width", "large_logits"]
    assert sorted({c["specs"][0]["D"] for c in by["input_width"]}) == list(R.INPUT_WIDTHS) and len(by["input_width"]) == 26
    assert {c["specs"][0]["hidden"] for c in by["hidden_width"]} == set(R.HIDDEN_WIDTHS) and len(by["hidden_width"]) == 18
    assert sorted(c["B"] for c in by["batch"]) == sorted(R.BATCHES + (257,))
    kinds = {(s["movable"], s["speaks"], c["dim_c"] * s["speaks"]) for c in by["heads"] for s in c["specs"]}
    assert kinds >= set(R.HEAD_KINDS)
    for c in by["heads"]:
        if len(c["specs"]) == 16:
            assert len({s["D"] for s in c["specs"]}) == 16 and c["B"] == 257
    assert len(set(R.CASE_NAMES)) == len(R.CASES)


@pytest.mark.parametrize("width", [1, 31, 32, 33, 63, 64])
@pytest.mark.parametrize("n_layers", [1, 2, 3])
def test_pack_is_pack_actor16(width, n_layers):
    rs = np.random.RandomState(width * 4 + n_layers)
    hidden = {1: (), 2: (width,), 3: (width, 64 if width % 2 else 20)}[n_layers]
    for D, n_out in [(width if n_layers == 1 else 18, n) for n in (5, 16, 1)] + [(1, 5), (256, 16)]:      # + the input width's two ends
        layers = R.make_layers(rs, D, hidden, n_out)
        want = policy.pack_actor16(R.as_module(layers, R.TANH), n_out).numpy()
        got = R.pack(layers)
        assert got.dtype == np.float32 and got.size % 16 == 0
        assert got.tobytes() == want.tobytes()
        # a Linear layer built with bias=False packs what a zero bias packs
        m = R.as_module(layers, R.TANH)
        m[0].bias = None
        assert R.pack([(layers[0][0], np.zeros_like(layers[0][1]))] + layers[1:]).tobytes() == policy.pack_actor16(m, n_out).numpy().tobytes()
    if n_layers == 3:      # the narrow layer second
        layers = R.make_layers(rs, D, (64, width), 5)
        assert R.pack(layers).tobytes() == policy.pack_actor16(R.as_module(layers, R.RELU), 5).numpy().tobytes()


def test_draw_u_is_the_counter_layout_of_the_gpu_file():
    """the same words as draw_bits of tests/test_gpu_actor.py (restated here: that module needs a device to import its envs)"""
    from oracle import philox
    B, t, off, seed = 70, R.BIG_STEP, R.BIG_OFFSET, 0x1234567890ABCDEF
    b = np.arange(B, dtype=np.uint64) + np.uint64(off)
    for stream in (R.STREAM_POLICY, R.STREAM_POLICY_COMM):
        for agent in (0, 3, 4, 15):
            o = philox.philox4x32_10(b & philox.MASK, ((b >> np.uint64(32)) ^ np.uint64(t >> 32)) & philox.MASK,
                                     np.full(B, agent // 4, np.uint64), np.full(B, (stream ^ (t & 0xFFFFFFFF)) & 0xFFFFFFFF, np.uint64),
                                     seed & 0xFFFFFFFF, seed >> 32)
            want = (o[agent % 4] >> np.uint32(8)).astype(np.float64) / 16777216.0
            assert np.array_equal(R.draw_u(stream, seed, B, t, agent, off), want)
    assert int(b[0] >> np.uint64(32)) > 0      # the offset reaches the counter's high word
