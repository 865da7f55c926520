"""GPU: `mpe_render` (csrc/mpe_render.hip) at its C entry point on the hand-built cases of tests/_render_edges.py -- blocks inside
one pixel row, blocks across frames and viewers, per-frame colours with a world list, sub-pixel and frame-filling entities, the
64-entity chunks of the cull, cameras far from the origin, non-finite positions, alpha and colours off [0, 1] -- against the
NumPy rule (tests/_render_ref.py) under the bar of tests/test_gpu_render.py: every differing pixel is a knife-edge pixel of the
reference, and they are at most 0.01 % of the case's pixels.  The frames sit between sentinel bytes, a second launch gives the
same bytes, and the facts a case exists for are read off the frames directly.  tests/test_render_edges_cpu.py holds the table
to its caps and paths first."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_edges as X  # noqa: E402
import _render_ref as R  # noqa: E402
from test_gpu_render import _check, _host_pos  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd import _abi  # noqa: E402

pytestmark = pytest.mark.gpu


def launch(case):
    """One `mpe_render` call of a case into the middle of a sentinel-filled buffer -> the whole buffer on the host."""
    dev = torch.device("cuda", torch.cuda.current_device())
    n = case.pixels * 3
    buf = torch.full((X.PAD + n + X.PAD,), X.SENTINEL, dtype=torch.uint8, device=dev)
    assert X.PAD % 16 == 0 and buf.data_ptr() % 16 == 0
    pos, rgba, worlds = (None if a is None else torch.as_tensor(a, device=dev) for a in X.device_arrays(case))
    desc, args, _cam = X.fill_args(case, pos.data_ptr(), rgba.data_ptr(), buf.data_ptr() + X.PAD,
                                   None if worlds is None else worlds.data_ptr())
    _abi.check(_abi.lib().mpe_render(C.byref(desc), C.byref(args), _abi.raw_stream(dev)), "mpe_render")
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def frames_of(case, host):
    return host[X.PAD:X.PAD + case.pixels * 3].reshape(case.V, case.K, case.size, case.size, 3)


def run_case(name, record_parity):
    """Launch twice, check the pads, the repeat and the bar; return (case, frames, reference)."""
    case = X.CASES[name]
    ref, knife = X.reference(name)
    host = launch(case)
    assert (host[:X.PAD] == X.SENTINEL).all(), "bytes in front of the frames were written"
    assert (host[-X.PAD:] == X.SENTINEL).all(), "bytes behind the frames were written"
    got = frames_of(case, host)
    assert got.shape == ref.shape
    bad = (got != ref).any(axis=-1)
    off = bad & ~knife
    print("%s: %d pixels, %d differ, %d of them off the knife edge, %d knife-edge pixels in the reference"
          % (name, bad.size, int(bad.sum()), int(off.sum()), int(knife.sum())))
    record_parity("render_edges_" + name, {"pixels": int(bad.size), "differing": int(bad.sum()), "off_knife": int(off.sum()),
                                           "knife": int(knife.sum())})
    assert not off.any(), "%d pixels differ off the knife edge, first at %s" % (int(off.sum()), np.argwhere(off)[:3].tolist())
    assert bad.sum() <= X.CAP * bad.size, int(bad.sum())
    assert np.array_equal(launch(case), host), "a second launch into a fresh buffer gave other bytes"
    for v in range(case.V):
        for k in range(case.K):
            assert (got[v, k] == 255).all() == ((v, k) in case.white), (v, k)
    return case, got, ref


PLAIN = [n for n in X.NAMES if not n.startswith("chunk_") and n not in ("per_frame_colours_world_list", "huge", "non_finite")]


@pytest.mark.parametrize("name", PLAIN)
def test_case_against_the_rule(name, record_parity):
    run_case(name, record_parity)


@pytest.mark.parametrize("name", ["chunk_64", "chunk_65", "chunk_512"])
def test_chunks_keep_the_draw_order(name, record_parity):
    case, got, _ = run_case(name, record_parity)
    for k, first, later in case.pairs:
        r, c = X.centre_pixel(case, k, later)
        assert tuple(got[0, k, r, c]) == tuple(R.q(v) for v in case.rgba[later, :3]), (k, first, later)
        ring = int(round(0.15 * case.size / 2))       # between the two radii the earlier one shows: both were drawn
        assert tuple(got[0, k, r, c + ring]) == tuple(R.q(v) for v in case.rgba[first, :3]), (k, first, later)


def test_per_frame_colours_world_list(record_parity):
    case, got, _ = run_case("per_frame_colours_world_list", record_parity)
    assert case.worlds[1] == case.worlds[2]
    for v in range(case.V):       # frames 1 and 2: the same world (the same pixels covered) in each frame's own colours
        assert np.array_equal((got[v, 1] != 255).any(axis=-1), (got[v, 2] != 255).any(axis=-1))
        assert not np.array_equal(got[v, 1], got[v, 2])
    # an opaque entity's centre pixel has frame k's colour of it, at world worlds[k]'s position, unless a later one covers it
    seen = 0
    for k in range(case.K):
        for e in range(case.E):
            if case.rgba[k, e, 3] != 1:
                continue
            p = case.pos[case.worlds[k], e]
            if any(np.hypot(*(case.pos[case.worlds[k], j] - p)) < case.sizes[j] + 0.1 for j in range(e + 1, case.E)):
                continue
            r, c = X.centre_pixel(case, k, e)
            assert tuple(got[0, k, r, c]) == tuple(R.q(v) for v in case.rgba[k, e, :3]), (k, e)
            seen += 1
    assert seen >= 2


def test_huge_entities_leave_no_white_pixel(record_parity):
    _, got, _ = run_case("huge", record_parity)
    assert not (got == 255).all(axis=-1).any()


def test_non_finite_positions_draw_nothing(record_parity):
    case, got, _ = run_case("non_finite", record_parity)
    assert (got[1] == 255).all()                  # the viewer centred on the NaN entity
    finite = [e for e in range(case.E) if np.isfinite(case.pos[:, e]).all()]
    assert finite == [0, 3, 4]
    sub = X.Case("finite_only", case.size, [-1, 0], case.sizes[finite], case.pos[:, finite], case.rgba[finite])
    alone = frames_of(sub, launch(sub))
    assert np.array_equal(got[0], alone[0]) and np.array_equal(got[2], alone[1])      # as if the others were absent


# ---- through env.render ---------------------------------------------------------------------------------------------------------
def test_world_list_with_per_world_colours():
    env = mpe.make_env("simple_adversary", batch_size=64, seed=6)     # (a seed whose picks differ among the worlds below)
    env.reset()                                   # per-world goal picks -> per-world colours
    sel = [5, 2, 2, 60]
    rgba = R.env_colours(env)[sel]
    assert not (np.array_equal(rgba[0], rgba[1]) and np.array_equal(rgba[0], rgba[3])), "the selected worlds share their goal"
    full = env.render("rgb_array", size=40)
    part = env.render("rgb_array", worlds=sel, size=40)
    assert len(full) == len(part) == 1 and part[0].shape == (4, 40, 40, 3)
    assert torch.equal(part[0], full[0][sel])
    _check(env, part, 40, worlds=sel)


def test_agent_view_far_from_the_origin():
    env = mpe.make_env("simple_tag", batch_size=8)
    env.shared_viewer = False
    rs = np.random.RandomState(23)
    pos = rs.uniform(-1.0, 1.0, size=(8, len(env.world.entities), 2)).astype(np.float32)
    pos[:, 1] = (1000.3, -999.7)
    pos[:, 4:] = pos[:, 1:2] + rs.uniform(-0.9, 0.9, size=pos[:, 4:].shape).astype(np.float32)     # the landmarks in its view
    env.world.set_state(pos)
    assert np.array_equal(_host_pos(env), pos)
    frames = env.render("rgb_array", size=64)
    assert len(frames) == env.n
    got, _ = _check(env, frames, 64)
    assert (got[1, :, 31:33, 31:33] != 255).any(axis=-1).all()       # the far agent's own disc on the middle pixels
    for v in (0, 2, 3):                                                # ... as every other agent's is in its own view
        assert (got[v, :, 31:33, 31:33] != 255).any(axis=-1).all()
    # the far view shows the landmarks beside the agent too: more than one 0.075 disc (a 2.4-pixel radius) can cover
    assert ((got[1] != 255).any(axis=-1).sum(axis=(1, 2)) > 40).all()
