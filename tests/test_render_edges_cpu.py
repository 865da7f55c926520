"""The case table of tests/_render_edges.py held to its own claims without a GPU: every case's knife-edge share under the NumPy
rule (tests/_render_ref.py) stays inside the cap the GPU tests rely on, every case reaches the path it is named for (by the
index arithmetic of the output alone: size, V, K and the 1024 pixels of a block), and the three-normal shortcut of the kernel
holds the 30-normal max on sector boundaries, at the magnitudes a far camera gives, with the quotient a few ulps off."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_edges as X  # noqa: E402
import _render_ref as R  # noqa: E402

F = np.float32
ROW_BLOCKS = ["row_blocks_1024", "row_blocks_2048", "row_blocks_1536", "row_blocks_4096"]


def test_the_table_holds_every_case_of_the_sweep():
    assert set(X.NAMES) == {
        "row_blocks_1024", "row_blocks_2048", "row_blocks_1536", "row_blocks_4096", "tiny_frames_viewers", "odd_tail_viewers",
        "per_frame_colours_world_list", "subpixel_8", "subpixel_64", "huge", "chunk_64", "chunk_65", "chunk_512",
        "far_camera_64", "far_camera_1024", "non_finite", "alpha_and_clamp"}


@pytest.mark.parametrize("name", X.NAMES)
def test_knife_share_and_drawn_frames(name):
    c = X.CASES[name]
    ref, knife = X.reference(name)
    assert ref.shape == (c.V, c.K, c.size, c.size, 3) and knife.shape == ref.shape[:-1]
    n = int(knife.sum())
    print("%s: %d pixels, %d on a knife edge" % (name, c.pixels, n))
    assert n <= X.CAP * c.pixels, (n, c.pixels)
    if c.pixels < 10000:          # 1e-4 of them is no pixel at all
        assert n == 0, n
    for v in range(c.V):
        for k in range(c.K):
            assert (ref[v, k] == 255).all() == ((v, k) in c.white), (v, k)


# ---- the paths, from the index arithmetic of the output -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROW_BLOCKS)
def test_row_blocks_lie_inside_one_row(name):
    c = X.CASES[name]
    assert (c.V, c.K) == (1, 1)
    parts = [p for block in X.block_parts(c.size, c.V, c.K) for p in block]
    one_row = [(qa, qb) for _, qa, qb in parts if qa // c.size == qb // c.size]
    inner = [(qa, qb) for qa, qb in one_row if qa % c.size > 0]
    print("%s: %d blocks, %d inside one row, %d of them starting past column 0" % (name, len(parts), len(one_row), len(inner)))
    if c.size == 1024:            # a block is a whole row: column 0 .. 1023 of row b, never a sub-range
        assert len(one_row) == len(parts) == 1024
        assert all((qa % 1024, qb % 1024) == (0, 1023) for _, qa, qb in parts)
    else:
        assert inner
    if c.size == 1536:            # one-row and two-row blocks alternate
        kinds = [qa // c.size == qb // c.size for _, qa, qb in parts]
        assert kinds[:6] == [True, False, True, True, False, True] and all(a or b for a, b in zip(kinds, kinds[1:]))
    if c.size in (2048, 4096):    # half-row / quarter-row blocks
        assert len(one_row) == len(parts) and {qa % c.size for qa, _ in one_row} == set(range(0, c.size, 1024))


def test_row_blocks_2048_entities_against_the_seam():
    c = X.CASES["row_blocks_2048"]
    xs, _ = R.pixel_centres(2048, 0.0, 0.0)
    h = 1.0 / 2048

    def columns(e, reach):
        return np.nonzero(np.abs(xs.astype(np.float64) - float(c.pos[0, e, 0])) <= reach)[0]

    inside = columns(0, float(R.apothem(c.sizes[0])))              # the fill along the entity's own row
    assert 1023 in inside and 1024 in inside
    assert columns(1, float(c.sizes[1]) + 3 * h).max() < 1023      # everything entity 1 can reach: left half only
    assert columns(2, float(c.sizes[2]) + 3 * h).min() > 1024      # ... entity 2: right half only
    edge = columns(3, float(c.sizes[3]) + 1.0056 * h)              # entity 3's outline ends within two columns of the seam
    assert 1021 <= edge.max() <= 1023
    ref, _ = X.reference("row_blocks_2048")
    r, _ = X.centre_pixel(c, 0, 0)
    assert (ref[0, 0, r, 1023] != 255).any() and (ref[0, 0, r, 1024] != 255).any()


def test_row_blocks_4096_entities_on_every_seam():
    c = X.CASES["row_blocks_4096"]
    assert c.sizes.max() <= F(0.05)
    xs, _ = R.pixel_centres(4096, 0.0, 0.0)
    for e, seam in ((0, 1024), (1, 2048), (2, 3072)):
        cols = np.nonzero(np.abs(xs.astype(np.float64) - float(c.pos[0, e, 0])) <= float(R.apothem(c.sizes[e])))[0]
        assert seam - 1 in cols and seam in cols, (e, seam)


def test_tiny_frames_blocks_hold_several_viewers():
    c = X.CASES["tiny_frames_viewers"]
    assert (c.size, c.cameras, c.K, c.B, c.worlds) == (8, [-1, 0, 2, 1], 3, 5, [4, 0, 4])
    blocks = X.block_parts(c.size, c.V, c.K)
    assert len(blocks) == 1 and len(blocks[0]) == 12                      # all 12 frames in one block
    assert {img // c.K for img, _, _ in blocks[0]} == {0, 1, 2, 3}        # ... of four viewers
    c = X.CASES["odd_tail_viewers"]
    assert (c.size, c.V, c.K) == (11, 3, 5) and (c.size * c.size) % 16 != 0 and c.pixels % 16 != 0
    blocks = X.block_parts(c.size, c.V, c.K)
    assert len(blocks) == 2 and any(len({img // c.K for img, _, _ in b}) > 1 for b in blocks)
    assert all(qa == 0 or img == b[0][0] for b in blocks for img, qa, _ in b)


def test_per_frame_colours_are_distinct_and_worlds_repeat():
    c = X.CASES["per_frame_colours_world_list"]
    assert (c.size, c.K, c.B, c.worlds, c.V) == (32, 4, 9, [7, 2, 2, 0], 2) and c.rgba.shape == (4, c.E, 4)
    for a in range(4):
        for b in range(a + 1, 4):
            assert (np.abs(c.rgba[a, :, :3] - c.rgba[b, :, :3]).max(axis=1) > 0.01).all(), (a, b)
    for a in range(9):            # ... and no two worlds look alike, so a frame drawn from world k instead of worlds[k] differs
        for b in range(a + 1, 9):
            assert np.abs(c.pos[a] - c.pos[b]).max() > 0.05
    ref, _ = X.reference(c.name)
    assert np.array_equal((ref[:, 1] != 255).any(axis=-1), (ref[:, 2] != 255).any(axis=-1))    # the same world ...
    assert not np.array_equal(ref[:, 1], ref[:, 2])                                             # ... in other colours


@pytest.mark.parametrize("name", ["subpixel_8", "subpixel_64"])
def test_subpixel_entities_have_no_inner_disc(name):
    c = X.CASES[name]
    h = F(1) / F(c.size)
    assert np.allclose(c.sizes[:4] * c.size, [1e-4 * c.size, 0.5, 1.0, 2.0]) and np.array_equal(c.sizes[:4], c.sizes[4:])
    assert all(R.apothem(s) - F(2) * h <= 0 for s in c.sizes)
    xs, ys = R.pixel_centres(c.size, 0.0, 0.0)
    for e in range(3):            # on a pixel centre to the bit: dx = dy = 0 there
        assert c.pos[0, e, 0] in xs and c.pos[0, e, 1] in ys
    s = F(2) / F(c.size)
    for e in range(4, 8):         # on a pixel corner
        assert (c.pos[0, e, 0] + F(1)) / s == np.round((c.pos[0, e, 0] + F(1)) / s)
        assert (F(1) - c.pos[0, e, 1]) / s == np.round((F(1) - c.pos[0, e, 1]) / s)


def test_huge_entities_cover_every_pixel():
    c = X.CASES["huge"]
    assert c.size == 96 and sorted(c.sizes.tolist()) == [1.5, 3.0]
    assert sorted(c.rgba[0, :, 3].tolist()) == [0.5, 1.0] and sorted(c.rgba[1, :, 3].tolist()) == [0.5, 1.0]
    assert {tuple(p) for p in c.pos.reshape(-1, 2).tolist()} == {(0.0, 0.0), (F(0.9).item(), F(-0.9).item())}
    ref, _ = X.reference("huge")
    assert not (ref == 255).all(axis=-1).any()
    assert len(np.unique(ref[0, 0].reshape(-1, 3), axis=0)) > 2       # the smaller one's outline crosses the frame


@pytest.mark.parametrize("name", ["chunk_64", "chunk_65", "chunk_512"])
def test_chunk_pairs_show_the_later_entity(name):
    c = X.CASES[name]
    assert (c.size, c.K, c.E) == (64, 2, int(name.split("_")[1]))
    want = {"chunk_64": {(0, 0, 63), (1, 62, 63)}, "chunk_65": {(0, 63, 64), (1, 0, 64)},
            "chunk_512": {(0, 0, 511), (0, 63, 64), (1, 0, 511), (1, 447, 448)}}[name]
    assert set(c.pairs) == want
    ref, _ = X.reference(name)
    for k, first, later in c.pairs:
        assert np.array_equal(c.pos[k, first], c.pos[k, later]) and c.sizes[first] > c.sizes[later]
        assert c.rgba[first, 3] == 1 and c.rgba[later, 3] == 1
        r, col = X.centre_pixel(c, k, later)
        assert tuple(ref[0, k, r, col]) == tuple(R.q(v) for v in c.rgba[later, :3]), (k, first, later)
        assert tuple(R.q(v) for v in c.rgba[later, :3]) != tuple(R.q(v) for v in c.rgba[first, :3])
        ring = int(round(0.15 * c.size / 2))      # between the two radii: the earlier one shows
        assert tuple(ref[0, k, r, col + ring]) == tuple(R.q(v) for v in c.rgba[first, :3]), (k, first, later)


@pytest.mark.parametrize("name", ["far_camera_64", "far_camera_1024"])
def test_far_cameras_and_their_neighbours(name):
    c = X.CASES[name]
    assert c.V == 2 and c.cameras == [0, 1]
    assert np.array_equal(c.pos[0, 0], F([1000.3, -999.7])) and np.array_equal(c.pos[0, 1], F([-37.25, 512.5]))
    for k in range(c.K):
        near = [np.abs(c.pos[k, 2:] - c.pos[k, cam]).max(axis=1) <= 1.0 for cam in (0, 1)]
        assert near[0].sum() >= 2 and near[1].sum() >= 2
    ref, _ = X.reference(name)
    mid = c.size // 2
    for v in range(2):            # each view is centred on its agent: its disc covers the middle pixels
        assert (ref[v, :, mid - 1:mid + 1, mid - 1:mid + 1] != 255).any(axis=-1).all()
        assert ((ref[v] != 255).any(axis=-1).sum(axis=(1, 2)) > (ref[v, :, mid, :] != 255).any(axis=-1).sum(axis=1)).all()


def test_non_finite_entities_leave_the_rest_as_it_is():
    c = X.CASES["non_finite"]
    assert (c.size, c.V, c.cameras[1]) == (32, 3, 1)
    assert np.isnan(c.pos[:, 1]).any(axis=1).all() and np.isinf(c.pos[:, 2]).any(axis=1).all()
    assert np.isnan(c.pos[0, 1]).all() and (c.pos[0, 2] == np.inf).all()
    finite = [0, 3, 4]
    assert np.isfinite(c.pos[:, finite]).all()
    ref, _ = X.reference("non_finite")
    for v, cam in ((0, -1), (2, 0)):
        alone, _ = R.render_frames(c.pos[:, finite], c.sizes[finite], c.rgba[finite], c.size, [cam])
        assert np.array_equal(ref[v], alone[0])
    assert (ref[1] == 255).all()


def test_alpha_and_clamp_values_overlap():
    c = X.CASES["alpha_and_clamp"]
    assert c.size == 48 and {0.0, 0.25, 1.0, 1.5, -0.5} <= set(c.rgba[:, 3].tolist())
    assert F(-0.3) in c.rgba[:, :3] and F(1.5) in c.rgba[:, :3]
    for e in range(1, c.E):       # every entity overlaps the first one
        assert np.hypot(*(c.pos[0, e] - c.pos[0, 0])) < c.sizes[e] + c.sizes[0]
    # ... and each odd alpha changes the picture: without that entity the reference differs (alpha 0 draws nothing)
    ref, _ = X.reference("alpha_and_clamp")
    for e in range(c.E):
        keep = [i for i in range(c.E) if i != e]
        other, _ = R.render_frame(c.pos[0, keep], c.sizes[keep], c.rgba[keep], c.size)
        assert np.array_equal(other, ref[0, 0]) == (c.rgba[e, 3] == 0), e


# ---- the three-normal shortcut on sector boundaries ------------------------------------------------------------------------------
def _ulps(x, n):
    """fp32 x moved by n units in its last place."""
    return (x + F(n) * np.spacing(np.abs(x))).astype(F)


def test_three_nearest_normals_hold_the_max_on_sector_boundaries():
    """tests/test_render_cpu.py draws random directions and divides exactly.  Here: every multiple of 6 degrees (the sector
    boundaries and the normals themselves), each component moved by 0, +-1, +-2 and +-16 ulps, at |d| from 1e-30 to 2e3 (a far
    camera's), and the quotient t moved by up to +-2 ulps where the kernel takes the hardware reciprocal.  The max over the
    estimated sector's normal and its two neighbours is still the fp32 value of the max over all 30."""
    moves = [0, 1, -1, 2, -2, 16, -16]
    ang = np.deg2rad(6.0 * np.arange(60))
    cx, cy = np.cos(ang).astype(F), np.sin(ang).astype(F)
    ux = np.stack([_ulps(cx, m) for m in moves])                        # [7, 60]
    uy = np.stack([_ulps(cy, m) for m in moves])
    mags = np.concatenate([np.logspace(-30, 3, 67), [0.7, 1.0, 1000.3, 1414.2, 2e3]]).astype(F)
    shape = (7, 7, 60, mags.size)
    dx = np.broadcast_to(ux[:, None, :, None] * mags, shape).ravel()
    dy = np.broadcast_to(uy[None, :, :, None] * mags, shape).ravel()
    assert dx.dtype == F and dy.dtype == F
    full = (R.NX[None] * dx[:, None] + R.NY[None] * dy[:, None]).max(axis=1)
    ax, ay = np.abs(dx), np.abs(dy)
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    t0 = np.where(mx > 0, mn / np.where(mx > 0, mx, F(1)), F(0)).astype(F)
    worst = 0
    for m in (0, 1, -1, 2, -2):
        t = _ulps(t0, m)
        th = t * (F(0.7853982) + F(0.273) * (F(1) - t))
        th = np.where(ay > ax, F(1.5707964) - th, th)
        th = np.where(dx < 0, F(3.1415927) - th, th)
        th = np.where(dy < 0, F(6.2831855) - th, th)
        k = np.clip(np.floor(th * (F(30) / F(6.2831855))).astype(int), 0, 29)
        cand = np.stack([(k + 29) % 30, k, (k + 1) % 30], axis=1)
        part = (R.NX[cand] * dx[:, None] + R.NY[cand] * dy[:, None]).max(axis=1)
        assert np.array_equal(part, full), (m, int((part != full).sum()))
        true_k = np.floor(np.degrees(np.arctan2(dy.astype(np.float64), dx.astype(np.float64))) % 360.0 / 12.0).astype(int) % 30
        off = np.minimum((k - true_k) % 30, (true_k - k) % 30)[mx > 0]
        worst = max(worst, int(off.max()))
    assert worst == 1            # the estimate does land in the neighbouring sector on some boundary, and never further
