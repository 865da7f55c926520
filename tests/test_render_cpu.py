"""The rendering rule ("Rendering") pinned without a GPU: the NumPy restatement tests/_render_ref.py
against values worked out by hand, the three-normal shortcut the kernel takes against the full 30-normal max, and the
host-side refusals of mpe_render / MultiAgentEnv.render."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_ref as R  # noqa: E402

from multiagent_particle_envs_amd import _abi  # noqa: E402

F = np.float32


def _sigma(x, y, ex, ey, size):
    d = (F(x) - F(ex), F(y) - F(ey))
    return (R.NX * d[0] + R.NY * d[1]).max() - R.apothem(size)


def test_opaque_landmark_at_the_origin():
    S, size, rgb = 100, 0.5, [0.2, 0.6, 0.4]
    img, knife = R.render_frame([[0.0, 0.0]], [size], [rgb + [1.0]], S)
    assert img.shape == (S, S, 3) and img.dtype == np.uint8
    assert tuple(img[S // 2, S // 2]) == tuple(R.q(v) for v in rgb)
    for r, c in ((0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)):
        assert tuple(img[r, c]) == (255, 255, 255)
    # the filled pixels cover the 30-gon's area, to within its perimeter (both in pixels)
    s = 2.0 / S
    area = 0.5 * 30 * size ** 2 * np.sin(2 * np.pi / 30) / s ** 2
    perimeter = 30 * 2 * size * np.sin(np.pi / 30) / s
    filled = int((img == np.array([R.q(v) for v in rgb], np.uint8)).all(axis=2).sum())
    assert abs(filled - area) <= perimeter, (filled, area, perimeter)
    # row 49 (y = 0.01), column 74 (x = 0.49): inside the fill and within half a pixel of the edge -> fill, then outline
    x, y = F(-1) + (F(74) + F(0.5)) * F(0.02), F(1) - (F(49) + F(0.5)) * F(0.02)
    sg = _sigma(x, y, 0.0, 0.0, size)
    assert -0.01 <= sg <= 0, sg
    want = []
    for v in rgb:
        fb = np.floor(F(v) * F(255) + F(0.5))                                    # the fill at alpha 1: q(v)
        f = (F(0.5) * F(v)) * (F(0.5) * F(1)) + (F(fb) / F(255)) * (F(1) - F(0.5))   # outline: rgb / 2 at alpha 1 / 2
        want.append(int(np.floor(f * F(255) + F(0.5))))
    assert tuple(img[49, 74]) == tuple(want)
    # column 75 (x = 0.51): more than half a pixel outside -> untouched
    assert _sigma(F(-1) + (F(75) + F(0.5)) * F(0.02), y, 0.0, 0.0, size) > 0.01
    assert tuple(img[49, 75]) == (255, 255, 255)
    assert not knife[49, 74] and not knife[49, 75]


def test_agent_alpha_and_draw_order():
    S, rgb = 64, [0.35, 0.35, 0.85]
    img, _ = R.render_frame([[0.0, 0.0]], [0.3], [rgb + [0.5]], S)
    assert tuple(img[S // 2, S // 2]) == tuple(R.q(F(0.5) * F(v) + F(0.5)) for v in rgb)
    # a landmark drawn after an overlapping agent wins where it is opaque
    land = [0.15, 0.65, 0.15]
    img, _ = R.render_frame([[0.0, 0.0], [0.0, 0.0]], [0.3, 0.1], [rgb + [0.5], land + [1.0]], S)
    assert tuple(img[S // 2, S // 2]) == tuple(R.q(v) for v in land)
    # ... and in the other order the agent tints it
    img, _ = R.render_frame([[0.0, 0.0], [0.0, 0.0]], [0.1, 0.3], [land + [1.0], rgb + [0.5]], S)
    assert tuple(img[S // 2, S // 2]) != tuple(R.q(v) for v in land)


def test_colours_are_clamped_and_size_scales():
    img, _ = R.render_frame([[0.0, 0.0]], [0.2], [[1.5, -0.3, 0.5, 1.0]], 64)
    assert tuple(img[32, 32]) == (255, 0, R.q(0.5))
    counts = []
    for S in (50, 100):
        img, _ = R.render_frame([[0.0, 0.0]], [0.4], [[0.0, 0.0, 0.0, 1.0]], S)
        counts.append(int((img == 0).all(axis=2).sum()))
    assert 3.6 < counts[1] / counts[0] < 4.4, counts


def test_row_zero_is_the_top():
    S = 64
    img, _ = R.render_frame([[0.0, 0.5]], [0.1], [[0.0, 0.0, 0.0, 1.0]], S)
    rows = np.nonzero((img != 255).any(axis=(1, 2)))[0]
    assert rows.max() < S // 2 and rows.min() > 0
    # a viewer centred on the entity puts it in the middle
    img, _ = R.render_frame([[0.0, 0.5]], [0.1], [[0.0, 0.0, 0.0, 1.0]], S, centre=(0.0, 0.5))
    rows = np.nonzero((img != 255).any(axis=(1, 2)))[0]
    assert rows.min() < S // 2 < rows.max()


def test_partly_outside_the_view_is_clipped():
    S = 64
    img, _ = R.render_frame([[1.02, 0.0]], [0.1], [[0.0, 0.0, 0.0, 1.0]], S)
    cols = np.nonzero((img != 255).any(axis=(0, 2)))[0]
    assert cols.size and cols.max() == S - 1 and cols.min() > S // 2     # the visible part at the right edge, nothing wrapped


def test_three_nearest_normals_hold_the_max():
    """The kernel's sigma takes the max over the normals of the sector the direction of d falls in and its two neighbours
    (the sector from a polynomial atan); over all 30 it is the same fp32 value."""
    rs = np.random.RandomState(0)
    d = (rs.uniform(-1, 1, size=(200000, 2)) * rs.choice([1e-4, 1e-2, 1.0], size=(200000, 1))).astype(F)
    d[:64] = 0
    d[64:128, 1] = 0
    d[128:192, 0] = 0
    full = (R.NX[None] * d[:, :1] + R.NY[None] * d[:, 1:]).max(axis=1)
    ax, ay = np.abs(d[:, 0]), np.abs(d[:, 1])
    mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
    t = np.where(mx > 0, mn / np.where(mx > 0, mx, F(1)), F(0)).astype(F)
    th = t * (F(0.7853982) + F(0.273) * (F(1) - t))
    th = np.where(ay > ax, F(1.5707964) - th, th)
    th = np.where(d[:, 0] < 0, F(3.1415927) - th, th)
    th = np.where(d[:, 1] < 0, F(6.2831855) - th, th)
    k = np.minimum(np.floor(th * F(30 / 6.2831855)).astype(int), 29)
    cand = np.stack([(k + 29) % 30, k, (k + 1) % 30], axis=1)
    part = (R.NX[cand] * d[:, :1] + R.NY[cand] * d[:, 1:]).max(axis=1)
    assert np.array_equal(part, full)


def test_render_abi_rejects_bad_arguments_without_a_gpu():
    L = _abi.lib()
    assert L.mpe_sizeof_render_args() == C.sizeof(_abi.MpeRenderArgs)
    d = _abi.MpeScenarioDesc()
    d.n_agents, d.n_landmarks = 3, 3
    for e in range(6):
        d.size[e] = 0.1
    buf = (C.c_float * 64)()
    out = (C.c_uint64 * 64)()        # 16-byte aligned host words stand in for device pointers: nothing is launched

    def args(**kw):
        a = _abi.MpeRenderArgs()
        a.pos, a.B, a.K, a.n_entities = C.addressof(buf), 4, 4, 6
        a.rgba, a.n_viewers, a.size, a.out = C.addressof(buf), 1, 64, (C.addressof(out) + 15) // 16 * 16
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def rejected(desc, a, words):
        assert L.mpe_render(desc, a, None) == -1
        msg = L.mpe_last_error().decode()
        assert "mpe_render" in msg and all(w in msg for w in words), msg

    rejected(None, C.byref(args()), ["desc"])
    rejected(C.byref(d), None, ["args"])
    rejected(C.byref(d), C.byref(args(pos=None)), ["pos"])
    rejected(C.byref(d), C.byref(args(out=None)), ["out"])
    rejected(C.byref(d), C.byref(args(K=0)), ["K"])
    rejected(C.byref(d), C.byref(args(K=5)), ["B"])           # worlds 0 .. K-1 of 4
    rejected(C.byref(d), C.byref(args(size=7)), ["size"])
    rejected(C.byref(d), C.byref(args(size=4097)), ["size"])
    rejected(C.byref(d), C.byref(args(n_entities=5)), ["n_entities"])
    rejected(C.byref(d), C.byref(args(n_viewers=0)), ["n_viewers"])
    rejected(C.byref(d), C.byref(args(rgba_world_stride=3)), ["rgba_world_stride"])
    rejected(C.byref(d), C.byref(args(out=args().out + 4)), ["aligned"])
    cam = (C.c_int32 * 2)(0, 6)
    rejected(C.byref(d), C.byref(args(n_viewers=2, camera=cam)), ["camera[1]"])


def test_render_on_a_cpu_env_has_no_fallback():
    import multiagent_particle_envs_amd as mpe
    env = mpe.make_env("simple_spread", batch_size=4, device="cpu")
    assert env.metadata["render.modes"] == ["rgb_array"]
    with pytest.raises(_abi.MpeError, match="no CPU fallback"):
        env.render("rgb_array")
    with pytest.raises(NotImplementedError):
        env.render()                      # mode='human': no display
    with pytest.raises(ValueError, match="unknown mode"):
        env.render("ansi")
