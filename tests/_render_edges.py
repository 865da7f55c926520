"""The edge cases of `mpe_render` (csrc/mpe_render.hip) as plain data, for tests/test_render_edges_cpu.py (the reference alone)
and tests/test_gpu_render_edges.py (the kernel at its C entry point).  A case is a frame size, the viewers' cameras, K frames
of B worlds (through a world list or not), E entity sizes, pos [B, E, 2] and rgba [E, 4] or [K, E, 4]; the reference is
tests/_render_ref.render_frames, computed once per case and shared read-only.

`block_parts` is the index arithmetic of the output alone (size, V, K and the 1024 pixels of a block): which pixels of which
image a block holds.  Nothing else of the kernel is restated here."""
import ctypes as C
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_ref as R  # noqa: E402

F = np.float32
BLOCK_PX = 1024          # pixels of the flat [V][K][S][S] range per workgroup
PAD = 256                # sentinel bytes in front of and behind the frames (a multiple of 16: `out` stays aligned)
SENTINEL = 0xA5
CAP = 1e-4               # differing (knife-edge) pixels per pixel of a case: the bar of test_gpu_render._check


class Case:
    def __init__(self, name, size, cameras, sizes, pos, rgba, worlds=None, K=None, white=(), pairs=()):
        self.name, self.size, self.cameras = name, int(size), [int(c) for c in cameras]
        self.sizes = np.asarray(sizes, F)
        self.pos = np.ascontiguousarray(pos, F)                  # [B, E, 2]
        self.rgba = np.ascontiguousarray(rgba, F)                # [E, 4] or [K, E, 4]
        self.B, self.E = self.pos.shape[:2]
        self.worlds = None if worlds is None else [int(w) for w in worlds]
        self.K = int(K) if K is not None else (self.B if worlds is None else len(self.worlds))
        self.V = len(self.cameras)
        self.white = set(white)      # (v, k) frames that must stay white; every other frame must show something
        self.pairs = tuple(pairs)    # (k, earlier, later): concentric opaque entities of frame k, the later one on top
        assert self.pos.shape == (self.B, self.E, 2) and self.sizes.shape == (self.E,)
        assert self.rgba.shape in ((self.E, 4), (self.K, self.E, 4))
        assert self.worlds is None or (len(self.worlds) == self.K and all(0 <= w < self.B for w in self.worlds))
        assert self.worlds is not None or self.K <= self.B
        assert all(-1 <= c < self.E for c in self.cameras)
        assert np.isfinite(self.rgba).all()                      # np.clip and fminf(fmaxf(.)) disagree on NaN: undefined

    @property
    def world_index(self):
        return np.arange(self.K) if self.worlds is None else np.asarray(self.worlds)

    @property
    def pixels(self):
        return self.V * self.K * self.size * self.size


def _colours(rs, n, alpha=None):
    c = rs.uniform(0.05, 0.9, size=(n, 4)).astype(F)
    c[:, 3] = rs.choice([0.5, 1.0], size=n) if alpha is None else alpha
    return c


def _row_blocks(name, size, sizes, xy, seed):
    rs = np.random.RandomState(seed)
    return Case(name, size, [-1], sizes, np.asarray(xy, F)[None], _colours(rs, len(sizes)))


def _chunk(name, E, pairs, seed):
    """E entities in two worlds, random but for `pairs`: per world a list of (earlier, later) entities made concentric and
    opaque, the later one smaller, with nothing else near them -- so the centre pixel tells which one was drawn last."""
    rs = np.random.RandomState(seed)
    spots = np.array([[-0.47, 0.53], [0.51, -0.45]], F)
    sizes = rs.uniform(0.02, 0.08, size=E).astype(F)
    rgba = _colours(rs, E)
    pos = np.zeros((2, E, 2), F)
    for b in range(2):
        for e in range(E):
            while True:
                p = rs.uniform(-1.0, 1.0, size=2)
                if (np.hypot(*(spots - p).T) > 0.36).all():
                    break
            pos[b, e] = p
    marks = []
    for b, world_pairs in enumerate(pairs):
        for spot, (first, later) in zip(spots, world_pairs):
            pos[b, first] = pos[b, later] = spot
            marks.append((b, first, later))
    for j, e in enumerate(sorted({e for _, f, l in marks for e in (f, l)})):
        later = any(e == l for _, _, l in marks)
        sizes[e] = 0.1 if later else 0.2
        rgba[e] = [0.9, 0.1, 0.2 + 0.1 * j, 1.0] if later else [0.1, 0.2 + 0.1 * j, 0.9, 1.0]
    return Case(name, 64, [-1], sizes, pos, rgba, pairs=marks)


def _subpixel(name, size, seed):
    """sizes 1e-4, 0.5/S, 1/S, 2/S: once on a pixel centre, once on a pixel corner; world 1 the same entities moved off the
    grid.  The 30-gon of size 2/S centred on a pixel centre has its vertices at 0 and 180 degrees exactly on the neighbouring
    pixels' centres (sigma = 0 there: a knife edge by construction), so in world 0 that one entity sits off the centre too;
    the three smaller sizes keep dx = dy = 0."""
    rs = np.random.RandomState(seed)
    s = 2.0 / size
    sizes = np.array([1e-4, 0.5 / size, 1.0 / size, 2.0 / size] * 2, F)
    cols = [1, 3, 5, 7] if size == 8 else [9, 22, 37, 52]
    rows = (1, 5) if size == 8 else (13, 41)
    centre = [[-1 + (c + 0.5) * s, 1 - (rows[0] + 0.5) * s] for c in cols]
    corner = [[-1 + c * s, 1 - rows[1] * s] for c in cols]
    pos = np.array([centre + corner, centre + corner], F)
    pos[1] += np.array([0.0137, -0.0071], F) * (8.0 / size)
    pos[0, 3] += np.array([0.0091, 0.0053], F) * (8.0 / size)
    return Case(name, size, [-1], sizes, pos, _colours(rs, 8))


def _far(name, size, seed):
    rs = np.random.RandomState(seed)
    cams = np.array([[1000.3, -999.7], [-37.25, 512.5]], F)
    E = 6
    pos = np.zeros((2, E, 2), F)
    for b in range(2):
        pos[b, :2] = cams + (0.0 if b == 0 else rs.uniform(-3.0, 3.0, size=(2, 2)))
        for e in range(2, E):
            pos[b, e] = pos[b, e % 2] + rs.uniform(-1.0, 1.0, size=2)
    sizes = np.array([0.06, 0.11, 0.15, 0.04, 0.09, 0.2], F)
    return Case(name, size, [0, 1], sizes, pos, _colours(rs, E))


def _build():
    cases = []
    nan, inf = float("nan"), float("inf")
    # ---- blocks inside one pixel row (size >= 1024): the column range of a block decides the cull
    cases.append(_row_blocks("row_blocks_1024", 1024, [0.15, 0.05, 0.08, 0.03, 0.1],
                             [[0.013, 0.137], [-0.93, 0.91], [0.97, -0.4], [-0.31, -0.77], [0.52, 0.96]], 1))
    # entity 0 centred on x = 0 straddles columns 1023 | 1024; 1 wholly left, 2 wholly right, 3 ends at the seam from the left
    cases.append(_row_blocks("row_blocks_2048", 2048, [0.1, 0.1, 0.08, 0.1, 0.04],
                             [[0.0, 0.137], [-0.5, 0.317], [0.6, -0.213], [-0.1007, -0.533], [0.0413, 0.137]], 2))
    cases.append(_row_blocks("row_blocks_1536", 1536, [0.12, 0.06, 0.09, 0.05],
                             [[-0.3331, 0.2113], [0.3329, -0.4713], [0.0007, 0.7411], [-0.6671, -0.8137]], 3))
    # quarter-row blocks: seams at x = -0.5, 0 and 0.5
    cases.append(_row_blocks("row_blocks_4096", 4096, [0.05, 0.04, 0.05, 0.03, 0.02, 0.05],
                             [[-0.5, 0.7113], [0.0, -0.3371], [0.5003, 0.1139], [-0.7519, -0.9871], [0.2507, 0.9907],
                              [0.9913, 0.0131]], 4))
    # ---- blocks that span many frames and viewers
    rs = np.random.RandomState(5)
    cases.append(Case("tiny_frames_viewers", 8, [-1, 0, 2, 1], [0.3, 0.2, 0.4, 0.15],
                      rs.uniform(-0.8, 0.8, size=(5, 4, 2)), _colours(rs, 4), worlds=[4, 0, 4]))
    rs = np.random.RandomState(6)
    cases.append(Case("odd_tail_viewers", 11, [-1, 1, 0], [0.25, 0.18, 0.35, 0.1],
                      rs.uniform(-0.8, 0.8, size=(5, 4, 2)), _colours(rs, 4)))
    # ---- colours by frame k, positions by world worlds[k]
    rs = np.random.RandomState(7)
    rgba = np.stack([_colours(rs, 5) for _ in range(4)])
    cases.append(Case("per_frame_colours_world_list", 32, [-1, 0], [0.2, 0.1, 0.15, 0.25, 0.08],
                      rs.uniform(-0.8, 0.8, size=(9, 5, 2)), rgba, worlds=[7, 2, 2, 0]))
    # ---- entity sizes off the built-in range
    cases.append(_subpixel("subpixel_8", 8, 8))
    cases.append(_subpixel("subpixel_64", 64, 9))
    rs = np.random.RandomState(10)
    rgba = np.stack([_colours(rs, 2, alpha=[1.0, 0.5]), _colours(rs, 2, alpha=[0.5, 1.0])])
    cases.append(Case("huge", 96, [-1, 1], [3.0, 1.5], [[[0.0, 0.0], [0.9, -0.9]], [[0.9, -0.9], [0.0, 0.0]]], rgba))
    # ---- chunks of 64 entities in the cull
    cases.append(_chunk("chunk_64", 64, [[(0, 63)], [(62, 63)]], 11))
    cases.append(_chunk("chunk_65", 65, [[(63, 64)], [(0, 64)]], 12))
    cases.append(_chunk("chunk_512", 512, [[(0, 511), (63, 64)], [(0, 511), (447, 448)]], 17))
    # ---- cameras far from the origin
    cases.append(_far("far_camera_64", 64, 14))
    cases.append(_far("far_camera_1024", 1024, 15))
    # ---- non-finite positions: entity 1 at NaN, entity 2 at +-inf, viewer 1 centred on the NaN entity
    rs = np.random.RandomState(16)
    pos = rs.uniform(-0.7, 0.7, size=(2, 5, 2))
    pos[0, 1], pos[0, 2] = (nan, nan), (inf, inf)
    pos[1, 1], pos[1, 2] = (nan, 0.2), (-inf, 0.1)
    cases.append(Case("non_finite", 32, [-1, 1, 0], [0.2, 0.3, 0.25, 0.15, 0.1], pos, _colours(rs, 5),
                      white=[(1, 0), (1, 1)]))
    # ---- alpha and colour values off [0, 1]
    rgba = np.array([[0.2, 0.5, 0.8, 1.0], [0.9, 0.3, 0.1, 0.0], [0.1, 0.7, 0.3, 0.25], [1.5, -0.3, 0.6, 1.5],
                     [0.4, 0.4, 1.5, -0.5], [-0.3, 0.9, 0.2, 0.5], [0.6, 1.5, -0.3, 0.25]], F)
    cases.append(Case("alpha_and_clamp", 48, [-1], [0.5, 0.3, 0.35, 0.3, 0.3, 0.25, 0.4],
                      [[[0.013, 0.021], [-0.21, 0.17], [0.23, 0.11], [-0.07, -0.19], [0.19, -0.23], [-0.33, -0.05],
                        [0.05, 0.31]]], rgba))
    return {c.name: c for c in cases}


CASES = _build()
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(uint8 [V, K, S, S, 3], knife bool [V, K, S, S]) of a case by the NumPy rule: computed once, read-only."""
    c = CASES[name]
    ref, knife = R.render_frames(c.pos[c.world_index], c.sizes, c.rgba, c.size, c.cameras)
    ref.setflags(write=False)
    knife.setflags(write=False)
    return ref, knife


def block_parts(size, V, K):
    """For every block of 1024 consecutive pixels of the flat [V][K][size][size] range, the images it holds pixels of:
    a list per block of (image = v K + k, first pixel, last pixel) with the pixels counted inside the image."""
    SS = size * size
    total = V * K * SS
    out = []
    for base in range(0, total, BLOCK_PX):
        last = min(base + BLOCK_PX, total) - 1
        out.append([(img, max(base - img * SS, 0), min(last - img * SS, SS - 1)) for img in range(base // SS, last // SS + 1)])
    return out


def centre_pixel(case, k, e):
    """(row, column) of the pixel that holds entity e's centre in frame k of the origin viewer."""
    x, y = case.pos[case.world_index[k], e]
    return int(np.floor((1.0 - float(y)) * case.size / 2.0)), int(np.floor((float(x) + 1.0) * case.size / 2.0))


def fill_args(case, pos_ptr, rgba_ptr, out_ptr, worlds_ptr=None):
    """(MpeScenarioDesc, MpeRenderArgs, the host camera array the arguments point into) of a case, for device buffers laid
    out as `device_arrays` returns them."""
    from multiagent_particle_envs_amd import _abi
    desc = _abi.MpeScenarioDesc()
    desc.kind, desc.n_agents = _abi.MPE_SCN_GENERIC, 1 + max(case.cameras + [0])
    desc.n_landmarks = case.E - desc.n_agents
    for e in range(case.E):
        desc.size[e] = float(case.sizes[e])
    cam = (C.c_int32 * case.V)(*case.cameras)
    a = _abi.MpeRenderArgs()
    a.pos, a.B, a.worlds, a.K, a.n_entities = pos_ptr, case.B, worlds_ptr, case.K, case.E
    a.rgba, a.rgba_world_stride = rgba_ptr, 4 if case.rgba.ndim == 3 else 0
    a.n_viewers, a.camera, a.size, a.out = case.V, cam, case.size, out_ptr
    return desc, a, cam


def device_arrays(case):
    """The case's arrays in the layouts include/mpe_hip.h gives them: pos [E][2][B], rgba [E][K][4] or [E][4], worlds [K]."""
    pos = np.ascontiguousarray(case.pos.transpose(1, 2, 0))
    rgba = np.ascontiguousarray(case.rgba.transpose(1, 0, 2)) if case.rgba.ndim == 3 else case.rgba
    worlds = None if case.worlds is None else np.asarray(case.worlds, np.int32)
    return pos, rgba, worlds
