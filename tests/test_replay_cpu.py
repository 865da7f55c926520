"""The replay buffer without a GPU: the draw rule's restatement (tests/_replay_ref.py), the MpeReplay binding against the header
(a C program prints sizeof / offsetof), and every refusal that is decided on the host before anything is launched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.replay import ReplayBuffer
from oracle.philox import philox4x32_10

import _replay_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n_valid", [1, 5, 2 ** 31 + 7])
def test_restated_draw_lies_in_the_valid_part(n_valid):
    idx = R.draw_indices(0x1234567890ABCDEF, 3, 2001, n_valid)
    assert all(0 <= j < n_valid for j in idx)
    if n_valid == 1:
        assert set(idx) == {0}
    if n_valid == 5:
        assert set(idx) == set(range(5))
    if n_valid > 2 ** 31:
        assert max(idx) >= 2 ** 30 > min(idx)      # (2001 draws all in one half of the range: probability 2^-2000)


def test_samples_k_and_k_plus_1_are_the_two_halves_of_one_block():
    seed, draw = (7 << 32) | 9, (5 << 32) | 11
    hi, lo = R.draw_words(seed, draw, 10)
    for k in range(0, 10, 2):
        x, y, z, w = [int(v[0]) for v in philox4x32_10([k >> 1], [0 ^ (draw >> 32)], [0], [R.STREAM_REPLAY ^ (draw & R.M32)],
                                                         seed & R.M32, seed >> 32)]
        assert (int(hi[k]), int(lo[k]), int(hi[k + 1]), int(lo[k + 1])) == (x, y, z, w)
    n = 12345
    assert R.draw_indices(seed, draw, 10, n) == [(((int(h) << 32) | int(l)) * n) >> 64 for h, l in zip(hi, lo)]
    assert R.draw_indices(seed, draw + 1, 10, 2 ** 39) != R.draw_indices(seed, draw, 10, 2 ** 39)
    assert R.draw_indices(seed + 1, draw, 10, 2 ** 39) != R.draw_indices(seed, draw, 10, 2 ** 39)


@pytest.mark.parametrize("seed,draw,n_valid,M", [(0xC0FFEE12345, 1, 21, 21000), (9, 0, 1000, 200000), (0x1234567890ABCDEF, 3, 65, 65000)])
def test_restated_draw_is_flat(seed, draw, n_valid, M):
    """Chi-square of j = (u * n_valid) >> 64 over its n_valid cells, at most four standard deviations (sqrt(2 dof)) above its mean
    (dof).  The rule is deterministic: the three values are 18.4 (dof 20, bound 45.3), 1020.0 (dof 999, bound 1177.8) and 54.7
    (dof 64, bound 109.3)."""
    counts = np.bincount(np.array(R.draw_indices(seed, draw, M, n_valid), dtype=np.int64), minlength=n_valid)
    assert len(counts) == n_valid and counts.sum() == M
    expect = M / n_valid
    chi2 = float(((counts - expect) ** 2).sum() / expect)
    dof = n_valid - 1
    print("chi2 %.1f, dof %d, bound %.1f" % (chi2, dof, dof + 4 * (2 * dof) ** 0.5))
    assert chi2 <= dof + 4 * (2 * dof) ** 0.5


def test_reciprocal_rule_is_division():
    """gather_rows finds element e's row as umulhi(e, ceil(2^32 / W)) and takes e itself for W = 1 (magic 0): for every row width
    up to MPE_REPLAY_MAX_WIDTH and every element of a full tile (e < 64 * W) that is e // W.  This tests the RULE the kernel
    file's static_assert claims, restated in uint64 -- not the compiled code (tests/test_gpu_replay.py runs that)."""
    tile, top = 64, _abi.MPE_REPLAY_MAX_WIDTH
    assert tile * top * top < 2 ** 32      # the static_assert's bound
    e_all = np.arange(tile * top, dtype=np.uint64)
    rows = np.arange(tile, dtype=np.uint64)
    for W in range(1, top + 1):
        magic = 0 if W < 2 else (2 ** 32 + W - 1) // W      # replay_magic
        assert magic < 2 ** 32
        e = e_all[:tile * W]
        r = (e * np.uint64(magic)) >> np.uint64(32) if magic else e
        assert np.array_equal(r, np.repeat(rows, W)), W      # (np.repeat(rows, W)[e] is e // W)
    assert np.array_equal(np.repeat(rows, 7), np.arange(tile * 7, dtype=np.uint64) // np.uint64(7))


def test_header_names_the_stream_and_the_limits():
    hdr = open(os.path.join(ROOT, "include", "mpe_hip.h")).read()
    assert int(re.search(r"#define MPE_STREAM_REPLAY (0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == _abi.MPE_STREAM_REPLAY == R.STREAM_REPLAY
    assert _abi.MPE_STREAM_REPLAY == int.from_bytes(b"REPL", "big")
    assert int(re.search(r"#define MPE_REPLAY_MAX_AGENTS (\d+)", hdr).group(1)) == _abi.MPE_REPLAY_MAX_AGENTS
    assert int(re.search(r"#define MPE_REPLAY_MAX_WIDTH (\d+)", hdr).group(1)) == _abi.MPE_REPLAY_MAX_WIDTH


def test_binding_layout_matches_the_header(tmp_path):
    names = [f[0] for f in _abi.MpeReplay._fields_]
    src = tmp_path / "replay_layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mpe_hip.h\"\nint main(void) {\n"
                   "  printf(\"sizeof %zu\\n\", sizeof(MpeReplay));\n" +
                   "".join("  printf(\"%s %%zu\\n\", offsetof(MpeReplay, %s));\n" % (n, n) for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "replay_layout")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = dict((ln.split()[0], int(ln.split()[1])) for ln in r.stdout.strip().splitlines())
    assert got.pop("sizeof") == C.sizeof(_abi.MpeReplay) == _abi.lib().mpe_sizeof_replay()
    assert got == {n: getattr(_abi.MpeReplay, n).offset for n in names}


def _desc(A=2, B=4, S=3, dim_c=0):
    d = _abi.MpeReplay()
    d.n_agents, d.dim_c, d.B, d.S = A, dim_c, B, S
    for i in range(min(A, _abi.MPE_REPLAY_MAX_AGENTS)):
        d.obs_width[i], d.movable[i] = 6, 1
    return d


def test_supported_follows_the_convention():
    L = _abi.lib()
    assert L.mpe_replay_supported(C.byref(_desc())) == 1
    assert L.mpe_replay_supported(None) < 0 and b"replay is NULL" in L.mpe_last_error()
    d = _desc(A=17)
    assert L.mpe_replay_supported(C.byref(d)) == 0 and b"MPE_REPLAY_MAX_AGENTS" in L.mpe_last_error()
    d = _desc()
    d.obs_width[1] = 4097
    assert L.mpe_replay_supported(C.byref(d)) == 0 and b"MPE_REPLAY_MAX_WIDTH" in L.mpe_last_error()
    for edit, word in ((lambda d: setattr(d, "S", 0), b"S = 0"), (lambda d: setattr(d, "B", 0), b"B = 0"),
                       (lambda d: setattr(d, "S", 2 ** 38), b"2^40"), (lambda d: d.speaks.__setitem__(0, 1), b"speaks but dim_c = 0"),
                       (lambda d: d.movable.__setitem__(1, 0), b"no head"), (lambda d: setattr(d, "n_agents", 0), b"n_agents"),
                       (lambda d: d.obs_width.__setitem__(0, 0), b"obs_width")):
        d = _desc()
        edit(d)
        assert L.mpe_replay_supported(C.byref(d)) < 0 and word in L.mpe_last_error(), L.mpe_last_error()
    d = _desc(S=2 ** 38 - 1)      # 2^40 - 4 transitions: the largest ring of 4 worlds
    assert L.mpe_replay_supported(C.byref(d)) == 1


def test_null_pointers_are_refused_before_any_launch():
    """No device memory exists here: each of these calls returns from the host-side checks (a launch would need a device)."""
    L = _abi.lib()
    d = _desc()
    assert L.mpe_replay_push(C.byref(d), None, None, None, None, None, None, None) == -1 and b"replay->obs is NULL" in L.mpe_last_error()
    assert L.mpe_replay_sample(C.byref(d), 8, 0, *([None] * 10)) == -1 and b"replay->obs is NULL" in L.mpe_last_error()
    for name in ("obs", "next_obs", "act", "rew", "done", "head", "ticket"):      # (fake, aligned, never dereferenced: the check stops first)
        setattr(d, name, 4096)
    assert L.mpe_replay_push(C.byref(d), None, None, None, None, None, None, None) == -1 and b"obs_ptrs is NULL" in L.mpe_last_error()
    assert L.mpe_replay_sample(C.byref(d), 0, 0, *([None] * 10)) == -1 and b"M = 0" in L.mpe_last_error()
    assert L.mpe_replay_sample(C.byref(d), 8, 0, *([None] * 10)) == -1 and b"idx is NULL" in L.mpe_last_error()
    d.head = 4100
    assert L.mpe_replay_sample(C.byref(d), 8, 0, *([None] * 10)) == -1 and b"replay->head is not 8-byte aligned" in L.mpe_last_error()
    d = _desc(dim_c=3)
    d.speaks[0] = 1
    for name in ("obs", "next_obs", "act", "rew", "done", "head", "ticket"):
        setattr(d, name, 4096)
    assert L.mpe_replay_sample(C.byref(d), 8, 0, *([None] * 10)) == -1 and b"replay->utter is NULL" in L.mpe_last_error()


def test_constructor_and_sample_refusals():
    env = mpe.make_env("simple_adversary", batch_size=4, device="cpu")
    buf = ReplayBuffer(env, steps=3, seed=5)
    assert (buf.A, buf.B, buf.S, buf.count, len(buf)) == (3, 4, 3, 0, 0)
    assert buf.obs_widths == [8, 10, 10] and buf.dim_c == 0 and buf.joint_width == 28 + 15
    with pytest.raises(_abi.MpeError, match="empty"):
        buf.sample(8)
    with pytest.raises(_abi.MpeError, match="M = 0"):
        buf.sample(0)
    with pytest.raises(_abi.MpeError, match="steps = 0"):
        ReplayBuffer(env, steps=0)
    with pytest.raises(_abi.MpeError, match="2\\^40"):
        ReplayBuffer(env, steps=2 ** 38)

    class NoLayout(object):
        world = env.world
    with pytest.raises(_abi.MpeError, match="no device-side observation layout"):
        ReplayBuffer(NoLayout(), steps=3)
    sl = mpe.make_env("simple_speaker_listener", batch_size=4, device="cpu")
    b2 = ReplayBuffer(sl, steps=2)
    assert b2.dim_c == 3 and b2.movable == [False, True] and b2.speaks == [True, False] and b2.n_act == [3, 5]
    assert set(("ReplayBuffer", "ReplayBatch")) <= set(mpe.__all__)
