"""THE GAE RULE of include/mpe_hip.h restated in NumPy float32 (gae), an independent float64 textbook form to hold it against
(gae_textbook64), the shapes and inputs of the sweep, the file format of tests/c/gae_host_walk.cpp, and the one ABI call of the GPU
sweep (run_abi).  Shared by tests/test_gae_cpu.py and tests/test_gpu_gae.py; importing it touches no device."""
import ctypes as C
import struct

import numpy as np

# (T, A, B, L, p): the smallest shapes that cover a partly filled wave, the scalar and the 16-byte path with a tail, a segment end
# on the first and on the last step, K = 1 and K > 1, and the full agent count
SHAPES = [(1, 1, 1, 0, 0), (2, 3, 7, 0, 0), (25, 3, 65, 25, 0), (26, 2, 260, 5, 3), (7, 16, 63, 3, 2), (50, 3, 257, 25, 24),
          (300, 1, 5, 0, 0)]
SHAPE_IDS = ["T%d_A%d_B%d_L%d_p%d" % s for s in SHAPES]
KINDS = ("random", "one_agent", "all_done", "nonfinite")
GAMMA, LAM = 0.95, 0.9
CANARY_ROWS, CANARY_F = 16, -777.25


def ends(t, T, L, p):
    """step t ends a segment"""
    return t == T - 1 or (L > 0 and (p + t + 1) % L == 0)


def segments_brute(T, L, p):
    return sum(1 for t in range(T) if ends(t, T, L, p))


def segments(T, L, p):
    return (p + T) // L + ((p + T) % L != 0) if L > 0 else 1


def boot_index(t, T, L, p):
    """the boot row of a segment-ending step"""
    return segments(T, L, p) - 1 if t == T - 1 else (p + t + 1) // L - 1


def gae(rew, done, val, boot, gamma, lam, L=0, p=0):
    """The rule, every float32 operation rounded on its own and in the stated order -> (adv, ret) [T, A, B] float32."""
    f = np.float32
    rew, val, boot = np.asarray(rew, f), np.asarray(val, f), np.asarray(boot, f)
    d = np.asarray(done) != 0
    T = rew.shape[0]
    g = f(gamma)
    c = f(g * f(lam))
    adv, ret = np.empty_like(rew), np.empty_like(rew)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            e = ends(t, T, L, p)
            own = d[t]
            cut = d[t].any(axis=0, keepdims=True) | e
            nv = boot[boot_index(t, T, L, p)] if e else val[t + 1]
            delta = np.where(own, rew[t] - val[t], (rew[t] + g * nv) - val[t])
            adv[t] = delta if e else np.where(cut, delta, delta + c * adv[t + 1])
            ret[t] = adv[t] + val[t]
    return adv, ret


def gae_textbook64(rew, done, val, boot, gamma, lam, L=0, p=0):
    """A_t = sum_l (gamma lambda)^l delta_{t+l} over the rest of t's segment, summed forward in float64 (gamma, lambda: the float32
    values) -> (adv, ret) float64.  Finite inputs only."""
    d = np.asarray(done) != 0
    rew, val, boot = np.asarray(rew, np.float64), np.asarray(val, np.float64), np.asarray(boot, np.float64)
    T = rew.shape[0]
    g = float(np.float32(gamma))
    c = float(np.float32(np.float32(gamma) * np.float32(lam)))      # (the rule's c IS the rounded product)
    delta, cut = np.empty_like(rew), np.empty(rew.shape, bool)
    for t in range(T):
        e = ends(t, T, L, p)
        nv = boot[boot_index(t, T, L, p)] if e else val[t + 1]
        delta[t] = rew[t] + g * np.where(d[t], 0.0, nv) - val[t]
        cut[t] = d[t].any(axis=0, keepdims=True) | e
    adv = np.empty_like(rew)
    for t in range(T):
        acc, w, alive = delta[t].copy(), 1.0, ~cut[t]
        for l in range(1, T - t):
            if not alive.any():
                break
            w *= c
            acc += np.where(alive, w * delta[t + l], 0.0)
            alive &= ~cut[t + l]
        adv[t] = acc
    return adv, adv + val


def make_inputs(shape, kind, seed=0):
    """-> rew, done (uint8), val, boot for one (T, A, B, L, p) and one input kind of the sweep."""
    T, A, B, L, p = shape
    K = segments(T, L, p)
    rs = np.random.RandomState(1000 * SHAPES.index(tuple(shape)) + 10 * KINDS.index(kind) + seed if tuple(shape) in SHAPES else seed)
    rew = rs.standard_normal((T, A, B)).astype(np.float32)
    val = (rs.standard_normal((T, A, B)) * 2).astype(np.float32)
    boot = (rs.standard_normal((K, A, B)) * 2).astype(np.float32)
    done = (rs.uniform(size=(T, A, B)) < 0.1).astype(np.uint8)
    if kind == "one_agent":      # a single agent's dones only: every other agent's rows are cut without own
        done[:, :A - 1] = 0
    elif kind == "all_done":
        done[:] = 1
    elif kind == "nonfinite":    # +inf and NaN in boot ONLY behind own rows (their adv is rew - val exactly)
        enders = [t for t in range(T) if ends(t, T, L, p)]
        for k, t in enumerate(enders):
            done[t][rs.uniform(size=(A, B)) < 0.4] = 1
            done[t].reshape(-1)[k % (A * B)] = 1
            own = done[t] != 0
            bad = np.where((np.arange(A * B).reshape(A, B) + k) % 2 == 0, np.float32(np.inf), np.float32(np.nan))
            boot[k][own] = bad[own]
    return rew, done, val, boot


# ---- tests/c/gae_host_walk.cpp: its input and output files ----------------------------------------------------------------------
def write_walk_input(path, rew, done, val, boot, gamma, lam, L, p, want_adv=True, want_ret=True, scalar=False):
    """int64 T, A, B, L, p | float32 gamma, lambda | int32 want_adv, want_ret, force_scalar, 0 | rew | val | boot | done"""
    T, A, B = rew.shape
    with open(path, "wb") as fh:
        fh.write(struct.pack("<5q2f4i", T, A, B, L, p, gamma, lam, int(want_adv), int(want_ret), int(scalar), 0))
        for x in (rew, val, boot):
            fh.write(np.ascontiguousarray(x, np.float32).tobytes())
        fh.write(np.ascontiguousarray(done, np.uint8).tobytes())


def read_walk_output(path, shape3, want_adv=True, want_ret=True):
    """adv then ret, each [T, A, B] float32 and present only if asked for -> (adv or None, ret or None)"""
    raw = np.fromfile(path, np.float32)
    n = int(np.prod(shape3))
    assert raw.size == n * (int(want_adv) + int(want_ret)), (raw.size, n)
    adv = raw[:n].reshape(shape3) if want_adv else None
    ret = raw[n * int(want_adv):].reshape(shape3) if want_ret else None
    return adv, ret


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float32).view(np.int32).tobytes() == np.ascontiguousarray(b, np.float32).view(np.int32).tobytes()


# ---- the one ABI call of the GPU sweep ------------------------------------------------------------------------------------------
def run_abi(rew, done, val, boot, gamma, lam, L, p, want=("adv", "ret"), misalign=False):
    """mpe_gae on the current device.  Each output asked for has CANARY_ROWS rows of B canary floats behind it and is canary-filled
    in front of the call.  misalign: the outputs start 4 bytes past a 16-byte boundary, so the launch takes the scalar path at any
    B.  -> dict: rc, error, adv, ret (host arrays or None), canary_ok."""
    import torch
    from multiagent_particle_envs_amd import _abi
    T, A, B = rew.shape
    dev = torch.device("cuda", torch.cuda.current_device())
    n, can = T * A * B, CANARY_ROWS * B
    ins = [torch.as_tensor(np.array(x), device=dev) for x in (rew, done, val, boot)]
    lead = 1 if misalign else 0
    outs = {k: torch.full((lead + n + can,), CANARY_F, dtype=torch.float32, device=dev)[lead:] if k in want else None for k in ("adv", "ret")}
    g = _abi.MpeGae()
    g.gamma, g.lambda_, g.episode_len, g.episode_phase = gamma, lam, L, p
    L_ = _abi.lib()
    rc = L_.mpe_gae(C.byref(g), T, A, B, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(),
                    outs["adv"].data_ptr() if outs["adv"] is not None else None,
                    outs["ret"].data_ptr() if outs["ret"] is not None else None, _abi.raw_stream(dev))
    out = {"rc": rc, "error": L_.mpe_last_error().decode() if rc else "", "adv": None, "ret": None, "canary_ok": True}
    torch.cuda.synchronize()
    for k, t in outs.items():
        if t is not None:
            host = t.cpu().numpy()
            out[k] = host[:n].reshape(T, A, B)
            out["canary_ok"] = out["canary_ok"] and bool((host[n:] == CANARY_F).all())
    return out
