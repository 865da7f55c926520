"""THE MINIBATCH RULE and THE ADVANTAGE STATISTICS RULE of include/mpe_hip.h restated in NumPy (perm, adv_stats, batch), the shapes
and synthetic trajectories of the sweep, the file format of tests/c/onpolicy_host_walk.cpp, and the ABI calls of the GPU sweep.
Shared by tests/test_onpolicy_batch_cpu.py and tests/test_gpu_onpolicy_batch.py; importing it touches no device."""
import ctypes as C
import struct

import numpy as np

from oracle.philox import philox4x32_10

M32, M64 = 0xFFFFFFFF, 2 ** 64 - 1
STREAM_MINIBATCH = 0x4D494E49
TILE, CHUNK, LANES = 64, 4096, 256
CANARY_ROWS, CANARY_F, CANARY_I = 16, -777.25, -777
EPS = 1e-8

# (T, A, B, widths, dim_c, M): the smallest case; N = 14 with a short last minibatch of 4 and partial tiles; one minibatch spanning
# many tiles, and 4 full plus a short one of 25; the agent cap, a wide row and utterances; N = 4098: a statistics chunk of 2 elements
WIDE16 = [3, 1, 7, 257, 2, 5, 4, 9, 1, 6, 8, 2, 11, 3, 5, 4]
SHAPES = [(1, 1, 1, [1], 0, 1), (2, 3, 7, [5, 1, 3], 0, 5), (25, 3, 65, [18, 18, 18], 0, 1625), (25, 3, 65, [18, 18, 18], 0, 400),
          (7, 16, 63, WIDE16, 4, 441), (3, 2, 1366, [16, 14], 0, 4098)]
SHAPE_IDS = ["T%d_A%d_B%d_c%d_M%d" % (s[0], s[1], s[2], s[4], s[5]) for s in SHAPES]
# the statistics alone, on the GPU: N = T * B = 1 048 578 is 257 chunks of 4096, which the second launch takes in pieces of 256 -- a
# second piece of one chunk of two elements.  Not in SHAPES: the batch sweep and the host walk do not take it.
STATS_SHAPES = [(2, 2, 524289, [1, 1], 0, 1)]
STATS_IDS = ["T%d_A%d_B%d_stats_only" % s[:3] for s in STATS_SHAPES]
SEED = 0x1234567800000055      # (a non-zero high word)


# ---- THE MINIBATCH RULE ---------------------------------------------------------------------------------------------------------
def fmix32(h):
    h = np.asarray(h, np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def half_width(N):
    return max(1, (int(N - 1).bit_length() + 1) // 2)


def round_keys(seed, epoch):
    seed, epoch = int(seed) & M64, int(epoch) & M64
    o = philox4x32_10(np.array([epoch & M32]), np.array([epoch >> 32]), np.array([0]), np.array([STREAM_MINIBATCH]), seed & M32, seed >> 32)
    return [int(x[0]) & M32 for x in o]


def one_pass(x, w, keys):
    mask = np.uint64((1 << w) - 1)
    L, R = x >> np.uint64(w), x & mask
    for k in keys:
        L, R = R, L ^ (fmix32((R & np.uint64(M32)) ^ np.uint64(k)) & mask)
    return (L << np.uint64(w)) | R


def perm(N, seed, epoch, q=None, keys=None, walks=None):
    """perm(q) for every q of `q` (default: all of [0, N)) -> uint64 array.  walks: a list that receives the longest walk."""
    w = half_width(N)
    keys = round_keys(seed, epoch) if keys is None else keys
    x = np.arange(N, dtype=np.uint64) if q is None else np.asarray(q, np.uint64).copy()
    x = one_pass(x, w, keys)
    n = 1
    while True:
        out = x >= np.uint64(N)
        if not out.any():
            break
        x[out] = one_pass(x[out], w, keys)
        n += 1
    if walks is not None:
        walks.append(n)
    return x


# ---- THE ADVANTAGE STATISTICS RULE ----------------------------------------------------------------------------------------------
def sums(x):
    """S and Q of one agent's elements in the rule's order (x: float32 [N])"""
    x = np.asarray(x, np.float32).astype(np.float64)
    N = x.size
    S = Q = np.float64(0.0)
    for c in range((N + CHUNK - 1) // CHUNK):
        blk = np.zeros(CHUNK, np.float64)      # (a skipped element and an added +0.0 leave a sum that started at +0.0 the same)
        part = x[c * CHUNK:(c + 1) * CHUNK]
        blk[:part.size] = part
        blk = blk.reshape(CHUNK // LANES, LANES)
        s, q = np.zeros(LANES, np.float64), np.zeros(LANES, np.float64)
        for k in range(CHUNK // LANES):
            s = s + blk[k]
            q = q + blk[k] * blk[k]
        stride = LANES // 2
        while stride >= 1:
            s[:stride] = s[:stride] + s[stride:2 * stride]
            q[:stride] = q[:stride] + q[stride:2 * stride]
            stride //= 2
        S = S + s[0]
        Q = Q + q[0]
    return S, Q


def moments(x):
    """-> (mean, var) float64 by the rule"""
    S, Q = sums(x)
    N = np.asarray(x).size
    mean = S / np.float64(N)
    var = np.float64(0.0)
    if N > 1:
        var = (Q - S * mean) / (np.float64(N) - np.float64(1.0))
        var = var if var > 0.0 else np.float64(0.0)
    return mean, var


def adv_stats(adv, eps=EPS):
    """adv [T, A, B] float32 -> stats [A, 2] float32"""
    T, A, B = adv.shape
    out = np.zeros((A, 2), np.float32)
    with np.errstate(all="ignore"):
        for i in range(A):
            mean, var = moments(np.ascontiguousarray(adv[:, i, :]).reshape(-1))
            out[i, 0] = np.float32(mean)
            out[i, 1] = np.float32(1.0) / (np.float32(np.sqrt(var)) + np.float32(eps))
    return out


def normalise(x, stats_i):
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        return (x - np.float32(stats_i[0])) * np.float32(stats_i[1])


# ---- synthetic trajectories -----------------------------------------------------------------------------------------------------
def coded(field, shape):
    """float32 whose BIT PATTERN is field * 2^26 + the element's flat position + 1: every element of every row tensor differs, none
    is a NaN or an infinity (patterns below 2^30), so a misplaced element is identifiable from its bits"""
    n = int(np.prod(shape))
    assert n < (1 << 26) and field < 16
    return (np.arange(1, n + 1, dtype=np.uint32) + np.uint32(field << 26)).view(np.float32).reshape(shape)


def make_traj(shape, seed=0):
    """-> dict of host arrays: obs_in [T, sum D * B], act [T,A,B,5], utter [T,A,B,dim_c] or None, logp, adv, ret, val [T,A,B]"""
    T, A, B, widths, dim_c, M = shape
    rs = np.random.RandomState(100 + seed + T + 7 * A + 13 * B)
    tr = {"obs_in": coded(1, (T, sum(widths) * B)), "act": coded(2, (T, A, B, 5)),
          "utter": coded(3, (T, A, B, dim_c)) if dim_c else None}
    tr["logp"] = -np.abs(rs.standard_normal((T, A, B))).astype(np.float32)
    tr["adv"] = (0.3 + 2.0 * rs.standard_normal((T, A, B))).astype(np.float32)
    tr["val"] = rs.standard_normal((T, A, B)).astype(np.float32)
    tr["ret"] = (tr["adv"] + tr["val"]).astype(np.float32)
    return tr


def make_adv(shape, seed=0):
    """-> adv [T, A, B] float32 alone, drawn as make_traj draws it (what the statistics read)"""
    T, A, B = shape[:3]
    rs = np.random.RandomState(200 + seed + T + 7 * A + 13 * B)
    return (0.3 + 2.0 * rs.standard_normal((T, A, B))).astype(np.float32)


def batch(tr, shape, idx, stats=None):
    """The gather for the pairs idx (t * B + b) -> dict: idx, obs (list of [m, D_i]), act [A,m,5], utter, logp, adv, ret, val, joint"""
    T, A, B, widths, dim_c, M = shape
    idx = np.asarray(idx, np.int64)
    t, b = idx // B, idx % B
    off = np.concatenate([[0], np.cumsum(widths)])
    obs = []
    for i in range(A):
        blk = tr["obs_in"][:, off[i] * B:off[i + 1] * B].reshape(T, B, widths[i])
        obs.append(blk[t, b])
    out = {"idx": idx, "obs": obs, "joint": np.concatenate(obs, axis=1),
           "act": np.stack([tr["act"][t, i, b] for i in range(A)]),
           "utter": np.stack([tr["utter"][t, i, b] for i in range(A)]) if dim_c else None}
    for k in ("logp", "adv", "ret", "val"):
        out[k] = np.stack([tr[k][t, i, b] for i in range(A)]) if tr[k] is not None else None
    if stats is not None:
        out["adv"] = np.stack([normalise(out["adv"][i], stats[i]) for i in range(A)])
    return out


def minibatches(N, M):
    """(first, m) of every minibatch of an epoch"""
    return [(f, min(M, N - f)) for f in range(0, N, M)]


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype == np.float32 else np.uint64 if x.dtype in (np.int64, np.float64) else x.dtype).tobytes()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bits(a) == bits(b)


FIELDS = ("idx", "obs", "act", "utter", "logp", "adv", "ret", "val", "joint")


def first_difference(got, want):
    """the first field of two batch dicts that differs, or None"""
    for k in FIELDS:
        g, w = got.get(k), want.get(k)
        if (g is None) != (w is None):
            return k + " (present on one side only)"
        if g is None:
            continue
        if k == "obs":
            for i, (x, y) in enumerate(zip(g, w)):
                if not same_bits(x, y):
                    return "obs[%d]" % i
        elif not same_bits(g, w):
            return k
    return None


# ---- tests/c/onpolicy_host_walk.cpp: its input and output files -----------------------------------------------------------------
def write_walk_input(path, tr, shape, keys, want_logp=True, want_stats=True, want_joint=True, eps=EPS):
    """int64 T, A, B, dim_c, M, want_logp, want_stats, want_joint | uint32 keys[4] | float32 eps | int32 widths[16] |
    obs_in | act | utter | logp (if wanted) | adv | ret | val"""
    T, A, B, widths, dim_c, M = shape
    with open(path, "wb") as fh:
        fh.write(struct.pack("<8q4If16i", T, A, B, dim_c, M, int(want_logp), int(want_stats), int(want_joint), *keys, eps,
                             *(list(widths) + [0] * (16 - A))))
        for k in ("obs_in", "act", "utter", "logp", "adv", "ret", "val"):
            if tr[k] is not None and (k != "logp" or want_logp):
                fh.write(np.ascontiguousarray(tr[k], np.float32).tobytes())


def read_walk_output(path, shape, want_logp=True, want_joint=True):
    """stats [A][2], then per minibatch of the epoch: idx | obs | act | utter | logp | adv | ret | val | joint -> (stats, [dict])"""
    T, A, B, widths, dim_c, M = shape
    raw = np.fromfile(path, np.uint8)
    pos = [0]

    def take(dtype, *dims):
        n = int(np.prod(dims)) * np.dtype(dtype).itemsize
        out = raw[pos[0]:pos[0] + n].view(dtype).reshape(dims)
        assert out.size == int(np.prod(dims)), "the output file is short"
        pos[0] += n
        return out
    stats = take(np.float32, A, 2)
    outs = []
    for first, m in minibatches(T * B, M):
        o = {"idx": take(np.int64, m), "obs": [take(np.float32, m, d) for d in widths], "act": take(np.float32, A, m, 5),
             "utter": take(np.float32, A, m, dim_c) if dim_c else None, "logp": take(np.float32, A, m) if want_logp else None,
             "adv": take(np.float32, A, m), "ret": take(np.float32, A, m), "val": take(np.float32, A, m),
             "joint": take(np.float32, m, sum(widths)) if want_joint else None}
        outs.append(o)
    assert pos[0] == raw.size, "the output file holds more than the epoch's minibatches"
    return stats, outs


# ---- the ABI calls of the GPU sweep ---------------------------------------------------------------------------------------------
def device_traj(tr):
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    return {k: (torch.as_tensor(np.array(v), device=dev) if v is not None else None) for k, v in tr.items()}


def abi_traj(dt, shape, want_logp=True):
    from multiagent_particle_envs_amd import _abi
    T, A, B, widths, dim_c, M = shape
    s = _abi.MpeOnPolicyTraj()
    s.T, s.A, s.B, s.dim_c = T, A, B, dim_c
    for i, d in enumerate(widths):
        s.obs_width[i] = d
    for k in ("obs_in", "act", "utter", "logp", "adv", "ret", "val"):
        setattr(s, k, dt[k].data_ptr() if dt[k] is not None and (k != "logp" or want_logp) else None)
    return s


def run_stats(dt, shape, eps=EPS, poison=False):
    """mpe_adv_stats on the current device -> (rc, stats [A, 2] host array, canary_ok)"""
    import torch
    from multiagent_particle_envs_amd import _abi
    T, A, B = shape[:3]
    dev = dt["adv"].device
    L_ = _abi.lib()
    n = L_.mpe_adv_stats_work(T, A, B)
    assert n >= 0
    work = torch.full((n + 32,), float("nan") if poison else 0.0, dtype=torch.float64, device=dev)
    work[n:] = CANARY_F
    stats = torch.full((A + CANARY_ROWS, 2), CANARY_F, dtype=torch.float32, device=dev)
    rc = L_.mpe_adv_stats(T, A, B, dt["adv"].data_ptr(), eps, work.data_ptr(), stats.data_ptr(), _abi.raw_stream(dev))
    torch.cuda.synchronize()
    ok = bool((stats[A:] == CANARY_F).all()) and bool((work[n:] == CANARY_F).all())
    return rc, stats[:A].cpu().numpy(), ok


def run_batch(dt, shape, first, m, seed, epoch, stats=None, epoch_add=None, want_logp=True, want_joint=True):
    """mpe_onpolicy_batch on the current device: every output canary-filled in front of the call, CANARY_ROWS rows of canaries
    behind it.  stats: a device tensor or None.  -> dict: rc, error, the outputs as host arrays, canary_ok, logp_untouched."""
    import torch
    from multiagent_particle_envs_amd import _abi
    T, A, B, widths, dim_c, M = shape
    dev = dt["adv"].device
    D = sum(widths)

    def can(rows, cols, dtype=torch.float32):
        return torch.full(((rows + CANARY_ROWS) * cols,), CANARY_I if dtype == torch.int64 else CANARY_F, dtype=dtype, device=dev)
    o = {"idx": can(m, 1, torch.int64), "obs": can(m, D), "act": can(A * m, 5), "utter": can(A * m, dim_c) if dim_c else None,
         "logp": can(A * m, 1), "adv": can(A * m, 1), "ret": can(A * m, 1), "val": can(A * m, 1), "joint": can(m, D) if want_joint else None}
    ptr = lambda x: x.data_ptr() if x is not None else None      # noqa: E731
    L_ = _abi.lib()
    s = abi_traj(dt, shape, want_logp)
    rc = L_.mpe_onpolicy_batch(C.byref(s), m, first, seed, epoch, ptr(epoch_add), ptr(stats), ptr(o["idx"]), ptr(o["obs"]), ptr(o["act"]),
                               ptr(o["utter"]), ptr(o["logp"]) if want_logp else None, ptr(o["adv"]), ptr(o["ret"]), ptr(o["val"]),
                               ptr(o["joint"]), _abi.raw_stream(dev))
    out = {"rc": rc, "error": L_.mpe_last_error().decode() if rc else ""}
    torch.cuda.synchronize()
    h = {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}
    sizes = {"idx": m, "obs": m * D, "act": A * m * 5, "utter": A * m * dim_c, "logp": A * m, "adv": A * m, "ret": A * m, "val": A * m,
             "joint": m * D}
    ok = True
    for k, v in h.items():
        if v is not None and not (k == "logp" and not want_logp):
            ok = ok and bool((v[sizes[k]:] == (CANARY_I if k == "idx" else CANARY_F)).all())
    out["canary_ok"] = ok
    out["logp_untouched"] = bool((h["logp"] == CANARY_F).all())
    off = np.concatenate([[0], np.cumsum(widths)])
    out["idx"] = h["idx"][:m]
    out["obs"] = [h["obs"][off[i] * m:off[i + 1] * m].reshape(m, widths[i]) for i in range(A)]
    out["act"] = h["act"][:A * m * 5].reshape(A, m, 5)
    out["utter"] = h["utter"][:A * m * dim_c].reshape(A, m, dim_c) if dim_c else None
    out["logp"] = h["logp"][:A * m].reshape(A, m) if want_logp else None
    for k in ("adv", "ret", "val"):
        out[k] = h[k][:A * m].reshape(A, m)
    out["joint"] = h["joint"][:m * D].reshape(m, D) if want_joint else None
    return out
