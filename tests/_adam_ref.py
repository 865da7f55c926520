"""THE ADAM RULE of include/mpe_hip.h in NumPy, twice: `step(..., dtype=np.float32)` restates mpe_adam_step operation by operation --
the tiling, the lane sums and the fixed tree of the norm, the state pair, the skip, and the five float32 statements per element, each
operation rounded on its own -- and is what the host walk and the GPU must equal BIT FOR BIT; `dtype=np.float64` is the same order
without the float32 casts, the form held against float64 torch.  Also the sweep's shapes and inputs, and the host walk's file format
(tests/c/adam_host_walk.cpp)."""
import struct

import numpy as np

TILE, LANES, MAX_PARTIALS, MAX_SETS, STATE_DOUBLES = 1024, 256, 256, 8, 16

# the sweep: the same sizes on the host walk and on the GPU
SHAPES = [(16,), (1008,), (1024,), (1040,), (262160,), (6416, 16, 20000), (32784,) * 8]
SHAPE_IDS = ["n16", "n1008", "n1024", "n1040", "span2_one_set", "three_unequal_sets", "span2_by_roundings"]
STEPS = 3


def fresh_state():
    s = np.zeros(STATE_DOUBLES, dtype=np.float64)
    s[1] = s[2] = s[4] = s[5] = 1.0
    return s


def span_of(ns):
    span = 1
    while sum(-(-n // (TILE * span)) for n in ns) > MAX_PARTIALS:
        span += 1
    return span


def tiles_of(ns):
    span = span_of(ns)
    return [-(-n // (TILE * span)) for n in ns]


def fold(x):
    """the fixed tree over the last axis (256 wide): for stride = 128 .. 1: x[l] += x[l + stride], l < stride"""
    x = np.array(x, dtype=np.float64)
    stride = LANES // 2
    while stride >= 1:
        x[..., :stride] = x[..., :stride] + x[..., stride:2 * stride]
        stride //= 2
    return x[..., 0]


def partials(grads):
    """work[0..P): per tile the folded lane sums of (double) g * (double) g"""
    ns = [g.size for g in grads]
    span = span_of(ns)
    out = []
    for g in grads:
        t = -(-g.size // (TILE * span))
        # (a float at or beyond n adds nothing: here it adds +0.0 to a sum that is never -0.0)
        sq = np.zeros(t * TILE * span, dtype=np.float64)
        with np.errstate(all="ignore"):
            sq[:g.size] = g.astype(np.float64) * g.astype(np.float64)
        sq = sq.reshape(t, span, LANES, 4)
        acc = np.zeros((t, LANES), dtype=np.float64)
        with np.errstate(all="ignore"):
            for j in range(span):
                for k in range(4):
                    acc = acc + sq[:, j, :, k]
            out.append(fold(acc))
    return np.concatenate(out)


def scalars(cfg, state, work, dtype):
    """launch 2's scalars from work and the committed triple -> dict, and what lane 0 of workgroup 0 writes to the state"""
    x = np.zeros(LANES, dtype=np.float64)
    x[:work.size] = work
    with np.errstate(all="ignore"):
        S = fold(x)
        norm = np.sqrt(np.float64(S))
    t, p1, p2 = (np.float64(state[k]) for k in range(3))
    if not np.isfinite(norm):
        state[3:6] = state[0:3]
        state[6], state[7] = norm, 0.0
        state[8] += 1.0
        return None
    f = dtype
    lr = np.float64(cfg["lr"]) if cfg.get("lr_value") is None else np.float64(np.float32(cfg["lr_value"]))
    b1, b2, eps, wd, mg = (np.float64(cfg[k]) for k in ("beta1", "beta2", "eps", "weight_decay", "max_grad_norm"))
    c = min(np.float64(1.0), mg / (norm + np.float64(1e-6))) if mg > 0 else np.float64(1.0)
    t1, q1, q2 = t + 1.0, p1 * b1, p2 * b2
    k = dict(cf=f(c), a1=f(1.0 - b1), a2=f(1.0 - b2), b2=f(b2), step=f(lr / (1.0 - q1)), s2=f(np.sqrt(1.0 - q2)), e=f(eps),
             dec=f(1.0 - lr * wd), decay=bool(wd != 0))
    state[3:6] = (t1, q1, q2)
    state[6], state[7] = norm, c
    return k


def step(cfg, sets, state, dtype=np.float32):
    """One mpe_adam_step.  sets: list of dicts with arrays w, g, m, v of `dtype` (g is the norm's input as it stands: float32 for
    the bit-exact form); w, m, v and state are updated in place.  -> work (float64 [P])."""
    state[0:3] = state[3:6]                                    # launch 1: the commit
    work = partials([s["g"] for s in sets])
    k = scalars(cfg, state, work, dtype)
    if k is None:
        return work
    with np.errstate(all="ignore"):
        for s in sets:
            g = s["g"].astype(dtype) * k["cf"]
            w = s["w"] * k["dec"] if k["decay"] else s["w"]
            m = s["m"] + (g - s["m"]) * k["a1"]
            v = s["v"] * k["b2"] + (g * g) * k["a2"]
            w = w - k["step"] * (m / (np.sqrt(v) / k["s2"] + k["e"]))
            assert w.dtype == m.dtype == v.dtype == dtype
            s["w"][...], s["m"][...], s["v"][...] = w, m, v
    return work


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the sweep's inputs -----------------------------------------------------------------------------------------------------------
def make_sets(ns, seed):
    """Per set w, m = v = 0 and STEPS gradients: magnitudes log-uniform over 1e-22 .. 1e3 (g * g is denormal in places), both signs,
    exact zeros, and a block of padding -- the last 8 floats of every set and floats 5..7 -- with w = g = m = v = +0.0."""
    rng = np.random.RandomState(seed)
    sets, grads = [], []
    for n in ns:
        pad = np.zeros(n, dtype=bool)
        pad[-8:] = True
        pad[5:8] = True
        w = rng.standard_normal(n).astype(np.float32)
        w[pad] = 0.0
        gs = []
        for _ in range(STEPS):
            mag = 10.0 ** rng.uniform(-22.0, 3.0, n)
            g = (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
            g[rng.random_sample(n) < 0.05] = 0.0
            g[pad] = 0.0
            gs.append(g)
        sets.append(dict(w=w, m=np.zeros(n, np.float32), v=np.zeros(n, np.float32), pad=pad))
        grads.append(gs)
    return sets, grads


def run_ref(cfg, sets, grads, state=None, lr_values=None, dtype=np.float32):
    """STEPS (len(grads[0])) steps of the restatement on copies -> (sets, per step (state, work))"""
    state = fresh_state() if state is None else state.copy()
    cur = [dict(w=s["w"].astype(dtype), m=s["m"].astype(dtype), v=s["v"].astype(dtype)) for s in sets]
    log = []
    for t in range(len(grads[0])):
        for s, gs in zip(cur, grads):
            s["g"] = gs[t]
        c = dict(cfg)
        if lr_values is not None:
            c["lr_value"] = lr_values[t]
        work = step(c, cur, state, dtype)
        log.append((state.copy(), work))
    return cur, log


CFG = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_grad_norm=0.0)


# ---- the host walk's files --------------------------------------------------------------------------------------------------------
def write_walk_input(path, cfg, sets, grads, state, lr_values=None):
    """int64 n_sets, steps, has_lr_ptr | int64 n[8] | float64 lr, beta1, beta2, eps, weight_decay, max_grad_norm | float64 state[16] |
    per set w, m, v | per step: float32 lr value (if has_lr_ptr), then per set g"""
    ns = [s["w"].size for s in sets]
    steps = len(grads[0])
    with open(path, "wb") as f:
        f.write(struct.pack("<3q", len(sets), steps, int(lr_values is not None)))
        f.write(struct.pack("<8q", *(ns + [0] * (MAX_SETS - len(ns)))))
        f.write(struct.pack("<6d", *(cfg[k] for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "max_grad_norm"))))
        f.write(state.astype("<f8").tobytes())
        for s in sets:
            for k in ("w", "m", "v"):
                f.write(s[k].astype("<f4").tobytes())
        for t in range(steps):
            if lr_values is not None:
                f.write(np.float32(lr_values[t]).tobytes())
            for gs in grads:
                f.write(gs[t].astype("<f4").tobytes())


def read_walk_output(path, ns, steps):
    """per step: state[16], work[P] | per set w, m, v -> (sets, per step (state, work))"""
    P = sum(tiles_of(ns))
    raw = open(path, "rb").read()
    at, log = 0, []
    for _ in range(steps):
        st = np.frombuffer(raw, "<f8", STATE_DOUBLES, at)
        at += 8 * STATE_DOUBLES
        wk = np.frombuffer(raw, "<f8", P, at)
        at += 8 * P
        log.append((st, wk))
    sets = []
    for n in ns:
        d = {}
        for k in ("w", "m", "v"):
            d[k] = np.frombuffer(raw, "<f4", n, at)
            at += 4 * n
        sets.append(d)
    assert at == len(raw), "the walk's output does not hold exactly its tensors"
    return sets, log
