"""THE PPO LOSS RULE of include/mpe_hip.h restated in NumPy: (a) `rule64`, the rule in float64 with analytic gradients, and (b)
`fold_stats`, the chunk / fold / ascending-partial sums on given float32 rows.  Beside them the same loss in torch autograd
(`torch_loss`: the formula of examples/ppo_spread.py plus the clipped-value and entropy terms), the fixed cases and inputs of the GPU
sweep, the band condition, the parity bound, and the file format of tests/c/ppo_loss_host_walk.cpp.  Shared by
tests/test_ppo_loss_cpu.py and tests/test_gpu_ppo_loss.py; importing it touches no device."""
import numpy as np

MOVE = 5
SUMS = 6           # surr, vl, ent, kl, clipped rows, ratio
BLOCK = 256        # rows per chunk
F32, F64 = np.float32, np.float64


# ---- cases --------------------------------------------------------------------------------------------------------------------------
class Case(object):
    """heads: per agent (movable, speaks); cfg: clip, value_clip (None: off), vf_coef, ent_coef; values: False for a policy-only loss"""

    def __init__(self, name, heads, dim_c, M, seed, clip=0.2, value_clip=0.2, vf_coef=0.5, ent_coef=0.01, values=True, unaligned=False):
        self.name, self.heads, self.dim_c, self.M, self.seed = name, list(heads), dim_c, M, seed
        self.clip, self.value_clip, self.vf_coef, self.ent_coef, self.values, self.unaligned = clip, value_clip, vf_coef, ent_coef, values, unaligned
        self.A = len(self.heads)
        self.n_out = [MOVE * int(mv) + dim_c * int(sp) for mv, sp in self.heads]

    def but(self, name, **kw):
        d = dict(heads=self.heads, dim_c=self.dim_c, M=self.M, seed=self.seed, clip=self.clip, value_clip=self.value_clip,
                 vf_coef=self.vf_coef, ent_coef=self.ent_coef, values=self.values, unaligned=self.unaligned)
        d.update(kw)
        return Case(name, **d)


MOVER, SPEAKER, BOTH = (True, False), (False, True), (True, True)
_SPREAD = Case("spread_A3_M257", [MOVER] * 3, 0, 257, 11)              # two blocks, the second holding one row
_PAIR = Case("speaker_listener_M257", [SPEAKER, MOVER], 3, 257, 14)      # n_out 3, immovable; n_out 5, silent
GPU_CASES = [
    Case("one_row", [MOVER], 0, 1, 10),
    _SPREAD,
    Case("M320", [MOVER] * 2, 0, 320, 12),                               # a whole number of waves, a partial block
    _PAIR,
    Case("both_heads_M130", [BOTH], 10, 130, 15),                        # 5 + 10 logits
    Case("unaligned_M257", [MOVER], 0, 257, 16, unaligned=True),         # the logits start 4 bytes into an allocation
    _SPREAD.but("spread_value_clip_off", value_clip=None),
    _SPREAD.but("spread_ent_coef_0", ent_coef=0.0),
    _SPREAD.but("spread_no_values", values=False),
    _PAIR.but("pair_value_clip_off_ent_0", value_clip=None, ent_coef=0.0),
]
GPU_IDS = [c.name for c in GPU_CASES]
# The second launch's loops past their first trip, on the GPU (the float64 torch comparison and the host walk do not take them).  It
# stages the chunks' partials in pieces of 6144 / (6 A) chunks and loads a piece of one agent, 6 x chunks doubles, 8 x 256 at a trip:
# 16 movers, 65 chunks in pieces of 64 -- a second piece of one chunk of one row; the pair at 342 chunks, ONE piece of 2052 doubles
# per agent -- a second trip of the load; one mover, 1025 chunks in pieces of 1024 -- three trips and a second piece of one chunk of
# one row.  With these seeds the band holds 9, 7 and 6 agent-rows (test_band_rows_are_at_most_a_thousandth).
PIECE_CASES = [
    Case("A16_M16385", [MOVER] * 16, 0, 64 * BLOCK + 1, 41),
    Case("pair_A2_M87297", [SPEAKER, MOVER], 3, 341 * BLOCK + 1, 44),
    Case("A1_M262145", [MOVER], 0, 1024 * BLOCK + 1, 42),
]
PIECE_IDS = [c.name for c in PIECE_CASES]

# the host walk's sweep: every M x the three head layouts x A in (1, 3)
WALK_M = [1, 63, 64, 65, 255, 256, 257, 513]
WALK_LAYOUTS = {"move": (0, [MOVER] * 3), "utter": (3, [SPEAKER] * 3), "both": (10, [BOTH, MOVER, SPEAKER])}


# The walk's seeds are 1000 + 7 M + A, but for one shape: with that seed the draw of (both, A = 1, M = 64) has a loss that nearly
# cancels (|loss| = 0.03 beside terms of 0.3), and the host walk's loss, 1.5e-8 off, stands against a floor of 2 ulps of 0.03 =
# 7.5e-9 that float32 torch holds on that draw and the walk does not.  The shape keeps its place in the sweep with another draw.
WALK_SEEDS = {("both", 1, 64): 2449}


def walk_case(layout, A, M):
    dim_c, heads = WALK_LAYOUTS[layout]
    return Case("%s_A%d_M%d" % (layout, A, M), heads[:A], dim_c, M, WALK_SEEDS.get((layout, A, M), 1000 + 7 * M + A))


# ---- the float64 pieces -------------------------------------------------------------------------------------------------------------
def _head64(z, onehot):
    """z [M, n] float64, onehot [M, n] -> lp [M], H [M], p [M, n], l [M, n], c [M]"""
    c = np.argmax(onehot, axis=1)
    zm = z.max(axis=1, keepdims=True)
    e = np.exp(z - zm)
    s = e.sum(axis=1, keepdims=True)
    p = e / s
    l = (z - zm) - np.log(s)
    return l[np.arange(len(c)), c], -(p * l).sum(axis=1), p, l, c


def _logp64(case, i, logits, act, utter):
    mv, sp = case.heads[i]
    z = logits.astype(F64)
    out, lp, H = [], 0.0, 0.0
    if mv:
        h = _head64(z[:, :MOVE], act[i].astype(F64))
        out.append(h)
        lp, H = lp + h[0], H + h[1]
    if sp:
        h = _head64(z[:, -case.dim_c:], utter[i].astype(F64))
        out.append(h)
        lp, H = lp + h[0], H + h[1]
    return lp, H, out


def make_inputs(case):
    """The fixed inputs of one case, float32: logits N(0, 1.5); the rows played drawn uniformly; logp_old = the reference's own logp
    + N(0, 0.3), so a good share of rows clips on each side under both advantage signs; a few rows with adv == 0 and a few with the
    ratio far outside the clip (logp_old moved by 3)."""
    rs = np.random.RandomState(case.seed)
    A, M = case.A, case.M
    x = dict(logits=[(1.5 * rs.standard_normal((M, n))).astype(F32) for n in case.n_out])
    x["act"] = np.zeros((A, M, MOVE), F32)
    x["utter"] = np.zeros((A, M, case.dim_c), F32) if case.dim_c else None
    for i, (mv, sp) in enumerate(case.heads):
        if mv:
            x["act"][i, np.arange(M), rs.randint(0, MOVE, M)] = 1.0
        if sp:
            x["utter"][i, np.arange(M), rs.randint(0, case.dim_c, M)] = 1.0
    x["adv"] = rs.standard_normal((A, M)).astype(F32)
    x["ret"] = rs.standard_normal((A, M)).astype(F32)
    x["val_old"] = (x["ret"] + 0.5 * rs.standard_normal((A, M))).astype(F32)
    values = [(x["val_old"][i] + 0.25 * rs.standard_normal(M)).astype(F32) for i in range(A)]
    x["values"] = values if case.values else None      # (drawn either way: a policy-only case has its twin's other inputs)
    lp = np.stack([_logp64(case, i, x["logits"][i], x["act"], x["utter"])[0] for i in range(A)])
    noise = 0.3 * rs.standard_normal((A, M))
    far = rs.rand(A, M) < 0.02
    noise[far] += np.where(rs.rand(A, M) < 0.5, 3.0, -3.0)[far]
    x["logp_old"] = (lp + noise).astype(F32)
    x["adv"][rs.rand(A, M) < 0.02] = 0.0
    return x


# ---- (a): the rule in float64 with analytic gradients ------------------------------------------------------------------------------
def rule64(case, x):
    """-> dict: rows [A, M, 4] (logp, surr, vl, ent), kl, ratio, clipped [A, M], dlogits (list of [M, n_out_i]), dvalues [A, M] or
    None, stats [A, 8], loss, and band [A, M]: the rows within the band of a select's threshold.  The scalars are the float32
    values the kernel is given; every operation is float64."""
    A, M = case.A, case.M
    clip, vf, ec = F64(F32(case.clip)), F64(F32(case.vf_coef)), F64(F32(case.ent_coef))
    lo, hi = 1.0 - clip, 1.0 + clip
    rows, kl, ratios, clipped, band = np.zeros((A, M, 4)), np.zeros((A, M)), np.zeros((A, M)), np.zeros((A, M), bool), np.zeros((A, M), bool)
    dlogits, dvalues = [], (np.zeros((A, M)) if case.values else None)
    ent_operand = np.zeros((A, M))      # per row the largest ent_coef / M * p_j * max(|l_j|, |H|): what l_j + H is formed from
    for i in range(A):
        logp, ent, heads = _logp64(case, i, x["logits"][i], x["act"], x["utter"])
        adv = x["adv"][i].astype(F64)
        lr = logp - x["logp_old"][i].astype(F64)
        ratio = np.exp(lr)
        s1, s2 = ratio * adv, np.minimum(np.maximum(ratio, lo), hi) * adv
        surr = np.minimum(s1, s2)
        g = np.where(((lo <= ratio) & (ratio <= hi)) | (s1 < s2), adv, 0.0)
        band[i] = (np.abs(ratio - lo) <= 1e-5 * lo) | (np.abs(ratio - hi) <= 1e-5 * hi)
        vl = np.zeros(M)
        if case.values:
            v, ret, vo = x["values"][i].astype(F64), x["ret"][i].astype(F64), x["val_old"][i].astype(F64)
            a = (v - ret) ** 2
            vl, on = a, np.ones(M, bool)
            if case.value_clip is not None:
                vc_ = F64(F32(case.value_clip))
                b = ((vo + np.minimum(np.maximum(v - vo, -vc_), vc_)) - ret) ** 2
                inside = np.abs(v - vo) <= vc_
                vl, on = np.where(inside, a, np.maximum(a, b)), inside | (a >= b)
                band[i] |= np.abs(np.abs(v - vo) - vc_) <= 1e-6
                band[i] |= ~inside & (np.abs(a - b) <= 1e-6 * np.maximum(a, b))
            dvalues[i] = vf * np.where(on, 2.0 * (v - ret), 0.0) / M
        dz = []
        for lp_h, H_h, p, l, c in heads:
            ent_operand[i] = np.maximum(ent_operand[i], ((ec / M) * p * np.maximum(np.abs(l), np.abs(H_h)[:, None])).max(axis=1))
            onehot = np.zeros_like(p)
            onehot[np.arange(M), c] = 1.0
            dz.append(-((g * ratio / M)[:, None] * (onehot - p)) - (ec / M) * (-(p * (l + H_h[:, None]))))
        dlogits.append(np.concatenate(dz, axis=1))
        rows[i] = np.stack([logp, surr, vl, ent], axis=1)
        kl[i], ratios[i], clipped[i] = (ratio - 1.0) - lr, ratio, (g == 0.0) & (adv != 0.0)
    stats = np.zeros((A, 8))
    stats[:, 0], stats[:, 1], stats[:, 2] = rows[:, :, 1].mean(axis=1), rows[:, :, 2].mean(axis=1), rows[:, :, 3].mean(axis=1)
    stats[:, 3], stats[:, 4], stats[:, 5] = kl.mean(axis=1), clipped.mean(axis=1), ratios.mean(axis=1)
    stats[:, 6] = -stats[:, 0] + vf * stats[:, 1] - ec * stats[:, 2]
    return dict(rows=rows, kl=kl, ratio=ratios, clipped=clipped, dlogits=dlogits, dvalues=dvalues, stats=stats, loss=stats[:, 6].sum(), band=band,
                ent_operand=ent_operand)


# ---- (b): the sums on given float32 rows --------------------------------------------------------------------------------------------
def fold_sum(col):
    """col [M] float32 -> S: chunks of 256 lane values (a lane at or beyond M holds +0.0), each folded s_j += s_(j + stride) for
    stride = 128 .. 1 in float64; the chunk partials added in ascending order"""
    M = len(col)
    S = F64(0.0)
    for c0 in range(0, M, BLOCK):
        s = np.zeros(BLOCK, F64)
        s[:min(BLOCK, M - c0)] = col[c0:c0 + BLOCK].astype(F64)
        stride = BLOCK // 2
        while stride >= 1:
            s[:stride] = s[:stride] + s[stride:2 * stride]
            stride //= 2
        S = S + s[0]
    return S


def fold_stats(case, rows32):
    """rows32 [A, M, 4] float32 (the kernel's own `rows`) -> (stats [A, 8] float32 with columns 0, 1, 2 and 6 filled, loss float32)"""
    A, M = case.A, case.M
    vf, ec = F64(F32(case.vf_coef)), F64(F32(case.ent_coef))
    stats, total = np.zeros((A, 8), F32), F64(0.0)
    for i in range(A):
        mean = [fold_sum(rows32[i, :, k]) / F64(M) for k in (1, 2, 3)]
        Li = ((-mean[0]) + vf * mean[1]) - ec * mean[2]
        stats[i, 0], stats[i, 1], stats[i, 2], stats[i, 6] = F32(mean[0]), F32(mean[1]), F32(mean[2]), F32(Li)
        total = total + Li
    return stats, F32(total)


# ---- the same loss in torch autograd ------------------------------------------------------------------------------------------------
def torch_loss_terms(case, logits_n, values_n, act, utter, logp_old, adv, ret, val_old):
    """On torch tensors of any dtype / device: the formula of examples/ppo_spread.py's losses() plus the clipped-value and entropy
    terms -> (loss, rows [A, M, 4], kl, ratio [A, M])"""
    import torch
    import torch.nn.functional as F
    r32 = lambda c: float(F32(c))      # noqa: E731  (the scalars are the float32 values the kernel is given)
    clip, vf_coef, ent_coef = r32(case.clip), r32(case.vf_coef), r32(case.ent_coef)
    value_clip = None if case.value_clip is None else r32(case.value_clip)
    total, rows, kls, ratios = 0.0, [], [], []
    for i, (mv, sp) in enumerate(case.heads):
        logp, ent = 0.0, 0.0
        for on, z, played in ((mv, logits_n[i][:, :MOVE], act[i]), (sp, logits_n[i][:, logits_n[i].shape[1] - case.dim_c:], utter[i] if sp else None)):
            if on:
                ls = F.log_softmax(z, dim=-1)
                logp = logp + (ls * played).sum(dim=-1)
                ent = ent - (ls.exp() * ls).sum(dim=-1)
        lr = logp - logp_old[i]
        ratio = torch.exp(lr)
        surr = torch.min(ratio * adv[i], ratio.clamp(1 - clip, 1 + clip) * adv[i])
        L = -surr.mean() - ent_coef * ent.mean()
        vl = torch.zeros_like(surr)
        if values_n is not None:
            v = values_n[i].reshape(-1)
            vl = (v - ret[i]) ** 2
            if value_clip is not None:
                vc = val_old[i] + (v - val_old[i]).clamp(-value_clip, value_clip)
                vl = torch.max(vl, (vc - ret[i]) ** 2)
            L = L + vf_coef * vl.mean()
        total = total + L
        rows.append(torch.stack([logp, surr, vl, ent], dim=1))
        kls.append((ratio - 1) - lr)
        ratios.append(ratio)
    return total, torch.stack(rows), torch.stack(kls), torch.stack(ratios)


def torch_loss(case, x, dtype, device="cpu"):
    """torch autograd on the inputs `x` in `dtype` -> the dict rule64 returns (float64 NumPy arrays; no band)"""
    import torch
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype, device=device)      # noqa: E731
    logits_n = [t(z).requires_grad_() for z in x["logits"]]
    values_n = [t(v).requires_grad_() for v in x["values"]] if case.values else None
    utter = t(x["utter"]) if case.dim_c else None
    loss, rows, kl, ratio = torch_loss_terms(case, logits_n, values_n, t(x["act"]), utter, t(x["logp_old"]), t(x["adv"]), t(x["ret"]), t(x["val_old"]))
    loss.backward()
    n = lambda a: a.detach().double().cpu().numpy()      # noqa: E731
    rows = n(rows)
    stats = np.zeros((case.A, 8))
    stats[:, 0], stats[:, 1], stats[:, 2] = rows[:, :, 1].mean(axis=1), rows[:, :, 2].mean(axis=1), rows[:, :, 3].mean(axis=1)
    stats[:, 3], stats[:, 5] = n(kl).mean(axis=1), n(ratio).mean(axis=1)
    r32 = lambda c: float(F32(c))      # noqa: E731
    stats[:, 6] = -stats[:, 0] + r32(case.vf_coef) * stats[:, 1] - r32(case.ent_coef) * stats[:, 2]
    return dict(rows=rows, kl=n(kl), ratio=n(ratio), dlogits=[n(z.grad) for z in logits_n],
                dvalues=np.stack([n(v.grad) for v in values_n]) if case.values else None, stats=stats, loss=float(n(loss)))


# ---- parity: the kernel against (a), the bound taken from float32 torch autograd on the same inputs ---------------------------------
LOGP_TOL = 1e-5      # the project's bound on a log probability (tests/test_gpu_actor.py)


def _dev(got, want, keep=None):
    d = np.abs(np.asarray(got, F64) - np.asarray(want, F64))
    if keep is not None:
        d = d[keep]
    return float(d.max()) if d.size else 0.0


def deviations(case, out, ref):
    """max |out - ref| over the rows outside the band, per output -> dict name -> (deviation, largest magnitude of the reference)"""
    keep = ~ref["band"]
    mag = lambda a, k=None: float(np.abs(a[k] if k is not None else a).max()) if np.size(a) else 0.0      # noqa: E731
    d = {}
    for k, name in ((0, "logp"), (1, "surr"), (2, "vl"), (3, "ent")) if out["rows"] is not None else ():
        d[name] = (_dev(out["rows"][:, :, k], ref["rows"][:, :, k], keep), mag(ref["rows"][:, :, k], keep))
    d["dlogits"] = (max(_dev(out["dlogits"][i], ref["dlogits"][i], keep[i]) for i in range(case.A)),
                    max(mag(ref["dlogits"][i], keep[i]) for i in range(case.A)))
    if case.M == 1 and ref["clipped"].any():
        # A single row that clips: dlogits is the entropy gradient ent_coef / M * p_j * (l_j + H) ALONE, a difference of two float32
        # values of magnitude max(|l_j|, |H|), each half an ulp of THAT magnitude off.  No float32 evaluation, torch's included, holds
        # 2 ulps of the difference except by luck, so here, and only here, the floor's magnitude is that of the operands.  From two
        # rows on the clipped rows' entropy gradient is held to the output's own magnitude beside the unclipped rows.
        d["dlogits"] = (d["dlogits"][0], max(d["dlogits"][1], float(ref["ent_operand"][ref["clipped"]].max())))
    if case.values:
        d["dvalues"] = (_dev(out["dvalues"], ref["dvalues"], keep), mag(ref["dvalues"], keep))
    # the means and the loss run over every row: compared when the band is empty (the cases' seeds are picked for that)
    if not ref["band"].any():
        for k, name in ((0, "mean_surr"), (1, "mean_vl"), (2, "mean_ent"), (3, "mean_kl"), (5, "mean_ratio")):
            d[name] = (_dev(out["stats"][:, k], ref["stats"][:, k]), mag(ref["stats"][:, k]))
        d["L_i"] = (_dev(out["stats"][:, 6], ref["stats"][:, 6]), mag(ref["stats"][:, 6]))
        d["loss"] = (abs(float(out["loss"]) - float(ref["loss"])), abs(float(ref["loss"])))
    return d


def bounds(dev_torch):
    """The kernel's deviation may be at most 4 x that of float32 torch autograd, with a floor of 2 float32 ulps of the output's
    largest magnitude; logp: the project's 1e-5."""
    b = {}
    for name, (dev, mag) in dev_torch.items():
        b[name] = LOGP_TOL if name == "logp" else max(4.0 * dev, 2.0 * float(np.spacing(F32(mag))))
    return b


# ---- tests/c/ppo_loss_host_walk.cpp: its input and output files ---------------------------------------------------------------------
def write_walk_input(path, case, x, want_rows):
    with open(path, "wb") as f:
        np.array([case.A, case.M, case.dim_c, int(case.values), int(want_rows)], np.int64).tofile(f)
        hd = np.zeros((2, 16), np.uint8)
        for i, (mv, sp) in enumerate(case.heads):
            hd[0, i], hd[1, i] = mv, sp
        hd.tofile(f)
        np.array([case.clip, -1.0 if case.value_clip is None else case.value_clip, case.vf_coef, case.ent_coef], F32).tofile(f)
        for i in range(case.A):
            x["logits"][i].tofile(f)
        if case.values:
            for i in range(case.A):
                x["values"][i].tofile(f)
        x["act"].tofile(f)
        if case.dim_c:
            x["utter"].tofile(f)
        for k in ("logp_old", "adv", "ret", "val_old"):
            x[k].tofile(f)


def read_walk_output(path, case, want_rows):
    A, M = case.A, case.M
    with open(path, "rb") as f:
        take = lambda shape: np.fromfile(f, F32, int(np.prod(shape))).reshape(shape)      # noqa: E731
        out = dict(dlogits=[take((M, n)) for n in case.n_out])
        out["dvalues"] = take((A, M)) if case.values else None
        out["rows"] = take((A, M, 4)) if want_rows else None
        out["stats"], out["loss"] = take((A, 8)), take((1,))[0]
        assert f.read() == b""
    return out
