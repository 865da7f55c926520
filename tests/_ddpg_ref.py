"""The four rules of the off-policy update (include/mpe_hip.h: THE TD LOSS RULE, THE POLICY ROWS RULE, THE POLICY ROWS GRADIENT RULE,
THE POLYAK RULE) restated in NumPy: (a) float64 restatements with analytic gradients, held against torch float64 autograd of the
MADDPG example's own formulas, and (b) float32 restatements of the rules without a transcendental (TD loss, Polyak), operation by
operation, to which the kernels are bit-equal.  Beside them the fixed layouts, row counts and inputs of the sweeps, the parity bound
and the file format of tests/c/ddpg_host_walk.cpp.  Shared by tests/test_ddpg_cpu.py, tests/test_gpu_ddpg.py and
tools/ddpg_parity.py; importing it touches no device."""
import numpy as np

from _ppo_loss_ref import BLOCK, LOGP_TOL, fold_sum  # noqa: F401

MOVE = 5
F32, F64 = np.float32, np.float64


class Layout(object):
    """W floats per joint row; per agent the first column of its window and its heads; n = 5 * movable + dim_c * speaks"""

    def __init__(self, name, W, dim_c, col, movable, speaks):
        self.name, self.W, self.dim_c, self.col, self.movable, self.speaks = name, W, dim_c, list(col), list(movable), list(speaks)
        self.A = len(self.col)
        self.n = [MOVE * int(m) + dim_c * int(s) for m, s in zip(self.movable, self.speaks)]

    def heads(self, i):
        """[(first logit, logits)] of agent i's heads, in the logits' order"""
        out, at = [], 0
        if self.movable[i]:
            out.append((0, MOVE))
            at = MOVE
        if self.speaks[i]:
            out.append((at, self.dim_c))
        return out


# simple_spread (3 x 18 observations, 3 move rows), speaker_listener (3 + 11; a speaker that does not move, a silent listener),
# simple_reference (2 x 21; both heads each: the last window ends at W), and the widest set: 16 agents with one logit each
LAYOUTS = {
    "L69": Layout("L69", 69, 0, [54, 59, 64], [True] * 3, [False] * 3),
    "L22": Layout("L22", 22, 3, [14, 17], [False, True], [True, False]),
    "L72": Layout("L72", 72, 10, [42, 57], [True, True], [True, True]),
    "L32": Layout("L32", 32, 1, list(range(16, 32)), [False] * 16, [True] * 16),
}
ROWS = [1, 63, 64, 65, 255, 256, 257, 1025]
POLYAK_N = [16, 1008, 1024, 1040, 38496]
POLYAK_TAU = [0.0, 0.01, 0.5, 1.0]


def make_inputs(lay, M, seed=None):
    """float32: joint N(0, 1) with a NaN of a rare payload outside the windows; logits uniform in [-10, 10] (no e_j underflows:
    check_logits); g, the upstream gradient of the windows, N(0, 1) as a full [M, W] row gradient per agent; q, y [A, M] and the
    weights w [M] in (0.5, 1.5)."""
    rs = np.random.RandomState(1000 + 7 * M + lay.A + lay.W if seed is None else seed)
    x = dict(joint=rs.standard_normal((M, lay.W)).astype(F32))
    x["joint"].view(np.uint32)[M // 2, 0] = 0x7fc12345
    x["logits"] = [rs.uniform(-10.0, 10.0, (M, n)).astype(F32) for n in lay.n]
    x["G"] = [rs.standard_normal((M, lay.W)).astype(F32) for _ in lay.n]
    x["q"] = rs.standard_normal((lay.A, M)).astype(F32)
    x["y"] = (x["q"] + 0.5 * rs.standard_normal((lay.A, M))).astype(F32)
    x["w"] = rs.uniform(0.5, 1.5, M).astype(F32)
    return x


def check_logits(lay, x):
    """no e_j = exp(z_j - zm) of any head underflows in float32 (nor comes near: the smallest is far above 2^-126)"""
    for i, z in enumerate(x["logits"]):
        for k0, n in lay.heads(i):
            h = z[:, k0:k0 + n].astype(F64)
            assert (h - h.max(axis=1, keepdims=True)).min() >= -20.0


# ---- (b) float32, operation by operation ---------------------------------------------------------------------------------------------
def td_loss32(q, y, w):
    """q, y [A, M] float32, w [M] or None -> dict dq [A, M], td_abs [M], stats [A, 8], loss: the kernel's bits"""
    A, M = q.shape
    Mf = F32(M)
    d = q - y
    wd = d if w is None else w[None, :] * d
    sq = wd * d
    dq = (F32(2.0) * wd) / Mf
    ad = np.abs(d)
    t = ad[0].copy()
    for i in range(1, A):
        take = (ad[i] > t) | np.isnan(ad[i])
        t = np.where(take, ad[i], t)
    stats, total = np.zeros((A, 8), F32), F64(0.0)
    for i in range(A):
        mean = [fold_sum(c[i]) / F64(M) for c in (sq, ad, q, y)]
        stats[i, :4] = [F32(v) for v in mean]
        stats[i, 6] = F32(mean[0])
        total = total + mean[0]
    return dict(dq=dq.astype(F32), td_abs=t.astype(F32), stats=stats, loss=F32(total))


def polyak32(x, w, tau):
    """x, w float32 -> the target after one step: torch.lerp's branch form"""
    t = F32(tau)
    d = w - x
    if t < F32(0.5):
        return x + t * d
    return w - d * (F32(1.0) - t)


# ---- (a) float64 -------------------------------------------------------------------------------------------------------------------
def td_loss64(q, y, w):
    A, M = q.shape
    q, y = q.astype(F64), y.astype(F64)
    w = np.ones(M) if w is None else w.astype(F64)
    d = q - y
    sq = w * d * d
    stats = np.zeros((A, 8))
    stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3] = sq.mean(axis=1), np.abs(d).mean(axis=1), q.mean(axis=1), y.mean(axis=1)
    stats[:, 6] = stats[:, 0]
    return dict(dq=2.0 * w * d / M, td_abs=np.abs(d).max(axis=0), stats=stats, loss=stats[:, 6].sum())


def softmax64(lay, i, z):
    """z [M, n_i] (any float dtype) -> (p [M, n_i], H [M]) in float64, head by head"""
    z = z.astype(F64)
    p, H = np.zeros_like(z), np.zeros(len(z))
    for k0, n in lay.heads(i):
        h = z[:, k0:k0 + n]
        zm = h.max(axis=1, keepdims=True)
        e = np.exp(h - zm)
        s = e.sum(axis=1, keepdims=True)
        p[:, k0:k0 + n] = e / s
        H -= ((e / s) * ((h - zm) - np.log(s))).sum(axis=1)
    return p, H


def rows64(lay, x):
    """-> per agent the [M, W] float64 rows: joint with the window replaced by the heads' softmax"""
    out = []
    for i in range(lay.A):
        r = x["joint"].astype(F64)
        r[:, lay.col[i]:lay.col[i] + lay.n[i]] = softmax64(lay, i, x["logits"][i])[0]
        out.append(r)
    return out


def windows(lay, G):
    """per agent the window's columns of a full-row gradient"""
    return [g[:, c:c + n] for g, c, n in zip(G, lay.col, lay.n)]


def rows_grad64(lay, x, reg_coef, q=None):
    """-> dict dlogits (per agent [M, n_i]), operand (per agent the largest p_j * max(|g_j|, |dot|) (+ |cr z_j|): what g_j - dot is
    formed from), and with q: stats [A, 8], loss"""
    M = len(x["joint"])
    out = dict(dlogits=[], operand=[])
    stats = np.zeros((lay.A, 8))
    for i in range(lay.A):
        z = x["logits"][i].astype(F64)
        g = windows(lay, x["G"])[i].astype(F64)
        p, H = softmax64(lay, i, z)
        dz, op = np.zeros_like(z), 0.0
        for k0, n in lay.heads(i):
            ph, gh = p[:, k0:k0 + n], g[:, k0:k0 + n]
            dot = (ph * gh).sum(axis=1, keepdims=True)
            dz[:, k0:k0 + n] = ph * (gh - dot)
            op = max(op, float((ph * np.maximum(np.abs(gh), np.abs(dot))).max()))
        cr = 2.0 * reg_coef / (M * lay.n[i])
        out["dlogits"].append(dz + cr * z)
        out["operand"].append(op + float(np.abs(cr * z).max()))
        if q is not None:
            stats[i, 0], stats[i, 1], stats[i, 2] = q[i].astype(F64).mean(), (z * z).mean(), H.mean()
            stats[i, 6] = -stats[i, 0] + reg_coef * stats[i, 1]
    if q is not None:
        out["stats"], out["loss"] = stats, stats[:, 6].sum()
    return out


# ---- the example's formulas in torch autograd ------------------------------------------------------------------------------------------
def torch_td(x, weighted, dtype, device="cpu"):
    """sum over the agents of mean(w * (q_i - y_i)^2): F.mse_loss per agent where w is 1 -> the dict td_loss64 returns"""
    import torch
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype, device=device)      # noqa: E731
    q, y = t(x["q"]).requires_grad_(), t(x["y"])
    w = t(x["w"]) if weighted else torch.ones_like(y[0])
    sq = w * (q - y) ** 2
    loss = sq.mean(dim=1).sum()
    loss.backward()
    n = lambda a: a.detach().double().cpu().numpy()      # noqa: E731
    stats = np.zeros((q.shape[0], 8))
    stats[:, 0], stats[:, 1], stats[:, 2], stats[:, 3] = n(sq.mean(dim=1)), n((q - y).abs().mean(dim=1)), n(q.mean(dim=1)), n(y.mean(dim=1))
    stats[:, 6] = stats[:, 0]
    return dict(dq=n(q.grad), td_abs=n((q - y).abs().max(dim=0).values), stats=stats, loss=float(n(loss)))


def torch_rows(lay, x, reg_coef, dtype, device="cpu", q=None):
    """The example's actor loss up to the critics: joint.clone(), F.softmax per head, the column write; the critics stand in as a
    linear functional G_i of the rows (their input gradient), so L = sum_i <rows_i, G_i> + reg_coef * mean(logits_i^2)
    -> dict rows (per agent [M, W]), dlogits (per agent), and with q: stats, loss = sum_i -mean q_i + reg_coef * mean z_i^2"""
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype, device=device)      # noqa: E731
    joint = t(x["joint"])
    zs = [t(z).requires_grad_() for z in x["logits"]]
    rows, total, reg, ent = [], 0.0, [], []
    for i, z in enumerate(zs):
        r = joint.clone()
        ps = [F.softmax(z[:, k0:k0 + n], dim=1) for k0, n in lay.heads(i)]
        r[:, lay.col[i]:lay.col[i] + lay.n[i]] = torch.cat(ps, dim=1)
        rows.append(r)
        reg.append((z ** 2).mean())
        ent.append(sum(-(F.softmax(z[:, k0:k0 + n], dim=1) * F.log_softmax(z[:, k0:k0 + n], dim=1)).sum(dim=1) for k0, n in lay.heads(i)).mean())
        total = total + torch.nan_to_num(r * t(x["G"][i])).sum() + reg_coef * reg[-1]
    total.backward()
    n_ = lambda a: a.detach().double().cpu().numpy()      # noqa: E731
    out = dict(rows=[n_(r) for r in rows], dlogits=[n_(z.grad) for z in zs])
    if q is not None:
        stats = np.zeros((lay.A, 8))
        qt = t(q)
        for i in range(lay.A):
            stats[i, 0], stats[i, 1], stats[i, 2] = float(n_(qt[i].mean())), float(n_(reg[i])), float(n_(ent[i]))
            stats[i, 6] = float(n_(-qt[i].mean() + reg_coef * reg[i]))
        out["stats"], out["loss"] = stats, float(n_(sum(-qt[i].mean() + reg_coef * reg[i] for i in range(lay.A))))
    return out


# ---- parity: the kernel against (a), the bound taken from float32 torch autograd on the same inputs ----------------------------------
def _dev(got, want):
    d = np.abs(np.asarray(got, F64) - np.asarray(want, F64))
    return float(d.max()) if d.size else 0.0


def _mag(a):
    return float(np.abs(np.asarray(a, F64)).max()) if np.size(a) else 0.0


def grad_deviations(lay, out, ref):
    """out: dlogits (per agent) and optionally stats, loss -> name -> (deviation, the magnitude its floor takes).  dlogits: g_j - dot
    is a difference of rounded operands, so the floor takes the operands' magnitude (as _ppo_loss_ref does for l_j + H)."""
    d = {"dlogits": (max(_dev(out["dlogits"][i], ref["dlogits"][i]) for i in range(lay.A)),
                     max(max(_mag(ref["dlogits"][i]), ref["operand"][i]) if "operand" in ref else _mag(ref["dlogits"][i]) for i in range(lay.A)))}
    if "stats" in out and out["stats"] is not None and "stats" in ref:
        for k, name in ((0, "mean_q"), (1, "mean_z2"), (2, "mean_H"), (6, "L_i")):
            d[name] = (_dev(np.asarray(out["stats"])[:, k], ref["stats"][:, k]), _mag(ref["stats"][:, k]))
        d["loss"] = (abs(float(out["loss"]) - float(ref["loss"])), abs(float(ref["loss"])))
    return d


def bounds(dev_torch):
    """tests/_ppo_loss_ref.py's bound: at most 4 x the deviation of float32 torch autograd, floor 2 float32 ulps of the magnitude"""
    return {name: max(4.0 * dev, 2.0 * float(np.spacing(F32(mag)))) for name, (dev, mag) in dev_torch.items()}


def logp_deviation(lay, rows, x):
    """max |log p - log p64| over every window of the rows the kernel wrote (held to LOGP_TOL)"""
    worst = 0.0
    for i in range(lay.A):
        p64 = softmax64(lay, i, x["logits"][i])[0]
        got = np.asarray(rows[i], F64)[:, lay.col[i]:lay.col[i] + lay.n[i]]
        assert (got > 0).all()
        worst = max(worst, float(np.abs(np.log(got) - np.log(p64)).max()))
    return worst


def outside_equal(lay, rows, x):
    """outside the windows every output row is joint, bit for bit"""
    for i in range(lay.A):
        keep = np.ones(lay.W, bool)
        keep[lay.col[i]:lay.col[i] + lay.n[i]] = False
        if not np.array_equal(np.asarray(rows[i]).view(np.uint32)[:, keep], x["joint"].view(np.uint32)[:, keep]):
            return False
    return True


# ---- tests/c/ddpg_host_walk.cpp: its input and output files ---------------------------------------------------------------------------
def write_walk_input(path, lay, M, x, reg_coef, polyak):
    """polyak: [(x, w, tau)]"""
    with open(path, "wb") as f:
        np.array([lay.A, M, lay.W, lay.dim_c, len(polyak)], np.int64).tofile(f)
        hd = np.zeros((2, 16), np.uint8)
        hd[0, :lay.A], hd[1, :lay.A] = lay.movable, lay.speaks
        hd.tofile(f)
        col = np.zeros(16, np.int32)
        col[:lay.A] = lay.col
        col.tofile(f)
        np.array([reg_coef], F64).tofile(f)
        x["joint"].tofile(f)
        for z in x["logits"]:
            z.tofile(f)
        for g in x["G"]:
            g.tofile(f)
        for k in ("q", "y", "w"):
            x[k].tofile(f)
        for xs, ws, tau in polyak:
            np.array([len(xs)], np.int64).tofile(f)
            np.array([tau], F64).tofile(f)
            xs.tofile(f)
            ws.tofile(f)


def read_walk_output(path, lay, M, polyak):
    A, W = lay.A, lay.W
    with open(path, "rb") as f:
        take = lambda shape: np.fromfile(f, F32, int(np.prod(shape))).reshape(shape)      # noqa: E731
        out = {}
        for tag in ("td_w", "td"):
            out[tag] = dict(dq=take((A, M)), td_abs=take((M,)), stats=take((A, 8)), loss=take((1,))[0])
        out["rows"] = [take((M, W)) for _ in range(A)]
        for tag in ("grad_packed", "grad_inplace"):
            out[tag] = dict(dlogits=[take((M, n)) for n in lay.n], stats=take((A, 8)), loss=take((1,))[0])
        out["grad_nostats"] = dict(dlogits=[take((M, n)) for n in lay.n])
        out["polyak"] = [take((len(xs),)) for xs, _, _ in polyak]
        assert f.read() == b""
    return out
