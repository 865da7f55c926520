"""THE Q LOSS RULE and THE EXPLORATION RULE (include/mpe_hip.h) restated in NumPy: (a) a float64 form of the loss with
analytic gradients, held against torch float64 autograd (gather, max / double-Q gather, mse), (b) a float32 restatement, operation by
operation, to which the kernel is bit-equal, and the integer exploration rule on the SAMPLE draws' own bits.  Beside them the case
table, the row counts and inputs of the sweeps and the file format of tests/c/q_loss_host_walk.cpp.  Shared by
tests/test_q_loss_cpu.py, tests/test_gpu_q_loss.py and tests/test_gpu_actor_explore.py; importing it touches no device."""
import numpy as np

from _ppo_loss_ref import fold_sum

MOVE, ROW = 5, 16
F32, F64 = np.float32, np.float64
INDEPENDENT, VDN = 0, 1
MIXES = {"independent": INDEPENDENT, "vdn": VDN}


class Case(object):
    """the heads of a set of Q-networks: n_i = 5 * movable + dim_c * speaks logits, the move head first"""

    def __init__(self, name, dim_c, movable, speaks):
        self.name, self.dim_c, self.movable, self.speaks = name, dim_c, list(movable), list(speaks)
        self.A = len(self.movable)
        self.n = [MOVE * int(m) + dim_c * int(s) for m, s in zip(self.movable, self.speaks)]

    def heads(self, i):
        """[(first logit, logits, the rows that choose: 'act' / 'utter')] of agent i, in the logits' order"""
        out = []
        if self.movable[i]:
            out.append((0, MOVE, "act"))
        if self.speaks[i]:
            out.append((MOVE if self.movable[i] else 0, self.dim_c, "utter"))
        return out


# simple_spread N = 3 (move heads), simple_speaker_listener (an utterance-only agent, a move-only agent), simple_reference (both
# heads each) and one agent alone
CASES = {
    "spread3": Case("spread3", 0, [True] * 3, [False] * 3),
    "speaker_listener": Case("speaker_listener", 3, [False, True], [True, False]),
    "reference": Case("reference", 10, [True, True], [True, True]),
    "single": Case("single", 0, [True], [False]),
}
ROWS = [1, 63, 64, 65, 255, 256, 257, 1029]      # a wave's and a block's edges; 1029 rows of 5 floats end in a 16-byte tail
GAMMA = 0.95
# (mix, double, weighted, n-step) of the host walk's eight passes, in the order of its output
VARIANTS = [(mix, dbl, wn, wn) for mix in (INDEPENDENT, VDN) for dbl in (False, True) for wn in (False, True)]


def _choice_rows(rs, M, n):
    """[M, n] action rows: one-hot rows, softmax (non-one-hot) rows where m % 3 == 0, and a tie of two maxima where m % 13 == 7"""
    rows = np.zeros((M, n), F32)
    rows[np.arange(M), rs.randint(0, n, M)] = 1.0
    soft = rs.uniform(0.05, 1.0, (M, n))
    soft = (soft / soft.sum(axis=1, keepdims=True)).astype(F32)
    m = np.arange(M)
    rows[m % 3 == 0] = soft[m % 3 == 0]
    if n >= 3:
        tie = np.zeros(n, F32)
        tie[1:3] = 0.5
        rows[m % 13 == 7] = tie
    return rows


def make_inputs(case, M, seed=None, nan=False):
    """float32 inputs of one call: q_n[i] [M, n_i]; nt, no [A, M, 16] (zero beyond n_i; every head of no ties over all its entries
    where m % 7 == 3, the first two entries of every head of nt tie at the top where m % 11 == 5); act [A, M, 5], utter [A, M, dim_c];
    ret [A, M]; done uint8 [A, M] (all agents done where m % 5 == 0, none where m % 5 == 1); discount [M]; w [M] in (0.5, 1.5).
    nan: agent 0's row M // 2 of q is NaN."""
    rs = np.random.RandomState(4000 + 13 * M + case.A + case.dim_c if seed is None else seed)
    A, m = case.A, np.arange(M)
    x = dict(q_n=[rs.standard_normal((M, n)).astype(F32) for n in case.n])
    x["nt"], x["no"] = np.zeros((A, M, ROW), F32), np.zeros((A, M, ROW), F32)
    x["act"], x["utter"] = np.zeros((A, M, MOVE), F32), np.zeros((A, M, case.dim_c), F32)
    for i in range(A):
        x["nt"][i, :, :case.n[i]] = rs.standard_normal((M, case.n[i]))
        x["no"][i, :, :case.n[i]] = rs.standard_normal((M, case.n[i]))
        for k0, n, rows in case.heads(i):
            x["no"][i, m % 7 == 3, k0:k0 + n] = 0.25
            x["nt"][i, m % 11 == 5, k0:k0 + 2] = 3.0
            x[rows][i] = _choice_rows(rs, M, n)
    x["ret"] = rs.standard_normal((A, M)).astype(F32)
    done = rs.uniform(size=(A, M)) < 0.2
    done[:, m % 5 == 0], done[:, m % 5 == 1] = True, False
    x["done"] = done.astype(np.uint8)
    x["discount"] = (F32(GAMMA) ** rs.randint(1, 4, M)).astype(F32)
    x["w"] = rs.uniform(0.5, 1.5, M).astype(F32)
    if nan:
        x["q_n"][0][M // 2, :] = np.nan
    return x


def _chosen(case, x, i):
    """per head of agent i: (the column of the logits, [M]) the batch's rows choose -- np.argmax, the lowest index on ties"""
    return [k0 + x[rows][i].argmax(axis=1) for k0, n, rows in case.heads(i)]


def _taken(case, x, double, dtype):
    """q [A, M] and v [A, M]: the sums over the heads, the move head first, each addition rounded in dtype"""
    M = x["ret"].shape[1]
    q, v, rows = np.zeros((case.A, M), dtype), np.zeros((case.A, M), dtype), np.arange(M)
    for i in range(case.A):
        T, S = x["nt"][i].astype(dtype), (x["no"][i] if double else x["nt"][i]).astype(dtype)
        z = x["q_n"][i].astype(dtype)
        for h, ((k0, n, _), col) in enumerate(zip(case.heads(i), _chosen(case, x, i))):
            qh, vh = z[rows, col], T[rows, k0 + S[:, k0:k0 + n].argmax(axis=1)]
            q[i], v[i] = (qh, vh) if h == 0 else (q[i] + qh, v[i] + vh)
    return q, v


def _scatter(case, x, g, dtype):
    """g [A, M] (INDEPENDENT) or [M] (VDN) -> dq_n: g at the chosen column of each head, +0.0 everywhere else"""
    M = x["ret"].shape[1]
    out = []
    for i in range(case.A):
        d = np.zeros((M, case.n[i]), dtype)
        for col in _chosen(case, x, i):
            d[np.arange(M), col] = g[i] if g.ndim == 2 else g
        out.append(d)
    return out


# ---- (b) float32, operation by operation ---------------------------------------------------------------------------------------------
def q_loss32(case, x, mix, double, weighted, nstep):
    """-> dict dq_n (A arrays [M, n_i]), q_taken [A, M], y [A, M], td_abs [M], stats [A, 8], loss: the kernel's bits"""
    A, M = x["ret"].shape
    Mf = F32(M)
    q, v = _taken(case, x, double, F32)
    d = x["discount"] if nstep else np.full(M, F32(GAMMA), F32)
    w = x["w"] if weighted else None
    ret, done = x["ret"], x["done"] != 0
    with np.errstate(invalid="ignore"):
        if mix == INDEPENDENT:
            y = np.where(done, ret, ret + d[None, :] * v).astype(F32)
            delta = q - y
            ad = np.abs(delta)
            t = ad[0].copy()
            for i in range(1, A):
                t = np.where((ad[i] > t) | np.isnan(ad[i]), ad[i], t)
        else:
            Q, V, R = q[0].copy(), v[0].copy(), ret[0].copy()
            for i in range(1, A):
                Q, V, R = Q + q[i], V + v[i], R + ret[i]
            r = R * (F32(1.0) / F32(A))
            yt = np.where(done.any(axis=0), r, r + d * V).astype(F32)
            delta = np.broadcast_to(Q - yt, (A, M))
            y = np.broadcast_to(yt, (A, M)).copy()
            ad = np.abs(delta)
            t = ad[0].copy()
        wd = delta if w is None else w[None, :] * delta
        sq = wd * delta
        g = (F32(2.0) * wd) / Mf
    stats, total = np.zeros((A, 8), F32), F64(0.0)
    for i in range(A):
        mean = [fold_sum(c[i]) / F64(M) for c in (sq, ad, q, y)]
        stats[i, :4] = [F32(m_) for m_ in mean]
        stats[i, 6] = F32(mean[0])
        if mix == INDEPENDENT:
            total = total + mean[0]
        elif i == 0:
            total = mean[0]
    return dict(dq_n=_scatter(case, x, g.astype(F32) if mix == INDEPENDENT else g[0].astype(F32), F32), q_taken=q, y=y,
                td_abs=t.astype(F32), stats=stats, loss=F32(total))


# ---- (a) float64 -------------------------------------------------------------------------------------------------------------------
def q_loss64(case, x, mix, double, weighted, nstep):
    A, M = x["ret"].shape
    q, v = _taken(case, x, double, F64)
    d = x["discount"].astype(F64) if nstep else np.full(M, F64(F32(GAMMA)))
    w = x["w"].astype(F64) if weighted else np.ones(M)
    ret, done = x["ret"].astype(F64), x["done"] != 0
    if mix == INDEPENDENT:
        y = np.where(done, ret, ret + d[None, :] * v)
        delta = q - y
        loss, g, td = (w * delta * delta).mean(axis=1).sum(), 2.0 * w * delta / M, np.abs(delta).max(axis=0)
    else:
        r = ret.sum(axis=0) / A
        y = np.where(done.any(axis=0), r, r + d * v.sum(axis=0))
        delta = q.sum(axis=0) - y
        loss, g, td = (w * delta * delta).mean(), 2.0 * w * delta / M, np.abs(delta)
    return dict(dq_n=_scatter(case, x, g, F64), td_abs=td, loss=loss)


def torch_q(case, x, mix, double, weighted, nstep, dtype):
    """the same loss as a learner writes it in torch: gather, max / double-Q gather, (weighted) mse; autograd for dq"""
    import torch
    import torch.nn.functional as Fn
    A, M = x["ret"].shape
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)      # noqa: E731
    zs = [t(z).requires_grad_(True) for z in x["q_n"]]
    d = t(x["discount"]) if nstep else torch.full((M,), float(F32(GAMMA)), dtype=dtype)
    w = t(x["w"]) if weighted else None
    qs, vs = [], []
    for i in range(A):
        T, S = t(x["nt"][i]), t(x["no"][i] if double else x["nt"][i])
        q = v = None
        for k0, n, rows in case.heads(i):
            a = torch.as_tensor(x[rows][i].argmax(axis=1))[:, None]
            qh = zs[i][:, k0:k0 + n].gather(1, a)[:, 0]
            if double:
                # (np.argmax's tie rule: torch.argmax does not promise the lowest index)
                vh = T[:, k0:k0 + n].gather(1, torch.as_tensor(S[:, k0:k0 + n].numpy().argmax(axis=1))[:, None])[:, 0]
            else:
                vh = T[:, k0:k0 + n].max(dim=1).values
            q, v = (qh, vh) if q is None else (q + qh, v + vh)
        qs.append(q), vs.append(v)
    ret, live = t(x["ret"]), t(1 - (x["done"] != 0))
    if mix == INDEPENDENT:
        ys = [(ret[i] + d * live[i] * vs[i]).detach() for i in range(A)]
        loss = sum((Fn.mse_loss(qs[i], ys[i]) if w is None else (w * (qs[i] - ys[i]) ** 2).mean()) for i in range(A))
        td = torch.stack([(qs[i] - ys[i]).abs() for i in range(A)]).max(dim=0).values
    else:
        Q, y = sum(qs), (ret.sum(dim=0) / A + d * live.min(dim=0).values * sum(vs)).detach()
        loss = Fn.mse_loss(Q, y) if w is None else (w * (Q - y) ** 2).mean()
        td = (Q - y).abs()
    loss.backward()
    return dict(dq_n=[z.grad.numpy() for z in zs], td_abs=td.detach().numpy(), loss=loss.item())


def same_bits(a, b):
    """bit-equal, a NaN standing where a NaN stands (its payload and sign are the adder's)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---- THE EXPLORATION RULE -------------------------------------------------------------------------------------------------------------
def explore_E(epsilon):
    return min(65536, int(np.floor(epsilon * 65536.0 + 0.5)))


def head_bits(stream, seed, B, t, agent, world_offset):
    """the 32 bits of (world_offset + b, step t, agent) on `stream` (tests/_actor_ref.py draw_u's block, all 32 bits) -> uint32 [B]"""
    from oracle import philox
    b = np.arange(B, dtype=np.uint64) + np.uint64(world_offset)
    o = philox.philox4x32_10(b & philox.MASK, ((b >> np.uint64(32)) ^ np.uint64(t >> 32)) & philox.MASK,
                             np.full(B, agent >> 2, np.uint64), np.full(B, (stream ^ (t & 0xFFFFFFFF)) & 0xFFFFFFFF, np.uint64),
                             seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return np.asarray(o[agent & 3]).astype(np.uint32)


def explore_pick(bits, n, E, greedy):
    """bits uint32 [B], greedy int [B] -> (the chosen index [B], explored bool [B])"""
    b = bits.astype(np.uint64)
    explored = (b >> np.uint64(16)) < np.uint64(E)
    idx = ((b & np.uint64(0xFFFF)) * np.uint64(n)) >> np.uint64(16)
    return np.where(explored, idx.astype(np.int64), np.asarray(greedy, np.int64)), explored


# ---- the file format of tests/c/q_loss_host_walk.cpp ------------------------------------------------------------------------------------
def write_walk_input(path, case, M, x):
    """int64 A, M, dim_c; uint8 movable[16], speaks[16]; float32 gamma; then float32 q_n (agent by agent), nt, no, act, utter, ret,
    discount, w; uint8 done"""
    with open(path, "wb") as f:
        np.array([case.A, M, case.dim_c], np.int64).tofile(f)
        for flags in (case.movable, case.speaks):
            b = np.zeros(16, np.uint8)
            b[:case.A] = flags
            b.tofile(f)
        np.array([GAMMA], F32).tofile(f)
        for z in x["q_n"]:
            z.tofile(f)
        for k in ("nt", "no", "act", "utter", "ret", "discount", "w"):
            np.ascontiguousarray(x[k], F32).tofile(f)
        np.ascontiguousarray(x["done"], np.uint8).tofile(f)


def read_walk_output(path, case, M):
    """-> one dict per VARIANTS entry: dq_n, q_taken, y, td_abs, stats, loss"""
    raw, at, out = np.fromfile(path, F32), 0, []

    def take(*shape):
        nonlocal at
        k = int(np.prod(shape))
        v = raw[at:at + k].reshape(shape)
        at += k
        return v
    for _ in VARIANTS:
        o = dict(dq_n=[take(M, n) for n in case.n])
        o["q_taken"], o["y"], o["td_abs"], o["stats"], o["loss"] = take(case.A, M), take(case.A, M), take(M), take(case.A, 8), take(1)[0]
        out.append(o)
    assert at == raw.size
    return out
