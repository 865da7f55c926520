"""THE MLP INPUT GRADIENT RULE of include/mpe_hip.h restated in NumPy float64 from the header's words, the cases and windows the CPU
and GPU tests of mpe_mlp_dinput share, float32 / float64 torch autograd with respect to the input on the same inputs, and the files
of tests/c/mlp_dinput_host_walk.cpp.  Nets, fixed inputs (the ReLU band redraw included), the packed layout and the parity bound are
tests/_mlp_grad_ref.py's.  Nothing here reads the kernel's code."""
import numpy as np

import _mlp_grad_ref as R
from _mlp_grad_ref import Net, case, make_inputs, pack, fill_set, forward64, bounds, offsets, widths      # noqa: F401

F32, F64 = R.F32, R.F64
ROWS, MAX_BLOCKS = 64, 512      # rows of a group, blocks per agent at most (the cut of the rows: not part of the rule)
PAD, SENTINEL = 8, -777.25      # tests/c/mlp_dinput_host_walk.cpp: sentinel floats around every din buffer

CR = Net(60, (64, 64), 1, "relu", True)
CRT = CR._replace(act="tanh")
CASES = [case("critics_M%d" % M, [CR, CRT], [0, 1], M, 100 + M) for M in (1, 63, 64, 65, 129)] + [
    case("mixed_M65", R.MIXED, range(len(R.MIXED)), 65, 121),
    case("shared_M65", [CR], [0, 0, 0], 65, 122),
    case("tail_bias3_M65", [CR, CRT, Net(18, (33,), 5, "tanh", True)], [0, 1, 2], 65, 125, bias_scale=3.0),
    case("wide_M65", [Net(256, (64, 64), 1, "relu", True)], [0], 65, 126),
]
IDS = [c.name for c in CASES]
# a block that walks two groups: 514 groups in 257 blocks (the sanitizer host walk's own; the GPU runs SPAN2)
WALK_EXTRA = case("span2_M32833", [Net(18, (64, 64), 1, "relu", True), Net(40, (), 3, "tanh", True)], [0, 1], ROWS * MAX_BLOCKS + 65, 131)
KINDS = ["whole", "first", "last", "last5", "straddle"]
# A block that walks two groups, on the GPU: the smallest M of span 2 -- 513 groups in 257 blocks, the last of one group holding one
# row -- with a 256-wide net, whose output takes several rounds of the stage tile inside a multi-group block.  Not in CASES: the
# host walk's sweep does not grow.  Windows: SPAN2_KINDS on the 16-byte path, SPAN2_SENTINEL_KINDS on the 4-byte path.
SPAN2 = case("span2_M32769", [CR, CRT, Net(256, (64, 64), 1, "relu", True)], [0, 1, 2], ROWS * MAX_BLOCKS + 1, 141)
SPAN2_KINDS, SPAN2_SENTINEL_KINDS = ["whole", "straddle"], ["last5"]


def span(M):
    return max(1, ((M + ROWS - 1) // ROWS + MAX_BLOCKS - 1) // MAX_BLOCKS)


def blocks(M):
    g = (M + ROWS - 1) // ROWS
    return (g + span(M) - 1) // span(M)


def window(kind, D):
    """(col0, ncol) of a D-wide input, clipped to D; None where the window does not exist at this D"""
    if kind == "whole":
        return 0, D
    if kind == "first":
        return 0, 1
    if kind == "last":
        return D - 1, 1
    if kind == "last5":
        return max(0, D - 5), min(5, D)
    if kind == "straddle":      # across a 32-column tile
        return (30, 6) if D >= 36 else None
    raise KeyError(kind)


def windows(c, kind):
    """per agent (col0, ncol); an agent whose input is too narrow for the kind takes its whole row; None: no agent has the window"""
    w = [window(kind, c.nets[m].D) for m in c.agents]
    if all(x is None for x in w):
        return None
    return [x if x is not None else (0, c.nets[m].D) for x, m in zip(w, c.agents)]


def runs(cases=None):
    """every (case, kind) that exists"""
    return [(c, k) for c in (CASES if cases is None else cases) for k in KINDS if windows(c, k) is not None]


def run_id(ck):
    return "%s-%s" % (ck[0].name, ck[1])


def din64(net, params, x, dout):
    """THE MLP INPUT GRADIENT RULE for one agent in float64 -> din [M, D]: h_l recomputed, delta_(L-1) = dout,
    delta_(l-1) = (delta_l . W_l^T) * phi'(h_(l-1)), din = delta_0 . W_0^T"""
    hs, _ = forward64(net, params, x)
    delta = dout.astype(F64).reshape(x.shape[0], net.n_out)
    for l in range(len(net.hidden), 0, -1):
        back = delta @ params[l][0].astype(F64).T
        h = hs[l - 1]
        delta = back * (1.0 - h * h) if net.act == "tanh" else np.where(h > 0, back, 0.0)
    return delta @ params[0][0].astype(F64).T


def rule64(c, x):
    """-> per AGENT din [M, D_i], float64"""
    return [din64(c.nets[m], x["params"][m], x["in"][i], x["dout"][i]) for i, m in enumerate(c.agents)]


def torch_din(c, x, dtype, device="cpu"):
    """torch.autograd.grad with respect to the input on the same inputs -> per agent [M, D_i] float64 arrays"""
    import torch
    mods = R.torch_modules(c, x, dtype, device)
    out = []
    for i, m in enumerate(c.agents):
        inp = torch.from_numpy(x["in"][i]).to(dtype).to(device).requires_grad_()
        g, = torch.autograd.grad(mods[m](inp), inp, torch.from_numpy(x["dout"][i]).to(dtype).to(device))
        out.append(g.double().cpu().numpy())
    return out


def deviations(got, ref, win):
    """{agent: (max |got - ref|, max |ref|)} over each agent's window; got[i]: [M, ncol_i], ref[i]: [M, D_i]"""
    d = {}
    for i, (g, r, (c0, nc)) in enumerate(zip(got, ref, win)):
        r = r[:, c0:c0 + nc]
        d[i] = (float(np.abs(np.asarray(g, F64) - r).max()), float(np.abs(r).max()))
    return d


def cut(full, win):
    return [f[:, c0:c0 + nc] for f, (c0, nc) in zip(full, win)]


# ---- tests/c/mlp_dinput_host_walk.cpp: its input and output files ------------------------------------------------------------------------
def walk_layout(c, win, vec):
    """per agent (ld, rows of the buffer, shift): vec -> a 16-byte aligned window and ld a multiple of 4; else ld = ncol + 3, 4 bytes off"""
    return [((nc + 3) // 4 * 4, c.M + 2, 0) if vec else (nc + 3, c.M + 2, 1) for _, nc in win]


def write_walk_input(path, c, x, win, lay):
    off, total = offsets(c)
    with open(path, "wb") as f:
        np.array([len(c.agents)], np.int32).tofile(f)
        np.array([c.M], np.int64).tofile(f)
        for m, (c0, nc), (ld, rows, shift) in zip(c.agents, win, lay):
            net, w = c.nets[m], widths(c.nets[m])
            np.array([len(w) - 1, 1 if net.act == "tanh" else 0] + (w + [0, 0, 0])[:4] + [off[m], c0, nc, ld, rows, shift], np.int32).tofile(f)
        np.array([total], np.int32).tofile(f)
        pack(c, x).tofile(f)
        for i in range(len(c.agents)):
            x["in"][i].tofile(f)
            x["dout"][i].tofile(f)


def read_walk_output(path, c, win, lay):
    """-> (per agent the windows [M, ncol_i], True if every sentinel is intact: in front, behind, between ncol and ld, in rows >= M)"""
    flat, at, got, intact = np.fromfile(path, F32), 0, [], True
    for (c0, nc), (ld, rows, shift) in zip(win, lay):
        n = PAD + shift + rows * ld + PAD
        buf = flat[at:at + n]
        at += n
        body = buf[PAD + shift:PAD + shift + rows * ld].reshape(rows, ld)
        intact = intact and np.all(buf[:PAD + shift] == SENTINEL) and np.all(buf[n - PAD:] == SENTINEL) and \
            np.all(body[:c.M, nc:] == SENTINEL) and np.all(body[c.M:] == SENTINEL) and not np.any(body[:c.M, :nc] == SENTINEL)
        got.append(body[:c.M, :nc].copy())
    assert at == flat.size
    return got, bool(intact)
