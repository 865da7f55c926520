"""THE MLP GRADIENT RULE of include/mpe_hip.h restated in NumPy float64 from the header's words, the cases the CPU and GPU tests of
mpe_mlp_grad share, their fixed inputs, float32 / float64 torch autograd on the same inputs, the packed layout, the parity bound
and the files of tests/c/mlp_grad_host_walk.cpp.  Nothing here reads the kernel's code."""
import collections

import numpy as np

F32, F64 = np.float32, np.float64
HW, LW, ROWS, MAX_CHUNKS = 64, 16, 64, 128      # packed widths (hidden, last), rows of a group, chunks at most (the header's numbers)
BIAS_SLOTS = 2 * HW + LW                        # floats behind a partial's block: the low halves of the chunk's bias sums
BAND = 1e-4                                     # no ReLU pre-activation of the float64 reference lies this close to 0

# one module: input width, hidden widths, outputs, activation, bias
Net = collections.namedtuple("Net", "D hidden n_out act bias")
# nets: the distinct modules; agents: the module of every agent; bias_scale: None (nn.Linear's own range) or the biases' magnitude;
# shift: in and dout start 4 bytes into their allocations; value: the set's mode is MPE_POLICY_VALUE
Case = collections.namedtuple("Case", "name nets agents M seed bias_scale shift value")


def case(name, nets, agents, M, seed, bias_scale=None, shift=False, value=False):
    return Case(name, tuple(nets), tuple(agents), M, seed, bias_scale, shift, value)


ACTOR, CRITIC = Net(18, (64, 64), 5, "tanh", True), Net(18, (64, 64), 1, "relu", True)
CHUNK = ROWS      # the chunk size at these M: one group (span = max(1, ceil(groups / 128)) = 1)
MIXED = [Net(1, (1,), 1, "relu", True), Net(31, (32, 33), 5, "tanh", True), Net(32, (), 9, "relu", False),
         Net(33, (64, 1), 16, "relu", True), Net(256, (33, 64), 16, "tanh", True), Net(5, (), 1, "tanh", True)]
GPU_CASES = [case("M%d" % M, [ACTOR, ACTOR._replace(act="relu")], [0, 1], M, 10 + M) for M in (1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)] + [
    case("mixed_M65", MIXED, range(len(MIXED)), 65, 21),
    case("shared_all_M65", [ACTOR._replace(act="relu")], [0, 0, 0], 65, 22),
    case("shared_two_of_three_M65", [ACTOR, CRITIC._replace(n_out=5)], [0, 1, 0], 65, 23),
    case("shifted_M65", [ACTOR, Net(33, (32,), 9, "relu", True)], [0, 1], 65, 24, shift=True),
    case("tail_bias3_M65", [ACTOR, ACTOR._replace(act="relu"), Net(18, (33,), 5, "tanh", True)], [0, 1, 2], 65, 25, bias_scale=3.0),
    case("spread_actors_M257", [ACTOR] * 3, [0, 1, 2], 257, 26),
    case("spread_critics_M257", [CRITIC] * 3, [0, 1, 2], 257, 27, value=True),
]
GPU_IDS = [c.name for c in GPU_CASES]
# Chunks of more than one group, on the GPU: the smallest M of span 2 and of span 3 whose last chunk is short and ends in a group of one
# row (131 groups in 66 chunks, the last of one group; 257 groups in 86 chunks, the last of two), and a shared module at span 2 for the
# fixed-order sum over 2 x 66 partials.  The sanitizer host walk does not take them (its span 2 is WALK_EXTRA).
SPAN_CASES = [
    case("span2_M8321", [ACTOR, ACTOR._replace(act="relu"), Net(40, (), 3, "relu", True)], [0, 1, 2], ROWS * MAX_CHUNKS + 2 * ROWS + 1, 41),
    case("span3_M16385", [ACTOR, CRITIC, Net(33, (32,), 9, "relu", True)], [0, 1, 2], 2 * ROWS * MAX_CHUNKS + 1, 42),
    case("shared_span2_M8321", [ACTOR._replace(act="relu")], [0, 0], ROWS * MAX_CHUNKS + 2 * ROWS + 1, 43),
]
SPAN_IDS = [c.name for c in SPAN_CASES]
# a span of 2 groups and the most chunks there are: the sanitizer host walk's own (the GPU runs SPAN_CASES)
WALK_EXTRA = case("span2_M8257", [Net(18, (64, 64), 5, "tanh", True), Net(40, (), 3, "relu", True)], [0, 1], 64 * MAX_CHUNKS + 65, 31)


def groups(M):
    return (M + ROWS - 1) // ROWS


def span(M):
    return max(1, (groups(M) + MAX_CHUNKS - 1) // MAX_CHUNKS)


def chunks(M):
    return (groups(M) + span(M) - 1) // span(M)


def widths(net):
    return [net.D] + list(net.hidden) + [net.n_out]


def module_size(net):
    L = len(net.hidden) + 1
    return sum(((net.D if l == 0 else HW) + 1) * (LW if l == L - 1 else HW) for l in range(L))


def offsets(c):
    off, at = [], 0
    for n in c.nets:
        off.append(at)
        at += module_size(n)
    return off, at


def work_floats(c):
    return chunks(c.M) * sum(module_size(c.nets[m]) + BIAS_SLOTS for m in c.agents)


def act64(x, act):
    return np.tanh(x) if act == "tanh" else np.maximum(x, 0.0)


def forward64(net, params, x):
    """-> (the hidden activations h_0 .. h_(L-2), the pre-activations), float64"""
    hs, pre, h = [], [], x.astype(F64)
    for l in range(len(net.hidden)):
        W, b = params[l]
        z = h @ W.astype(F64) + b.astype(F64)
        h = act64(z, net.act)
        pre.append(z)
        hs.append(h)
    return hs, pre


def make_inputs(c):
    """The case's fixed weights (float32, W_l as [in_l, out_l], b_l; a module without bias has zero biases) and per-agent rows.  The
    rows of a ReLU agent are redrawn until no pre-activation of the float64 reference lies within BAND of 0."""
    rng = np.random.RandomState(c.seed)
    params = []
    for net in c.nets:
        w, p = widths(net), []
        for l in range(len(w) - 1):
            k = 1.0 / np.sqrt(w[l])
            W = rng.uniform(-k, k, (w[l], w[l + 1])).astype(F32)
            b = rng.uniform(-k, k, w[l + 1]).astype(F32)
            if c.bias_scale is not None:
                b = (c.bias_scale * np.sign(b + (b == 0))).astype(F32)
            if not net.bias:
                b[:] = 0
            p.append((W, b))
        params.append(p)
    xs, ds, redrawn = [], [], 0
    for m in c.agents:
        net = c.nets[m]
        x = rng.standard_normal((c.M, net.D)).astype(F32)
        if net.act == "relu":
            for _ in range(200):
                _, pre = forward64(net, params[m], x)
                bad = np.zeros(c.M, bool)
                for z in pre:
                    bad |= (np.abs(z) < BAND).any(axis=1)
                if not bad.any():
                    break
                redrawn += int(bad.sum())
                x[bad] = rng.standard_normal((int(bad.sum()), net.D)).astype(F32)
            else:
                raise AssertionError("%s: the band condition was not reached" % c.name)
        xs.append(x)
        ds.append((rng.standard_normal((c.M, net.n_out)) / max(c.M, 1)).astype(F32))
    return {"params": params, "in": xs, "dout": ds, "redrawn": redrawn}


def agent_grads64(net, params, x, dout):
    """THE MLP GRADIENT RULE for one agent in float64 -> [(dW_l [in_l, out_l], db_l [out_l])]"""
    hs, _ = forward64(net, params, x)
    L = len(net.hidden) + 1
    delta, out = dout.astype(F64), [None] * L
    for l in range(L - 1, -1, -1):
        h_prev = x.astype(F64) if l == 0 else hs[l - 1]
        out[l] = (h_prev.T @ delta, delta.sum(axis=0))
        if l > 0:
            back = delta @ params[l][0].astype(F64).T
            delta = back * (1.0 - h_prev * h_prev) if net.act == "tanh" else np.where(h_prev > 0, back, 0.0)
    return out


def agent_deltas64(net, params, x, dout):
    """-> [delta_l [M, out_l]] in float64: the rows that db_l is the column sum of (agent_grads64's own chain)"""
    hs, _ = forward64(net, params, x)
    L = len(net.hidden) + 1
    delta, out = dout.astype(F64), [None] * L
    for l in range(L - 1, -1, -1):
        out[l] = delta
        if l > 0:
            back = delta @ params[l][0].astype(F64).T
            delta = back * (1.0 - hs[l - 1] * hs[l - 1]) if net.act == "tanh" else np.where(hs[l - 1] > 0, back, 0.0)
    return out


def rule64(c, x):
    """-> per distinct module [(dW_l, db_l)]: the sharing agents' gradients added in ascending agent order"""
    total = [None] * len(c.nets)
    for i, m in enumerate(c.agents):
        g = agent_grads64(c.nets[m], x["params"][m], x["in"][i], x["dout"][i])
        total[m] = g if total[m] is None else [(a + dW, b + db) for (a, b), (dW, db) in zip(total[m], g)]
    return total


def torch_modules(c, x, dtype, device="cpu"):
    import torch
    import torch.nn as nn
    mods = []
    for net, p in zip(c.nets, x["params"]):
        layers = []
        for l, (W, b) in enumerate(p):
            lin = nn.Linear(W.shape[0], W.shape[1], bias=net.bias)
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(W.T.copy()))
                if net.bias:
                    lin.bias.copy_(torch.from_numpy(b))
            layers.append(lin)
            if l + 1 < len(p):
                layers.append(nn.Tanh() if net.act == "tanh" else nn.ReLU())
        mods.append(nn.Sequential(*layers).to(dtype).to(device))
    return mods


def torch_grads(c, x, dtype, device="cpu"):
    """torch autograd on the same inputs -> rule64's structure (a module without bias: db is None), float64 arrays"""
    import torch
    mods = torch_modules(c, x, dtype, device)
    for i, m in enumerate(c.agents):
        out = mods[m](torch.from_numpy(x["in"][i]).to(dtype).to(device))
        out.backward(torch.from_numpy(x["dout"][i]).to(dtype).to(device))
    res = []
    for mod in mods:
        lins = [k for k in mod if hasattr(k, "weight")]
        res.append([(lin.weight.grad.t().double().cpu().numpy(), None if lin.bias is None else lin.bias.grad.double().cpu().numpy())
                    for lin in lins])
    return res


def deviations(c, got, ref):
    """{(module, layer, 'W' | 'b'): (max |got - ref|, max |ref|)}; a block `got` does not have (db of a module without bias) is left out"""
    d = {}
    for m, (gm, rm) in enumerate(zip(got, ref)):
        if m not in c.agents:
            continue
        for l, ((gW, gb), (rW, rb)) in enumerate(zip(gm, rm)):
            d[(m, l, "W")] = (float(np.abs(gW - rW).max()), float(np.abs(rW).max()))
            if gb is not None and c.nets[m].bias:
                d[(m, l, "b")] = (float(np.abs(gb - rb).max()), float(np.abs(rb).max()))
    return d


def bounds(dev_torch):
    """The kernel's deviation may be at most 4 x that of float32 torch autograd, with a floor of 2 float32 ulps of the block's largest
    magnitude (the project's bar for the loss head, tests/_ppo_loss_ref.py::bounds)."""
    return {k: max(4.0 * dev, 2.0 * float(np.spacing(F32(mag)))) for k, (dev, mag) in dev_torch.items()}


# ---- the packed layout ------------------------------------------------------------------------------------------------------------
def pack(c, x):
    """-> the float32 packed weights of the case's modules, one block per module at offsets(c)"""
    off, total = offsets(c)
    w = np.zeros(total, F32)
    for net, p, o in zip(c.nets, x["params"], off):
        L = len(p)
        for l, (W, b) in enumerate(p):
            n_in, wide = (net.D if l == 0 else HW), (LW if l == L - 1 else HW)
            blk = np.zeros((n_in + 1, wide), F32)
            blk[:W.shape[0], :W.shape[1]] = W
            blk[n_in, :b.shape[0]] = b
            w[o:o + blk.size] = blk.reshape(-1)
            o += blk.size
    return w


def unpack(c, flat):
    """the packed gradient -> (rule64's structure as float64, the padding entries as one array)"""
    off, _ = offsets(c)
    res, pad = [], []
    for net, o in zip(c.nets, off):
        w, L, layers = widths(net), len(net.hidden) + 1, []
        for l in range(L):
            n_in, wide = (net.D if l == 0 else HW), (LW if l == L - 1 else HW)
            blk = np.asarray(flat[o:o + (n_in + 1) * wide]).reshape(n_in + 1, wide)
            live = np.zeros(blk.shape, bool)
            live[:w[l], :w[l + 1]] = True
            live[n_in, :w[l + 1]] = True
            pad.append(blk[~live])
            layers.append((blk[:w[l], :w[l + 1]].astype(F64), blk[n_in, :w[l + 1]].astype(F64)))
            o += blk.size
        res.append(layers)
    return res, np.concatenate(pad)


def fill_set(aset, c, weights_ptr, mode):
    """an _abi.MpeActorSet of the case (heads as mpe_actor_act wants them where the outputs allow: not read by mpe_mlp_grad)"""
    off, _ = offsets(c)
    aset.n_agents, aset.mode, aset.seed, aset.dim_c = len(c.agents), mode, 0, 0
    aset.weights = weights_ptr
    for i, m in enumerate(c.agents):
        net, w = c.nets[m], widths(c.nets[m])
        aset.n_layers[i] = len(w) - 1
        for l, v in enumerate(w):
            aset.width[i][l] = v
        aset.activation[i] = 1 if net.act == "tanh" else 0
        aset.offset[i] = off[m]
        aset.movable[i], aset.speaks[i] = 1, 0
    return aset


# ---- tests/c/mlp_grad_host_walk.cpp: its input and output files ----------------------------------------------------------------------
def write_walk_input(path, c, x):
    off, total = offsets(c)
    with open(path, "wb") as f:
        np.array([len(c.agents)], np.int32).tofile(f)
        np.array([c.M], np.int64).tofile(f)
        for m in c.agents:
            net, w = c.nets[m], widths(c.nets[m])
            np.array([len(w) - 1, 1 if net.act == "tanh" else 0] + (w + [0, 0, 0])[:4] + [off[m]], np.int32).tofile(f)
        np.array([total], np.int32).tofile(f)
        pack(c, x).tofile(f)
        for i in range(len(c.agents)):
            x["in"][i].tofile(f)
            x["dout"][i].tofile(f)


def read_walk_output(path, c):
    return np.fromfile(path, F32)
