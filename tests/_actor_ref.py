"""Helpers of tests/test_actor_ref_cpu.py and tests/test_gpu_actor_edges.py (no tests in here): the actor kernel's contract restated
in NumPy fp64 from include/mpe_hip.h (MpeActorSet, mpe_actor_act and the head rule of mpe_rollout_policy's comment), a plain fp32
comparator, the packed layout, a caller of the C entry point on hand-built sets, and the case table both files walk.

An actor here is `layers`: a list of (W [out, in] float32, b [out] float32), torch.nn.Linear's orientation.

Bars (the project's, tests/test_gpu_policy.py and tests/test_gpu_actor.py): logits and softmax rows within 1e-5 * max(1, max|z|);
chosen indices exact wherever the fp64 reference is outside the band -- greedy: top-two margin > 1e-5 * max(1, max|z|), sample:
|cum_j - u| > 1e-5 for every j; rows inside the band are counted, at most 0.1 % of the rows checked (+ 1).  logp: per head three
times the logit bar (two logit differences and a 1-Lipschitz log-sum-exp) and 2e-6 once for the exp / log intrinsics."""
import ctypes as C

import numpy as np

from oracle import philox

MODES = {"greedy": 0, "sample": 1, "softmax": 2}          # MPE_POLICY_GREEDY / SAMPLE / SOFTMAX
RELU, TANH = 0, 1                                         # MPE_POLICY_RELU / TANH
STREAM_POLICY, STREAM_POLICY_COMM = 0x504F4C49, 0x504F4C43
HIDDEN_PAD, LAST_PAD, MOVE = 64, 16, 5                    # MPE_POLICY_MAX_WIDTH, MPE_ACTOR_MAX_OUT, MPE_ACTION_DIM
BAND, CAP = 1e-5, 1e-3
# canary rows behind every output buffer.  256 = the worlds of one workgroup: a dead wave of the last tile that stored anyway
# would still land in checked memory (the first 64 of them are what a single wave could reach).
CANARY_ROWS = 256
CANARY_F, CANARY_I = -777.25, -777


# ---- the references ---------------------------------------------------------------------------------------------------------
def _forward(layers, act, x, dtype):
    for k, (W, b) in enumerate(layers):
        W, b = W.astype(dtype), b.astype(dtype)
        if dtype == np.float64:
            x = x @ W.T + b
        else:      # fp32: the accumulator starts at the bias, k ascending, one rounded multiply and one rounded add per term
            acc = np.broadcast_to(b, (x.shape[0], W.shape[0])).copy()
            for c in range(W.shape[1]):
                acc += x[:, c:c + 1] * W[None, :, c]
            x = acc
        if k + 1 < len(layers):
            x = np.maximum(x, 0) if act == RELU else np.tanh(x)
    return x


def split_heads(z, movable, speaks, dim_c):
    """the first 5 logits are the move head, the last dim_c the utterance head -> [move or None, utterance or None]"""
    return [z[:, :MOVE] if movable else None, z[:, z.shape[1] - dim_c:] if speaks else None]


def draw_u(stream, seed, B, t, agent, world_offset):
    """the 24-bit uniform of (world_offset + b, step t, agent) on `stream`: key = seed, counter = (world lo, world hi ^ step hi,
    agent >> 2, stream ^ step lo), word agent & 3; u = (bits >> 8) * 2^-24.  -> fp64 [B]"""
    b = np.arange(B, dtype=np.uint64) + np.uint64(world_offset)
    o = philox.philox4x32_10(b & philox.MASK, ((b >> np.uint64(32)) ^ np.uint64(t >> 32)) & philox.MASK,
                             np.full(B, agent >> 2, np.uint64), np.full(B, (stream ^ (t & 0xFFFFFFFF)) & 0xFFFFFFFF, np.uint64),
                             seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return (o[agent & 3] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def _log_softmax(z):
    s = z - z.max(axis=1, keepdims=True)
    return s - np.log(np.exp(s).sum(axis=1, keepdims=True))


def ref_decide(layers, act, movable, speaks, dim_c, obs, mode, seed, t, agent, world_offset):
    """fp64.  -> dict: z [B, n_out]; scale [B] = max(1, max|z|); heads = [move, utterance], each None or a dict of
    z, p (softmax rows), logsm, scale, greedy, sample (int64 [B]; sample only in SAMPLE mode), chosen (mode's choice: argmax in
    SOFTMAX mode), ok (bool [B]: the row is outside the band under mode's rule); logp [B] at `chosen`."""
    x = np.asarray(obs, np.float64)
    B = x.shape[0]
    z = _forward(layers, act, x, np.float64)
    assert z.shape[1] == MOVE * bool(movable) + dim_c * bool(speaks)
    out = {"z": z, "scale": np.maximum(1.0, np.abs(z).max(axis=1)), "heads": [], "logp": np.zeros(B)}
    for h, zh in enumerate(split_heads(z, movable, speaks, dim_c)):
        if zh is None:
            out["heads"].append(None)
            continue
        n = zh.shape[1]
        logsm = _log_softmax(zh)
        p = np.exp(logsm)
        hs = np.maximum(1.0, np.abs(zh).max(axis=1))
        greedy = zh.argmax(axis=1)      # (np.argmax: the first of equal maxima)
        if n > 1:
            top = np.sort(zh, axis=1)
            ok = (top[:, -1] - top[:, -2]) > BAND * hs
        else:
            ok = np.ones(B, bool)
        d = {"z": zh, "p": p, "logsm": logsm, "scale": hs, "greedy": greedy, "chosen": greedy, "ok": ok}
        if mode == "sample":
            u = draw_u(STREAM_POLICY_COMM if h else STREAM_POLICY, seed, B, t, agent, world_offset)
            cum = np.cumsum(p, axis=1)[:, :n - 1]
            d["u"] = u
            d["sample"] = d["chosen"] = np.minimum((cum <= u[:, None]).sum(axis=1), n - 1)
            d["ok"] = (np.abs(cum - u[:, None]) > BAND).all(axis=1)
        out["logp"] += np.take_along_axis(logsm, d["chosen"][:, None], 1)[:, 0]
        out["heads"].append(d)
    return out


def ref_f32(layers, act, movable, speaks, dim_c, obs, chosen=None):
    """The same pass in plain float32 (what fp32 alone costs on a case: not an oracle).  chosen: per head the indices logp is taken
    at (ref_decide's).  -> dict: z, heads = [None or dict(p)], logp (when chosen is given)."""
    z = _forward(layers, act, np.asarray(obs, np.float32), np.float32)
    out = {"z": z, "heads": [], "logp": np.zeros(z.shape[0], np.float32)}
    for h, zh in enumerate(split_heads(z, movable, speaks, dim_c)):
        if zh is None:
            out["heads"].append(None)
            continue
        zm = zh.max(axis=1, keepdims=True)
        e = np.exp(zh - zm)
        s = np.zeros(zh.shape[0], np.float32)
        for j in range(zh.shape[1]):
            s += e[:, j]
        out["heads"].append({"p": e / s[:, None]})
        if chosen is not None:
            out["logp"] += (np.take_along_axis(zh, chosen[h][:, None], 1)[:, 0] - zm[:, 0]) - np.log(s)
    return out


def logp_bar(ref):
    """three logit bars per head the agent has, and 2e-6"""
    return sum(3 * BAND * d["scale"] for d in ref["heads"] if d is not None) + 2e-6


# ---- the packed layout --------------------------------------------------------------------------------------------------------
def pack(layers):
    """include/mpe_hip.h, MpeActorSet: per layer W as [in'][out'] row-major (W[k][j] = weight[j][k]) then bias[out']; in' = the input
    width for the first layer and 64 behind it, out' = 64 for a hidden layer and 16 for the last; padding is zero."""
    parts = []
    for k, (W, b) in enumerate(layers):
        n_in = W.shape[1] if k == 0 else HIDDEN_PAD
        wide = LAST_PAD if k + 1 == len(layers) else HIDDEN_PAD
        w = np.zeros((n_in, wide), np.float32)
        w[:W.shape[1], :W.shape[0]] = W.T
        bb = np.zeros(wide, np.float32)
        bb[:b.shape[0]] = b
        parts += [w.ravel(), bb]
    return np.concatenate(parts)


def as_module(layers, act, dtype=None):
    """the same actor as a torch.nn.Sequential (float32, or `dtype`)"""
    import torch
    mods = []
    for k, (W, b) in enumerate(layers):
        lin = torch.nn.Linear(W.shape[1], W.shape[0])
        with torch.no_grad():
            lin.weight.copy_(torch.as_tensor(W))
            lin.bias.copy_(torch.as_tensor(b))
        mods.append(lin)
        if k + 1 < len(layers):
            mods.append(torch.nn.ReLU() if act == RELU else torch.nn.Tanh())
    m = torch.nn.Sequential(*mods)
    return m if dtype is None else m.to(dtype)


# ---- the C entry point on a hand-built set ------------------------------------------------------------------------------------------
def make_set(agents, dim_c, mode, seed, offsets=None):
    """-> (MpeActorSet without its weights pointer, the packed float32 blob).  agents: dicts of layers, act, movable, speaks."""
    from multiagent_particle_envs_amd import _abi
    aset = _abi.MpeActorSet()
    aset.n_agents, aset.mode, aset.seed, aset.dim_c = len(agents), MODES[mode], seed, dim_c
    blobs, off = [], 0
    for i, a in enumerate(agents):
        blob = pack(a["layers"])
        assert blob.size % 16 == 0
        aset.offset[i] = off if offsets is None else offsets[i]
        aset.n_layers[i] = len(a["layers"])
        aset.width[i][0] = a["layers"][0][0].shape[1]
        for k, (W, _) in enumerate(a["layers"]):
            aset.width[i][k + 1] = W.shape[0]
        aset.activation[i] = a["act"]
        aset.movable[i], aset.speaks[i] = int(a["movable"]), int(a["speaks"])
        blobs.append(blob)
        off += blob.size
    return aset, np.concatenate(blobs)


def run_abi(agents, dim_c, obs, mode, seed, t, world_offset, B=None, offsets=None, misalign=None, want=("utter", "ids", "logp", "logits")):
    """One mpe_actor_act call on torch device tensors.  obs: one float32 [B, D_i] array per agent.  Every output buffer has
    CANARY_ROWS rows of a canary value behind it, and is filled with that value in front of the call too.  misalign: 'weights' /
    'logits' hands that pointer over 4 bytes off.  -> dict: rc, error, moves [A,B,5], utter [A,B,dim_c] or None, ids [2,A,B],
    logp [A,B], logits [A,B,16] (NumPy), canary_ok, untouched (no output element was written at all)."""
    import torch
    from multiagent_particle_envs_amd import _abi
    dev = torch.device("cuda", torch.cuda.current_device())
    A = len(agents)
    B = int(obs[0].shape[0]) if B is None else B
    aset, blob = make_set(agents, dim_c, mode, seed, offsets)
    wts = torch.zeros(blob.size + 4, dtype=torch.float32, device=dev)
    shift = 1 if misalign == "weights" else 0
    wts[shift:shift + blob.size] = torch.as_tensor(blob, device=dev)
    aset.weights = wts.data_ptr() + 4 * shift
    # (zeros behind each block: a read a pass of columns past the last row would stay inside the allocation)
    obs_t = [torch.cat([torch.as_tensor(np.ascontiguousarray(o, np.float32)).reshape(-1), torch.zeros(64)]).to(dev) for o in obs]
    ptrs = (C.c_void_p * A)(*[o.data_ptr() for o in obs_t])
    rows = A * B

    def buf(per_row, copies=1, dtype=torch.float32, fill=CANARY_F):
        return torch.full(((copies * rows + CANARY_ROWS) * per_row + 4,), fill, dtype=dtype, device=dev) if per_row else None
    bufs = {"moves": buf(MOVE), "utter": buf(dim_c) if "utter" in want else None,
            "ids": buf(1, 2, torch.int32, CANARY_I) if "ids" in want else None, "logp": buf(1) if "logp" in want else None,
            "logits": buf(LAST_PAD) if "logits" in want else None}

    def ptr(name):
        if bufs[name] is None:
            return None
        return bufs[name].data_ptr() + (4 if misalign == name else 0)
    rc = _abi.lib().mpe_actor_act(C.byref(aset), ptrs, B, int(t), int(world_offset), ptr("moves"), ptr("utter"), ptr("ids"),
                                  ptr("logp"), ptr("logits"), _abi.raw_stream(dev))
    err = _abi.lib().mpe_last_error().decode("utf-8", "replace") if rc else ""
    torch.cuda.synchronize()
    out = {"rc": rc, "error": err, "canary_ok": True, "untouched": True}
    shapes = {"moves": (A, B, MOVE), "utter": (A, B, dim_c), "ids": (2, A, B), "logp": (A, B), "logits": (A, B, LAST_PAD)}
    for name, b in bufs.items():
        if b is None:
            out[name] = None
            continue
        host = b.cpu().numpy()
        live = int(np.prod(shapes[name]))
        can = CANARY_I if name == "ids" else CANARY_F
        out["canary_ok"] = out["canary_ok"] and bool((host[live:] == can).all())
        out["untouched"] = out["untouched"] and bool((host == can).all())
        out[name] = host[:live].reshape(shapes[name]).copy()
    del wts, obs_t
    return out


# ---- comparing a run with the reference ---------------------------------------------------------------------------------------
class Tally(object):
    """what a sweep reports: rows checked, rows inside the band, worst margins (error / bar), canaries"""

    def __init__(self):
        self.checked = self.inband = 0
        self.worst = {"logits": 0.0, "softmax": 0.0, "logp": 0.0}
        self.canary_ok = True

    def margin(self, what, err, bar):
        m = float(np.max(np.asarray(err, np.float64) / bar)) if np.size(err) else 0.0
        self.worst[what] = max(self.worst[what], m)
        return m

    def report(self):
        return {"rows_checked": self.checked, "rows_in_band": self.inband, "canary_rows_intact": self.canary_ok,
                "worst_error_over_bar": dict(self.worst)}


def check_agent(out, i, ref, mode, tally, tag=""):
    """agent i's rows of a run_abi result against ref_decide's dict: asserts the bars, counts the rows left out."""
    B = ref["z"].shape[0]
    n_out = ref["z"].shape[1]
    if out["logits"] is not None:
        got = out["logits"][i].astype(np.float64)
        assert not np.isnan(got).any(), (tag, i, "NaN logits")
        m = tally.margin("logits", np.abs(got[:, :n_out] - ref["z"]).max(axis=1), BAND * ref["scale"])
        print("%s agent %d logits: worst error / bar %.3f" % (tag, i, m))
        assert m < 1.0, (tag, i, "logits", m)
        assert (got[:, n_out:] == 0).all(), (tag, i, "logits beyond n_out")
    lp = np.zeros(B)
    for h, d in enumerate(ref["heads"]):
        rows = out["utter"] if h else out["moves"]
        if d is None:
            if rows is not None:
                assert (rows[i] == 0).all(), (tag, i, h, "a head the agent does not have")
            if out["ids"] is not None:
                assert (out["ids"][h, i] == -1).all(), (tag, i, h)
            continue
        a, n = rows[i].astype(np.float64), d["z"].shape[1]
        assert not np.isnan(a).any(), (tag, i, h, "NaN rows")
        ids = out["ids"][h, i].astype(np.int64) if out["ids"] is not None else None
        if mode == "softmax":
            m = tally.margin("softmax", np.abs(a - d["p"]).max(axis=1), BAND * d["scale"])
            print("%s agent %d head %d softmax: worst error / bar %.3f" % (tag, i, h, m))
            assert m < 1.0, (tag, i, h, "softmax", m)
            assert (np.abs(a.sum(axis=1) - 1) < BAND * d["scale"]).all(), (tag, i, h, "rows do not sum to 1")
            idx = ids if ids is not None else d["greedy"]
        else:
            idx = a.argmax(axis=1)
            assert (a.sum(axis=1) == 1).all() and (a.max(axis=1) == 1).all() and ((a == 0) | (a == 1)).all(), (tag, i, h, "one-hot")
            if ids is not None:
                assert np.array_equal(ids, idx), (tag, i, h, "ids")
        bad = d["ok"] & (idx != d["chosen"])
        assert not bad.any(), (tag, i, h, mode, "rows", np.nonzero(bad)[0][:8], idx[bad][:8], d["chosen"][bad][:8])
        tally.checked += B
        tally.inband += int((~d["ok"]).sum())
        assert ((idx >= 0) & (idx < n)).all(), (tag, i, h, "index out of range")
        lp += np.take_along_axis(d["logsm"], idx[:, None], 1)[:, 0]
    if out["logp"] is not None:
        got = out["logp"][i].astype(np.float64)
        assert np.isfinite(got).all(), (tag, i, "logp not finite")
        m = tally.margin("logp", np.abs(got - lp), logp_bar(ref))
        print("%s agent %d logp: worst error / bar %.3f" % (tag, i, m))
        assert m < 1.0, (tag, i, "logp", m)


# ---- the case table -----------------------------------------------------------------------------------------------------------
def make_layers(rs, D, hidden, n_out, wscale=1.0):
    """torch.nn.Linear's default init (uniform in +-1/sqrt(fan_in)) times wscale, float32"""
    sizes = [D] + list(hidden) + [n_out]
    layers = []
    for k in range(len(sizes) - 1):
        r = wscale / np.sqrt(sizes[k])
        layers.append((rs.uniform(-r, r, (sizes[k + 1], sizes[k])).astype(np.float32), rs.uniform(-r, r, sizes[k + 1]).astype(np.float32)))
    return layers


def agent_spec(D, hidden=(64, 64), act=RELU, movable=1, speaks=0):
    return {"D": D, "hidden": tuple(hidden), "act": act, "movable": movable, "speaks": speaks}


def case(name, sweep, specs, dim_c=0, B=333, seed=0, t=3, world_offset=777, zmax=None):
    return {"name": name, "sweep": sweep, "specs": specs, "dim_c": dim_c, "B": B, "seed": seed, "t": t, "world_offset": world_offset,
            "zmax": zmax, "draw_seed": 9}


def build_case(c):
    """-> (agents: dicts with layers / act / movable / speaks, obs: float32 [B, D_i] per agent); deterministic in the case's seed.
    zmax: the last layer is scaled so that the largest |logit| of the case's rows is zmax."""
    rs = np.random.RandomState(1000 + c["seed"])
    agents, obs = [], []
    for s in c["specs"]:
        n_out = MOVE * s["movable"] + c["dim_c"] * s["speaks"]
        layers = make_layers(rs, s["D"], s["hidden"], n_out)
        x = rs.uniform(-1, 1, (c["B"], s["D"])).astype(np.float32)
        if c["zmax"] is not None:
            z = _forward(layers, s["act"], x.astype(np.float64), np.float64)
            f = c["zmax"] / np.abs(z).max()
            layers[-1] = ((layers[-1][0] * f).astype(np.float32), (layers[-1][1] * f).astype(np.float32))
        agents.append({"layers": layers, "act": s["act"], "movable": s["movable"], "speaks": s["speaks"]})
        obs.append(x)
    return agents, obs


INPUT_WIDTHS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 128, 255, 256)
HIDDEN_WIDTHS = ((1,), (31,), (32,), (33,), (63,), (64, 20), (20, 64), (33, 32), (1, 1))
HEAD_KINDS = ((1, 1, 11), (1, 1, 1), (0, 1, 16), (0, 1, 1), (1, 0, 0))      # (movable, speaks, dim_c)
BATCHES = (1, 5, 63, 64, 65, 256, 257, 4097)
BIG_OFFSET, BIG_STEP = 123456789012, (5 << 32) + 11


def _mixed_set(dim_c, kinds):
    """16 agents that alternate kinds, every agent with an input width of its own"""
    widths = (18, 1, 33, 64, 7, 96, 2, 31, 65, 32, 10, 3, 255, 21, 63, 14)
    hid = ((64, 64), (), (20,), (64,), (33, 32), (64, 20), (1,), (32,))
    return [agent_spec(widths[i], hid[i % len(hid)], (RELU, TANH)[(i // 2) % 2], *kinds[i % len(kinds)]) for i in range(16)]


def _cases():
    out = []
    for D in INPUT_WIDTHS:
        out.append(case("width_D%d_64x64" % D, "input_width", [agent_spec(D, (64, 64), RELU)]))
        out.append(case("width_D%d_1layer" % D, "input_width", [agent_spec(D, (), RELU)]))
    for hid in HIDDEN_WIDTHS:
        for act in (RELU, TANH):
            out.append(case("hidden_%s_%s" % ("x".join(map(str, hid)), ("relu", "tanh")[act]), "hidden_width", [agent_spec(18, hid, act)]))
    for mv, sp, dc in HEAD_KINDS:
        out.append(case("head_m%d_s%d_c%d" % (mv, sp, dc), "heads", [agent_spec(21, (64, 64), RELU, mv, sp)], dim_c=dc))
    # one set has ONE dim_c, so the five kinds cannot all sit in one set: three 16-agent sets, each with every kind its dim_c admits
    # (5 * movable + dim_c * speaks <= 16), B = 257: a workgroup with one live world, every agent's rows behind another's
    out.append(case("heads_mixed16_c11", "heads", _mixed_set(11, ((1, 1), (0, 1), (1, 0))), dim_c=11, B=257))
    out.append(case("heads_mixed16_c1", "heads", _mixed_set(1, ((1, 1), (0, 1), (1, 0))), dim_c=1, B=257))
    out.append(case("heads_mixed16_c16", "heads", _mixed_set(16, ((0, 1), (1, 0))), dim_c=16, B=257))
    two = [agent_spec(18, (64, 64), RELU, 1, 1), agent_spec(10, (20,), TANH, 1, 0)]
    for B in BATCHES:
        out.append(case("batch_B%d" % B, "batch", two, dim_c=3, B=B))
    out.append(case("batch_B257_big_offset", "batch", two, dim_c=3, B=257, t=BIG_STEP, world_offset=BIG_OFFSET))
    for zmax in (30.0, 80.0):
        out.append(case("large_logits_%d" % zmax, "large_logits", [agent_spec(18, (64, 64), RELU, 1, 1)], dim_c=11, B=1024, zmax=zmax))
    return out


# seeds moved off a case's default (0) because, on the CPU, the fp64 reference itself put more than half the cap's share of that
# case's rows inside the band (tests/test_actor_ref_cpu.py: the cap condition); nothing else about the case changes
SEEDS = {"width_D255_64x64": 1}      # (seed 0: 1 of its 333 greedy rows inside the band)
CASES = _cases()
for _c in CASES:
    _c["seed"] = SEEDS.get(_c["name"], 0)
CASE_NAMES = [c["name"] for c in CASES]


def case_refs(c, mode, agents=None, obs=None):
    """ref_decide of every agent of a case"""
    if agents is None:
        agents, obs = build_case(c)
    return [ref_decide(a["layers"], a["act"], a["movable"], a["speaks"], c["dim_c"], obs[i], mode, c["draw_seed"], c["t"], i,
                       c["world_offset"]) for i, a in enumerate(agents)]
