"""Helpers of tests/test_td_target_cpu.py and tests/test_gpu_td_target.py (no tests in here): the two rules of include/mpe_hip.h's
TD-target section restated in NumPy -- the joint row of mpe_actor_act_rows and y of mpe_critic_q --, a critic pass in fp64 and in
plain fp32, the case tables both files walk, and callers of the two C entry points on hand-built sets with canaries behind every
output.  Actors, draws and bars are those of tests/_actor_ref.py."""
import ctypes as C

import numpy as np

import _actor_ref as R

F32 = np.float32
JOINT_TAIL = 3      # the joint buffer's stride is the joint width + 3: columns nobody may write


# ---- the case tables --------------------------------------------------------------------------------------------------------
def _cases():
    A, RELU, TANH = R.agent_spec, R.RELU, R.TANH
    tag = [A(16), A(16), A(16), A(14, (64,), TANH)]
    return [
        R.case("spread_M1", "rows", [A(18), A(18), A(18)], B=1, world_offset=0),
        R.case("spread_M63", "rows", [A(18), A(18), A(18)], B=63, world_offset=0),
        R.case("speaker_listener_M65", "rows", [A(3, movable=0, speaks=1), A(11, movable=1, speaks=0)], dim_c=3, B=65, world_offset=0),
        R.case("both_heads_M257_off5", "rows", [A(33, (33, 32), TANH, 1, 1), A(2, (), RELU, 1, 1)], dim_c=4, B=257, world_offset=5),
        R.case("tag_M300", "rows", tag, B=300, world_offset=0),
        # joint width 255 + 64 + (5 + 11) + 11 = 346: wider than a critic's input may be, which mpe_actor_act_rows does not mind
        R.case("wide_joint346_M130", "rows", [A(255, movable=1, speaks=1), A(64, movable=0, speaks=1)], dim_c=11, B=130, world_offset=0),
    ]


CASES = _cases()      # (all with seed 0; B is M and world_offset is row_offset)
CASE_NAMES = [c["name"] for c in CASES]
# (joint width, hidden widths, M) of the critic checks
CRITIC_SHAPES = [(1, (64, 64), 1), (33, (33,), 64), (69, (64, 64), 65), (256, (64, 64), 300), (82, (), 257)]
CRITIC_IDS = ["W%d_%s_M%d" % (w, "x".join(map(str, h)) or "1layer", m) for w, h, m in CRITIC_SHAPES]
Q_BAR = 1e-5      # |q - q64| <= Q_BAR * max(1, |q64|)


# ---- the joint-row rule -----------------------------------------------------------------------------------------------------
def joint_layout(widths, movable, speaks, dim_c):
    """-> (off [A + 1], joint width, col_move [A], col_utter [A]): every observation in agent order, then per agent its move row
    [5] if movable, directly followed by its utterance row [dim_c] if it speaks (None: the agent has no such columns)"""
    off = [0]
    for d in widths:
        off.append(off[-1] + d)
    col, cm, cu = off[-1], [], []
    for m, s in zip(movable, speaks):
        cm.append(col if m else None)
        col += R.MOVE if m else 0
        cu.append(col if s else None)
        col += dim_c if s else 0
    return off, col, cm, cu


def case_layout(c):
    return joint_layout([s["D"] for s in c["specs"]], [s["movable"] for s in c["specs"]], [s["speaks"] for s in c["specs"]], c["dim_c"])


def joint_rows(obs, moves, utter, movable, speaks, dim_c):
    """The joint rows [M, joint width] of obs (per agent [M, D_i]), moves [A, M, 5] and utter [A, M, dim_c] (or None): written
    column block by column block at the layout's offsets, every column exactly once (asserted)."""
    off, width, cm, cu = joint_layout([o.shape[1] for o in obs], movable, speaks, dim_c)
    M = obs[0].shape[0]
    out = np.zeros((M, width), F32)
    seen = np.zeros(width, np.int64)
    for i, o in enumerate(obs):
        out[:, off[i]:off[i + 1]] = o
        seen[off[i]:off[i + 1]] += 1
        if cm[i] is not None:
            out[:, cm[i]:cm[i] + R.MOVE] = moves[i]
            seen[cm[i]:cm[i] + R.MOVE] += 1
        if cu[i] is not None:
            out[:, cu[i]:cu[i] + dim_c] = utter[i]
            seen[cu[i]:cu[i] + dim_c] += 1
    assert (seen == 1).all()
    return out


# ---- the TD-target rule -----------------------------------------------------------------------------------------------------
def y_rule(ret, done, q, discount=None, gamma=None):
    """y[i][m] = done[i][m] ? ret[i][m] : ret[i][m] + d_m * q[i][m], d_m = discount ? discount[m] : gamma: float32, the product
    rounded, then the sum rounded; a select, so a done row is ret whatever q is.  ret, q [A, M]; done [A, M]; discount [M]."""
    ret, q = np.asarray(ret, F32), np.asarray(q, F32)
    d = np.broadcast_to(F32(gamma), q.shape) if discount is None else np.broadcast_to(np.asarray(discount, F32)[None, :], q.shape)
    with np.errstate(all="ignore"):
        dq = np.multiply(d, q, dtype=F32)
        s = np.add(ret, dq, dtype=F32)
    return np.where(np.asarray(done) != 0, ret, s).astype(F32)


def same_floats(a, b):
    """bit-equal float32 arrays, a NaN standing for any NaN"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | nan).all())


# ---- critics ----------------------------------------------------------------------------------------------------------------
def build_critics(shape, A=3, seed=0):
    """-> (critics: A lists of layers with a one-output last layer, rows: float32 [M, W]); deterministic"""
    W, hidden, M = shape
    rs = np.random.RandomState(2000 + seed)
    critics = [R.make_layers(rs, W, hidden, 1) for _ in range(A)]
    return critics, rs.uniform(-1, 1, (M, W)).astype(F32)


def critic_q(layers, rows, dtype, act=R.RELU):
    """one critic over the rows -> [M] in dtype (fp64: the reference; fp32: the plain k-ordered chain of _actor_ref._forward)"""
    return R._forward(layers, act, np.asarray(rows, dtype), dtype)[:, 0]


def make_critic_set(critics, act=R.RELU):
    """-> (MpeActorSet in mode MPE_POLICY_VALUE without its weights pointer, the packed blob)"""
    from multiagent_particle_envs_amd import _abi
    agents = [{"layers": l, "act": act, "movable": 0, "speaks": 0} for l in critics]
    aset, blob = R.make_set(agents, 0, "greedy", 0)
    aset.mode = _abi.MPE_POLICY_VALUE
    return aset, blob


# ---- the C entry points on hand-built sets ----------------------------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda", torch.cuda.current_device())


def _canaried(n_live, n_canary, dtype=None, fill=R.CANARY_F):
    import torch
    return torch.full((n_live + n_canary,), fill, dtype=dtype or torch.float32, device=_dev())


def run_rows_abi(agents, dim_c, obs, mode, seed, t, row_offset, joint=True, moves=True):
    """One mpe_actor_act_rows call.  Every output has R.CANARY_ROWS canary rows behind it and is canary-filled in front of the
    call; the joint buffer's stride is the joint width + JOINT_TAIL.  joint / moves False: that pointer (and utter with moves) is
    NULL.  -> dict: rc, error, moves, utter, ids, logp, logits (NumPy, None where not asked), joint [M, width + JOINT_TAIL]
    (tail columns included), width, canary_ok."""
    import torch
    from multiagent_particle_envs_amd import _abi
    dev = _dev()
    A, M = len(agents), int(obs[0].shape[0])
    aset, blob = R.make_set(agents, dim_c, mode, seed)
    wts = torch.as_tensor(blob, device=dev)
    aset.weights = wts.data_ptr()
    obs_t = [torch.as_tensor(np.ascontiguousarray(o, F32)).to(dev) for o in obs]
    ptrs = (C.c_void_p * A)(*[o.data_ptr() for o in obs_t])
    width = joint_layout([o.shape[1] for o in obs], [a["movable"] for a in agents], [a["speaks"] for a in agents], dim_c)[1]
    stride = width + JOINT_TAIL
    rows, can = A * M, R.CANARY_ROWS
    bufs = {"moves": _canaried(rows * R.MOVE, can * R.MOVE) if moves else None,
            "utter": _canaried(rows * dim_c, can * dim_c) if moves and dim_c else None,
            "ids": _canaried(2 * rows, can, torch.int32, R.CANARY_I), "logp": _canaried(rows, can),
            "logits": _canaried(rows * R.LAST_PAD, can * R.LAST_PAD),
            "joint": _canaried(M * stride, can * stride) if joint else None}

    def ptr(name):
        return bufs[name].data_ptr() if bufs[name] is not None else None
    rc = _abi.lib().mpe_actor_act_rows(C.byref(aset), ptrs, M, int(t), int(row_offset), ptr("moves"), ptr("utter"), ptr("ids"),
                                       ptr("logp"), ptr("logits"), ptr("joint"), stride if joint else 0, _abi.raw_stream(dev))
    err = _abi.lib().mpe_last_error().decode("utf-8", "replace") if rc else ""
    torch.cuda.synchronize()
    out = {"rc": rc, "error": err, "canary_ok": True, "width": width}
    shapes = {"moves": (A, M, R.MOVE), "utter": (A, M, dim_c), "ids": (2, A, M), "logp": (A, M), "logits": (A, M, R.LAST_PAD),
              "joint": (M, stride)}
    for name, b in bufs.items():
        if b is None:
            out[name] = None
            continue
        host = b.cpu().numpy()
        live = int(np.prod(shapes[name]))
        out["canary_ok"] = out["canary_ok"] and bool((host[live:] == (R.CANARY_I if name == "ids" else R.CANARY_F)).all())
        out[name] = host[:live].reshape(shapes[name]).copy()
    del wts, obs_t
    return out


def run_critic_abi(critics, rows, td=None, act=R.RELU):
    """One mpe_critic_q call, the same rows for every critic.  td: None or dict(ret [A, M], done [A, M] uint8, discount [M] or
    None, gamma).  -> dict: rc, error, q [A, M], y [A, M] or None, canary_ok (R.CANARY_ROWS canary floats behind q and y)."""
    import torch
    from multiagent_particle_envs_amd import _abi
    dev = _dev()
    A, M = len(critics), int(rows.shape[0])
    aset, blob = make_critic_set(critics, act)
    wts = torch.as_tensor(blob, device=dev)
    aset.weights = wts.data_ptr()
    x = torch.as_tensor(np.ascontiguousarray(rows, F32)).to(dev)
    ptrs = (C.c_void_p * A)(*([x.data_ptr()] * A))
    q = _canaried(A * M, R.CANARY_ROWS)
    y = _canaried(A * M, R.CANARY_ROWS) if td is not None else None
    keep, tdp = [], None
    if td is not None:
        s = _abi.MpeTdTarget()
        keep = [torch.as_tensor(np.ascontiguousarray(td["ret"], F32)).to(dev), torch.as_tensor(np.ascontiguousarray(td["done"], np.uint8)).to(dev)]
        s.ret, s.done = keep[0].data_ptr(), keep[1].data_ptr()
        if td.get("discount") is not None:
            keep.append(torch.as_tensor(np.ascontiguousarray(td["discount"], F32)).to(dev))
            s.discount = keep[2].data_ptr()
        else:
            s.discount, s.gamma = None, td["gamma"]
        tdp = C.byref(s)
    rc = _abi.lib().mpe_critic_q(C.byref(aset), ptrs, M, q.data_ptr(), tdp, y.data_ptr() if y is not None else None, _abi.raw_stream(dev))
    err = _abi.lib().mpe_last_error().decode("utf-8", "replace") if rc else ""
    torch.cuda.synchronize()
    out = {"rc": rc, "error": err, "canary_ok": True, "y": None}
    for name, b in (("q", q), ("y", y)):
        if b is not None:
            host = b.cpu().numpy()
            out["canary_ok"] = out["canary_ok"] and bool((host[A * M:] == R.CANARY_F).all())
            out[name] = host[:A * M].reshape(A, M).copy()
    del wts, x, keep
    return out
