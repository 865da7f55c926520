"""The no-grad half of an off-policy (MADDPG-style) update on the device: `Critics` evaluates one MLP critic per agent over M joint
rows in ONE launch (mpe_critic_q: the actor kernel's MFMA body with a one-output last layer and no head), and `TdTargets` turns a
sampled ReplayBatch into the TD target in TWO launches -- the target actors decide on batch.next_obs_n and write complete critic
input rows (Actors.act_rows, joint=True), the target critics read those rows and write Q' and y.  DESIGN.md 2.14; the two rules
(joint rows, y) are stated in include/mpe_hip.h.  The loss heads of the update are here too: `TdLoss` (the critics'
weighted squared TD error and its gradient, mpe_td_loss) and `ActorLoss` (the relaxed action rows, the critics on them, their input
gradient and the softmax Jacobian: mpe_policy_rows, mpe_critic_q, mpe_mlp_dinput, mpe_policy_rows_grad), both behind torch autograd
with a one-multiply backward; the networks' own backward passes are train.py's.  The value-based learners (independent Q-learning,
VDN) have `QTargets` (the target and, for double-Q, the online networks' logits of the next observations) and `QLoss`
(mpe_q_loss: from the logits to dL/dlogits in two launches).

    mu_t, q_t = Actors(env, target_actor_modules, mode="softmax"), Critics(env, target_critic_modules)
    td = TdTargets(mu_t, q_t)
    batch = buf.sample(1024, joint=True, n_step=3, gamma=0.95, episode_len=25)
    y = td.compute(batch)                       # [A, M]: ret + discount * (1 - done) * Q'(next_obs, mu'(next_obs))
"""
import ctypes as C
import math

import torch

from . import _abi
from .netset import Cache, Generations, NetSet, check_tensor
from .policy import Actors, env_joint_layout
from .replay import NStepReplayBatch, ReplayBatch


class Critics(NetSet):
    """Per-agent MLP critics over the centralised joint row: `modules` is one nn.Sequential per agent, or one module every agent
    shares (the layer rules of Actors: Linear layers with ReLU / Tanh between them, at most 3, hidden widths <= 64, float32).  The
    first Linear takes joint_width inputs (ReplayBatch.joint's row: at most MPE_ACTOR_MAX_INPUT = 256 floats), the last gives 1
    output.  The weights are packed again at every call unless freeze() was called, so in-place (soft) updates are seen."""
    who, noun = "Critics", "critics"

    def __init__(self, env, modules):
        NetSet.__init__(self, env, modules)
        self._out = Cache()

    def _widths(self):
        self.off, self.joint_width, self.col_move, self.col_utter = env_joint_layout(self.env, "Critics")
        if self.joint_width > _abi.MPE_ACTOR_MAX_INPUT:
            raise _abi.MpeError("Critics: the joint row has %d floats, a critic's input is at most MPE_ACTOR_MAX_INPUT = %d wide"
                                % (self.joint_width, _abi.MPE_ACTOR_MAX_INPUT))
        self.in_widths, self.n_out = [self.joint_width] * self.A, [1] * self.A

    def _input_refusal(self, i, n, D):
        return "Critics: agent %d's critic takes %d inputs, the joint row has %d" % (i, n, D)

    def _rows_check(self, rows, who):
        """rows: ONE tensor every critic reads, or a list of A tensors (agent i's critic reads rows[i]) -> (M, the A tensors)"""
        many = isinstance(rows, (list, tuple))
        each = list(rows) if many else [rows]
        if many and len(each) != self.A:
            raise _abi.MpeError("%s: rows is one tensor every critic reads, or a list of %d tensors, one per agent (got %d)"
                                % (who, self.A, len(each)))
        for i, r in enumerate(each):
            if not torch.is_tensor(r) or r.dtype != torch.float32 or r.dim() != 2 or r.shape[1] != self.joint_width or \
                    not r.is_contiguous() or r.device != self.world.device or r.shape[0] != each[0].shape[0]:
                raise _abi.MpeError("%s: rows%s is a contiguous float32 [M, %d] tensor on the env's device"
                                    % (who, "[%d]" % i if many else "", self.joint_width))
        return int(each[0].shape[0]), each if many else each * self.A

    def _launch(self, rows_n, M, td=None, _packed=None):
        """The one launch: q [A, M] (and y [A, M] when td, an MpeTdTarget, is given) -> (q, y); tensors cached per M.  rows_n[i]:
        the rows agent i's critic reads."""
        q, y = self._out.get(M, lambda: tuple(torch.zeros((self.A, M), dtype=torch.float32, device=self.world.device) for _ in range(2)))
        wts, aset = _packed if _packed is not None else self.packed()
        ptrs = (C.c_void_p * self.A)(*[r.data_ptr() for r in rows_n])
        _abi.check(_abi.lib().mpe_critic_q(C.byref(aset), ptrs, M, q.data_ptr(), C.byref(td) if td is not None else None,
                                           y.data_ptr() if td is not None else None, _abi.raw_stream(self.world.device)), "mpe_critic_q")
        del wts
        return q, (y if td is not None else None)

    def q(self, rows):
        """One launch: every agent's critic on the joint rows [M, joint_width] -- ONE tensor, or a list of A (agent i's critic reads
        rows[i]: MADDPG's actor loss gives every critic its own rows) -> q [A, M] (this object's tensor per M)."""
        M, rows_n = self._rows_check(rows, "Critics.q")
        return self._launch(rows_n, M)[0]

    def train_forward(self, rows, packed):
        """The forward Trainable runs, on the packed pair it hands to the backward: q -> (M, q[i] [M] per agent, the input rows)."""
        M, rows_n = self._rows_check(rows, "Critics.q")
        q = self._launch(rows_n, M, _packed=packed)[0]
        return M, [q[i].clone() for i in range(self.A)], rows_n

    def reference(self, rows):
        """The fp64 torch forward pass, on whatever device the modules and rows are -> [A, M] float64."""
        import copy
        out = []
        for m in self.modules:
            m = copy.deepcopy(m).double()
            with torch.no_grad():
                out.append(m(torch.as_tensor(rows).to(next(m.parameters()).device).double())[:, 0])
        return torch.stack(out)


class TdTargets(object):
    """The TD target of a sampled batch in two launches: compute(batch) = ret + discount * (1 - done) * Q'(next_obs, mu'(next_obs))
    with `actors` the TARGET actors (an Actors of the batch's env; softmax mode gives MADDPG's relaxed actions, greedy / sample
    one-hot rows) and `critics` the TARGET critics.  After a call: joint_next_act [M, joint_width] (the critics' input rows: the
    batch's next observations and the target actors' rows), q_next [A, M] and y [A, M]; the tensors belong to the two objects and
    are rewritten by the next call of that M.  No host synchronisation: {push, sample, compute} captures into a HIP graph."""

    def __init__(self, actors, critics):
        if not isinstance(actors, Actors):
            raise _abi.MpeError("TdTargets: actors is an Actors(env, target_modules, ...)")
        if not isinstance(critics, Critics):
            raise _abi.MpeError("TdTargets: critics is a Critics(env, target_modules)")
        if actors.env is not critics.env:
            raise _abi.MpeError("TdTargets: the Actors and the Critics were built for different envs")
        if actors.joint_width != critics.joint_width:
            raise _abi.MpeError("TdTargets: the actors' joint row has %d floats, the critics' %d" % (actors.joint_width, critics.joint_width))
        self.actors, self.critics = actors, critics
        self.t = 0
        self.joint_next_act = self.q_next = self.y = None

    def compute(self, batch, gamma=None, t=None):
        """batch: what ReplayBuffer.sample / gather returned.  An NStepReplayBatch brings ret and discount (gamma is refused);
        a one-step ReplayBatch: ret = batch.rew and gamma is required.  t: the key of the target actors' SAMPLE draws (None: an
        internal counter advanced by the call).  -> y [A, M]."""
        if not isinstance(batch, ReplayBatch):
            raise _abi.MpeError("TdTargets.compute: batch is a ReplayBatch (ReplayBuffer.sample / gather)")
        td = _abi.MpeTdTarget()
        if isinstance(batch, NStepReplayBatch) or getattr(batch, "ret", None) is not None:
            if gamma is not None:
                raise _abi.MpeError("TdTargets.compute: an n-step batch carries its own discount (gamma^m per row); gamma is not taken")
            td.ret, td.discount = batch.ret.data_ptr(), batch.discount.data_ptr()
        else:
            if gamma is None:
                raise _abi.MpeError("TdTargets.compute: gamma is required for a one-step batch")
            if not math.isfinite(float(gamma)):
                raise _abi.MpeError("TdTargets.compute: gamma = %r is not finite" % (gamma,))
            td.ret, td.discount, td.gamma = batch.rew.data_ptr(), None, float(gamma)
        td.done = batch._done_u8.data_ptr()
        M = int(batch.rew.shape[1])
        if t is None:
            t = self.t
            self.t += 1
        self.actors.act_rows(batch.next_obs_n, t, joint=True)
        self.joint_next_act = self.actors.joint_rows
        self.q_next, self.y = self.critics._launch([self.joint_next_act] * self.critics.A, M, td)
        return self.y


# ---- the TD loss head: the weighted squared TD error and its gradient in two launches (mpe_td_loss) -------------------
class TdLossResult(object):
    """What td_loss_tensors wrote: loss [1]; stats [A, 8] (per agent the means of the weighted squared error, |d|, q and y, then 0,
    0, L_i, 0); dq [A, M] = dL/dq, already scaled by 2 / M (and the weights); td_abs [M], per row the largest |q_i - y_i| over the
    agents (what PrioritizedReplayBuffer.update_td takes); work, the launches' workspace."""
    __slots__ = ("A", "M", "loss", "stats", "dq", "td_abs", "work")

    STATS = ("loss", "abs_td", "q", "y", "reserved", "reserved", "loss", "reserved")


def _work(name, A, M, dev):
    n = getattr(_abi.lib(), name)(A, M)      # (host only: the size checks)
    if n < 0:
        _abi.check(int(n), name)
    return torch.empty((max(int(n), 1),), dtype=torch.float64, device=dev)


def td_loss_tensors(q_n, y, weights=None, out=None):
    """THE TD LOSS RULE in two launches for every agent, no host synchronisation (captures into a HIP graph).  q_n[i]: agent i's
    [M] or [M, 1] float32 values; y [A, M]: TdTargets.y; weights [M]: the importance weights of a prioritized batch (None: 1).
    out: a TdLossResult to rewrite.  -> TdLossResult."""
    who = "td_loss_tensors"
    if not isinstance(q_n, (list, tuple)) or not 1 <= len(q_n) <= _abi.MPE_ACTOR_MAX_AGENTS:
        raise _abi.MpeError("%s: q_n is a list of 1..MPE_ACTOR_MAX_AGENTS = %d tensors, one per agent" % (who, _abi.MPE_ACTOR_MAX_AGENTS))
    A, q0 = len(q_n), q_n[0]
    if not torch.is_tensor(q0) or q0.dim() not in (1, 2):
        raise _abi.MpeError("%s: q_n[0] is a contiguous float32 [M] or [M, 1] tensor on a GPU" % who)
    M, dev = int(q0.shape[0]), q0.device
    for i, q in enumerate(q_n):
        check_tensor(who, q, "q_n[%d]" % i, [(M,), (M, 1)], "q_n[0]'s device", dev)
    check_tensor(who, y, "y", [(A, M)], "q_n[0]'s device", dev)
    if weights is not None:
        check_tensor(who, weights, "weights", [(M,)], "q_n[0]'s device", dev)
    if out is not None and (not isinstance(out, TdLossResult) or out.A != A or out.M != M or out.dq.device != dev):
        raise _abi.MpeError("%s: out is a TdLossResult of %d agents and M = %d (what an earlier call returned)" % (who, A, M))
    if not q0.is_cuda:
        raise _abi.MpeError("%s: q_n[0] is on %s (the tensors live on a GPU: there is no CPU path)" % (who, dev))
    if out is None:
        out = TdLossResult()
        out.A, out.M = A, M
        out.dq = torch.zeros((A, M), dtype=torch.float32, device=dev)
        out.td_abs = torch.zeros((M,), dtype=torch.float32, device=dev)
        out.stats = torch.zeros((A, 8), dtype=torch.float32, device=dev)
        out.loss = torch.zeros((1,), dtype=torch.float32, device=dev)
        out.work = _work("mpe_td_loss_work", A, M, dev)
    qp = (C.c_void_p * A)(*[q.data_ptr() for q in q_n])
    _abi.check(_abi.lib().mpe_td_loss(A, qp, y.data_ptr(), weights.data_ptr() if weights is not None else None, M, out.dq.data_ptr(),
                                      out.td_abs.data_ptr(), out.work.data_ptr(), out.stats.data_ptr(), out.loss.data_ptr(),
                                      _abi.raw_stream(dev)), "mpe_td_loss")
    return out


class _TdLossFn(torch.autograd.Function):
    """forward: the two launches; backward: grad_output * the gradients the forward wrote (ONE multiply)"""

    @staticmethod
    def forward(ctx, head, y, weights, *q_n):
        qs = [q.detach() for q in q_n]
        M = int(qs[0].shape[0]) if torch.is_tensor(qs[0]) and qs[0].dim() in (1, 2) else -1
        key = (len(qs), M, qs[0].device if torch.is_tensor(qs[0]) else None)
        res = td_loss_tensors(qs, y, weights, out=head._out.get(key))
        head._out.get(key, lambda: res)
        ctx.res, ctx.shapes, ctx.owner = res, [tuple(q.shape) for q in q_n], (head, key, head._generation.next(key))
        head.last = res
        return res.loss.view(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        res = ctx.res
        head, key, generation = ctx.owner
        if head._generation.stale(key, generation) or head._out.get(key) is not res:
            raise _abi.MpeError("TdLoss: backward() of a loss whose buffers a later forward with the same M has rewritten (the "
                                "buffers are cached per M: call backward() before the next forward)")
        g = grad_output * res.dq      # out of place: the buffer is rewritten by the next forward of the same M
        return (None, None, None) + tuple(g[i].view(s) for i, s in enumerate(ctx.shapes))


class TdLoss(object):
    """The TD loss head behind torch autograd: loss = TdLoss()(q_n, y, weights=None) is the sum over the agents of
    mean(weights * (q_i - y_i)^2) -- F.mse_loss per agent without weights.  The forward is mpe_td_loss's two launches for all
    agents, the backward ONE multiply of grad_output with the gradients the forward wrote; no host read anywhere.  loss.stats
    [A, 8] (device) carries TdLossResult.STATS; .last is the TdLossResult of the last call (its td_abs [M] is what a prioritized
    buffer's update_td takes).  The buffers are cached per M and rewritten by the next call with the same M: call backward()
    before the next forward; a backward() behind such a forward is refused.  Once differentiable."""

    def __init__(self):
        self._out, self._generation, self.last = Cache(), Generations(), None

    def __call__(self, q_n, y, weights=None):
        who = "TdLoss"
        if not isinstance(q_n, (list, tuple)) or not q_n:
            raise _abi.MpeError("%s: q_n is a list of tensors, one per agent" % who)
        for i, t in enumerate(q_n):
            if not torch.is_tensor(t):
                raise _abi.MpeError("%s: q_n[%d] is not a tensor" % (who, i))
        if torch.is_tensor(y) and y.requires_grad:
            raise _abi.MpeError("%s: y requires grad (the TD target is a constant of the loss)" % who)
        loss = _TdLossFn.apply(self, y, weights, *q_n)
        loss.stats = self.last.stats
        return loss


# ---- the relaxed action rows and their gradient (mpe_policy_rows, mpe_policy_rows_grad) ------------------------------
class RowsLayout(object):
    """Where each agent's action window sits in the critic's joint row: W floats per row, dim_c, and per agent col (the first column of
    its window), movable and speaks; n[i] = 5 * movable + dim_c * speaks logits fill the window.  RowsLayout.of(actors) reads an
    Actors' joint layout."""

    def __init__(self, W, dim_c, col, movable, speaks):
        self.W, self.dim_c = int(W), int(dim_c)
        self.col, self.movable, self.speaks = [int(c) for c in col], [bool(m) for m in movable], [bool(s) and self.dim_c > 0 for s in speaks]
        self.A = len(self.col)
        if not 1 <= self.A <= _abi.MPE_ACTOR_MAX_AGENTS or len(self.movable) != self.A or len(self.speaks) != self.A:
            raise _abi.MpeError("RowsLayout: col, movable and speaks are lists of 1..MPE_ACTOR_MAX_AGENTS = %d entries, one per agent"
                                % _abi.MPE_ACTOR_MAX_AGENTS)
        self.n = [_abi.MPE_ACTION_DIM * m + self.dim_c * s for m, s in zip(self.movable, self.speaks)]

    @staticmethod
    def of(layout, who="RowsLayout"):
        if isinstance(layout, RowsLayout):
            return layout
        if isinstance(layout, Actors):
            col = [m if m is not None else u for m, u in zip(layout.col_move, layout.col_utter)]
            return RowsLayout(layout.joint_width, layout.dim_c, col, layout.movable, layout.speaks)
        raise _abi.MpeError("%s: layout is an Actors or a RowsLayout(W, dim_c, col, movable, speaks)" % who)

    def cfg(self):
        c = _abi.MpePolicyRows()
        c.n_agents, c.W, c.dim_c = self.A, self.W, self.dim_c
        for i in range(self.A):
            c.col[i], c.movable[i], c.speaks[i], c.ld[i] = self.col[i], int(self.movable[i]), int(self.speaks[i]), self.n[i]
        return c


def _logits_check(who, lay, logits_n):
    if not isinstance(logits_n, (list, tuple)) or len(logits_n) != lay.A:
        raise _abi.MpeError("%s: logits_n is a list of %d tensors, one per agent" % (who, lay.A))
    z0 = logits_n[0]
    if not torch.is_tensor(z0) or z0.dim() != 2:
        raise _abi.MpeError("%s: logits_n[0] is a contiguous float32 [M, %d] tensor on a GPU" % (who, lay.n[0]))
    M, dev = int(z0.shape[0]), z0.device
    for i, z in enumerate(logits_n):
        check_tensor(who, z, "logits_n[%d]" % i, [(M, lay.n[i])], "logits_n[0]'s device", dev)
    return M, dev


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def policy_rows_tensors(layout, joint, logits_n, out=None):
    """THE POLICY ROWS RULE in one launch, no host synchronisation: per agent the batch's joint rows with its own action window
    replaced by the softmax of its logits, head by head.  layout: an Actors or a RowsLayout; joint: contiguous float32 [M, W];
    logits_n[i]: [M, n_i].  out: a list of A contiguous [M, W] tensors to rewrite (they overlap neither joint nor one another: not
    checked).  -> the list of A tensors."""
    who = "policy_rows_tensors"
    lay = RowsLayout.of(layout, who)
    M, dev = _logits_check(who, lay, logits_n)
    check_tensor(who, joint, "joint", [(M, lay.W)], "logits_n[0]'s device", dev)
    if out is not None:
        if not isinstance(out, (list, tuple)) or len(out) != lay.A:
            raise _abi.MpeError("%s: out is a list of %d tensors, one per agent" % (who, lay.A))
        for i, o in enumerate(out):
            check_tensor(who, o, "out[%d]" % i, [(M, lay.W)], "logits_n[0]'s device", dev)
    if not joint.is_cuda:
        raise _abi.MpeError("%s: joint is on %s (the tensors live on a GPU: there is no CPU path)" % (who, dev))
    if out is None:
        out = [torch.zeros((M, lay.W), dtype=torch.float32, device=dev) for _ in range(lay.A)]
    cfg = lay.cfg()
    _abi.check(_abi.lib().mpe_policy_rows(C.byref(cfg), joint.data_ptr(), _ptrs(logits_n), M, _ptrs(out), _abi.raw_stream(dev)),
               "mpe_policy_rows")
    return list(out)


class PolicyRowsGradResult(object):
    """What policy_rows_grad_tensors wrote: dlogits_n, A views [M, n_i] of ONE flat float32 buffer `grads` (every block starts at a
    multiple of 4 floats); with stats: loss [1] and stats [A, 8] (per agent mean q, mean z^2, mean entropy, 0, 0, 0, L_i, 0)."""
    __slots__ = ("M", "n", "grads", "dlogits_n", "stats", "loss", "work")

    STATS = ("q", "logits_sq", "entropy", "reserved", "reserved", "reserved", "loss", "reserved")


def _rows_grad_result(n, M, dev):
    r = PolicyRowsGradResult()
    off, at = [], 0
    for k in n:
        off.append(at)
        at += (M * k + 3) // 4 * 4
    r.M, r.n = M, list(n)
    r.grads = torch.zeros((max(at, 1),), dtype=torch.float32, device=dev)
    r.dlogits_n = [r.grads[o:o + M * k].view(M, k) for o, k in zip(off, n)]
    r.stats = torch.zeros((len(n), 8), dtype=torch.float32, device=dev)
    r.loss = torch.zeros((1,), dtype=torch.float32, device=dev)
    r.work = _work("mpe_policy_rows_grad_work", len(n), M, dev)
    return r


def policy_rows_grad_tensors(layout, logits_n, g_n, reg_coef=0.0, q=None, out=None):
    """THE POLICY ROWS GRADIENT RULE in one launch (two with stats), no host synchronisation: dL/d(window) -> dL/dlogits through
    the softmax Jacobian, plus the gradient of reg_coef * mean(logits^2).  g_n[i]: float32 [M, >= n_i] whose last dimension is
    contiguous -- its row stride is the launch's ld (mlp_dinput_tensors' packed [M, n_i] window, or a [M, W] gradient's columns
    col_i..: full[:, col_i:col_i + n_i]).  q [A, M]: the critics' values on policy_rows_tensors' rows; given: the launch also writes
    the loss -mean q + reg_coef * mean z^2 and the stats.  out: a PolicyRowsGradResult to rewrite.  -> PolicyRowsGradResult."""
    who = "policy_rows_grad_tensors"
    lay = RowsLayout.of(layout, who)
    M, dev = _logits_check(who, lay, logits_n)
    if not isinstance(g_n, (list, tuple)) or len(g_n) != lay.A:
        raise _abi.MpeError("%s: g_n is a list of %d tensors, one per agent" % (who, lay.A))
    for i, (g, k) in enumerate(zip(g_n, lay.n)):
        if not torch.is_tensor(g) or g.dtype != torch.float32 or g.dim() != 2 or g.shape[0] != M or g.shape[1] < k or \
                (g.shape[1] > 1 and g.stride(1) != 1) or (M > 1 and g.stride(0) < k) or g.device != dev:
            raise _abi.MpeError("%s: g_n[%d] is a float32 [%d, >= %d] tensor on logits_n[0]'s device, its last dimension contiguous and "
                                "its row stride at least %d" % (who, i, M, k, k))
    if not math.isfinite(float(reg_coef)) or float(reg_coef) < 0:
        raise _abi.MpeError("%s: reg_coef = %r (a finite value >= 0)" % (who, reg_coef))
    if q is not None:
        check_tensor(who, q, "q", [(lay.A, M)], "logits_n[0]'s device", dev)
    if out is not None and (not isinstance(out, PolicyRowsGradResult) or out.M != M or out.n != lay.n or out.grads.device != dev):
        raise _abi.MpeError("%s: out is a PolicyRowsGradResult of the same heads and M = %d (what an earlier call returned)" % (who, M))
    if not logits_n[0].is_cuda:
        raise _abi.MpeError("%s: logits_n[0] is on %s (the tensors live on a GPU: there is no CPU path)" % (who, dev))
    if out is None:
        out = _rows_grad_result(lay.n, M, dev)
    cfg = lay.cfg()
    cfg.reg_coef = float(reg_coef)
    for i, (g, k) in enumerate(zip(g_n, lay.n)):
        cfg.ld[i] = max(int(g.stride(0)), k) if M > 1 else k
    st = q is not None
    _abi.check(_abi.lib().mpe_policy_rows_grad(C.byref(cfg), _ptrs(logits_n), _ptrs(g_n), M, _ptrs(out.dlogits_n),
                                               q.data_ptr() if st else None, out.work.data_ptr() if st else None,
                                               out.stats.data_ptr() if st else None, out.loss.data_ptr() if st else None,
                                               _abi.raw_stream(dev)), "mpe_policy_rows_grad")
    return out


class _ActorLossFn(torch.autograd.Function):
    """forward: rows, critics, dQ/d(window), softmax Jacobian -- four launches and the finish; backward: ONE multiply"""

    @staticmethod
    def forward(ctx, head, joint, *logits_n):
        from .train import mlp_dinput_tensors      # (train.py imports this file)
        lay, critics = head.layout, head.critics
        zs = [z.detach() for z in logits_n]
        M, dev = _logits_check("ActorLoss", lay, zs)
        key = (M, dev)
        bufs = head._out.get(key)
        if bufs is None:
            if not zs[0].is_cuda:
                raise _abi.MpeError("ActorLoss: logits_n[0] is on %s (the tensors live on a GPU: there is no CPU path)" % (dev,))
            bufs = head._out.get(key, lambda: ([torch.zeros((M, lay.W), dtype=torch.float32, device=dev) for _ in range(lay.A)],
                                               torch.full((M,), -1.0, dtype=torch.float32, device=dev) / torch.tensor(float(M), dtype=torch.float32, device=dev),
                                               _rows_grad_result(lay.n, M, dev)))
        rows, dout, res = bufs
        policy_rows_tensors(lay, joint, zs, out=rows)
        packed = critics.packed()      # (one pair for the forward and the input gradient: a DeviceAdam's live buffer is followed)
        q = critics._launch(rows, M, _packed=packed)[0]
        g = mlp_dinput_tensors(critics, rows, [dout] * lay.A, cols=[(c, k) for c, k in zip(lay.col, lay.n)], packed=packed)
        policy_rows_grad_tensors(lay, zs, g, head.reg_coef, q=q, out=res)
        ctx.res, ctx.shapes, ctx.owner = res, [tuple(z.shape) for z in logits_n], (head, key, head._generation.next(key))
        head.last = res
        return res.loss.view(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        res = ctx.res
        head, key, generation = ctx.owner
        if head._generation.stale(key, generation):
            raise _abi.MpeError("ActorLoss: backward() of a loss whose buffers a later forward with the same M has rewritten (the "
                                "buffers are cached per M: call backward() before the next forward)")
        g = grad_output * res.grads      # out of place: the buffer is rewritten by the next forward of the same M
        at, grads = 0, []
        for k, shape in zip(res.n, ctx.shapes):
            grads.append(g[at:at + res.M * k].view(shape))
            at += (res.M * k + 3) // 4 * 4
        return (None, None) + tuple(grads)


class ActorLoss(object):
    """MADDPG's actor loss behind torch autograd: loss = ActorLoss(actors, critics, reg_coef=0.0)(logits_n, batch.joint) is the sum
    over the agents of -mean Q_i(joint row with agent i's action window replaced by softmax(logits_i)) + reg_coef *
    mean(logits_i^2).  The forward runs mpe_policy_rows, critics.q on the A row tensors, mlp_dinput_tensors (dout = -1 / M, the
    windows) and mpe_policy_rows_grad with stats; the backward is ONE multiply of grad_output with the stored dlogits.  The
    critics are a constant of the loss: whatever critics.packed() is at the call is read, so a DeviceAdam's live buffer is
    followed.  actors: an Actors (its joint layout and heads), or a RowsLayout.  loss.stats [A, 8] carries
    PolicyRowsGradResult.STATS; .last the result of the last call.  Buffers cached per M, as PpoLoss's."""

    def __init__(self, actors, critics, reg_coef=0.0):
        self.layout = RowsLayout.of(actors, "ActorLoss")
        if not isinstance(critics, Critics):
            raise _abi.MpeError("ActorLoss: critics is a Critics(env, modules)")
        if critics.A != self.layout.A or critics.joint_width != self.layout.W:
            raise _abi.MpeError("ActorLoss: the critics read %d agents' rows of %d floats, the layout has %d agents and W = %d"
                                % (critics.A, critics.joint_width, self.layout.A, self.layout.W))
        if not math.isfinite(float(reg_coef)) or float(reg_coef) < 0:
            raise _abi.MpeError("ActorLoss: reg_coef = %r (a finite value >= 0)" % (reg_coef,))
        self.critics, self.reg_coef = critics, float(reg_coef)
        self._out, self._generation, self.last = Cache(), Generations(), None

    def __call__(self, logits_n, joint):
        who = "ActorLoss"
        if not isinstance(logits_n, (list, tuple)) or len(logits_n) != self.layout.A:
            raise _abi.MpeError("%s: logits_n is a list of %d tensors, one per agent" % (who, self.layout.A))
        for i, t in enumerate(logits_n):
            if not torch.is_tensor(t):
                raise _abi.MpeError("%s: logits_n[%d] is not a tensor" % (who, i))
        if not torch.is_tensor(joint) or joint.requires_grad:
            raise _abi.MpeError("%s: joint is the batch's joint rows, a tensor that does not require grad" % who)
        loss = _ActorLossFn.apply(self, joint, *logits_n)
        loss.stats = self.last.stats
        return loss


# ---- the value-based learners: next-state logits and the Q-loss head (mpe_q_loss) ------------------------------------
_Q_MIXES = {"independent": _abi.MPE_Q_INDEPENDENT, "vdn": _abi.MPE_Q_VDN}


class QTargets(object):
    """The next-state action values of a sampled batch: compute(batch) runs target_actors.act_rows(batch.next_obs_n) and, with
    online_actors (double-Q), online_actors.act_rows(batch.next_obs_n) -- one launch each -- and returns (next_target,
    next_online or None), the [A, M, 16] logits tensors q_loss_tensors / QLoss take.  Both sets are Actors(env, modules,
    mode="greedy", logits=True) of the batch's env; next_target is the target set's own tensor, next_online a copy kept here (the
    online set's next launch over M rows rewrites its own); both cached per M.  act_rows never explores."""

    def __init__(self, target_actors, online_actors=None):
        for name, a in (("target_actors", target_actors), ("online_actors", online_actors)):
            if a is None and name == "online_actors":
                continue
            if not isinstance(a, Actors):
                raise _abi.MpeError("QTargets: %s is an Actors(env, modules, mode=\"greedy\", logits=True)" % name)
            if not a._want[2]:
                raise _abi.MpeError("QTargets: %s was built without logits=True (the launch writes no logits)" % name)
        if online_actors is not None and online_actors.env is not target_actors.env:
            raise _abi.MpeError("QTargets: online_actors and target_actors were built for different envs")
        self.target, self.online = target_actors, online_actors
        self.next_target = self.next_online = None
        self._keep = Cache()

    def compute(self, batch):
        if not isinstance(batch, ReplayBatch):
            raise _abi.MpeError("QTargets.compute: batch is a ReplayBatch (ReplayBuffer.sample / gather)")
        obs = batch.next_obs_n
        if len(obs) != self.target.A or any(int(o.shape[1]) != d for o, d in zip(obs, self.target.obs_widths)) or \
                obs[0].device != self.target.world.device:
            raise _abi.MpeError("QTargets.compute: batch was sampled from another env's buffer (its next_obs_n are not the actors' "
                                "observation blocks)")
        self.target.act_rows(obs)
        self.next_target = self.target.rows.logits
        self.next_online = None
        if self.online is not None:
            # a copy of this object's: the online set's next act_rows of this M (a Trainable's forward on batch.obs_n) rewrites its own
            self.online.act_rows(obs)
            z = self.online.rows.logits
            self.next_online = self._keep.get(int(z.shape[1]), lambda: torch.empty_like(z))
            self.next_online.copy_(z)
        return self.next_target, self.next_online


class QLossResult(object):
    """What q_loss_tensors wrote: loss [1]; stats [A, 8] (TdLossResult.STATS, q the agent's mean utility of the actions taken; under
    VDN the error columns are the team's in every row); dq_n, A views [M, n_i] of ONE flat float32 buffer `grads` (every block
    starts at a multiple of 4 floats) = dL/dlogits; q_taken [A, M]; y [A, M] (VDN: the team's target in every row); td_abs [M]
    (what PrioritizedReplayBuffer.update_td takes); work, the launches' workspace."""
    __slots__ = ("A", "M", "n", "mix", "loss", "stats", "grads", "dq_n", "q_taken", "y", "td_abs", "work")

    STATS = TdLossResult.STATS


def _q_result(n, M, mix, dev):
    r = QLossResult()
    g = _rows_grad_result(n, M, dev)
    r.A, r.M, r.n, r.mix = len(n), M, list(n), mix
    r.grads, r.dq_n, r.stats, r.loss = g.grads, g.dlogits_n, g.stats, g.loss
    r.q_taken = torch.zeros((r.A, M), dtype=torch.float32, device=dev)
    r.y = torch.zeros((r.A, M), dtype=torch.float32, device=dev)
    r.td_abs = torch.zeros((M,), dtype=torch.float32, device=dev)
    r.work = _work("mpe_q_loss_work", r.A, M, dev)
    return r


def q_loss_tensors(layout, q_n, batch, next_target, next_online=None, gamma=None, mix="independent", weights=None, out=None):
    """THE Q LOSS RULE in two launches for every agent, no host synchronisation (captures into a HIP graph).  layout: an Actors (the
    Q-networks: its heads) or a RowsLayout; q_n[i]: agent i's online logits [M, n_i] (what Trainable(actors)(batch.obs_n)
    returns); batch: a ReplayBatch -- its act / utter rows choose, its rew (one-step, with gamma) or ret and discount (n-step:
    gamma is refused) and its done make the target; next_target, next_online: QTargets.compute's [A, M, 16] tensors (next_online
    None: the plain max-Q target, else double-Q); mix: "independent" or "vdn"; weights [M]: the importance weights of a
    prioritized batch (None: 1).  out: a QLossResult to rewrite.  -> QLossResult."""
    who = "q_loss_tensors"
    lay = RowsLayout.of(layout, who)
    if mix not in _Q_MIXES:
        raise _abi.MpeError("%s: mix is one of %s (got %r)" % (who, sorted(_Q_MIXES), mix))
    if not isinstance(q_n, (list, tuple)) or len(q_n) != lay.A:
        raise _abi.MpeError("%s: q_n is a list of %d tensors, one per agent" % (who, lay.A))
    q0 = q_n[0]
    if not torch.is_tensor(q0) or q0.dim() != 2:
        raise _abi.MpeError("%s: q_n[0] is a contiguous float32 [M, %d] tensor on a GPU" % (who, lay.n[0]))
    M, dev, A = int(q0.shape[0]), q0.device, lay.A
    for i, q in enumerate(q_n):
        check_tensor(who, q, "q_n[%d]" % i, [(M, lay.n[i])], "q_n[0]'s device", dev)
    if not isinstance(batch, ReplayBatch):
        raise _abi.MpeError("%s: batch is a ReplayBatch (ReplayBuffer.sample / gather)" % who)
    td = _abi.MpeTdTarget()
    if getattr(batch, "ret", None) is not None:
        if gamma is not None:
            raise _abi.MpeError("%s: an n-step batch carries its own discount (gamma^m per row); gamma is not taken" % who)
        check_tensor(who, batch.ret, "batch.ret", [(A, M)], "q_n[0]'s device", dev)
        check_tensor(who, batch.discount, "batch.discount", [(M,)], "q_n[0]'s device", dev)
        td.ret, td.discount = batch.ret.data_ptr(), batch.discount.data_ptr()
    else:
        if gamma is None:
            raise _abi.MpeError("%s: gamma is required for a one-step batch" % who)
        if not math.isfinite(float(gamma)):
            raise _abi.MpeError("%s: gamma = %r is not finite" % (who, gamma))
        check_tensor(who, batch.rew, "batch.rew", [(A, M)], "q_n[0]'s device", dev)
        td.ret, td.discount, td.gamma = batch.rew.data_ptr(), None, float(gamma)
    if not torch.is_tensor(batch._done_u8) or batch._done_u8.dtype != torch.uint8 or tuple(batch._done_u8.shape) != (A, M) or \
            not batch._done_u8.is_contiguous() or batch._done_u8.device != dev:
        raise _abi.MpeError("%s: batch.done is a contiguous [%d, %d] tensor on q_n[0]'s device" % (who, A, M))
    td.done = batch._done_u8.data_ptr()
    if any(lay.movable):
        check_tensor(who, batch.act, "batch.act", [(A, M, _abi.MPE_ACTION_DIM)], "q_n[0]'s device", dev)
    if any(lay.speaks):
        check_tensor(who, batch.utter, "batch.utter", [(A, M, lay.dim_c)], "q_n[0]'s device", dev)
    check_tensor(who, next_target, "next_target", [(A, M, _abi.MPE_ACTOR_MAX_OUT)], "q_n[0]'s device", dev)
    if next_online is not None:
        check_tensor(who, next_online, "next_online", [(A, M, _abi.MPE_ACTOR_MAX_OUT)], "q_n[0]'s device", dev)
    if weights is not None:
        check_tensor(who, weights, "weights", [(M,)], "q_n[0]'s device", dev)
    code = _Q_MIXES[mix]
    if out is not None and (not isinstance(out, QLossResult) or out.M != M or out.n != lay.n or out.mix != code or out.grads.device != dev):
        raise _abi.MpeError("%s: out is a QLossResult of the same heads, mix and M = %d (what an earlier call returned)" % (who, M))
    if not q0.is_cuda:
        raise _abi.MpeError("%s: q_n[0] is on %s (the tensors live on a GPU: there is no CPU path)" % (who, dev))
    if out is None:
        out = _q_result(lay.n, M, code, dev)
    cfg = _abi.MpeQLoss()
    cfg.n_agents, cfg.dim_c, cfg.mix = A, lay.dim_c, code
    for i in range(A):
        cfg.movable[i], cfg.speaks[i] = int(lay.movable[i]), int(lay.speaks[i])
    _abi.check(_abi.lib().mpe_q_loss(
        C.byref(cfg), _ptrs(q_n), next_target.data_ptr(), next_online.data_ptr() if next_online is not None else None,
        batch.act.data_ptr() if any(lay.movable) else None, batch.utter.data_ptr() if any(lay.speaks) else None, C.byref(td),
        weights.data_ptr() if weights is not None else None, M, _ptrs(out.dq_n), out.q_taken.data_ptr(), out.y.data_ptr(),
        out.td_abs.data_ptr(), out.work.data_ptr(), out.stats.data_ptr(), out.loss.data_ptr(), _abi.raw_stream(dev)), "mpe_q_loss")
    return out


class _QLossFn(torch.autograd.Function):
    """forward: the two launches; backward: grad_output * the gradients the forward wrote (ONE multiply)"""

    @staticmethod
    def forward(ctx, head, batch, next_target, next_online, gamma, weights, *q_n):
        qs = [q.detach() for q in q_n]
        M = int(qs[0].shape[0]) if qs[0].dim() == 2 else -1
        key = (M, qs[0].device)
        res = q_loss_tensors(head.layout, qs, batch, next_target, next_online, gamma, head.mix, weights, out=head._out.get(key))
        head._out.get(key, lambda: res)
        ctx.res, ctx.shapes, ctx.owner = res, [tuple(q.shape) for q in q_n], (head, key, head._generation.next(key))
        head.last = res
        return res.loss.view(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        res = ctx.res
        head, key, generation = ctx.owner
        if head._generation.stale(key, generation) or head._out.get(key) is not res:
            raise _abi.MpeError("QLoss: backward() of a loss whose buffers a later forward with the same M has rewritten (the "
                                "buffers are cached per M: call backward() before the next forward)")
        g = grad_output * res.grads      # out of place: the buffer is rewritten by the next forward of the same M
        at, grads = 0, []
        for k, shape in zip(res.n, ctx.shapes):
            grads.append(g[at:at + res.M * k].view(shape))
            at += (res.M * k + 3) // 4 * 4
        return (None,) * 6 + tuple(grads)


class QLoss(object):
    """The Q-loss head behind torch autograd: loss = QLoss(actors, mix="independent", double=True)(q_n, batch, next_target,
    next_online, gamma=None, weights=None) with q_n = Trainable(actors)(batch.obs_n) and (next_target, next_online) =
    QTargets(target_actors, actors).compute(batch).  mix="independent": the sum over the agents of mean(weights * (Q_i(s)[a_i] -
    y_i)^2), y_i = ret_i + discount * (1 - done_i) * Q'_i(s')[argmax Q_i(s')]; mix="vdn": mean(weights * (sum_i Q_i(s)[a_i] - y)^2)
    with the team's reward, any-agent done and the summed bootstrap.  double=False takes the plain max of the target net
    (next_online is refused); double=True requires next_online.  The forward is mpe_q_loss's two launches for all agents, the
    backward ONE multiply of grad_output with the gradients the forward wrote; no host read anywhere.  loss.stats [A, 8] (device)
    carries QLossResult.STATS; .last is the QLossResult of the last call (its td_abs [M] is what a prioritized buffer's update_td
    takes).  The buffers are cached per M and rewritten by the next call with the same M: call backward() before the next
    forward; a backward() behind such a forward is refused.  Once differentiable."""

    def __init__(self, actors, mix="independent", double=True):
        self.layout = RowsLayout.of(actors, "QLoss")
        if mix not in _Q_MIXES:
            raise _abi.MpeError("QLoss: mix is one of %s (got %r)" % (sorted(_Q_MIXES), mix))
        self.mix, self.double = mix, bool(double)
        self._out, self._generation, self.last = Cache(), Generations(), None

    def __call__(self, q_n, batch, next_target, next_online=None, gamma=None, weights=None):
        who = "QLoss"
        if not isinstance(q_n, (list, tuple)) or len(q_n) != self.layout.A:
            raise _abi.MpeError("%s: q_n is a list of %d tensors, one per agent" % (who, self.layout.A))
        for i, t in enumerate(q_n):
            if not torch.is_tensor(t):
                raise _abi.MpeError("%s: q_n[%d] is not a tensor" % (who, i))
        if self.double and next_online is None:
            raise _abi.MpeError("%s: double=True needs next_online (QTargets(target_actors, online_actors).compute)" % who)
        if not self.double and next_online is not None:
            raise _abi.MpeError("%s: double=False takes the target net's own maximum; next_online is not taken" % who)
        for name, t in (("next_target", next_target), ("next_online", next_online), ("weights", weights)):
            if torch.is_tensor(t) and t.requires_grad:
                raise _abi.MpeError("%s: %s requires grad (it is a constant of the loss)" % (who, name))
        loss = _QLossFn.apply(self, batch, next_target, next_online, gamma, weights, *q_n)
        loss.stats = self.last.stats
        return loss
