"""The no-grad half of an off-policy (MADDPG-style) update on the device: `Critics` evaluates one MLP critic per agent over M joint
rows in ONE launch (mpe_critic_q: the actor kernel's MFMA body with a one-output last layer and no head), and `TdTargets` turns a
sampled ReplayBatch into the TD target in TWO launches -- the target actors decide on batch.next_obs_n and write complete critic
input rows (Actors.act_rows, joint=True), the target critics read those rows and write Q' and y.  DESIGN.md 2.14; the two rules
(joint rows, y) are stated in include/mpe_hip.h.  Backward passes stay in torch autograd.

    mu_t, q_t = Actors(env, target_actor_modules, mode="softmax"), Critics(env, target_critic_modules)
    td = TdTargets(mu_t, q_t)
    batch = buf.sample(1024, joint=True, n_step=3, gamma=0.95, episode_len=25)
    y = td.compute(batch)                       # [A, M]: ret + discount * (1 - done) * Q'(next_obs, mu'(next_obs))
"""
import ctypes as C
import math

import torch

from . import _abi
from .netset import Cache, NetSet
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
