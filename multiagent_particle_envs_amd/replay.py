"""A device-resident replay buffer for off-policy learners: `ReplayBuffer` keeps the last S steps' transitions of all B worlds in a
ring on the device, filled by ONE launch per step (mpe_replay_push) and sampled by ONE launch per minibatch (mpe_replay_sample,
the same transition indices for every agent); both launches capture into a HIP graph, because the write position lives on the
device and the push advances it itself.  csrc/mpe_replay.hip, DESIGN.md 2.11.

    buf = ReplayBuffer(env, steps=1024, seed=0)
    next_obs_n, rew_n, done_n, _ = env.step(action)
    buf.push(obs_n, action, next_obs_n, rew_n, done_n)
    batch = buf.sample(1024, joint=True)        # batch.obs_n[i] [M, D_i], batch.act [A,M,5], batch.joint [M, sum D + sum n_act] ...
    PolicyLoop(env, pi).run(T, replay=buf)      # the closed loop pushes every step itself

`PrioritizedReplayBuffer` adds one float32 priority per transition and a device sum tree over them (csrc/mpe_replay_prio.hip,
DESIGN.md 2.12): proportional draws, importance weights and priority updates without a host round trip or a pass over all S * B
priorities.

    buf = PrioritizedReplayBuffer(env, steps=1024, alpha=0.6)
    buf.push(obs_n, action, next_obs_n, rew_n, done_n)       # a new transition enters at the largest priority seen so far
    batch = buf.sample(1024, joint=True)                     # a ReplayBatch plus batch.prio / .total / .n_valid / .weights(beta)
    buf.update_td(batch.idx, td_error)                       # priority = (|td| + eps) ** alpha

n-step returns (the rule is stated in include/mpe_hip.h): `sample(..., n_step=n, gamma=g)` and `gather(idx,
n_step=n, gamma=g)` of both buffers are still ONE launch of the gather (mpe_replay_sample_nstep / mpe_replay_gather_nstep) and
return an NStepReplayBatch: ret [A,M] = sum_k gamma^k rew over the m <= n steps that follow the transition in its world and stay
inside its episode and the ring, discount [M] = gamma^m, n_used [M] = m, last [M] the chain's last transition, from which done and
next_obs_n / joint_next are taken: the target is ret + discount * (1 - done) * Q(next_obs).

    batch = buf.sample(1024, joint=True, n_step=5, gamma=0.95, episode_len=25)      # PolicyLoop(env, pi, episode_len=25) pushed
"""
import ctypes as C
import math

import torch

from . import _abi


class ReplayBatch(object):
    """One minibatch of M transitions, the same for every agent: idx [M] int64 (transition slot * B + world), obs_n / next_obs_n
    (per agent [M, D_i]), act [A,M,5], utter [A,M,dim_c] or None, rew [A,M], done [A,M] (torch.bool), and with joint=True
    joint [M, sum D_i + sum n_act_i] (every agent's observation in agent order, then the action rows agent by agent: agent i's
    move row [5] if it is movable, directly followed by its utterance row [dim_c] if it speaks, then agent i + 1's -- for two
    agents with both heads [obs0 obs1 | move0 utter0 | move1 utter1]) and joint_next [M, sum D_i].  The tensors belong to the
    buffer."""
    __slots__ = ("idx", "obs_n", "next_obs_n", "act", "utter", "rew", "done", "joint", "joint_next", "_obs", "_next", "_done_u8")


class NStepReplayBatch(ReplayBatch):
    """A ReplayBatch with n-step returns: also ret [A,M] float32 (the discounted sum of the m rewards of the chain that starts
    at idx), discount [M] float32 (gamma^m), n_used [M] int32 (m) and last [M] int64 (the chain's last transition).  done,
    next_obs_n and joint_next are those of `last`; idx, obs_n, act, utter, rew (the one-step reward) and joint those of idx."""
    __slots__ = ("ret", "discount", "n_used", "last")


class ReplayBuffer(object):
    """The last `steps` steps of every world of `env`, on the env's device.  Widths, heads and dim_c are taken from the env as
    Actors takes them.  Ring tensors (slot = step number % steps; layouts of LoopTrajectory): obs, next_obs [S, sum D_i * B] (agent
    i's block of a slot at floats off[i] * B, [B, D_i]; obs_n[s][i] / next_obs_n[s][i] are views), act [S,A,B,5], utter
    [S,A,B,dim_c] or None, rew [S,A,B], done [S,A,B] (torch.bool).  head: the device-side int64 step count both launches read;
    count: its host mirror."""

    def __init__(self, env, steps, seed=0):
        w = env.world
        self.env, self.world = env, w
        self.S = int(steps)
        self.seed = int(seed) & (2 ** 64 - 1)
        self.A, self.B = len(w.agents), int(w.batch_size)
        if self.A > _abi.MPE_REPLAY_MAX_AGENTS:
            raise _abi.MpeError("ReplayBuffer: %d agents (at most MPE_REPLAY_MAX_AGENTS = %d)" % (self.A, _abi.MPE_REPLAY_MAX_AGENTS))
        off = getattr(env, "_obs_off", None)
        if off is None:
            raise _abi.MpeError("ReplayBuffer: this env has no device-side observation layout (env.fused is False)")
        if self.S < 1:
            raise _abi.MpeError("ReplayBuffer: steps = %d (need at least 1)" % self.S)
        if self.S * self.B >= 2 ** 40:
            raise _abi.MpeError("ReplayBuffer: steps * worlds = %d * %d transitions (need fewer than 2^40)" % (self.S, self.B))
        self.off = [int(o) for o in off[:self.A + 1]]
        self.obs_widths = [self.off[i + 1] - self.off[i] for i in range(self.A)]
        self.movable = [bool(a.movable) for a in w.agents]
        self.speaks = [not a.silent for a in w.agents]
        self.dim_c = int(w.dim_c) if any(self.speaks) else 0
        self.n_act = [_abi.MPE_ACTION_DIM * m + self.dim_c * s for m, s in zip(self.movable, self.speaks)]
        for i, n in enumerate(self.n_act):
            if n < 1:
                raise _abi.MpeError("ReplayBuffer: agent %d neither moves nor speaks: it has no head" % i)
        if max(self.obs_widths) > _abi.MPE_REPLAY_MAX_WIDTH:
            raise _abi.MpeError("ReplayBuffer: an observation row of %d floats (at most MPE_REPLAY_MAX_WIDTH = %d)"
                                % (max(self.obs_widths), _abi.MPE_REPLAY_MAX_WIDTH))
        self.joint_width = self.off[-1] + sum(self.n_act)
        self.count = 0
        self._draw = 0
        self._ptrs = {}
        self._batches = {}
        self._desc = None
        self.obs = None

    def _alloc(self):
        if self.obs is not None:
            return
        S, A, B, dev, off = self.S, self.A, self.B, self.world.device, self.off
        self.obs = torch.zeros((S, off[-1] * B), dtype=torch.float32, device=dev)
        self.next_obs = torch.zeros((S, off[-1] * B), dtype=torch.float32, device=dev)
        self.act = torch.zeros((S, A, B, _abi.MPE_ACTION_DIM), dtype=torch.float32, device=dev)
        self.utter = torch.zeros((S, A, B, self.dim_c), dtype=torch.float32, device=dev) if self.dim_c else None
        self.rew = torch.zeros((S, A, B), dtype=torch.float32, device=dev)
        self._done_u8 = torch.zeros((S, A, B), dtype=torch.uint8, device=dev)
        self.done = self._done_u8.view(torch.bool)
        self.head = torch.zeros(1, dtype=torch.int64, device=dev)
        self._ticket = torch.zeros(1, dtype=torch.int32, device=dev)

        def views(flat):
            return [[flat[s, off[i] * B: off[i + 1] * B].view(B, off[i + 1] - off[i]) for i in range(A)] for s in range(S)]
        self.obs_n, self.next_obs_n = views(self.obs), views(self.next_obs)
        d = _abi.MpeReplay()
        d.n_agents, d.dim_c, d.B, d.S, d.seed = A, self.dim_c, B, S, self.seed
        for i in range(A):
            d.obs_width[i], d.movable[i], d.speaks[i] = self.obs_widths[i], int(self.movable[i]), int(self.speaks[i])
        d.obs, d.next_obs, d.act, d.rew = self.obs.data_ptr(), self.next_obs.data_ptr(), self.act.data_ptr(), self.rew.data_ptr()
        d.utter = self.utter.data_ptr() if self.utter is not None else None
        d.done, d.head, d.ticket = self._done_u8.data_ptr(), self.head.data_ptr(), self._ticket.data_ptr()
        self._desc = d

    def __len__(self):
        """Valid transitions: min(count, steps) * worlds."""
        return min(self.count, self.S) * self.B

    # ---- push -------------------------------------------------------------------------------------------------------------------
    def _rows(self, x, dtype, what):
        """rew / done as env.step returns them (a list of A [B] rows of one [A,B] tensor) or one [A,B] tensor -> an [A,B] tensor."""
        A, B = self.A, self.B
        if torch.is_tensor(x):
            t = x
        else:
            x = list(x)
            if len(x) != A or not all(torch.is_tensor(r) for r in x):
                raise _abi.MpeError("ReplayBuffer.push: %s is an [A,B] tensor or a list of %d [B] tensors" % (what, A))
            r0 = x[0]
            step = B * r0.element_size()
            if all(r.dtype == r0.dtype and r.device == r0.device and tuple(r.shape) == (B,) and r.is_contiguous() and
                   r.data_ptr() == r0.data_ptr() + i * step for i, r in enumerate(x)):
                t = r0.as_strided((A, B), (B, 1))      # (the rows of one [A,B] tensor, as env.step hands them out: no copy)
            else:
                t = torch.stack(x)
        if t.dtype != dtype or tuple(t.shape) != (A, B) or not t.is_contiguous() or t.device != self.world.device:
            raise _abi.MpeError("ReplayBuffer.push: %s is [%d, %d] %s on the env's device" % (what, A, B, dtype))
        return t

    def _obs_check(self, obs_n, what):
        if len(obs_n) != self.A:
            raise _abi.MpeError("ReplayBuffer.push: %d %s blocks for %d agents" % (len(obs_n), what, self.A))
        for i, o in enumerate(obs_n):
            if not torch.is_tensor(o) or o.dtype != torch.float32 or not o.is_contiguous() or o.device != self.world.device or \
                    tuple(o.shape) != (self.B, self.obs_widths[i]):
                raise _abi.MpeError("ReplayBuffer.push: %s[%d] is a contiguous float32 [%d, %d] tensor on the env's device"
                                    % (what, i, self.B, self.obs_widths[i]))

    def push(self, obs_n, action, next_obs_n, rew, done):
        """One launch: the step's transitions into slot count % steps.  obs_n: the observations the action was chosen on;
        action: the [A,B,5] moves or (moves, utterances [A,B,dim_c]) env.step took; next_obs_n, rew, done: what it returned."""
        self._alloc()
        self._launch_push(self._push_args(obs_n, action, next_obs_n, rew, done))

    def _push_args(self, obs_n, action, next_obs_n, rew, done):
        """The checked arguments of one mpe_replay_push call (checked once per pointer set); nothing is launched."""
        pair = type(action) is tuple
        moves, utter = action if pair else (action, None)
        key = tuple(o.data_ptr() for o in obs_n) + tuple(o.data_ptr() for o in next_obs_n) + \
            (moves.data_ptr() if torch.is_tensor(moves) else None, utter.data_ptr() if torch.is_tensor(utter) else None) + \
            ((rew.data_ptr(),) if torch.is_tensor(rew) else tuple(r.data_ptr() for r in rew)) + \
            ((done.data_ptr(),) if torch.is_tensor(done) else tuple(r.data_ptr() for r in done))
        args = self._ptrs.get(key)
        if args is None:      # checked once per pointer set
            A, B, dev = self.A, self.B, self.world.device
            self._obs_check(obs_n, "obs_n")
            self._obs_check(next_obs_n, "next_obs_n")
            if not torch.is_tensor(moves) or moves.dtype != torch.float32 or tuple(moves.shape) != (A, B, _abi.MPE_ACTION_DIM) or \
                    not moves.is_contiguous() or moves.device != dev:
                raise _abi.MpeError("ReplayBuffer.push: action is a contiguous float32 [%d, %d, 5] device tensor, or (moves, utterances)"
                                    % (A, B))
            if self.dim_c:
                if not torch.is_tensor(utter) or utter.dtype != torch.float32 or tuple(utter.shape) != (A, B, self.dim_c) or \
                        not utter.is_contiguous() or utter.device != dev:
                    raise _abi.MpeError("ReplayBuffer.push: agents speak: action is (moves [A,B,5], utterances [%d, %d, %d]), two "
                                        "contiguous float32 device tensors" % (A, B, self.dim_c))
            r, d = self._rows(rew, torch.float32, "rew"), self._rows(done, torch.bool, "done")
            stacked = (not torch.is_tensor(rew) and r.data_ptr() != rew[0].data_ptr()) or \
                (not torch.is_tensor(done) and d.data_ptr() != done[0].data_ptr())
            args = ((C.c_void_p * A)(*[o.data_ptr() for o in obs_n]), (C.c_void_p * A)(*[o.data_ptr() for o in next_obs_n]),
                    moves.data_ptr(), utter.data_ptr() if self.dim_c else None, r, d)
            if not stacked:      # (rows stacked into a new tensor are re-stacked at every push)
                if len(self._ptrs) >= 64:
                    self._ptrs.clear()
                self._ptrs[key] = args
        return args

    def _launch_push(self, args):
        o, n, mv, ut, r, d = args
        _abi.check(_abi.lib().mpe_replay_push(C.byref(self._desc), o, n, mv, ut, r.data_ptr(), d.data_ptr(),
                                              _abi.raw_stream(self.world.device)), "mpe_replay_push")
        self.count += 1

    # ---- sample -----------------------------------------------------------------------------------------------------------------
    _batch_type = ReplayBatch
    _nstep_batch_type = NStepReplayBatch

    def _batch(self, M, joint, gathered=False, nstep=False):
        """The buffer's output tensors per (M, joint); gathered: a set of its own for gather(), whose idx is the caller's; nstep:
        sets of their own, (M, joint, "nstep"), with the four n-step outputs."""
        key = (M, joint) + (("nstep",) if nstep else ()) + (("gather",) if gathered else ())
        b = self._batches.get(key)
        if b is not None:
            return b
        A, dev, off = self.A, self.world.device, self.off
        if nstep:
            b = NStepReplayBatch() if gathered else self._nstep_batch_type()
            b.ret = torch.zeros((A, M), dtype=torch.float32, device=dev)
            b.discount = torch.zeros(M, dtype=torch.float32, device=dev)
            b.n_used = torch.zeros(M, dtype=torch.int32, device=dev)
            b.last = torch.zeros(M, dtype=torch.int64, device=dev)
        else:
            b = ReplayBatch() if gathered else self._batch_type()
        b.idx = None if gathered else torch.zeros(M, dtype=torch.int64, device=dev)
        b._obs = torch.zeros(off[-1] * M, dtype=torch.float32, device=dev)
        b._next = torch.zeros(off[-1] * M, dtype=torch.float32, device=dev)
        b.obs_n = [b._obs[off[i] * M: off[i + 1] * M].view(M, off[i + 1] - off[i]) for i in range(A)]
        b.next_obs_n = [b._next[off[i] * M: off[i + 1] * M].view(M, off[i + 1] - off[i]) for i in range(A)]
        b.act = torch.zeros((A, M, _abi.MPE_ACTION_DIM), dtype=torch.float32, device=dev)
        b.utter = torch.zeros((A, M, self.dim_c), dtype=torch.float32, device=dev) if self.dim_c else None
        b.rew = torch.zeros((A, M), dtype=torch.float32, device=dev)
        b._done_u8 = torch.zeros((A, M), dtype=torch.uint8, device=dev)
        b.done = b._done_u8.view(torch.bool)
        b.joint = torch.zeros((M, self.joint_width), dtype=torch.float32, device=dev) if joint else None
        b.joint_next = torch.zeros((M, off[-1]), dtype=torch.float32, device=dev) if joint else None
        if len(self._batches) >= 16:
            self._batches.clear()
        self._batches[key] = b
        return b

    def _nstep(self, who, n_step, gamma, episode_len, episode_phase):
        """The checked MpeReplayNStep of a call (the ABI refuses the same by name; here before anything else is looked at)."""
        if gamma is None:
            raise _abi.MpeError("%s: gamma is required when n_step is given" % who)
        n, g, L, p = int(n_step), float(gamma), int(episode_len), int(episode_phase)
        if not 1 <= n <= _abi.MPE_REPLAY_MAX_NSTEP:
            raise _abi.MpeError("%s: n_step = %d (need 1 <= n_step <= MPE_REPLAY_MAX_NSTEP = %d)" % (who, n, _abi.MPE_REPLAY_MAX_NSTEP))
        if not math.isfinite(g):
            raise _abi.MpeError("%s: gamma = %r is not finite" % (who, gamma))
        if L < 0 or L >= 2 ** 63:
            raise _abi.MpeError("%s: episode_len = %d (need 0 <= episode_len < 2^63; 0: the pushes are one episode)" % (who, L))
        if not 0 <= p < max(L, 1):
            raise _abi.MpeError("%s: episode_phase = %d (need 0 <= episode_phase < max(episode_len, 1) = %d)" % (who, p, max(L, 1)))
        ns = _abi.MpeReplayNStep()
        ns.n, ns.gamma, ns.episode_len, ns.episode_phase = n, g, L, p
        return ns

    def _launch(self, b, M, joint, ns=None, idx=None, draw=0):
        """The one launch of a batch.  idx given: read (mpe_replay_gather), else drawn into b.idx with the draws of (seed, draw)
        (mpe_replay_sample); ns given: the _nstep entry point of the two, which also takes the four n-step outputs."""
        name = ("mpe_replay_sample" if idx is None else "mpe_replay_gather") + ("" if ns is None else "_nstep")
        args = (C.byref(self._desc),) + (() if ns is None else (C.byref(ns),)) + (M,)
        args += (int(draw) & (2 ** 64 - 1), b.idx.data_ptr()) if idx is None else (idx.data_ptr(),)
        args += (b._obs.data_ptr(), b._next.data_ptr(), b.act.data_ptr(), b.utter.data_ptr() if b.utter is not None else None,
                 b.rew.data_ptr(), b._done_u8.data_ptr(), b.joint.data_ptr() if joint else None,
                 b.joint_next.data_ptr() if joint else None)
        if ns is not None:
            args += (b.ret.data_ptr(), b.discount.data_ptr(), b.n_used.data_ptr(), b.last.data_ptr())
        _abi.check(getattr(_abi.lib(), name)(*args, _abi.raw_stream(self.world.device)), name)

    def _idx_arg(self, who, idx):
        """idx as gather and update_priorities take it."""
        if not torch.is_tensor(idx) or idx.dtype != torch.int64 or idx.dim() != 1 or idx.numel() < 1 or not idx.is_contiguous() or \
                idx.device != self.world.device:
            raise _abi.MpeError("%s: idx is a contiguous int64 [M] tensor (M >= 1) on the env's device" % who)

    def _sample_args(self, who, M, n_step, gamma, episode_len, episode_phase):
        """The refusals both sample methods begin with -> (M, the checked MpeReplayNStep or None)."""
        M = int(M)
        if M < 1:
            raise _abi.MpeError("%s: M = %d samples (need at least 1)" % (who, M))
        ns = None if n_step is None else self._nstep(who, n_step, gamma, episode_len, episode_phase)
        if self.count < 1:
            raise _abi.MpeError("%s: the buffer is empty (nothing was pushed)" % who)
        return M, ns

    def _draw_arg(self, draw):
        """draw=None: the internal draw counter, advanced here -- so only after a sample method's last refusal."""
        if draw is None:
            draw = self._draw
            self._draw += 1
        return draw

    def gather(self, idx, joint=False, n_step=None, gamma=None, episode_len=0, episode_phase=0):
        """One launch: the transitions idx names (a contiguous int64 [M] tensor on the env's device, slot * steps' worlds + world,
        what ReplayBatch.idx holds) -> a ReplayBatch whose idx IS that tensor; the other tensors are this buffer's per (M, joint)
        and are rewritten by the next gather of that shape.  An index outside [0, steps * worlds) gathers transition 0.
        n_step (with gamma; episode_len, episode_phase: see sample): still one launch -> an NStepReplayBatch, tensors per
        (M, joint, "nstep"); there an index outside the VALID part of the ring, [0, len(self)), gathers transition 0."""
        joint = bool(joint)
        ns = None if n_step is None else self._nstep("ReplayBuffer.gather", n_step, gamma, episode_len, episode_phase)
        self._idx_arg("ReplayBuffer.gather", idx)
        if self.count < 1:
            raise _abi.MpeError("ReplayBuffer.gather: the buffer is empty (nothing was pushed)")
        M = int(idx.numel())
        b = self._batch(M, joint, gathered=True, nstep=ns is not None)
        b.idx = idx
        self._launch(b, M, joint, ns, idx=idx)
        return b

    # ---- taking pushes back (PolicyLoop.capture's warm-up steps) ----------------------------------------------------------------
    def _mark(self, steps):
        """What _rewind needs to take the next `steps` pushes back."""
        return self.head.clone()

    def _rewind(self, mark):
        self.head.copy_(mark)

    def sample(self, M, draw=None, joint=False, n_step=None, gamma=None, episode_len=0, episode_phase=0):
        """One launch: M transitions drawn uniformly with replacement from the valid part of the ring with the draws of (seed,
        draw) -> a ReplayBatch whose tensors are this buffer's per (M, joint) and are rewritten by the next sample of that shape.
        draw=None: an internal draw counter, advanced by the call.
        n_step=n (1..16; gamma is then required): the same draw and still one launch -> an NStepReplayBatch (tensors per
        (M, joint, "nstep")) with the n-step return of every drawn transition; the chain of a transition stops at a step where
        any agent is done, at the newest step in the ring and at the end of an episode.  episode_len / episode_phase say where
        episodes end when nothing in the ring does (PolicyLoop restarts worlds without reporting done); both count PUSHES:
        the world is restarted after every push number t with (t + 1 + episode_phase) % episode_len == 0, episode_phase being
        the episode-step index of push number 0.  For a PolicyLoop(env, pi, episode_len=L) whose first pushed step was loop
        step t0, pass episode_len=L, episode_phase=t0 % L.  episode_len=0: no restarts."""
        joint = bool(joint)
        M, ns = self._sample_args("ReplayBuffer.sample", M, n_step, gamma, episode_len, episode_phase)
        b = self._batch(M, joint, nstep=ns is not None)
        self._launch(b, M, joint, ns, draw=self._draw_arg(draw))
        return b


class PrioritizedReplayBatch(ReplayBatch):
    """A ReplayBatch drawn in proportion to the priorities: also prio [M] float32 (the drawn transitions' priorities as stored),
    total [1] float32 (the sum of all priorities), n_valid [1] int64 (the valid transitions), all on the device."""
    __slots__ = ("prio", "total", "n_valid")

    def weights(self, beta):
        """Importance weights [M]: (n_valid * prio / total) ** -beta, divided by their maximum.  Torch ops on device tensors only,
        so they stay correct inside a captured graph."""
        w = (self.prio * (self.n_valid.to(torch.float32) / self.total)).pow(-float(beta))
        return w / w.max()


class PrioritizedNStepReplayBatch(PrioritizedReplayBatch):
    """A PrioritizedReplayBatch with the n-step outputs of NStepReplayBatch (ret, discount, n_used, last)."""
    __slots__ = ("ret", "discount", "n_used", "last")


class PrioritizedReplayBuffer(ReplayBuffer):
    """A ReplayBuffer with proportional prioritized sampling (Schaul et al. 2016): one float32 priority per transition (leaf
    slot * worlds + world) and a sum tree of fan-out 16 over them in ONE device tensor `tree` (include/mpe_hip.h: the levels one
    after another, level l at floats level_off[l]); pmax [1]: the largest priority ever stored, what a new transition enters at.
    push takes one more launch than ReplayBuffer's, sample two launches (the draw, the gather), update_priorities
    2 + (levels - 1); all capture into a HIP graph.  alpha, eps: update_td's priority is (|td| + eps) ** alpha."""

    _batch_type = PrioritizedReplayBatch
    _nstep_batch_type = PrioritizedNStepReplayBatch

    def __init__(self, env, steps, seed=0, alpha=0.6, eps=1e-6):
        ReplayBuffer.__init__(self, env, steps, seed)
        self.alpha, self.eps = float(alpha), float(eps)
        if not self.alpha >= 0.0:
            raise _abi.MpeError("PrioritizedReplayBuffer: alpha = %r (need alpha >= 0)" % (alpha,))
        if not self.eps > 0.0:
            raise _abi.MpeError("PrioritizedReplayBuffer: eps = %r (need eps > 0: a zero priority is a transition never drawn again)" % (eps,))
        self.n_leaves = self.S * self.B
        self.level_off, self.n_floats = _abi.replay_prio_layout(self.n_leaves)
        self.tree = None

    def _alloc(self):
        if self.tree is not None:
            return
        ReplayBuffer._alloc(self)
        dev = self.world.device
        self.tree = torch.zeros(self.n_floats, dtype=torch.float32, device=dev)
        self.pmax = torch.ones(1, dtype=torch.float32, device=dev)
        self._prio_ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        p = _abi.MpeReplayPrio()
        p.n_leaves, p.tree, p.pmax, p.ticket = self.n_leaves, self.tree.data_ptr(), self.pmax.data_ptr(), self._prio_ticket.data_ptr()
        self._prio = p

    @property
    def priorities(self):
        """The leaves as a [steps, worlds] view of the tree."""
        self._alloc()
        return self.tree[:self.n_leaves].view(self.S, self.B)

    def level(self, l):
        """Level l of the tree (a view): level 0 the leaves, the last level the total."""
        self._alloc()
        n = self.n_leaves
        for _ in range(l):
            n = -(-n // 16)
        return self.tree[self.level_off[l]: self.level_off[l] + n]

    def push(self, obs_n, action, next_obs_n, rew, done):
        """Two launches: the slot's priorities = pmax (and the tree above them), then ReplayBuffer.push."""
        self._alloc()
        args = self._push_args(obs_n, action, next_obs_n, rew, done)      # (refusals come before anything is enqueued)
        _abi.check(_abi.lib().mpe_replay_prio_push(C.byref(self._desc), C.byref(self._prio), _abi.raw_stream(self.world.device)),
                   "mpe_replay_prio_push")
        self._launch_push(args)

    def _batch(self, M, joint, gathered=False, nstep=False):
        b = ReplayBuffer._batch(self, M, joint, gathered, nstep)
        if not gathered and getattr(b, "prio", None) is None:
            dev = self.world.device
            b.prio = torch.zeros(M, dtype=torch.float32, device=dev)
            b.total = torch.zeros(1, dtype=torch.float32, device=dev)
            b.n_valid = torch.zeros(1, dtype=torch.int64, device=dev)
        return b

    def sample(self, M, draw=None, joint=False, u24=None, n_step=None, gamma=None, episode_len=0, episode_phase=0):
        """Two launches: M transitions drawn in proportion to their priorities (stratified: sample k from the k-th M-th of the
        total, with the draws of (seed, draw)), then every field gathered for them -> a PrioritizedReplayBatch whose tensors are
        this buffer's per (M, joint).  draw=None: an internal draw counter, advanced by the call.  u24: an int32 [M] device tensor
        whose low 24 bits replace the drawn bits (tests, quasi-random sequences).  n_step (with gamma; episode_len,
        episode_phase: ReplayBuffer.sample): the same draw, then mpe_replay_gather_nstep in place of the gather -> a
        PrioritizedNStepReplayBatch; update_td(batch.idx, td) as before."""
        joint = bool(joint)
        M, ns = self._sample_args("PrioritizedReplayBuffer.sample", M, n_step, gamma, episode_len, episode_phase)
        if u24 is not None and (not torch.is_tensor(u24) or u24.dtype != torch.int32 or tuple(u24.shape) != (M,) or
                                not u24.is_contiguous() or u24.device != self.world.device):
            raise _abi.MpeError("PrioritizedReplayBuffer.sample: u24 is a contiguous int32 [%d] tensor on the env's device" % M)
        draw = self._draw_arg(draw)
        b = self._batch(M, joint, nstep=ns is not None)
        stream = _abi.raw_stream(self.world.device)
        _abi.check(_abi.lib().mpe_replay_prio_draw(
            C.byref(self._desc), C.byref(self._prio), M, int(draw) & (2 ** 64 - 1), u24.data_ptr() if u24 is not None else None,
            b.idx.data_ptr(), b.prio.data_ptr(), b.total.data_ptr(), b.n_valid.data_ptr(), stream), "mpe_replay_prio_draw")
        self._launch(b, M, joint, ns, idx=b.idx)
        return b

    def update_priorities(self, idx, priority):
        """Transition idx[k] takes priority[k] (clamped to [2^-40, 2^40], a NaN to 2^-40; the largest where several k name one
        transition); an idx outside the ring, or one that was never pushed, is ignored.  idx: int64 [M], priority: float32 [M],
        contiguous, on the env's device.  2 + (levels - 1) launches."""
        self._alloc()
        dev = self.world.device
        self._idx_arg("PrioritizedReplayBuffer.update_priorities", idx)
        if not torch.is_tensor(priority) or priority.dtype != torch.float32 or priority.shape != idx.shape or \
                not priority.is_contiguous() or priority.device != dev:
            raise _abi.MpeError("PrioritizedReplayBuffer.update_priorities: priority is a contiguous float32 [%d] tensor on the env's device"
                                % idx.numel())
        _abi.check(_abi.lib().mpe_replay_prio_update(C.byref(self._desc), C.byref(self._prio), int(idx.numel()), idx.data_ptr(),
                                                     priority.data_ptr(), _abi.raw_stream(dev)), "mpe_replay_prio_update")

    def update_td(self, idx, td):
        """update_priorities(idx, (|td| + eps) ** alpha): the power runs in torch, the kernels hold no transcendental."""
        if not torch.is_tensor(td) or not td.is_floating_point():
            raise _abi.MpeError("PrioritizedReplayBuffer.update_td: td is a floating-point tensor of idx's shape")
        self.update_priorities(idx, ((td.to(torch.float32).abs() + self.eps) ** self.alpha).contiguous())

    # ---- taking pushes back: the leaves of the slots the pushes will write, pmax, and the tree above them -----------------------
    def _mark(self, steps):
        self._alloc()
        slots = sorted(set((self.count + k) % self.S for k in range(int(steps))))
        return (ReplayBuffer._mark(self, steps), self.pmax.clone(), [(s, self.priorities[s].clone()) for s in slots])

    def _rewind(self, mark):
        head, pmax, leaves = mark
        ReplayBuffer._rewind(self, head)
        self.pmax.copy_(pmax)
        stream = _abi.raw_stream(self.world.device)
        for s, row in leaves:
            self.priorities[s].copy_(row)
            _abi.check(_abi.lib().mpe_replay_prio_repair(C.byref(self._desc), C.byref(self._prio), s * self.B, self.B, stream),
                       "mpe_replay_prio_repair")
