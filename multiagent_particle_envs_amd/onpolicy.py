"""The on-policy half of a learner on the device: `Values` evaluates one MLP critic per agent on the agents' OWN observations (or,
centralised, on all of them) in ONE launch (mpe_critic_q with per-agent pointers and widths), `PolicyLoop.run(T, values=V)` records
V along the closed loop -- of the observation every step was decided on, and of the output observation of every segment-ending
step --, and `gae` turns the recorded trajectory into advantages and returns in ONE launch (mpe_gae: THE GAE RULE of
include/mpe_hip.h).  `Minibatches` then hands the update loop its shuffled minibatches: the advantage statistics once
per trajectory (mpe_adv_stats) and ONE launch per minibatch that draws its rows from a keyed permutation of the (step, world) pairs
and gathers every field of every agent, the advantages normalised (mpe_onpolicy_batch).  `PpoLoss` is the loss
head on such a minibatch: the clipped surrogate, the value loss, the entropy and their gradients with respect to the logits and the
values in two launches for all agents (mpe_ppo_loss).  The networks' forward and backward passes and the optimiser
stay in torch autograd.

    V = Values(env, critic_modules)
    traj = loop.run(25, values=V)               # + traj.obs_in, traj.val [T,A,B], traj.boot [K,A,B]
    g = gae(traj, gamma=0.99, lam=0.95)         # g.adv, g.ret [T,A,B]
    for batch in Minibatches(traj, g, 4096).epoch(e): ...      # batch.obs_n[i] [M,D_i], batch.act, .logp, .adv, .ret, .val [A,M]
        loss = PpoLoss(env)(logits_n, values_n, batch)         # loss.backward(): dL/dlogits, dL/dvalues from the same two launches
"""
import ctypes as C
import math

import torch

from . import _abi
from .netset import Cache, Generations, NetSet, check_tensor
from .policy import _obs_blocks


class Values(NetSet):
    """Per-agent MLP state-value critics: `modules` is one nn.Sequential per agent, or one module every agent shares (Critics'
    layer rules: Linear layers with ReLU / Tanh between them, at most 3, hidden widths <= 64, float32, ONE output).  Decentralised
    (the default) critic i's first Linear takes agent i's observation width D_i and reads agent i's own [M, D_i] block, zero-copy;
    centralised=True: every critic takes all observations side by side, sum D_i <= MPE_ACTOR_MAX_INPUT inputs, from one [M, sum D_i]
    tensor of this object's (one torch.cat per call).  The weights are packed again at every call unless freeze() was called."""
    who, noun = "Values", "critics"

    def __init__(self, env, modules, centralised=False):
        self.centralised = bool(centralised)
        NetSet.__init__(self, env, modules)
        self._out, self._cat, self._ptrs = Cache(), Cache(), Cache(64)

    def _widths(self):
        total = sum(self.obs_widths)
        if self.centralised and total > _abi.MPE_ACTOR_MAX_INPUT:
            raise _abi.MpeError("Values(centralised=True): the observations together have %d floats, a critic's input is at most "
                                "MPE_ACTOR_MAX_INPUT = %d wide" % (total, _abi.MPE_ACTOR_MAX_INPUT))
        self.in_widths, self.n_out = [total] * self.A if self.centralised else list(self.obs_widths), [1] * self.A

    def _input_refusal(self, i, n, D):
        return "Values: agent %d's critic takes %d inputs, %s %d" % (
            i, n, "the observations together have" if self.centralised else "its observation has", D)

    def _inputs(self, obs_n):
        """-> (M, the HOST array of A device pointers, what keeps them alive); checked once per distinct set of blocks"""
        def make(ptrs):
            if not self.centralised:
                return (C.c_void_p * self.A)(*ptrs), None
            M = int(obs_n[0].shape[0])
            cat = self._cat.get(M, lambda: torch.zeros((M, self.in_widths[0]), dtype=torch.float32, device=self.world.device))
            return (C.c_void_p * self.A)(*([cat.data_ptr()] * self.A)), cat
        M, (ptrs, cat) = _obs_blocks(self, obs_n, "Values.v", make)
        if cat is not None:
            torch.cat(list(obs_n), dim=1, out=cat)
        return M, ptrs

    def v(self, obs_n, out=None, _packed=None):
        """One launch: critic i on obs_n[i] (a list of [M, D_i] device tensors: env.step's own output qualifies; centralised: every
        critic on all of them) -> v [A, M] float32 (this object's tensor per M, or `out`).  (_packed: the pair to read in place of
        packed().)"""
        M, ptrs = self._inputs(obs_n)
        dev = self.world.device
        if out is None:
            out = self._out.get(M, lambda: torch.zeros((self.A, M), dtype=torch.float32, device=dev))
        else:
            check_tensor("Values.v", out, "out", [(self.A, M)], "the env's device", dev)
        wts, aset = _packed if _packed is not None else self.packed()
        _abi.check(_abi.lib().mpe_critic_q(C.byref(aset), ptrs, M, out.data_ptr(), None, None, _abi.raw_stream(dev)), "mpe_critic_q")
        del wts      # (stream-ordered: the caching allocator reuses the block only behind the launch)
        return out

    def train_forward(self, obs_n, packed):
        """The forward Trainable runs, on the packed pair it hands to the backward: v -> (M, v[i] [M] per agent, the input rows: the
        side-by-side tensor for every agent where centralised)."""
        v = self.v(obs_n, _packed=packed)
        M = int(v.shape[1])
        return M, [v[i].clone() for i in range(self.A)], [self._cat[M]] * self.A if self.centralised else list(obs_n)

    def reference(self, obs_n):
        """The fp64 torch forward pass, on whatever device the modules and obs_n are -> [A, M] float64."""
        import copy
        out = []
        for i, m in enumerate(self.modules):
            m = copy.deepcopy(m).double()
            dev = next(m.parameters()).device
            x = torch.cat([torch.as_tensor(o).to(dev).double() for o in obs_n], dim=1) if self.centralised else \
                torch.as_tensor(obs_n[i]).to(dev).double()
            with torch.no_grad():
                out.append(m(x)[:, 0])
        return torch.stack(out)


def segments(T, episode_len=0, episode_phase=0):
    """K of the GAE rule: the steps of a T-step trajectory that end a segment (mpe_gae_segments, host only)."""
    K = _abi.lib().mpe_gae_segments(int(T), int(episode_len), int(episode_phase))
    if K < 0:
        _abi.check(int(K), "mpe_gae_segments")
    return int(K)


class _ValueRecord(object):
    """What PolicyLoop.run(T, values=V) adds to its LoopTrajectory, and the two hooks PolicyLoop.step calls: decided(k) in front
    of the decision of trajectory step k, stepped(k, obs_n) behind its env.step.  T + K launches and T flat copies in all."""

    def __init__(self, loop, traj, values):
        if not isinstance(values, Values) or values.env is not loop.env:
            raise _abi.MpeError("PolicyLoop.run: values is a Values(env, modules) built for this loop's env")
        env, w = loop.env, loop.world
        off, A, B, T, dev = env._obs_off, values.A, w.batch_size, traj.T, w.device
        if T < 1:
            raise _abi.MpeError("PolicyLoop.run(values=): T = %d (the returns of an empty trajectory are not defined)" % T)
        L = loop.episode_len
        self.loop, self.traj, self.values, self.k_boot = loop, traj, values, 0
        traj.episode_len, traj.episode_phase = L, (loop.t % L if L else 0)
        K = segments(T, L, traj.episode_phase)
        traj.obs_in_flat = torch.zeros((T, int(off[-1]) * B), dtype=torch.float32, device=dev)
        traj.obs_in = [[traj.obs_in_flat[t, off[i] * B: off[i + 1] * B].view(B, off[i + 1] - off[i]) for i in range(A)] for t in range(T)]
        traj.val = torch.zeros((T, A, B), dtype=torch.float32, device=dev)
        traj.boot = torch.zeros((K, A, B), dtype=torch.float32, device=dev)

    def decided(self, k):
        loop, traj = self.loop, self.traj
        first = loop.obs_n[0].data_ptr()
        src = next((s for s in loop.env._sets if s.obs_n[0].data_ptr() == first), None)
        if src is None:
            raise _abi.MpeError("PolicyLoop.run(values=): the observation to decide on is not one of the env's output sets")
        traj.obs_in_flat[k].copy_(src.obs)
        self.values.v(loop.obs_n, out=traj.val[k])

    def stepped(self, k, obs_n):
        loop, traj = self.loop, self.traj
        L = loop.episode_len
        if k == traj.T - 1 or (L and loop.t % L == 0):      # (loop.t is already the next step's number)
            self.values.v(obs_n, out=traj.boot[self.k_boot])
            self.k_boot += 1


class GaeResult(object):
    """adv, ret [T, A, B] float32: what gae / gae_tensors wrote."""
    __slots__ = ("adv", "ret")

    def __init__(self, adv, ret):
        self.adv, self.ret = adv, ret


def gae_tensors(rew, done, val, boot, gamma, lam, episode_len=0, episode_phase=0, out=None):
    """GAE(lambda) by THE GAE RULE in one launch, no host synchronisation (captures into a HIP graph).  rew, val [T, A, B] float32;
    done [T, A, B] bool or uint8; boot [K, A, B] float32 with K = segments(T, episode_len, episode_phase): V of the output
    observation of every segment-ending step.  out: a GaeResult to rewrite.  -> GaeResult(adv, ret)."""
    who = "gae_tensors"
    check_tensor(who, rew, "rew", None, "a GPU", text="[T, A, B]")
    if rew.dim() != 3:
        raise _abi.MpeError("%s: rew is a contiguous float32 [T, A, B] tensor on a GPU" % who)
    T, A, B = (int(n) for n in rew.shape)
    dev = rew.device
    if not math.isfinite(float(gamma)) or not math.isfinite(float(lam)):
        raise _abi.MpeError("%s: gamma = %r, lam = %r (both finite)" % (who, gamma, lam))
    K = segments(T, episode_len, episode_phase)
    check_tensor(who, done, "done", [(T, A, B)], "rew's device", dev, (torch.bool, torch.uint8))
    check_tensor(who, val, "val", [(T, A, B)], "rew's device", dev)
    check_tensor(who, boot, "boot", [(K, A, B)], "rew's device", dev)
    if out is None:
        out = GaeResult(torch.empty_like(rew), torch.empty_like(rew))
    else:
        if not isinstance(out, GaeResult):
            raise _abi.MpeError("%s: out is a GaeResult (what an earlier call returned)" % who)
        check_tensor(who, out.adv, "out.adv", [(T, A, B)], "rew's device", dev)
        check_tensor(who, out.ret, "out.ret", [(T, A, B)], "rew's device", dev)
    if not rew.is_cuda:
        raise _abi.MpeError("%s: rew is on %s (the tensors live on a GPU: there is no CPU path)" % (who, dev))
    g = _abi.MpeGae()
    g.gamma, g.lambda_, g.episode_len, g.episode_phase = float(gamma), float(lam), int(episode_len), int(episode_phase)
    d8 = done.view(torch.uint8) if done.dtype == torch.bool else done
    _abi.check(_abi.lib().mpe_gae(C.byref(g), T, A, B, rew.data_ptr(), d8.data_ptr(), val.data_ptr(), boot.data_ptr(),
                                  out.adv.data_ptr(), out.ret.data_ptr(), _abi.raw_stream(dev)), "mpe_gae")
    return out


def gae(traj, gamma, lam, out=None):
    """gae_tensors on what PolicyLoop.run(T, values=V) recorded (its rew, done, val, boot, episode_len and episode_phase)."""
    if getattr(traj, "val", None) is None or getattr(traj, "boot", None) is None:
        raise _abi.MpeError("gae: traj holds no values: record it with PolicyLoop.run(T, values=Values(env, modules))")
    return gae_tensors(traj.rew, traj.done, traj.val, traj.boot, gamma, lam, traj.episode_len, traj.episode_phase, out)


# ---- minibatches: advantage statistics and the shuffled one-launch gather (mpe_adv_stats / mpe_onpolicy_batch) ----
def perm(N, seed, epoch, q):
    """perm(q) of THE MINIBATCH RULE for a trajectory of N = T * B (step, world) pairs (mpe_onpolicy_perm, host only)."""
    j = _abi.lib().mpe_onpolicy_perm(int(N), int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1), int(q))
    if j < 0:
        _abi.check(int(j), "mpe_onpolicy_perm")
    return int(j)


def _stats_work(T, A, B, dev, cache=Cache()):
    """the float64 workspace of mpe_adv_stats for one shape on one device (every entry is written before it is read)"""
    n = _abi.lib().mpe_adv_stats_work(T, A, B)
    if n < 0:
        _abi.check(int(n), "mpe_adv_stats_work")
    return cache.get((T, A, B, dev), lambda: torch.empty((max(int(n), 1),), dtype=torch.float64, device=dev))


def adv_stats(g_or_adv, eps=1e-8, out=None):
    """Per-agent advantage mean and 1 / (std + eps) by THE ADVANTAGE STATISTICS RULE: two launches, no host synchronisation.
    g_or_adv: a GaeResult or an adv [T, A, B] float32 tensor on a GPU.  -> stats [A, 2] float32 (`out`, or a new tensor)."""
    who = "adv_stats"
    adv = g_or_adv.adv if isinstance(g_or_adv, GaeResult) else g_or_adv
    if not torch.is_tensor(adv) or adv.dtype != torch.float32 or adv.dim() != 3 or not adv.is_contiguous():
        raise _abi.MpeError("%s: adv is a contiguous float32 [T, A, B] tensor on a GPU" % who)
    T, A, B = (int(n) for n in adv.shape)
    dev = adv.device
    if not math.isfinite(float(eps)) or float(eps) < 0:
        raise _abi.MpeError("%s: eps = %r (a finite value >= 0)" % (who, eps))
    if out is None:
        out = torch.empty((A, 2), dtype=torch.float32, device=dev)
    else:
        check_tensor(who, out, "out", [(A, 2)], "adv's device", dev)
    if not adv.is_cuda:
        raise _abi.MpeError("%s: adv is on %s (the tensors live on a GPU: there is no CPU path)" % (who, dev))
    work = _stats_work(T, A, B, dev)
    _abi.check(_abi.lib().mpe_adv_stats(T, A, B, adv.data_ptr(), float(eps), work.data_ptr(), out.data_ptr(), _abi.raw_stream(dev)),
               "mpe_adv_stats")
    return out


class OnPolicyBatch(object):
    """One minibatch of M rows, every tensor this object's Minibatches owns (rewritten by the next batch() of the same M):
    idx [M] int64 (t * B + b), obs_n: A views [M, D_i] of the flat tensor `obs`, act [A, M, 5], utter [A, M, dim_c] or None, logp
    [A, M] or None, adv, ret, val [A, M], joint_obs [M, sum D_i] or None."""
    __slots__ = ("M", "B", "idx", "obs", "obs_n", "act", "utter", "logp", "adv", "ret", "val", "joint_obs")

    @property
    def t(self):
        return torch.div(self.idx, self.B, rounding_mode="floor")

    @property
    def b(self):
        return self.idx % self.B


class Minibatches(object):
    """Shuffled minibatches of a recorded trajectory by THE MINIBATCH RULE: batch(epoch, k) is ONE launch that draws rows
    k * M .. of the (seed, epoch) permutation of the T * B (step, world) pairs and gathers every field of every agent for them.
    traj: what PolicyLoop.run(T, values=V) recorded (obs_in_flat, act, utter, logp, val); g: gae's GaeResult.  normalise: adv is
    written (adv - mean) * rstd, the statistics (adv_stats(g, eps)) computed once here -- restats() after g.adv was rewritten.
    joint: also joint_obs [M, sum D_i], the input of Values(centralised=True).  epoch_counter: a device uint64 tensor of one
    element added to every batch's epoch by the launch itself (a captured graph reshuffles when the caller bumps it).
    No host synchronisation: {gae, adv_stats, batch} captures into a HIP graph."""

    def __init__(self, traj, g, M, seed=0, normalise=True, joint=False, eps=1e-8, epoch_counter=None):
        who = "Minibatches"
        if not isinstance(g, GaeResult):
            raise _abi.MpeError("%s: g is a GaeResult (what gae returned)" % who)
        flat = getattr(traj, "obs_in_flat", None)
        if flat is None or getattr(traj, "val", None) is None:
            raise _abi.MpeError("%s: traj holds no decision observations: record it with PolicyLoop.run(T, values=Values(env, modules))" % who)
        check_tensor(who, g.adv, "g.adv", None, "a GPU", text="[T, A, B]")
        if g.adv.dim() != 3:
            raise _abi.MpeError("%s: g.adv is a contiguous float32 [T, A, B] tensor on a GPU" % who)
        T, A, B = (int(n) for n in g.adv.shape)
        dev = g.adv.device

        def chk(x, name, shape):
            check_tensor(who, x, name, [tuple(shape)], "g.adv's device", dev)
        chk(g.ret, "g.ret", (T, A, B))
        chk(traj.val, "traj.val", (T, A, B))
        chk(traj.act, "traj.act", (T, A, B, _abi.MPE_ACTION_DIM))
        widths = getattr(traj, "obs_widths", None)
        if widths is None:
            widths = [int(o.shape[1]) for o in traj.obs_in[0]]
        widths = [int(d) for d in widths]
        if len(widths) != A:
            raise _abi.MpeError("%s: %d observation widths for %d agents" % (who, len(widths), A))
        chk(flat, "traj.obs_in_flat", (T, sum(widths) * B))
        utter, logp = getattr(traj, "utter", None), getattr(traj, "logp", None)
        dim_c = 0
        if utter is not None:
            if not torch.is_tensor(utter) or utter.dim() != 4:
                raise _abi.MpeError("%s: traj.utter is a contiguous float32 [T, A, B, dim_c] tensor on g.adv's device" % who)
            dim_c = int(utter.shape[3])
            chk(utter, "traj.utter", (T, A, B, dim_c))
        if logp is not None:
            chk(logp, "traj.logp", (T, A, B))
        if int(M) < 1:
            raise _abi.MpeError("%s: M = %r rows (need at least 1)" % (who, M))
        if epoch_counter is not None and (not torch.is_tensor(epoch_counter) or epoch_counter.dtype not in (torch.uint64, torch.int64) or
                                          epoch_counter.numel() != 1 or epoch_counter.device != dev):
            raise _abi.MpeError("%s: epoch_counter is a uint64 (or int64) tensor of one element on g.adv's device" % who)
        if not g.adv.is_cuda:
            raise _abi.MpeError("%s: g.adv is on %s (the tensors live on a GPU: there is no CPU path)" % (who, dev))
        self.traj, self.g, self.T, self.A, self.B, self.N, self.M = traj, g, T, A, B, T * B, int(M)
        self.widths, self.dim_c, self.device = widths, dim_c, dev
        self.seed, self.joint, self.eps, self.epoch_counter = int(seed) & (2 ** 64 - 1), bool(joint), float(eps), epoch_counter
        self._keep = (flat, traj.act, utter, logp, traj.val)
        tr = self._traj = _abi.MpeOnPolicyTraj()
        tr.T, tr.A, tr.B, tr.dim_c = T, A, B, dim_c
        for i, d in enumerate(widths):
            tr.obs_width[i] = d
        tr.obs_in, tr.act, tr.utter = flat.data_ptr(), traj.act.data_ptr(), utter.data_ptr() if dim_c else None
        tr.logp, tr.adv, tr.ret, tr.val = logp.data_ptr() if logp is not None else None, g.adv.data_ptr(), g.ret.data_ptr(), traj.val.data_ptr()
        self.stats = torch.empty((A, 2), dtype=torch.float32, device=dev) if normalise else None
        self._out = Cache()
        if normalise:
            self.restats()

    def restats(self):
        """The statistics of g.adv as it stands now (two launches, into this object's `stats`)."""
        if self.stats is None:
            raise _abi.MpeError("Minibatches.restats: built with normalise=False")
        return adv_stats(self.g, self.eps, out=self.stats)

    def __len__(self):
        return (self.N + self.M - 1) // self.M

    def _outputs(self, M):
        def make():
            A, dev, f = self.A, self.device, torch.float32
            o = OnPolicyBatch()
            o.M, o.B = M, self.B
            o.idx = torch.zeros((M,), dtype=torch.int64, device=dev)
            o.obs = torch.zeros((sum(self.widths) * M,), dtype=f, device=dev)
            off, o.obs_n = 0, []
            for d in self.widths:
                o.obs_n.append(o.obs[off * M:(off + d) * M].view(M, d))
                off += d
            o.act = torch.zeros((A, M, _abi.MPE_ACTION_DIM), dtype=f, device=dev)
            o.utter = torch.zeros((A, M, self.dim_c), dtype=f, device=dev) if self.dim_c else None
            o.logp = torch.zeros((A, M), dtype=f, device=dev) if self._keep[3] is not None else None
            o.adv, o.ret, o.val = (torch.zeros((A, M), dtype=f, device=dev) for _ in range(3))
            o.joint_obs = torch.zeros((M, sum(self.widths)), dtype=f, device=dev) if self.joint else None
            return o
        return self._out.get(M, make)

    def batch(self, epoch, k, M=None):
        """Minibatch k of `epoch`: rows k * self.M .. of the permutation (M rows; the default: self.M, or what is left of the
        trajectory behind k * self.M).  One launch.  -> OnPolicyBatch."""
        first = int(k) * self.M
        if int(k) < 0 or first >= self.N:
            raise _abi.MpeError("Minibatches.batch: k = %r (an epoch has %d minibatches of %d rows)" % (k, len(self), self.M))
        M = min(self.M, self.N - first) if M is None else int(M)
        o = self._outputs(M)
        ptr = lambda x: x.data_ptr() if x is not None else None      # noqa: E731
        _abi.check(_abi.lib().mpe_onpolicy_batch(
            C.byref(self._traj), M, first, self.seed, int(epoch) & (2 ** 64 - 1), ptr(self.epoch_counter), ptr(self.stats), o.idx.data_ptr(),
            o.obs.data_ptr(), o.act.data_ptr(), ptr(o.utter), ptr(o.logp), o.adv.data_ptr(), o.ret.data_ptr(), o.val.data_ptr(),
            ptr(o.joint_obs), _abi.raw_stream(self.device)), "mpe_onpolicy_batch")
        return o

    def epoch(self, e, drop_last=False):
        """Iterates the ceil(N / M) minibatches of epoch e (the last one short unless drop_last); together they hold every (step,
        world) pair once."""
        for k in range(len(self)):
            if drop_last and (k + 1) * self.M > self.N:
                return
            yield self.batch(e, k)


# ---- the PPO loss head: the clipped surrogate and its gradients in two launches (mpe_ppo_loss) ----------------------
class PpoLossResult(object):
    """What ppo_loss_tensors wrote: loss [1]; stats [A, 8] (per agent the means of the surrogate, the value loss, the entropy, the
    approximate KL (ratio - 1) - log ratio, the clipped rows and the ratio, then L_i, then 0); dlogits_n: A views [M, n_out_i] and
    dvalues [A, M] (None for a policy-only loss) of ONE flat float32 buffer `grads`, already scaled by 1 / M and the coefficients;
    rows [A, M, 4] (logp, surr, vl, ent) or None."""
    __slots__ = ("M", "n_out", "loss", "stats", "grads", "dlogits_n", "dvalues", "rows", "work")

    STATS = ("surrogate", "value_loss", "entropy", "approx_kl", "clip_fraction", "ratio", "loss", "reserved")


def _ppo_result(n_out, M, values, rows, dev):
    """the buffers of one (heads, M) on one device: every agent's dlogits block starts at a multiple of 4 floats of `grads`"""
    r = PpoLossResult()
    A, f = len(n_out), torch.float32
    off, at = [], 0
    for n in n_out:
        off.append(at)
        at += (M * n + 3) // 4 * 4
    r.M, r.n_out = M, list(n_out)
    r.grads = torch.zeros((at + (A * M if values else 0),), dtype=f, device=dev)
    r.dlogits_n = [r.grads[o:o + M * n].view(M, n) for o, n in zip(off, n_out)]
    r.dvalues = r.grads[at:at + A * M].view(A, M) if values else None
    r.rows = torch.zeros((A, M, 4), dtype=f, device=dev) if rows else None
    r.stats = torch.zeros((A, 8), dtype=f, device=dev)
    r.loss = torch.zeros((1,), dtype=f, device=dev)
    n = _abi.lib().mpe_ppo_loss_work(A, M)
    if n < 0:
        _abi.check(int(n), "mpe_ppo_loss_work")
    r.work = torch.empty((max(int(n), 1),), dtype=torch.float64, device=dev)
    return r


def ppo_loss_tensors(logits_n, values_n, act, utter, logp_old, adv, ret, val_old, movable, speaks, dim_c, clip=0.2, value_clip=None,
                     vf_coef=0.5, ent_coef=0.0, rows=False, out=None):
    """THE PPO LOSS RULE in two launches for every agent, no host synchronisation (captures into a HIP graph): the clipped
    surrogate, the (clipped) value loss and the entropy of a minibatch, and their gradients.  logits_n[i]: agent i's [M, n_out_i]
    float32 logits, n_out_i = 5 * movable[i] + dim_c * speaks[i]; values_n[i]: [M] or [M, 1], or values_n=None (policy only: ret and
    val_old are not read); act [A, M, 5], utter [A, M, dim_c] (None without speakers), logp_old, adv, ret, val_old [A, M]: an
    OnPolicyBatch's own tensors.  value_clip=None: the plain squared error.  rows=True: also the per-row logp, surr, vl, ent.
    out: a PpoLossResult to rewrite.  -> PpoLossResult."""
    who = "ppo_loss_tensors"
    if not isinstance(logits_n, (list, tuple)) or not 1 <= len(logits_n) <= _abi.MPE_ACTOR_MAX_AGENTS:
        raise _abi.MpeError("%s: logits_n is a list of 1..MPE_ACTOR_MAX_AGENTS = %d tensors, one per agent" % (who, _abi.MPE_ACTOR_MAX_AGENTS))
    A = len(logits_n)
    movable, speaks, dim_c = [bool(m) for m in movable], [bool(s) for s in speaks], int(dim_c)
    if len(movable) != A or len(speaks) != A:
        raise _abi.MpeError("%s: %d movable and %d speaks flags for %d agents" % (who, len(movable), len(speaks), A))
    if not 0 <= dim_c <= _abi.MPE_ACTOR_MAX_OUT:
        raise _abi.MpeError("%s: dim_c = %d (0..MPE_ACTOR_MAX_OUT = %d)" % (who, dim_c, _abi.MPE_ACTOR_MAX_OUT))
    speaks = [s and dim_c > 0 for s in speaks]
    n_out = [_abi.MPE_ACTION_DIM * m + dim_c * s for m, s in zip(movable, speaks)]
    for i, n in enumerate(n_out):
        if not 1 <= n <= _abi.MPE_ACTOR_MAX_OUT:
            raise _abi.MpeError("%s: agent %d has %d logits (5 * movable + dim_c * speaks), need 1..MPE_ACTOR_MAX_OUT = %d"
                                % (who, i, n, _abi.MPE_ACTOR_MAX_OUT))
    z0 = logits_n[0]
    if not torch.is_tensor(z0) or z0.dim() != 2:
        raise _abi.MpeError("%s: logits_n[0] is a contiguous float32 [M, %d] tensor on a GPU" % (who, n_out[0]))
    M, dev = int(z0.shape[0]), z0.device

    def chk(x, name, shapes):
        check_tensor(who, x, name, shapes, "logits_n[0]'s device", dev)
    for i, z in enumerate(logits_n):
        chk(z, "logits_n[%d]" % i, [(M, n_out[i])])
    if values_n is not None:
        if not isinstance(values_n, (list, tuple)) or len(values_n) != A:
            raise _abi.MpeError("%s: values_n is a list of %d tensors, one per agent, or None" % (who, A))
        for i, v in enumerate(values_n):
            chk(v, "values_n[%d]" % i, [(M,), (M, 1)])
    if any(movable):
        chk(act, "act", [(A, M, _abi.MPE_ACTION_DIM)])
    if any(speaks):
        chk(utter, "utter", [(A, M, dim_c)])
    chk(logp_old, "logp_old", [(A, M)])
    chk(adv, "adv", [(A, M)])
    if values_n is not None:
        chk(ret, "ret", [(A, M)])
        chk(val_old, "val_old", [(A, M)])
    if not math.isfinite(float(clip)) or float(clip) < 0:
        raise _abi.MpeError("%s: clip = %r (a finite value >= 0)" % (who, clip))
    if not math.isfinite(float(vf_coef)) or not math.isfinite(float(ent_coef)):
        raise _abi.MpeError("%s: vf_coef = %r, ent_coef = %r (both finite)" % (who, vf_coef, ent_coef))
    if value_clip is not None and (not math.isfinite(float(value_clip)) or float(value_clip) < 0):
        raise _abi.MpeError("%s: value_clip = %r (None, or a finite value >= 0)" % (who, value_clip))
    if out is not None:
        if not isinstance(out, PpoLossResult) or out.M != M or out.n_out != n_out or (out.dvalues is None) != (values_n is None) or \
                out.grads.device != dev or (rows and out.rows is None):
            raise _abi.MpeError("%s: out is a PpoLossResult of the same heads, M = %d, values and rows (what an earlier call returned)" % (who, M))
    n = _abi.lib().mpe_ppo_loss_work(A, M)      # (host only: the size check)
    if n < 0:
        _abi.check(int(n), "mpe_ppo_loss_work")
    if not z0.is_cuda:
        raise _abi.MpeError("%s: logits_n[0] is on %s (the tensors live on a GPU: there is no CPU path)" % (who, dev))
    if out is None:
        out = _ppo_result(n_out, M, values_n is not None, rows, dev)
    cfg = _abi.MpePpoLoss()
    cfg.n_agents, cfg.dim_c = A, dim_c
    for i in range(A):
        cfg.movable[i], cfg.speaks[i] = int(movable[i]), int(speaks[i])
    cfg.clip, cfg.value_clip, cfg.vf_coef, cfg.ent_coef = float(clip), -1.0 if value_clip is None else float(value_clip), float(vf_coef), float(ent_coef)
    ptr = lambda x: x.data_ptr() if x is not None else None      # noqa: E731
    zp = (C.c_void_p * A)(*[z.data_ptr() for z in logits_n])
    vp = (C.c_void_p * A)(*[v.data_ptr() for v in values_n]) if values_n is not None else None
    gp = (C.c_void_p * A)(*[g.data_ptr() for g in out.dlogits_n])
    use_rows = out.rows if rows else None
    _abi.check(_abi.lib().mpe_ppo_loss(C.byref(cfg), zp, vp, M, ptr(act) if any(movable) else None, ptr(utter) if any(speaks) else None,
                                       logp_old.data_ptr(), adv.data_ptr(), ptr(ret) if vp is not None else None,
                                       ptr(val_old) if vp is not None else None, gp, ptr(out.dvalues), ptr(use_rows), out.work.data_ptr(),
                                       out.stats.data_ptr(), out.loss.data_ptr(), _abi.raw_stream(dev)), "mpe_ppo_loss")
    return out


class _PpoLossFn(torch.autograd.Function):
    """forward: the two launches; backward: grad_output * the gradients the forward wrote (ONE multiply over the flat buffer)"""

    @staticmethod
    def forward(ctx, head, batch, n_values, *tensors):
        A = head.A
        logits_n = [t.detach() for t in tensors[:A]]
        values_n = [t.detach() for t in tensors[A:]] if n_values else None
        M = int(logits_n[0].shape[0]) if torch.is_tensor(logits_n[0]) and logits_n[0].dim() == 2 else -1
        key = (M, n_values > 0, logits_n[0].device if torch.is_tensor(logits_n[0]) else None)
        res = ppo_loss_tensors(logits_n, values_n, batch.act, batch.utter, batch.logp, batch.adv, batch.ret, batch.val, head.movable,
                               head.speaks, head.dim_c, head.clip, head.value_clip, head.vf_coef, head.ent_coef, out=head._out.get(key))
        head._out.get(key, lambda: res)
        ctx.res, ctx.shapes, ctx.owner = res, [tuple(t.shape) for t in tensors], (head, key, head._generation.next(key))
        head.last = res
        return res.loss.view(())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        res = ctx.res
        head, key, generation = ctx.owner
        if head._generation.stale(key, generation) or head._out.get(key) is not res:
            raise _abi.MpeError("PpoLoss: backward() of a loss whose buffers a later forward with the same M has rewritten (the "
                                "buffers are cached per M: call backward() before the next forward)")
        A = len(res.dlogits_n)
        g = grad_output * res.grads      # out of place: the buffer is rewritten by the next forward of the same M
        at, grads = 0, []
        for n in res.n_out:
            grads.append(g[at:at + res.M * n].view(res.M, n))
            at += (res.M * n + 3) // 4 * 4
        for i, shape in enumerate(ctx.shapes[A:]):
            grads.append(g[at + i * res.M:at + (i + 1) * res.M].view(shape))
        return (None, None, None) + tuple(grads)


class PpoLoss(object):
    """The PPO loss head behind torch autograd: loss = PpoLoss(env, clip, value_clip, vf_coef, ent_coef)(logits_n, values_n, batch).
    The heads (movable, speaks, dim_c) are the env's, as Actors takes them.  logits_n[i]: module i's [M, n_out_i] output;
    values_n[i]: [M] or [M, 1], or values_n=None; batch: an OnPolicyBatch (its act, utter, logp, adv, ret, val).  The forward is
    mpe_ppo_loss's two launches for all agents, the backward ONE multiply of grad_output with the gradients the forward wrote; no
    host read anywhere.  loss is the sum over the agents of -mean surr + vf_coef * mean vl - ent_coef * mean ent; loss.stats [A, 8]
    (device) carries PpoLossResult.STATS.  The buffers are cached per M: the loss, its stats and the gradients of one call are
    rewritten by the next call with the same M, so call backward() (and read the stats) before the next forward; a backward()
    behind such a forward is refused.  Once differentiable: the gradients are the forward's own, not a graph."""

    def __init__(self, env, clip=0.2, value_clip=None, vf_coef=0.5, ent_coef=0.0):
        w = env.world
        self.env, self.A = env, len(w.agents)
        if self.A > _abi.MPE_ACTOR_MAX_AGENTS:
            raise _abi.MpeError("PpoLoss: %d agents (at most MPE_ACTOR_MAX_AGENTS = %d)" % (self.A, _abi.MPE_ACTOR_MAX_AGENTS))
        self.movable = [bool(a.movable) for a in w.agents]
        self.speaks = [not a.silent for a in w.agents]
        self.dim_c = int(w.dim_c) if any(self.speaks) else 0
        self.n_out = [_abi.MPE_ACTION_DIM * m + self.dim_c * s for m, s in zip(self.movable, self.speaks)]
        for i, n in enumerate(self.n_out):
            if not 1 <= n <= _abi.MPE_ACTOR_MAX_OUT:
                raise _abi.MpeError("PpoLoss: agent %d has %d logits (5 * movable + dim_c * speaks), need 1..MPE_ACTOR_MAX_OUT = %d"
                                    % (i, n, _abi.MPE_ACTOR_MAX_OUT))
        if not math.isfinite(float(clip)) or float(clip) < 0:
            raise _abi.MpeError("PpoLoss: clip = %r (a finite value >= 0)" % (clip,))
        if value_clip is not None and (not math.isfinite(float(value_clip)) or float(value_clip) < 0):
            raise _abi.MpeError("PpoLoss: value_clip = %r (None, or a finite value >= 0)" % (value_clip,))
        if not math.isfinite(float(vf_coef)) or not math.isfinite(float(ent_coef)):
            raise _abi.MpeError("PpoLoss: vf_coef = %r, ent_coef = %r (both finite)" % (vf_coef, ent_coef))
        self.clip, self.value_clip, self.vf_coef, self.ent_coef = float(clip), value_clip, float(vf_coef), float(ent_coef)
        self._out, self._generation, self.last = Cache(), Generations(), None

    def __call__(self, logits_n, values_n, batch):
        who = "PpoLoss"
        if not isinstance(logits_n, (list, tuple)) or len(logits_n) != self.A:
            raise _abi.MpeError("%s: logits_n is a list of %d tensors, one per agent" % (who, self.A))
        if values_n is not None and (not isinstance(values_n, (list, tuple)) or len(values_n) != self.A):
            raise _abi.MpeError("%s: values_n is a list of %d tensors, one per agent, or None" % (who, self.A))
        if not isinstance(batch, OnPolicyBatch):
            raise _abi.MpeError("%s: batch is an OnPolicyBatch (what Minibatches.batch returned)" % who)
        if batch.logp is None:
            raise _abi.MpeError("%s: batch.logp is None: the trajectory was recorded without log probabilities (Actors(logp=True))" % who)
        for name, ts in (("logits_n", logits_n), ("values_n", values_n or ())):
            for i, t in enumerate(ts):
                if not torch.is_tensor(t):
                    raise _abi.MpeError("%s: %s[%d] is not a tensor" % (who, name, i))
        loss = _PpoLossFn.apply(self, batch, len(values_n) if values_n is not None else 0, *(list(logits_n) + list(values_n or ())))
        loss.stats = self.last.stats
        return loss
