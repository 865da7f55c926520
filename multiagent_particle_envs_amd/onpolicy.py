"""The on-policy half of a learner on the device: `Values` evaluates one MLP critic per agent on the agents' OWN observations (or,
centralised, on all of them) in ONE launch (mpe_critic_q with per-agent pointers and widths), `PolicyLoop.run(T, values=V)` records
V along the closed loop -- of the observation every step was decided on, and of the output observation of every segment-ending
step --, and `gae` turns the recorded trajectory into advantages and returns in ONE launch (mpe_gae: THE GAE RULE of
include/mpe_hip.h).  Backward passes, advantage normalisation and the clipped loss stay in torch autograd.

    V = Values(env, critic_modules)
    traj = loop.run(25, values=V)               # + traj.obs_in, traj.val [T,A,B], traj.boot [K,A,B]
    g = gae(traj, gamma=0.99, lam=0.95)         # g.adv, g.ret [T,A,B]
"""
import ctypes as C
import math

import torch

from . import _abi
from .learner import Critics
from .rollout import _actor_layers


class Values(object):
    """Per-agent MLP state-value critics: `modules` is one nn.Sequential per agent, or one module every agent shares (Critics'
    layer rules: Linear layers with ReLU / Tanh between them, at most 3, hidden widths <= 64, float32, ONE output).  Decentralised
    (the default) critic i's first Linear takes agent i's observation width D_i and reads agent i's own [M, D_i] block, zero-copy;
    centralised=True: every critic takes all observations side by side, sum D_i <= MPE_ACTOR_MAX_INPUT inputs, from one [M, sum D_i]
    tensor of this object's (one torch.cat per call).  The weights are packed again at every call unless freeze() was called."""

    def __init__(self, env, modules, centralised=False):
        import torch.nn as nn
        w = env.world
        self.env, self.world = env, w
        self.A = len(w.agents)
        if self.A > _abi.MPE_ACTOR_MAX_AGENTS:
            raise _abi.MpeError("Values: %d agents (at most MPE_ACTOR_MAX_AGENTS = %d per set)" % (self.A, _abi.MPE_ACTOR_MAX_AGENTS))
        off = getattr(env, "_obs_off", None)
        if off is None:
            raise _abi.MpeError("Values: this env has no device-side observation layout (env.fused is False)")
        self.obs_widths = [int(off[i + 1] - off[i]) for i in range(self.A)]
        self.centralised = bool(centralised)
        total = sum(self.obs_widths)
        if self.centralised and total > _abi.MPE_ACTOR_MAX_INPUT:
            raise _abi.MpeError("Values(centralised=True): the observations together have %d floats, a critic's input is at most "
                                "MPE_ACTOR_MAX_INPUT = %d wide" % (total, _abi.MPE_ACTOR_MAX_INPUT))
        self.in_widths = [total] * self.A if self.centralised else list(self.obs_widths)
        self.shared = isinstance(modules, nn.Module)
        self.modules = [modules] * self.A if self.shared else list(modules)
        if len(self.modules) != self.A:
            raise _abi.MpeError("Values: %d critics for %d agents" % (len(self.modules), self.A))
        self._frozen = None
        self._out, self._cat, self._ptrs = {}, {}, {}
        self._check()

    def _check(self):
        layers = []
        for i, m in enumerate(self.modules):
            try:
                lins, act = _actor_layers(m, 1, "Values")
            except _abi.MpeError as e:
                raise _abi.MpeError("%s [agent %d's critic: one output]" % (e, i))
            if lins[0].in_features != self.in_widths[i]:
                raise _abi.MpeError("Values: agent %d's critic takes %d inputs, %s %d" % (
                    i, lins[0].in_features, "the observations together have" if self.centralised else "its observation has",
                    self.in_widths[i]))
            if self.in_widths[i] > _abi.MPE_ACTOR_MAX_INPUT:
                raise _abi.MpeError("Values: agent %d's input width %d > MPE_ACTOR_MAX_INPUT = %d" % (i, self.in_widths[i], _abi.MPE_ACTOR_MAX_INPUT))
            layers.append((lins, act))
        return layers

    # a set of one-output critics is packed, frozen and thawed as Critics' is (mode MPE_POLICY_VALUE, one copy per module object)
    pack, freeze, unfreeze = Critics.pack, Critics.freeze, Critics.unfreeze

    def _inputs(self, obs_n):
        """-> (M, the HOST array of A device pointers, what keeps them alive); checked once per distinct set of blocks"""
        if len(obs_n) != self.A:
            raise _abi.MpeError("Values.v: %d observation blocks for %d agents" % (len(obs_n), self.A))
        if not torch.is_tensor(obs_n[0]) or obs_n[0].dim() != 2:
            raise _abi.MpeError("Values.v: obs_n[0] is a contiguous float32 [M, %d] tensor on the env's device" % self.obs_widths[0])
        M, dev = int(obs_n[0].shape[0]), self.world.device
        key = (M,) + tuple(o.data_ptr() if torch.is_tensor(o) else None for o in obs_n)
        hit = self._ptrs.get(key)
        if hit is None:
            for i, o in enumerate(obs_n):
                if not torch.is_tensor(o) or o.dtype != torch.float32 or not o.is_contiguous() or o.device != dev or \
                        tuple(o.shape) != (M, self.obs_widths[i]):
                    raise _abi.MpeError("Values.v: obs_n[%d] is a contiguous float32 [%d, %d] tensor on the env's device"
                                        % (i, M, self.obs_widths[i]))
            if len(self._ptrs) >= 64:
                self._ptrs.clear()
            if self.centralised:
                cat = self._cat.get(M)
                if cat is None:
                    if len(self._cat) >= 16:
                        self._cat.clear()
                    cat = self._cat[M] = torch.zeros((M, self.in_widths[0]), dtype=torch.float32, device=dev)
                hit = ((C.c_void_p * self.A)(*([cat.data_ptr()] * self.A)), cat)
            else:
                hit = ((C.c_void_p * self.A)(*key[1:]), None)
            self._ptrs[key] = hit
        if hit[1] is not None:
            torch.cat(list(obs_n), dim=1, out=hit[1])
        return M, hit[0]

    def v(self, obs_n, out=None):
        """One launch: critic i on obs_n[i] (a list of [M, D_i] device tensors: env.step's own output qualifies; centralised: every
        critic on all of them) -> v [A, M] float32 (this object's tensor per M, or `out`)."""
        M, ptrs = self._inputs(obs_n)
        dev = self.world.device
        if out is None:
            out = self._out.get(M)
            if out is None:
                if len(self._out) >= 16:
                    self._out.clear()
                out = self._out[M] = torch.zeros((self.A, M), dtype=torch.float32, device=dev)
        elif not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (self.A, M) or not out.is_contiguous() or \
                out.device != dev:
            raise _abi.MpeError("Values.v: out is a contiguous float32 [%d, %d] tensor on the env's device" % (self.A, M))
        wts, aset = self._frozen if self._frozen is not None else self.pack(dev)
        _abi.check(_abi.lib().mpe_critic_q(C.byref(aset), ptrs, M, out.data_ptr(), None, None, _abi.raw_stream(dev)), "mpe_critic_q")
        del wts      # (stream-ordered: the caching allocator reuses the block only behind the launch)
        return out

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


def _tensor_check(x, name, shape, dtypes, dev, who):
    if not torch.is_tensor(x) or x.dtype not in dtypes or (shape is not None and tuple(x.shape) != tuple(shape)) or \
            not x.is_contiguous() or (dev is not None and x.device != dev):
        raise _abi.MpeError("%s: %s is a contiguous %s %s tensor on %s" % (
            who, name, " / ".join(str(d).replace("torch.", "") for d in dtypes),
            list(shape) if shape is not None else "[T, A, B]", "rew's device" if dev is not None else "a GPU"))


def gae_tensors(rew, done, val, boot, gamma, lam, episode_len=0, episode_phase=0, out=None):
    """GAE(lambda) by THE GAE RULE in one launch, no host synchronisation (captures into a HIP graph).  rew, val [T, A, B] float32;
    done [T, A, B] bool or uint8; boot [K, A, B] float32 with K = segments(T, episode_len, episode_phase): V of the output
    observation of every segment-ending step.  out: a GaeResult to rewrite.  -> GaeResult(adv, ret)."""
    who = "gae_tensors"
    _tensor_check(rew, "rew", None, (torch.float32,), None, who)
    if rew.dim() != 3:
        raise _abi.MpeError("%s: rew is a contiguous float32 [T, A, B] tensor on a GPU" % who)
    T, A, B = (int(n) for n in rew.shape)
    dev = rew.device
    if not math.isfinite(float(gamma)) or not math.isfinite(float(lam)):
        raise _abi.MpeError("%s: gamma = %r, lam = %r (both finite)" % (who, gamma, lam))
    K = segments(T, episode_len, episode_phase)
    _tensor_check(done, "done", (T, A, B), (torch.bool, torch.uint8), dev, who)
    _tensor_check(val, "val", (T, A, B), (torch.float32,), dev, who)
    _tensor_check(boot, "boot", (K, A, B), (torch.float32,), dev, who)
    if out is None:
        out = GaeResult(torch.empty_like(rew), torch.empty_like(rew))
    else:
        if not isinstance(out, GaeResult):
            raise _abi.MpeError("%s: out is a GaeResult (what an earlier call returned)" % who)
        _tensor_check(out.adv, "out.adv", (T, A, B), (torch.float32,), dev, who)
        _tensor_check(out.ret, "out.ret", (T, A, B), (torch.float32,), dev, who)
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
