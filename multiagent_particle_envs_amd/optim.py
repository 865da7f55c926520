"""The optimiser step on the device: `DeviceAdam` keeps the packed weights of up to eight `Actors` / `Values` / `Critics` as the
MASTER copy in device memory, with Adam's moments in the same layout and the step count beside them, and `step()` updates all of
them in place in TWO launches (mpe_adam_step: THE ADAM RULE of include/mpe_hip.h) from the packed gradients
mpe_mlp_grad wrote.  The live buffers are attached to the nets (NetSet.attach): every forward launch reads the new weights, nothing
repacks, and a captured PolicyLoop graph keeps working across updates.  `PolyakTargets` is the soft target update of an off-policy
learner on the same buffers: target = lerp(target, online, tau) for every pair in ONE launch (mpe_polyak).

    pi, V = Trainable(Actors(env, actor_modules, logits=True)), Trainable(Values(env, critic_modules))
    opt = DeviceAdam([pi, V], lr=3e-4, max_grad_norm=0.5)
    loss = PpoLoss(env)(pi(batch.obs_n), V(batch.obs_n), batch)
    loss.backward()
    opt.step()                                  # no .grad is read: the packed gradients of the two backward launches are
    opt.write_back()                            # ... and only this copies the weights into the modules' parameters
"""
import ctypes as C
import math

import torch

from . import _abi
from .learner import Critics
from .netset import unpack_layers
from .onpolicy import Values
from .policy import Actors
from .train import MlpGradResult, Trainable

_STATE = _abi.MPE_ADAM_STATE_DOUBLES


class DeviceAdam(object):
    """Adam / AdamW (weight_decay > 0: decoupled) with global-norm clipping (max_grad_norm > 0: torch's clip_grad_norm_ over ALL
    nets together) on the packed buffers, in place.  nets: 1..MPE_ADAM_MAX_SETS of Actors / Values / Critics (a Trainable stands for
    its .net).  Each net is packed ONCE here into a persistent buffer, gets m and v as zeros in the same layout, and reads that
    buffer from now on (net.attach): the modules' own parameters are NOT updated until write_back().  lr_tensor: a one-element
    float32 device tensor the launch reads instead of lr (a schedule under a captured graph).  Refused, with the argument named: a
    module object that appears in two of the nets (two master copies), a net on another device, a net that is already frozen.
    Do NOT call freeze() / unfreeze() on a net the optimiser holds: either replaces the live buffer by a snapshot of the stale
    modules (or by nothing), and step() refuses to go on updating a buffer nobody reads."""

    def __init__(self, nets, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0, lr_tensor=None):
        who = "DeviceAdam"
        if not isinstance(nets, (list, tuple)) or not 1 <= len(nets) <= _abi.MPE_ADAM_MAX_SETS:
            raise _abi.MpeError("%s: nets is a list of 1..MPE_ADAM_MAX_SETS = %d Actors / Values / Critics (or their Trainable)"
                                % (who, _abi.MPE_ADAM_MAX_SETS))
        self._trainable = [n if isinstance(n, Trainable) else None for n in nets]
        self.nets = [n.net if isinstance(n, Trainable) else n for n in nets]
        owner = {}
        for k, net in enumerate(self.nets):
            if not isinstance(net, (Actors, Values, Critics)):
                raise _abi.MpeError("%s: nets[%d] is an Actors, a Values or a Critics, or a Trainable of one (got %s)"
                                    % (who, k, type(net).__name__))
            if any(net is other for other in self.nets[:k]):
                raise _abi.MpeError("%s: nets[%d] is nets[%d] again" % (who, k, [net is o for o in self.nets].index(True)))
            if net.attached() is not None:
                raise _abi.MpeError("%s: nets[%d] is already frozen (unfreeze() it, or release() the DeviceAdam that holds it: the "
                                    "optimiser packs the modules once itself)" % (who, k))
            for i, m in enumerate(net.modules):
                if owner.setdefault(id(m), k) != k:
                    raise _abi.MpeError("%s: nets[%d] and nets[%d] hold the same module object (agent %d of nets[%d]): it would get two "
                                        "master copies -- share(net, other) joins a second set to ONE copy" % (who, owner[id(m)], k, i, k))
        dev = self.nets[0].world.device
        for k, net in enumerate(self.nets):
            if net.world.device != dev:
                raise _abi.MpeError("%s: nets[%d] is on %s, nets[0] on %s (one step updates one device's buffers)"
                                    % (who, k, net.world.device, dev))
        b1, b2 = (float(b) for b in betas)
        scal = dict(lr=float(lr), beta1=b1, beta2=b2, eps=float(eps), weight_decay=float(weight_decay), max_grad_norm=float(max_grad_norm))
        for name, x in scal.items():
            if not math.isfinite(x) or x < 0 or (name == "eps" and x <= 0) or (name.startswith("beta") and x >= 1):
                raise _abi.MpeError("%s: %s = %r (lr, weight_decay, max_grad_norm: finite and >= 0; betas in [0, 1); eps > 0)"
                                    % (who, "betas" if name.startswith("beta") else name, x))
        if lr_tensor is not None:
            if not torch.is_tensor(lr_tensor) or lr_tensor.dtype != torch.float32 or lr_tensor.numel() != 1 or lr_tensor.device != dev:
                raise _abi.MpeError("%s: lr_tensor is a one-element float32 tensor on the nets' device (%s)" % (who, dev))
        if dev.type != "cuda":
            raise _abi.MpeError("%s: nets[0] is on %s (the buffers live on a GPU: there is no CPU path)" % (who, dev))
        self.device, self.lr_tensor = dev, lr_tensor
        self._cfg = _abi.MpeAdam()
        for name, x in scal.items():
            setattr(self._cfg, name, x)
        self._cfg.lr_ptr = lr_tensor.data_ptr() if lr_tensor is not None else None
        self._cfg.n_sets = len(self.nets)
        self.weights, self.m, self.v, self._asets = [], [], [], []
        for k, net in enumerate(self.nets):
            wts, aset = net.pack(dev)
            wts = wts.contiguous()
            aset.weights = wts.data_ptr()
            self.weights.append(wts)
            self.m.append(torch.zeros_like(wts))
            self.v.append(torch.zeros_like(wts))
            self._asets.append(aset)
            s = self._cfg.set[k]
            s.weights, s.m, s.v, s.n = wts.data_ptr(), self.m[k].data_ptr(), self.v[k].data_ptr(), wts.numel()
        self.state = torch.zeros((_STATE,), dtype=torch.float64, device=dev)
        self.state[[1, 2, 4, 5]] = 1.0
        self.work = torch.zeros((_abi.MPE_ADAM_MAX_PARTIALS,), dtype=torch.float64, device=dev)      # (mpe_adam_work(cfg) <= 256 doubles)
        self._shared = []
        for net, wts, aset in zip(self.nets, self.weights, self._asets):
            net.attach((wts, aset))

    def _index(self, net, who):
        net = net.net if isinstance(net, Trainable) else net
        for k, mine in enumerate(self.nets):
            if mine is net:
                return k
        raise _abi.MpeError("%s: net is none of this optimiser's nets" % who)

    def share(self, net, other):
        """Join `other` -- a second Actors / Values / Critics over the SAME module objects in the same order, such as the sampling
        Actors beside the logits=True one of a PPO learner -- to net's live buffer: other keeps its own MpeActorSet (mode, seed,
        heads), its offsets are checked equal, and its weights pointer is net's.  -> other."""
        who = "DeviceAdam.share"
        k = self._index(net, who)
        mine = self.nets[k]
        other = other.net if isinstance(other, Trainable) else other
        if not isinstance(other, (Actors, Values, Critics)):
            raise _abi.MpeError("%s: other is an Actors, a Values or a Critics (got %s)" % (who, type(other).__name__))
        if other.attached() is not None:
            raise _abi.MpeError("%s: other is already frozen" % who)
        if len(other.modules) != len(mine.modules) or any(a is not b for a, b in zip(other.modules, mine.modules)):
            raise _abi.MpeError("%s: other is built over other modules than net (the same module objects, in the same order)" % who)
        if other.world.device != self.device:
            raise _abi.MpeError("%s: other is on %s, the optimiser's buffers on %s" % (who, other.world.device, self.device))
        wts, aset = other.pack(self.device)
        if wts.numel() != self.weights[k].numel() or list(aset.offset) != list(self._asets[k].offset):
            raise _abi.MpeError("%s: other's packed layout differs from net's (offsets %s against %s)"
                                % (who, list(aset.offset)[:other.A], list(self._asets[k].offset)[:mine.A]))
        aset.weights = self.weights[k].data_ptr()
        other.attach((self.weights[k], aset))
        self._shared.append(other)
        return other

    def step(self, grads=None):
        """One mpe_adam_step for all nets, no host synchronisation (captures into a HIP graph).  grads: one MlpGradResult per net
        (mlp_grad_tensors' return: its .packed is read in place); None: each net's Trainable.last_grad, what its last backward()
        computed, which is set back to None here."""
        who = "DeviceAdam.step"
        for k, net in enumerate(self.nets):
            pair = net.attached()
            if pair is None or pair[0] is not self.weights[k]:
                raise _abi.MpeError("%s: nets[%d] no longer reads the optimiser's live buffer (freeze() / unfreeze() was called on it: "
                                    "the step would update weights nobody reads -- release() the optimiser first)" % (who, k))
        for other in self._shared:
            pair = other.attached()
            if pair is None or not any(pair[0] is w for w in self.weights):
                raise _abi.MpeError("%s: a set joined by share() no longer reads the optimiser's live buffer (freeze() / unfreeze() was "
                                    "called on it)" % who)
        if grads is None:
            grads = []
            for k, tr in enumerate(self._trainable):
                if tr is None:
                    raise _abi.MpeError("%s: nets[%d] was not given as a Trainable: pass grads=[MlpGradResult, ..]" % (who, k))
            for k, tr in enumerate(self._trainable):
                if tr.last_grad is None:
                    raise _abi.MpeError("%s: nets[%d].last_grad is None (no backward() since the last step)" % (who, k))
                grads.append(tr.last_grad)
            for tr in self._trainable:
                tr.last_grad = None
        elif not isinstance(grads, (list, tuple)) or len(grads) != len(self.nets):
            raise _abi.MpeError("%s: grads is a list of %d MlpGradResult, one per net" % (who, len(self.nets)))
        for k, g in enumerate(grads):
            if not isinstance(g, MlpGradResult) or g.packed.numel() != self.weights[k].numel() or g.packed.device != self.device:
                raise _abi.MpeError("%s: grads[%d] is the MlpGradResult of nets[%d] (mlp_grad_tensors' return: %d packed floats on %s)"
                                    % (who, k, k, self.weights[k].numel(), self.device))
            self._cfg.set[k].grad = g.packed.data_ptr()
        _abi.check(_abi.lib().mpe_adam_step(C.byref(self._cfg), self.state.data_ptr(), self.work.data_ptr(), _abi.raw_stream(self.device)),
                   "mpe_adam_step")

    def write_back(self):
        """Copy the live weights into the modules' parameters (plain torch, off the hot path: for evaluation or saving through
        torch)."""
        for net, wts in zip(self.nets, self.weights):
            at = 0
            for _, lins in net.distinct():
                at += unpack_layers(lins, wts, at=at)
        return self

    def release(self):
        """write_back(), then every net (and every shared one) packs from its modules again (nothing stays attached)."""
        self.write_back()
        for net in self.nets + self._shared:
            net.attach(None)
        self._shared = []
        return self

    def state_dict(self):
        """The state doubles and per-net clones of weights, m and v (synchronises only as a copy does)."""
        return dict(state=self.state.clone(), weights=[w.clone() for w in self.weights], m=[x.clone() for x in self.m],
                    v=[x.clone() for x in self.v])

    def load_state_dict(self, sd):
        who = "DeviceAdam.load_state_dict"
        if not isinstance(sd, dict) or sorted(sd) != ["m", "state", "v", "weights"] or any(len(sd[k]) != len(self.nets) for k in ("weights", "m", "v")):
            raise _abi.MpeError("%s: sd is what state_dict() returned for the same nets" % who)
        for name, mine in (("weights", self.weights), ("m", self.m), ("v", self.v)):
            for k, (dst, src) in enumerate(zip(mine, sd[name])):
                if not torch.is_tensor(src) or src.dtype != torch.float32 or src.shape != dst.shape:
                    raise _abi.MpeError("%s: sd[%r][%d] is a float32 tensor of %d elements" % (who, name, k, dst.numel()))
        if not torch.is_tensor(sd["state"]) or sd["state"].dtype != torch.float64 or sd["state"].numel() != _STATE:
            raise _abi.MpeError("%s: sd['state'] is a float64 tensor of %d elements" % (who, _STATE))
        for name, mine in (("weights", self.weights), ("m", self.m), ("v", self.v)):
            for dst, src in zip(mine, sd[name]):
                dst.copy_(src)
        self.state.copy_(sd["state"].reshape(-1))

    def _read(self, k):
        return float(self.state[k].item())

    @property
    def t(self):
        """Steps taken (skipped ones not counted).  Reads the device state: this call SYNCHRONISES."""
        return int(self._read(3))

    @property
    def grad_norm(self):
        """The global gradient norm of the last step, before clipping (float64).  This call SYNCHRONISES."""
        return self._read(6)

    @property
    def clip_coef(self):
        """The factor the last step's gradients were scaled by (1: not clipped; 0: the step was skipped).  This call SYNCHRONISES."""
        return self._read(7)

    @property
    def skipped(self):
        """Steps skipped because the gradient norm was not finite.  This call SYNCHRONISES."""
        return int(self._read(8))


class PolyakTargets(object):
    """The soft target updates of an off-policy learner on the packed buffers, ONE launch for all pairs (mpe_polyak: THE POLYAK RULE of
    include/mpe_hip.h): target = lerp(target, online, tau).  pairs: 1..MPE_ADAM_MAX_SETS of (online_net,
    target_net), each an Actors / Values / Critics (or its Trainable).  The online net must be attached -- to a DeviceAdam, whose
    live buffer is then read at every step, or through freeze() --; each target net is packed ONCE here into a persistent buffer
    and reads that buffer from now on (net.attach): its modules' own parameters are NOT updated until write_back().  The packed
    layouts of a pair are checked equal, as DeviceAdam.share checks them.  tau_tensor: a one-element float32 device tensor the
    launch reads instead of tau (a schedule under a captured graph)."""

    def __init__(self, pairs, tau, tau_tensor=None):
        who = "PolyakTargets"
        if not isinstance(pairs, (list, tuple)) or not 1 <= len(pairs) <= _abi.MPE_ADAM_MAX_SETS or \
                any(not isinstance(p, (list, tuple)) or len(p) != 2 for p in pairs):
            raise _abi.MpeError("%s: pairs is a list of 1..MPE_ADAM_MAX_SETS = %d (online_net, target_net) pairs" % (who, _abi.MPE_ADAM_MAX_SETS))
        strip = lambda n: n.net if isinstance(n, Trainable) else n      # noqa: E731
        self.online, self.targets = [strip(p[0]) for p in pairs], [strip(p[1]) for p in pairs]
        for k, (on, tg) in enumerate(zip(self.online, self.targets)):
            for name, net in (("online", on), ("target", tg)):
                if not isinstance(net, (Actors, Values, Critics)):
                    raise _abi.MpeError("%s: pairs[%d]'s %s net is an Actors, a Values or a Critics, or a Trainable of one (got %s)"
                                        % (who, k, name, type(net).__name__))
            if on is tg or any(a is b for a in on.modules for b in tg.modules):
                raise _abi.MpeError("%s: pairs[%d]: the target net holds the online net's module objects (a target is a copy)" % (who, k))
            if any(tg is other for other in self.targets[:k]):
                raise _abi.MpeError("%s: pairs[%d]'s target net is pairs[%d]'s again" % (who, k, [tg is o for o in self.targets].index(True)))
            if on.attached() is None:
                raise _abi.MpeError("%s: pairs[%d]'s online net is not attached (give it to a DeviceAdam, or freeze() it: the step reads "
                                    "its packed buffer)" % (who, k))
            if tg.attached() is not None:
                raise _abi.MpeError("%s: pairs[%d]'s target net is already frozen (unfreeze() it: the targets are packed once here)" % (who, k))
        tau = float(tau)
        if not math.isfinite(tau) or not 0.0 <= tau <= 1.0:
            raise _abi.MpeError("%s: tau = %r (need 0 <= tau <= 1)" % (who, tau))
        dev = self.online[0].world.device
        for k, net in enumerate(self.online + self.targets):
            if net.world.device != dev:
                raise _abi.MpeError("%s: a net of pairs[%d] is on %s, pairs[0]'s online net on %s" % (who, k % len(pairs), net.world.device, dev))
        if tau_tensor is not None:
            if not torch.is_tensor(tau_tensor) or tau_tensor.dtype != torch.float32 or tau_tensor.numel() != 1 or tau_tensor.device != dev:
                raise _abi.MpeError("%s: tau_tensor is a one-element float32 tensor on the nets' device (%s)" % (who, dev))
        if dev.type != "cuda":
            raise _abi.MpeError("%s: pairs[0]'s online net is on %s (the buffers live on a GPU: there is no CPU path)" % (who, dev))
        self.device, self.tau, self.tau_tensor = dev, tau, tau_tensor
        self._cfg = _abi.MpePolyak()
        self._cfg.tau, self._cfg.n_sets = tau, len(pairs)
        self._cfg.tau_ptr = tau_tensor.data_ptr() if tau_tensor is not None else None
        self.weights, self._online_w = [], []
        packs = []
        for k, (on, tg) in enumerate(zip(self.online, self.targets)):
            wts, aset = tg.pack(dev)
            wts = wts.contiguous()
            own, oset = on.attached()
            if wts.numel() != own.numel() or list(aset.offset) != list(oset.offset):
                raise _abi.MpeError("%s: pairs[%d]: the target's packed layout differs from the online net's (offsets %s against %s)"
                                    % (who, k, list(aset.offset)[:tg.A], list(oset.offset)[:on.A]))
            aset.weights = wts.data_ptr()
            packs.append((wts, aset))
            self.weights.append(wts)
            self._online_w.append(own)
            s = self._cfg.set[k]
            s.target, s.online, s.n = wts.data_ptr(), own.data_ptr(), wts.numel()
        for tg, pair in zip(self.targets, packs):
            tg.attach(pair)

    def _check(self, who):
        for k, (on, tg) in enumerate(zip(self.online, self.targets)):
            pair = tg.attached()
            if pair is None or pair[0] is not self.weights[k]:
                raise _abi.MpeError("%s: pairs[%d]'s target net no longer reads the live buffer (freeze() / unfreeze() was called on it: "
                                    "the step would update weights nobody reads -- release() first)" % (who, k))
            pair = on.attached()
            if pair is None or pair[0] is not self._online_w[k]:
                raise _abi.MpeError("%s: pairs[%d]'s online net no longer reads the buffer the step was built on (freeze() / unfreeze() "
                                    "was called on it, or its optimiser was released)" % (who, k))

    def step(self):
        """One mpe_polyak for all pairs, no host synchronisation (captures into a HIP graph)."""
        self._check("PolyakTargets.step")
        _abi.check(_abi.lib().mpe_polyak(C.byref(self._cfg), _abi.raw_stream(self.device)), "mpe_polyak")

    def hard_update(self):
        """target := online, a plain copy of every buffer."""
        self._check("PolyakTargets.hard_update")
        for wts, own in zip(self.weights, self._online_w):
            wts.copy_(own)
        return self

    def write_back(self):
        """Copy the target buffers into the target modules' parameters (plain torch, off the hot path)."""
        for net, wts in zip(self.targets, self.weights):
            at = 0
            for _, lins in net.distinct():
                at += unpack_layers(lins, wts, at=at)
        return self

    def release(self):
        """write_back(), then every target net packs from its modules again (nothing stays attached)."""
        self.write_back()
        for net in self.targets:
            net.attach(None)
        return self
