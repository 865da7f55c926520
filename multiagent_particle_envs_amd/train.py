"""The networks' own backward pass on the device: `mlp_grad_tensors` turns dL/doutput of every agent's MLP into the gradients of
every weight and bias in TWO launches for all agents (mpe_mlp_grad: THE MLP GRADIENT RULE of include/mpe_hip.h) --
the hidden activations are recomputed from the input rows, nothing is saved by the forward --, and `Trainable` joins an `Actors`, a
`Values` or a `Critics` to its modules' parameters behind torch autograd: the forward is the set's one launch, the backward those
two.  There is no gradient with respect to the inputs.

    pi, V = Trainable(Actors(env, actor_modules, logits=True)), Trainable(Values(env, critic_modules))
    loss = PpoLoss(env)(pi(batch.obs_n), V(batch.obs_n), batch)
    loss.backward()                             # .grad of every module parameter; then opt.step()
"""
import ctypes as C

import torch

from . import _abi
from .learner import Critics
from .netset import Cache, Generations, check_tensor, module_views
from .onpolicy import Values
from .policy import Actors

_module_views = module_views      # (the name this file had for it: existing importers keep working)

class MlpGradResult(object):
    """What mlp_grad_tensors wrote: packed, one flat float32 buffer in the layout and at the offsets of the set's packed weights
    (padding +0.0); modules, per distinct module object (in the order of its first agent) one (weight, bias) pair per Linear layer:
    views of `packed` shaped like Linear.weight ([out, in], a transposed view) and Linear.bias; work, the launches' workspace."""
    __slots__ = ("M", "packed", "modules", "work", "shape")


def _kind(net, who):
    if not isinstance(net, (Actors, Values, Critics)):
        raise _abi.MpeError("%s: net is an Actors, a Values or a Critics (got %s)" % (who, type(net).__name__))
    return type(net).__name__


def mlp_grad_tensors(net, in_n, dout_n, out=None, packed=None):
    """THE MLP GRADIENT RULE in two launches for every agent, no host synchronisation (captures into a HIP graph).  net: an Actors,
    a Values or a Critics; in_n[i]: agent i's contiguous float32 [M, D_i] input rows, or ONE tensor every agent reads (a Critics'
    joint rows, a centralised Values' side-by-side observations); dout_n[i]: dL/doutput of agent i, [M, n_out_i] (PpoLossResult's
    dlogits_n[i]), or [M] / [M, 1] for a one-output net (a row of dvalues).  out: an MlpGradResult to rewrite (else the buffers are
    cached on `net` per M, 16 at most).  packed: the (weights, MpeActorSet) pair of net.pack() the forward used (else packed here).
    -> MlpGradResult."""
    who = "mlp_grad_tensors"
    _kind(net, who)
    A = net.A
    layers = net._check()
    if torch.is_tensor(in_n):
        in_n = [in_n] * A
    if not isinstance(in_n, (list, tuple)) or len(in_n) != A:
        raise _abi.MpeError("%s: in_n is a list of %d tensors, one per agent, or one tensor every agent reads" % (who, A))
    if not isinstance(dout_n, (list, tuple)) or len(dout_n) != A:
        raise _abi.MpeError("%s: dout_n is a list of %d tensors, one per agent" % (who, A))
    x0 = in_n[0]
    if not torch.is_tensor(x0) or x0.dim() != 2:
        raise _abi.MpeError("%s: in_n[0] is a contiguous float32 [M, %d] tensor on a GPU" % (who, layers[0][0][0].in_features))
    M, dev = int(x0.shape[0]), x0.device
    for i, (lins, _) in enumerate(layers):
        n = lins[-1].out_features
        check_tensor(who, in_n[i], "in_n[%d]" % i, [(M, lins[0].in_features)], "in_n[0]'s device", dev)
        check_tensor(who, dout_n[i], "dout_n[%d]" % i, [(M, n)] + ([(M,)] if n == 1 else []), "in_n[0]'s device", dev)
    if not x0.is_cuda:
        raise _abi.MpeError("%s: in_n[0] is on %s (the tensors live on a GPU: there is no CPU path)" % (who, dev))
    wts, aset = packed if packed is not None else net.packed(dev)
    n = _abi.lib().mpe_mlp_grad_work(C.byref(aset), M)      # (host only: the set and size checks)
    if n < 0:
        _abi.check(int(n), "mpe_mlp_grad_work")
    shape = (M, int(wts.numel()), int(n))
    if out is not None:
        if not isinstance(out, MlpGradResult) or out.shape != shape or out.packed.device != dev:
            raise _abi.MpeError("%s: out is an MlpGradResult of the same net and M = %d (what an earlier call returned)" % (who, M))
    else:
        def make():
            out = MlpGradResult()
            out.M, out.shape = M, shape
            out.packed = torch.zeros((shape[1],), dtype=torch.float32, device=dev)
            out.work = torch.empty((max(shape[2], 1),), dtype=torch.float32, device=dev)
            out.modules, _ = module_views(net, out.packed)
            return out
        out = net.__dict__.setdefault("_mlp_grad", Cache()).get(shape, make)
    ip = (C.c_void_p * A)(*[t.data_ptr() for t in in_n])
    dp = (C.c_void_p * A)(*[t.data_ptr() for t in dout_n])
    _abi.check(_abi.lib().mpe_mlp_grad(C.byref(aset), ip, dp, M, out.packed.data_ptr(), out.work.data_ptr(), _abi.raw_stream(dev)),
               "mpe_mlp_grad")
    del wts      # (stream-ordered: the caching allocator reuses the block only behind the launches)
    return out


class _TrainFn(torch.autograd.Function):
    """forward: the set's one launch; backward: mpe_mlp_grad's two on the grad_outputs, and ONE out-of-place copy of the packed
    gradient whose views go to the parameters"""

    @staticmethod
    def forward(ctx, owner, inputs, *params):
        packed = owner.net.packed()      # (the launch and the backward read ONE packed copy)
        M, outs, in_n = owner.net.train_forward(inputs, packed)
        ctx.owner, ctx.in_n, ctx.packed, ctx.key = owner, in_n, packed, (M, owner._generation.next(M))
        ctx.shapes = [tuple(o.shape) for o in outs]
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grad_outputs):
        owner, (M, generation) = ctx.owner, ctx.key
        if owner._generation.stale(M, generation):
            raise _abi.MpeError("Trainable: backward() behind a later forward with the same M (the set's outputs and the gradient's "
                                "buffers are cached per M: call backward() before the next forward)")
        dev = owner.net.world.device
        dout = [torch.zeros(s, dtype=torch.float32, device=dev) if g is None else g.contiguous() for g, s in zip(grad_outputs, ctx.shapes)]
        res = mlp_grad_tensors(owner.net, ctx.in_n, dout, packed=ctx.packed)
        owner.last_grad = res      # (what DeviceAdam.step() reads in place of the parameters' .grad)
        flat = res.packed.clone()      # out of place: the cached buffer is rewritten by the next backward of the same M
        views, _ = module_views(owner.net, flat)
        grads = []
        for mv, lins in zip(views, owner._lins):
            for (w, b), lin in zip(mv, lins):
                grads.append(w)
                if lin.bias is not None:
                    grads.append(b)
        return (None, None) + tuple(grads)


class Trainable(object):
    """An Actors (built with logits=True), a Values or a Critics behind torch autograd: Trainable(net)(obs_n) -> per agent the
    module's output, [M, n_out_i] logits for Actors (the live columns of the launch's 16-wide rows), [M] for Values and Critics
    (whose argument is what net.v / net.q take), joined to the modules' parameters by one autograd Function.  The forward is net's
    existing launch (mpe_actor_act_rows / mpe_critic_q), the backward mpe_mlp_grad's two launches on the grad_outputs (None counts
    as zeros); the gradients handed to autograd are views of a fresh copy of the packed gradient.  Once differentiable.  Refused:
    an input that requires grad (there is no dL/din), and a backward() behind a later forward of the same M."""

    def __init__(self, net):
        _kind(net, "Trainable")
        if isinstance(net, Actors) and not net._want[2]:
            raise _abi.MpeError("Trainable: the Actors were built without logits=True (the forward hands autograd the launch's logits)")
        self.net = net
        self._generation = Generations()
        self.last_grad = None      # the MlpGradResult of the last backward(); DeviceAdam.step() consumes it
        self._lins, self._params = [], []
        for _, lins in net.distinct():
            self._lins.append(lins)
            for lin in lins:
                self._params.append(lin.weight)
                if lin.bias is not None:
                    self._params.append(lin.bias)

    def parameters(self):
        return list(self._params)

    def __call__(self, obs_n):
        for i, o in enumerate([obs_n] if torch.is_tensor(obs_n) else list(obs_n)):
            if torch.is_tensor(o) and o.requires_grad:
                raise _abi.MpeError("Trainable: obs_n%s requires grad: mpe_mlp_grad gives the weights' and biases' gradients, there is "
                                    "no dL/din" % ("" if torch.is_tensor(obs_n) else "[%d]" % i))
        return list(_TrainFn.apply(self, obs_n, *self._params))
