"""The networks' own backward pass on the device: `mlp_grad_tensors` turns dL/doutput of every agent's MLP into the gradients of
every weight and bias in TWO launches for all agents (mpe_mlp_grad: THE MLP GRADIENT RULE of include/mpe_hip.h) --
the hidden activations are recomputed from the input rows, nothing is saved by the forward --, and `Trainable` joins an `Actors`, a
`Values` or a `Critics` to its modules' parameters behind torch autograd: the forward is the set's one launch, the backward those
two.  The gradient with respect to the inputs is opt-in: `mlp_dinput_tensors` (mpe_mlp_dinput: THE MLP INPUT GRADIENT RULE, ONE
launch over a window of input columns) and `Trainable(net, input_grad=True)` -- what MADDPG's actor loss needs of
its critics.

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


def _rows_in_dout(who, net, in_n, dout_n):
    """The argument checks mlp_grad_tensors and mlp_dinput_tensors share -> (in_n as a list of A tensors, M, device)"""
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
    return list(in_n), M, dev


def _on_gpu(who, x0):
    if not x0.is_cuda:
        raise _abi.MpeError("%s: in_n[0] is on %s (the tensors live on a GPU: there is no CPU path)" % (who, x0.device))


def mlp_grad_tensors(net, in_n, dout_n, out=None, packed=None):
    """THE MLP GRADIENT RULE in two launches for every agent, no host synchronisation (captures into a HIP graph).  net: an Actors,
    a Values or a Critics; in_n[i]: agent i's contiguous float32 [M, D_i] input rows, or ONE tensor every agent reads (a Critics'
    joint rows, a centralised Values' side-by-side observations); dout_n[i]: dL/doutput of agent i, [M, n_out_i] (PpoLossResult's
    dlogits_n[i]), or [M] / [M, 1] for a one-output net (a row of dvalues).  out: an MlpGradResult to rewrite (else the buffers are
    cached on `net` per M, 16 at most).  packed: the (weights, MpeActorSet) pair of net.pack() the forward used (else packed here).
    -> MlpGradResult."""
    who = "mlp_grad_tensors"
    in_n, M, dev = _rows_in_dout(who, net, in_n, dout_n)
    A = net.A
    _on_gpu(who, in_n[0])
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


def _windows(who, net, cols):
    """cols: None (every agent's whole input) or per agent (col0, ncol) -> [(col0, ncol)] per agent, checked against the input widths"""
    D = net.in_widths
    if cols is None:
        return [(0, int(d)) for d in D]
    if not isinstance(cols, (list, tuple)) or len(cols) != net.A:
        raise _abi.MpeError("%s: cols is None (the whole input) or a list of %d (col0, ncol) pairs, one per agent" % (who, net.A))
    out = []
    for i, c in enumerate(cols):
        ok = isinstance(c, (list, tuple)) and len(c) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in c)
        if not ok or c[0] < 0 or c[1] < 1 or c[0] + c[1] > D[i]:
            raise _abi.MpeError("%s: cols[%d] = %r is no window of agent %d's %d input columns (0 <= col0, 1 <= ncol, col0 + ncol <= %d)"
                                % (who, i, c, i, D[i], D[i]))
        out.append((c[0], c[1]))
    return out


def mlp_dinput_tensors(net, in_n, dout_n, cols=None, out=None, packed=None):
    """THE MLP INPUT GRADIENT RULE in ONE launch for every agent, no host synchronisation (captures into a HIP graph): dL/din over a
    window of each agent's input columns.  net, in_n, dout_n, packed: as for mlp_grad_tensors.  cols: None (the whole input) or per
    agent (col0, ncol).  out: per agent a float32 [M, >= ncol_i] view whose last dimension is contiguous -- its row stride is the
    launch's ld, its data pointer the window's first float, columns at and beyond ncol_i are left alone; it may not overlap in_n,
    dout_n or the weights (not checked).  Else the tensors are cached on `net` per (M, windows), 16 at most.
    -> a list of A tensors [M, ncol_i]."""
    who = "mlp_dinput_tensors"
    in_n, M, dev = _rows_in_dout(who, net, in_n, dout_n)
    A = net.A
    win = _windows(who, net, cols)
    if out is not None:
        if not isinstance(out, (list, tuple)) or len(out) != A:
            raise _abi.MpeError("%s: out is a list of %d tensors, one per agent" % (who, A))
        for i, (o, (_, nc)) in enumerate(zip(out, win)):
            if not torch.is_tensor(o) or o.dtype != torch.float32 or o.dim() != 2 or o.shape[0] != M or o.shape[1] < nc or \
                    (o.shape[1] > 1 and o.stride(1) != 1) or (M > 1 and o.stride(0) < nc) or o.device != dev:
                raise _abi.MpeError("%s: out[%d] is a float32 [%d, >= %d] tensor on in_n[0]'s device, its last dimension contiguous and "
                                    "its row stride at least %d" % (who, i, M, nc, nc))
    _on_gpu(who, in_n[0])
    if out is None:
        out = net.__dict__.setdefault("_mlp_dinput", Cache()).get(
            (M, tuple(win)), lambda: [torch.zeros((M, nc), dtype=torch.float32, device=dev) for _, nc in win])
    wts, aset = packed if packed is not None else net.packed(dev)
    desc = _abi.MpeMlpDinput()
    for i, ((c0, nc), o) in enumerate(zip(win, out)):
        desc.col0[i], desc.ncol[i], desc.ld[i] = c0, nc, max(int(o.stride(0)), nc) if M > 1 else nc
    ptrs = [(C.c_void_p * A)(*[t.data_ptr() for t in ts]) for ts in (in_n, dout_n, out)]
    _abi.check(_abi.lib().mpe_mlp_dinput(C.byref(aset), C.byref(desc), ptrs[0], ptrs[1], M, ptrs[2], _abi.raw_stream(dev)), "mpe_mlp_dinput")
    del wts      # (stream-ordered: the caching allocator reuses the block only behind the launch)
    return [o[:, :nc] for o, (_, nc) in zip(out, win)]


class _TrainFn(torch.autograd.Function):
    """forward: the set's one launch; backward: mpe_mlp_grad's two on the grad_outputs, and ONE out-of-place copy of the packed
    gradient whose views go to the parameters; with input_grad, mpe_mlp_dinput's one launch, into fresh tensors shaped like the
    inputs.  The inputs are arguments of their own (n_in of them; one: the tensor every agent reads), so that autograd sees them."""

    @staticmethod
    def forward(ctx, owner, n_in, *args):
        inputs = args[0] if n_in is None else list(args[:n_in])
        packed = owner.net.packed()      # (the launch and the backward read ONE packed copy)
        M, outs, in_n = owner.net.train_forward(inputs, packed)
        ctx.owner, ctx.in_n, ctx.packed, ctx.key = owner, in_n, packed, (M, owner._generation.next(M))
        ctx.shapes = [tuple(o.shape) for o in outs]
        # ONE tensor read by every agent: the caller's own (n_in None), or the side-by-side copy of the caller's tensors
        ctx.one = n_in is None or (all(t is in_n[0] for t in in_n) and not any(t is in_n[0] for t in inputs))
        ctx.n_in, ctx.widths = n_in, None if n_in is None else [int(t.shape[1]) for t in inputs]
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grad_outputs):
        owner, (M, generation) = ctx.owner, ctx.key
        if owner._generation.stale(M, generation):
            raise _abi.MpeError("Trainable: backward() behind a later forward with the same M (the set's outputs and the gradient's "
                                "buffers are cached per M: call backward() before the next forward)")
        net = owner.net
        dev = net.world.device
        dout = [torch.zeros(s, dtype=torch.float32, device=dev) if g is None else g.contiguous() for g, s in zip(grad_outputs, ctx.shapes)]
        n_in = 1 if ctx.n_in is None else ctx.n_in
        din = [None] * n_in
        if owner.input_grad and any(ctx.needs_input_grad[2:2 + n_in]):
            din = _input_grads(net, ctx.in_n, dout, owner.cols, ctx.packed, ctx.one, ctx.widths)
        grads = [None] * len(owner._params)
        if owner.weight_grad:
            res = mlp_grad_tensors(net, ctx.in_n, dout, packed=ctx.packed)
            owner.last_grad = res      # (what DeviceAdam.step() reads in place of the parameters' .grad)
            flat = res.packed.clone()      # out of place: the cached buffer is rewritten by the next backward of the same M
            views, _ = module_views(net, flat)
            grads = []
            for mv, lins in zip(views, owner._lins):
                for (w, b), lin in zip(mv, lins):
                    grads.append(w)
                    if lin.bias is not None:
                        grads.append(b)
        return (None, None) + tuple(din) + tuple(grads)


def _input_grads(net, in_n, dout, win, packed, one, widths):
    """dL/d(input) shaped like the inputs, zeros outside the windows, in tensors made here (autograd may accumulate into what it is
    handed).  in_n: the rows each agent read.  Agents that read their own tensor: the launch writes the window straight into the
    zeros.  ONE tensor read by every agent: the agents' windows are added in ascending agent order; widths (None: the caller gave
    that tensor itself) cuts the sum into the caller's side-by-side tensors (a centralised Values)."""
    M, dev = int(in_n[0].shape[0]), in_n[0].device
    if not one:
        full = [torch.zeros(tuple(t.shape), dtype=torch.float32, device=dev) for t in in_n]
        mlp_dinput_tensors(net, in_n, dout, cols=win, out=[f[:, c0:c0 + nc] for f, (c0, nc) in zip(full, win)], packed=packed)
        return full
    full = torch.zeros(tuple(in_n[0].shape), dtype=torch.float32, device=dev)
    for g, (c0, nc) in zip(mlp_dinput_tensors(net, in_n, dout, cols=win, packed=packed), win):
        full[:, c0:c0 + nc] += g
    if widths is None:
        return [full]
    return [part.clone() for part in torch.split(full, widths, dim=1)]


class Trainable(object):
    """An Actors (built with logits=True), a Values or a Critics behind torch autograd: Trainable(net)(obs_n) -> per agent the
    module's output, [M, n_out_i] logits for Actors (the live columns of the launch's 16-wide rows), [M] for Values and Critics
    (whose argument is what net.v / net.q take), joined to the modules' parameters by one autograd Function.  The forward is net's
    existing launch (mpe_actor_act_rows / mpe_critic_q), the backward mpe_mlp_grad's two launches on the grad_outputs (None counts
    as zeros); the gradients handed to autograd are views of a fresh copy of the packed gradient.  Once differentiable.  Refused:
    an input that requires grad (there is no dL/din), and a backward() behind a later forward of the same M.
    input_grad=True accepts inputs that require grad: the backward then runs mpe_mlp_dinput's one launch as well and hands autograd,
    per input tensor, a fresh gradient of the input's shape, zeros outside the agent's window `cols[i]` = (col0, ncol) (None: the
    whole input); ONE tensor read by every agent (a Critics' joint rows) gets the agents' windows added in ascending agent order.
    weight_grad=False skips mpe_mlp_grad: the parameters get no gradient and last_grad is left alone (MADDPG's actor loss, of which
    the critic is a constant)."""

    def __init__(self, net, input_grad=False, weight_grad=True, cols=None):
        _kind(net, "Trainable")
        if isinstance(net, Actors) and not net._want[2]:
            raise _abi.MpeError("Trainable: the Actors were built without logits=True (the forward hands autograd the launch's logits)")
        if cols is not None and not input_grad:
            raise _abi.MpeError("Trainable: cols is the window of the input gradient: it needs input_grad=True")
        if not input_grad and not weight_grad:
            raise _abi.MpeError("Trainable: input_grad=False, weight_grad=False leaves nothing to differentiate")
        self.net = net
        self.input_grad, self.weight_grad = bool(input_grad), bool(weight_grad)
        self.cols = _windows("Trainable", net, cols) if input_grad else None
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
        one = torch.is_tensor(obs_n)
        inputs = [obs_n] if one else list(obs_n)
        if not self.input_grad:
            for i, o in enumerate(inputs):
                if torch.is_tensor(o) and o.requires_grad:
                    raise _abi.MpeError("Trainable: obs_n%s requires grad: mpe_mlp_grad gives the weights' and biases' gradients, there is "
                                        "no dL/din" % ("" if one else "[%d]" % i))
        return list(_TrainFn.apply(self, None if one else len(inputs), *(inputs + self._params)))
