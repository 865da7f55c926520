"""The one place on the host side that knows how a set of per-agent MLPs is packed for the kernels (include/mpe_hip.h: MpeActorSet,
MpePolicy) and who may rebind the weights a set's launches read: the module rules (`_actor_layers`), the packed layout
(`layout`, `module_views`, `pack_layers`, `unpack_layers`), the per-agent struct fill (`fill_set`), the base class of `Actors`,
`Values` and `Critics` (`NetSet`: constructor prologue, checks, pack / freeze / unfreeze, `packed` / `attach` / `attached`), and the
three small helpers the learner files share (`Cache`, `check_tensor`, `Generations`).  DESIGN.md 2.20."""
import torch

from . import _abi

_W, _LW = _abi.MPE_POLICY_MAX_WIDTH, _abi.MPE_ACTOR_MAX_OUT


def _actor_layers(module, n_out=_abi.MPE_ACTION_DIM, who="MlpPolicy"):
    """nn.Sequential (or a lone nn.Linear) -> ([Linear, ...], activation name); refuses anything the kernel does not evaluate.
    n_out: the width the last Linear layer must have; who: the class the refusals name (policy.Actors checks its modules here)."""
    import torch.nn as nn
    mods = [module] if isinstance(module, nn.Linear) else list(module.children()) if isinstance(module, nn.Sequential) else None
    if mods is None:
        raise _abi.MpeError(who + ": an actor is an nn.Sequential of Linear layers with ReLU / Tanh between them (got %s)"
                            % type(module).__name__)
    lins, acts = [], []
    for k, m in enumerate(mods):
        want_linear = k % 2 == 0
        if want_linear and isinstance(m, nn.Linear):
            lins.append(m)
        elif not want_linear and isinstance(m, (nn.ReLU, nn.Tanh)):
            acts.append(type(m).__name__.lower())
        else:
            raise _abi.MpeError(who + ": unsupported layer %d (%s): an actor alternates Linear and ReLU / Tanh and ends with a Linear"
                                % (k, type(m).__name__))
    if not lins or len(mods) % 2 == 0:
        raise _abi.MpeError(who + ": an actor ends with a Linear layer")
    if len(lins) > _abi.MPE_POLICY_MAX_LAYERS:
        raise _abi.MpeError(who + ": %d Linear layers (at most %d)" % (len(lins), _abi.MPE_POLICY_MAX_LAYERS))
    if len(set(acts)) > 1:
        raise _abi.MpeError(who + ": one activation per actor (got %s)" % sorted(set(acts)))
    for k, lin in enumerate(lins):
        if lin.weight.dtype != torch.float32 or (lin.bias is not None and lin.bias.dtype != torch.float32):
            raise _abi.MpeError(who + ": Linear layer %d is not float32" % k)
        if k > 0 and lin.in_features != lins[k - 1].out_features:
            raise _abi.MpeError(who + ": Linear layer %d takes %d inputs, layer %d gives %d"
                                % (k, lin.in_features, k - 1, lins[k - 1].out_features))
        if k + 1 < len(lins) and lin.out_features > _abi.MPE_POLICY_MAX_WIDTH:
            raise _abi.MpeError(who + ": hidden width %d > %d" % (lin.out_features, _abi.MPE_POLICY_MAX_WIDTH))
    if lins[-1].out_features != n_out:
        raise _abi.MpeError(who + ": the last Linear layer gives %d outputs (need %d)" % (lins[-1].out_features, n_out))
    return lins, (acts[0] if acts else "relu")


# ---- the packed layout ----------------------------------------------------------------------------------------------------------------
def layout(lins, last_wide=_LW):
    """THE packed layout of one module (include/mpe_hip.h): for each Linear layer l, W_l as [in_l][out_l'] (W_l[k][j] = weight[j][k])
    then bias[out_l'], with in_0 = the input width, in_l = 64 for l > 0, out_l' = 64 for a hidden layer and last_wide for the last
    (16: MpeActorSet, 8: MpePolicy), zero padding, the whole padded to a multiple of 16 floats (only the 8-wide layout needs it).
    -> ([(weight offset, n_in, wide, bias offset)] per layer, total floats)."""
    rows, at = [], 0
    for k, lin in enumerate(lins):
        n_in = lin.in_features if k == 0 else _W
        wide = last_wide if k + 1 == len(lins) else _W
        rows.append((at, n_in, wide, at + n_in * wide))
        at += (n_in + 1) * wide
    return rows, at + (-at) % 16


def distinct(modules, layers):
    """(module, its Linear layers) once per distinct module object, in the order of its first agent; layers[i] = (Linear layers,
    activation) of modules[i].  Agents handed the SAME module object share one packed copy."""
    seen = set()
    for m, (lins, _) in zip(modules, layers):
        if id(m) not in seen:
            seen.add(id(m))
            yield m, lins


def _layer_views(lins, flat, last_wide, at):
    """one module's [(weight view [out, in], bias view [out])] of the flat buffer, the module's block starting at float `at`
    -> (views, floats in the block)"""
    rows, total = layout(lins, last_wide)
    return [(flat[at + w0:at + b0].view(n_in, wide)[:lin.in_features, :lin.out_features].t(), flat[at + b0:at + b0 + lin.out_features])
            for lin, (w0, n_in, wide, b0) in zip(lins, rows)], total


def module_views(net_or_layers, flat, last_wide=_LW):
    """Per distinct module [(weight view [out, in], bias view [out])] of a flat buffer in the packed layout: views shaped like
    Linear.weight (a transposed view) and Linear.bias.  net_or_layers: a NetSet, or the Linear layers of each distinct module in
    packing order.  -> (views, floats spanned)."""
    per_module = [lins for _, lins in net_or_layers.distinct()] if isinstance(net_or_layers, NetSet) else net_or_layers
    out, at = [], 0
    for lins in per_module:
        views, n = _layer_views(lins, flat, last_wide, at)
        out.append(views)
        at += n
    return out, at


def _copy_layers(lins, flat, last_wide, at, back):
    views, n = _layer_views(lins, flat, last_wide, at)
    with torch.no_grad():
        for (w, b), lin in zip(views, lins):
            for view, param in ((w, lin.weight), (b, lin.bias)):
                if param is not None:
                    param.copy_(view) if back else view.copy_(param)
    return n


def pack_layers(lins, last_wide=_LW, flat=None, at=0):
    """One module's weights and biases into its block of `flat` (whose padding is already +0.0), or into fresh zeros on the module's
    device -> flat."""
    if flat is None:
        flat = torch.zeros(layout(lins, last_wide)[1], dtype=torch.float32, device=lins[0].weight.device)
    _copy_layers(lins, flat, last_wide, at, False)
    return flat


def unpack_layers(lins, flat, last_wide=_LW, at=0):
    """The same walk in the other direction: the module's block of `flat` into its parameters -> the floats in the block."""
    return _copy_layers(lins, flat, last_wide, at, True)


def fill_set(desc, modules, layers, last_wide=_LW, device=None):
    """The per-agent fields of an MpeActorSet or an MpePolicy -- n_layers, width, activation, offset -- for agent i = modules[i] with
    layers[i] = (Linear layers, activation), and the weights they index: one block per distinct module object.  -> the float32
    weights on `device` (None: the first module's)."""
    where, blocks, total = {}, [], 0
    for m, lins in distinct(modules, layers):
        where[id(m)] = total
        blocks.append((lins, total))
        total += layout(lins, last_wide)[1]
    wts = torch.zeros(total, dtype=torch.float32, device=layers[0][0][0].weight.device if device is None else device)
    for lins, at in blocks:
        pack_layers(lins, last_wide, wts, at)
    for i, (m, (lins, act)) in enumerate(zip(modules, layers)):
        desc.n_layers[i] = len(lins)
        desc.width[i][0] = lins[0].in_features
        for k, lin in enumerate(lins):
            desc.width[i][k + 1] = lin.out_features
        desc.activation[i] = _abi.MPE_POLICY_TANH if act == "tanh" else _abi.MPE_POLICY_RELU
        desc.offset[i] = where[id(m)]
    return wts


# ---- the base of Actors, Values and Critics ---------------------------------------------------------------------------------------------
class NetSet(object):
    """One MLP per agent of an env, evaluated by the MpeActorSet kernels: `modules` is one nn.Sequential per agent, or one module
    every agent shares.  A subclass gives `who` (the name its refusals carry), `noun` ("actors" / "critics") and
        _widths()                 sets in_widths [A] and n_out [A] from the env (and refuses what it cannot take),
        _input_refusal(i, n, D)   the text for a first layer that takes n inputs where agent i's input has D,
        _agent(i)                 the bracketed suffix of a layer refusal; what it refuses itself comes in front of the layer checks,
        _tail(aset)               the fields of the set behind the per-agent ones: mode, seed, dim_c, movable, speaks.
    The weights every launch reads are `packed()`: the pair attached to the set -- by freeze(), or by a DeviceAdam, whose live
    buffer it is -- or else a fresh pack of the modules.  `_frozen` holds that pair (or None); only this file assigns it."""
    who, noun = "NetSet", "nets"

    def __init__(self, env, modules):
        import torch.nn as nn
        w = env.world
        self.env, self.world = env, w
        self.A = len(w.agents)
        if self.A > _abi.MPE_ACTOR_MAX_AGENTS:
            raise _abi.MpeError("%s: %d agents (at most MPE_ACTOR_MAX_AGENTS = %d per set)" % (self.who, self.A, _abi.MPE_ACTOR_MAX_AGENTS))
        off = getattr(env, "_obs_off", None)
        if off is None:
            raise _abi.MpeError("%s: this env has no device-side observation layout (env.fused is False)" % self.who)
        self.obs_widths = [int(off[i + 1] - off[i]) for i in range(self.A)]
        self._widths()
        self.shared = isinstance(modules, nn.Module)
        self.modules = [modules] * self.A if self.shared else list(modules)
        if len(self.modules) != self.A:
            raise _abi.MpeError("%s: %d %s for %d agents" % (self.who, len(self.modules), self.noun, self.A))
        self._frozen = None
        self._check()

    def _agent(self, i):
        return "agent %d's critic: one output" % i

    def _tail(self, aset):
        aset.dim_c, aset.mode, aset.seed = 0, _abi.MPE_POLICY_VALUE, 0

    def _check(self):
        """Every module against its agent; -> [(Linear layers, activation)] per agent."""
        layers = []
        for i, m in enumerate(self.modules):
            suffix = self._agent(i)
            try:
                lins, act = _actor_layers(m, self.n_out[i], self.who)
            except _abi.MpeError as e:
                raise _abi.MpeError("%s [%s]" % (e, suffix))
            D = self.in_widths[i]
            if lins[0].in_features != D:
                raise _abi.MpeError(self._input_refusal(i, lins[0].in_features, D))
            if D > _abi.MPE_ACTOR_MAX_INPUT:
                raise _abi.MpeError("%s: agent %d's input width %d > MPE_ACTOR_MAX_INPUT = %d" % (self.who, i, D, _abi.MPE_ACTOR_MAX_INPUT))
            layers.append((lins, act))
        return layers

    def distinct(self):
        """(module, its Linear layers) per distinct module object, in packing order."""
        return distinct(self.modules, self._check())

    def pack(self, device=None):
        """-> (weights tensor, MpeActorSet): the set's packed modules, one copy per distinct module object."""
        aset = _abi.MpeActorSet()
        wts = fill_set(aset, self.modules, self._check(), _LW, device)
        aset.n_agents = self.A
        self._tail(aset)
        aset.weights = wts.data_ptr() if wts.is_cuda else None
        return wts, aset

    def packed(self, device=None):
        """The (weights, MpeActorSet) pair this forward reads: the attached one, else the modules packed now."""
        return self._frozen if self._frozen is not None else self.pack(self.world.device if device is None else device)

    def attach(self, pair):
        """Bind the pair every launch reads from now on (None: pack from the modules again).  For freeze() / unfreeze() and for
        DeviceAdam, which attaches its live buffer."""
        self._frozen = pair
        return self

    def attached(self):
        """The attached pair, or None."""
        return self._frozen

    def freeze(self):
        """Pack the weights once; the launches stop re-reading the modules (call again after an update; unfreeze() goes back)."""
        return self.attach(self.pack(self.world.device))

    def unfreeze(self):
        return self.attach(None)


# ---- helpers the learner files share ------------------------------------------------------------------------------------------------------
class Cache(dict):
    """Buffers kept per key (an M, a shape, a set of pointers): get(key, make) -> the entry, made by make() on a miss; a cache that
    already holds `limit` entries is emptied in front of the new one."""

    def __init__(self, limit=16):
        dict.__init__(self)
        self.limit = limit

    def get(self, key, make=None):
        x = dict.get(self, key)
        if x is None and make is not None:
            x = make()
            if len(self) >= self.limit:
                self.clear()
            self[key] = x
        return x


def check_tensor(who, x, name, shapes, tail, dev=None, dtypes=(torch.float32,), text=None):
    """x is a contiguous tensor of one of `dtypes` and one of `shapes` (None: any) on `dev` (None: anywhere), or MpeError
    "<who>: <name> is a contiguous <dtypes> <shapes, or text> tensor on <tail>"."""
    if not torch.is_tensor(x) or x.dtype not in dtypes or (shapes is not None and tuple(x.shape) not in shapes) or \
            not x.is_contiguous() or (dev is not None and x.device != dev):
        raise _abi.MpeError("%s: %s is a contiguous %s %s tensor on %s" % (
            who, name, " / ".join(str(d).replace("torch.", "") for d in dtypes),
            text if text is not None else " or ".join(str(list(s)) for s in shapes), tail))


class Generations(object):
    """The guard of an autograd Function whose buffers are cached per key: next(key) at a forward -> the ticket its backward shows
    to stale(key, ticket), which is True behind a later forward of the same key."""

    def __init__(self):
        self._n = {}

    def next(self, key):
        n = self._n[key] = self._n.get(key, 0) + 1
        return n

    def stale(self, key, n):
        return self._n.get(key) != n
