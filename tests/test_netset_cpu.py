"""CPU: netset.py -- the packed layout stated once.  For every kind of set (Actors with a mover, a speaker-only agent and moving
speakers; Values decentralised and centralised; Critics; MlpPolicy) and at the layout's shape edges, pack() is byte for byte the NumPy
restatement of tests/_actor_ref.py (MlpPolicy's 8-wide layout: rollout.pack_actor, which tests/test_policy_cpu.py pins), module_views
hands back the modules' own weights and biases, every float outside the views is +0.0 by bit pattern, and what is written through
the views comes back in the modules by the walk DeviceAdam.write_back makes.  Plus the structure itself: one pack() for the three
classes, and nobody outside netset.py assigns `_frozen`."""
import glob
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi, netset
from multiagent_particle_envs_amd.optim import DeviceAdam
from multiagent_particle_envs_amd.rollout import MlpPolicy, pack_actor

import _actor_ref as R


def mlp(sizes, bias=(), act=nn.Tanh, seed=0):
    """Linear layers of `sizes` with `act` between them; bias: the indices of the Linear layers built with bias=False"""
    torch.manual_seed(seed)
    mods = []
    for k in range(len(sizes) - 1):
        mods += [nn.Linear(sizes[k], sizes[k + 1], bias=k not in bias)] + ([act()] if k + 2 < len(sizes) else [])
    return nn.Sequential(*mods)


def lins_of(m):
    return [x for x in m if isinstance(x, nn.Linear)]


def ref_pack(modules):
    """_actor_ref.pack of each distinct module, in order (a layer without a bias packs a zero bias)"""
    seen, parts = set(), []
    for m in modules:
        if id(m) not in seen:
            seen.add(id(m))
            parts.append(R.pack([(lin.weight.detach().numpy(), lin.bias.detach().numpy() if lin.bias is not None else
                                  np.zeros(lin.out_features, np.float32)) for lin in lins_of(m)]))
    return np.concatenate(parts)


def check_views(what, flat, per_module, last_wide, back):
    """views == parameters; +0.0 outside the views; written through the views and copied back by back() == what was written"""
    views, total = netset.module_views(what, flat, last_wide)
    assert total == flat.numel() and len(views) == len(per_module)
    mask = torch.zeros_like(flat)
    for vs, ms, lins in zip(views, netset.module_views(what, mask, last_wide)[0], per_module):
        assert len(vs) == len(lins)
        for (w, b), (mw, mb), lin in zip(vs, ms, lins):
            assert w.shape == lin.weight.shape and torch.equal(w, lin.weight)
            assert b.shape == (lin.out_features,) and torch.equal(b, lin.bias if lin.bias is not None else torch.zeros_like(b))
            mw.fill_(1.0)
            mb.fill_(1.0)
    assert int(mask.sum()) == sum(lin.weight.numel() + lin.out_features for lins in per_module for lin in lins)      # (no view overlaps)
    assert not flat.view(torch.int32)[mask == 0].any(), "padding is not +0.0 bit for bit"
    written = []
    for vs in views:
        for w, b in vs:
            w.copy_(torch.randn(w.shape))
            b.copy_(torch.randn(b.shape))
            written.append((w.clone(), b.clone()))
    back()
    k = 0
    for lins in per_module:
        for lin in lins:
            assert torch.equal(lin.weight, written[k][0]) and (lin.bias is None or torch.equal(lin.bias, written[k][1]))
            k += 1


def make_net(kind):
    if kind == "actors_speaker_and_mover":      # a speaker-only agent (3 logits) and a mover (5); 2 and 3 layers, hidden 1 and 64
        env = mpe.make_env("simple_speaker_listener", batch_size=4, device="cpu")
        D = [int(env._obs_off[i + 1] - env._obs_off[i]) for i in range(2)]
        net = mpe.Actors(env, [mlp([D[0], 1, env.world.dim_c]), mlp([D[1], 64, 7, 5], bias=(1,), act=nn.ReLU, seed=1)])
        assert (net.movable, net.speaks) == ([False, True], [True, False])
    elif kind == "actors_moving_speakers_shared":      # 5 + dim_c logits, one module object for both agents
        env = mpe.make_env("simple_reference", batch_size=4, device="cpu")
        net = mpe.Actors(env, mlp([int(env._obs_off[1]), 33, 5 + env.world.dim_c]))
        assert net.movable == [True, True] and net.speaks == [True, True] and net.modules[0] is net.modules[1]
    else:
        env = mpe.make_env("simple_spread", batch_size=4, device="cpu")
        if kind == "values_two_agents_share":      # agents 0 and 2 share one module object; agent 1's is a lone Linear layer
            m = mlp([18, 64, 64, 1], bias=(0, 2))
            net = mpe.Values(env, [m, nn.Sequential(nn.Linear(18, 1)), m])
        elif kind == "values_centralised":
            net = mpe.Values(env, [mlp([54, 20, 1], seed=i) for i in range(3)], centralised=True)
        else:
            net = mpe.Critics(env, [mlp([69, 64, 1, 1], seed=i, bias=(2,)) for i in range(3)])
    return net


KINDS = ["actors_speaker_and_mover", "actors_moving_speakers_shared", "values_two_agents_share", "values_centralised", "critics"]


@pytest.mark.parametrize("kind", KINDS)
def test_pack_views_and_write_back(kind):
    net = make_net(kind)
    wts, aset = net.pack()
    assert wts.dtype == torch.float32 and wts.numel() % 16 == 0 and aset.weights is None      # (no device pointer on the CPU)
    assert wts.numpy().tobytes() == ref_pack(net.modules).tobytes()
    per_module = [lins_of(m) for m, _ in net.distinct()]
    assert [id(m) for m, _ in net.distinct()] == list(dict.fromkeys(id(m) for m in net.modules))
    offs, at = {}, 0
    for m, lins in net.distinct():
        offs[id(m)] = at
        at += netset.layout(lins)[1]
    assert [aset.offset[i] for i in range(net.A)] == [offs[id(m)] for m in net.modules] and at == wts.numel()
    for i, m in enumerate(net.modules):
        assert aset.n_layers[i] == len(lins_of(m))
        assert list(aset.width[i])[:aset.n_layers[i] + 1] == [lins_of(m)[0].in_features] + [lin.out_features for lin in lins_of(m)]
        assert aset.activation[i] == (_abi.MPE_POLICY_TANH if any(isinstance(x, nn.Tanh) for x in m) else _abi.MPE_POLICY_RELU)
    opt = object.__new__(DeviceAdam)      # (the constructor allocates device buffers; write_back reads these two only)
    opt.nets, opt.weights = [net], [wts]
    check_views(net, wts, per_module, 16, opt.write_back)


# input width 1 and MPE_ACTOR_MAX_INPUT, hidden width 1 and 64, last width 1, 5 and 16, 1 to 3 Linear layers, a layer without bias
EDGES = [([1, 1], ()), ([256, 16], (0,)), ([1, 64, 5], ()), ([256, 1, 16], (1,)), ([1, 1, 1, 1], ()), ([256, 64, 64, 16], (0, 1, 2)),
         ([_abi.MPE_ACTOR_MAX_INPUT, 64, 1, 5], (1,))]


@pytest.mark.parametrize("sizes,bias", EDGES, ids=["-".join(str(n) for n in s) + ("_nobias" + "".join(map(str, b)) if b else "")
                                                    for s, b in EDGES])
def test_layout_edges(sizes, bias):
    from multiagent_particle_envs_amd.policy import pack_actor16
    m = mlp(sizes, bias=bias, seed=len(sizes))
    lins = lins_of(m)
    rows, total = netset.layout(lins)
    assert total % 16 == 0 and rows[0][0] == 0 and [r[1] for r in rows] == [sizes[0]] + [64] * (len(lins) - 1)
    assert [r[2] for r in rows] == [64] * (len(lins) - 1) + [16]
    flat = pack_actor16(m, sizes[-1])
    assert flat.numpy().tobytes() == ref_pack([m]).tobytes()
    check_views([lins], flat, [lins], 16, lambda: netset.unpack_layers(lins, flat))
    if sizes[-1] == 5:      # the 8-wide layout of MpePolicy: the same walk, the whole padded to a multiple of 16 floats
        flat8 = pack_actor(m)
        assert flat8.numel() == netset.layout(lins, 8)[1] and flat8.numel() % 16 == 0
        check_views([lins], flat8, [lins], 8, lambda: netset.unpack_layers(lins, flat8, 8))


def test_mlp_policy_pack_is_pack_actor_per_distinct_module():
    a, b = mlp([10, 64, 5]), mlp([12, 5], bias=(0,), seed=1)
    pol = MlpPolicy([a, b, a])
    w, desc = pol.pack([10, 12, 10], "cpu", "sample", 3)
    assert w.numpy().tobytes() == torch.cat([pack_actor(a), pack_actor(b)]).numpy().tobytes()
    assert [desc.offset[i] for i in range(3)] == [0, pack_actor(a).numel(), 0] and desc.mode == _abi.MPE_POLICY_SAMPLE and desc.seed == 3
    assert [desc.n_layers[i] for i in range(3)] == [2, 1, 2] and list(desc.width[1])[:2] == [12, 5]

    def back():
        at = netset.unpack_layers(lins_of(a), w, 8)
        netset.unpack_layers(lins_of(b), w, 8, at)
    check_views([lins_of(a), lins_of(b)], w, [lins_of(a), lins_of(b)], 8, back)


def test_one_pack_for_the_three_classes():
    from multiagent_particle_envs_amd.learner import Critics
    from multiagent_particle_envs_amd.onpolicy import Values
    from multiagent_particle_envs_amd.policy import Actors
    for cls in (Actors, Values, Critics):
        assert issubclass(cls, netset.NetSet)
        for name in ("pack", "freeze", "unfreeze", "packed", "attach", "attached", "distinct", "_check"):
            assert getattr(cls, name) is getattr(netset.NetSet, name), (cls.__name__, name)


def test_nobody_outside_netset_assigns_frozen():
    pkg = os.path.dirname(os.path.abspath(netset.__file__))
    assigns = re.compile(r"_frozen\b[^=\n]*(?<![=!<>])=(?!=)|setattr\([^)\n]*_frozen")
    found = []
    for path in sorted(glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True)):
        with open(path) as f:
            for n, line in enumerate(f, 1):
                code = line.split("#", 1)[0]
                if os.path.basename(path) != "netset.py" and assigns.search(code):
                    found.append("%s:%d: %s" % (os.path.relpath(path, pkg), n, line.strip()))
    assert not found, found
    with open(os.path.join(pkg, "netset.py")) as f:
        assert len(assigns.findall(f.read())) == 2      # NetSet.__init__ and NetSet.attach: the scan sees what it looks for
