"""CPU: policy.Actors without a device -- the packed layout (include/mpe_hip.h, MpeActorSet) against a NumPy restatement, the head
layout per agent kind, the refusals by name, and Actors.reference against a NumPy fp64 forward pass."""
import numpy as np
import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.policy import Actors


def cpu_env(name, **kw):
    return mpe.make_env(name, batch_size=8, device="cpu", **kw)


def widths(env):
    return [int(env._obs_off[i + 1] - env._obs_off[i]) for i in range(len(env.world.agents))]


def n_out(env, i):
    a = env.world.agents[i]
    return 5 * bool(a.movable) + env.world.dim_c * (not a.silent)


def mlp(sizes, act=torch.nn.ReLU, dtype=torch.float32):
    layers = []
    for k in range(len(sizes) - 1):
        layers.append(torch.nn.Linear(sizes[k], sizes[k + 1], dtype=dtype))
        if k + 2 < len(sizes):
            layers.append(act())
    return torch.nn.Sequential(*layers)


def actors(env, hidden=(64, 64), act=torch.nn.ReLU, seed=0):
    torch.manual_seed(seed)
    return [mlp([D] + list(hidden) + [n_out(env, i)], act) for i, D in enumerate(widths(env))]


def np_pack(module):
    """[in][out'] + bias[out'] per layer: in = input width, then 64; out' = 64, 16 for the last; zero padding."""
    lins = [m for m in module if isinstance(m, torch.nn.Linear)]
    parts = []
    for k, lin in enumerate(lins):
        n_in = lin.in_features if k == 0 else 64
        wide = 16 if k + 1 == len(lins) else 64
        w = np.zeros((n_in, wide), np.float32)
        w[:lin.in_features, :lin.out_features] = lin.weight.detach().numpy().T
        b = np.zeros(wide, np.float32)
        b[:lin.out_features] = lin.bias.detach().numpy()
        parts += [w.ravel(), b]
    return np.concatenate(parts)


@pytest.mark.parametrize("hidden", [(64, 64), (20,), ()])
def test_packing_layout(hidden):
    env = cpu_env("simple_tag")
    mods = actors(env, hidden)
    wts, aset = Actors(env, mods, mode="greedy").pack()
    want, off = [], 0
    for i, m in enumerate(mods):
        blob = np_pack(m)
        assert aset.offset[i] == off and off % 16 == 0
        assert aset.n_layers[i] == len(hidden) + 1
        assert list(aset.width[i])[:len(hidden) + 2] == [widths(env)[i]] + list(hidden) + [5]
        want.append(blob)
        off += blob.size
    assert np.array_equal(wts.numpy(), np.concatenate(want))
    assert aset.n_agents == 4 and aset.dim_c == 0 and aset.mode == _abi.MPE_POLICY_GREEDY


def test_shared_modules_share_one_copy():
    env = cpu_env("simple_spread")
    m = mlp([18, 64, 5])
    wts, aset = Actors(env, m).pack()
    assert wts.numel() == np_pack(m).size and [aset.offset[i] for i in range(3)] == [0, 0, 0]
    other = mlp([18, 64, 5])
    wts, aset = Actors(env, [m, other, m]).pack()
    assert wts.numel() == 2 * np_pack(m).size and [aset.offset[i] for i in range(3)] == [0, np_pack(m).size, 0]


def test_head_layout():
    env = cpu_env("simple_speaker_listener")      # a speaker that cannot move, a listener that cannot speak
    pi = Actors(env, actors(env))
    assert pi.n_out == [3, 5] and pi.movable == [False, True] and pi.speaks == [True, False] and pi.dim_c == 3
    _, aset = pi.pack()
    assert [aset.movable[i] for i in range(2)] == [0, 1] and [aset.speaks[i] for i in range(2)] == [1, 0] and aset.dim_c == 3
    env = cpu_env("simple_reference")             # both heads
    pi = Actors(env, actors(env))
    assert pi.n_out == [15, 15] and pi.dim_c == 10
    env = cpu_env("simple_spread")                # moves only
    pi = Actors(env, actors(env))
    assert pi.n_out == [5, 5, 5] and pi.dim_c == 0


@pytest.mark.parametrize("build,needle", [
    (lambda: mlp([17, 64, 5]), "takes 17 inputs, its observation has 18"),
    (lambda: mlp([18, 64, 6]), "gives 6 outputs (need 5)"),
    (lambda: mlp([18, 65, 5]), "hidden width 65 > 64"),
    (lambda: mlp([18, 32, 32, 32, 5]), "4 Linear layers (at most 3)"),
    (lambda: mlp([18, 64, 5], act=torch.nn.Sigmoid), "unsupported layer 1 (Sigmoid)"),
    (lambda: mlp([18, 64, 5], dtype=torch.float64), "is not float32"),
])
def test_refusals_by_name(build, needle):
    env = cpu_env("simple_spread")
    with pytest.raises(_abi.MpeError) as e:
        Actors(env, build())
    assert "Actors" in str(e.value) and needle in str(e.value), str(e.value)


def test_speaking_output_width_refused():
    env = cpu_env("simple_reference")
    with pytest.raises(_abi.MpeError) as e:
        Actors(env, [mlp([21, 64, 5]), mlp([21, 64, 15])])
    assert "gives 5 outputs (need 15)" in str(e.value) and "agent 0" in str(e.value)


@pytest.mark.parametrize("act", [torch.nn.ReLU, torch.nn.Tanh])
def test_reference_against_numpy(act):
    env = cpu_env("simple_reference")
    mods = actors(env, (64, 20), act, seed=3)
    pi = Actors(env, mods)
    rs = np.random.RandomState(0)
    obs = [rs.uniform(-1, 1, size=(8, D)).astype(np.float32) for D in widths(env)]
    ref = pi.reference([torch.as_tensor(o) for o in obs])
    for i, m in enumerate(mods):
        x = obs[i].astype(np.float64)
        lins = [l for l in m if isinstance(l, torch.nn.Linear)]
        for k, lin in enumerate(lins):
            x = x @ lin.weight.detach().numpy().astype(np.float64).T + lin.bias.detach().numpy().astype(np.float64)
            if k + 1 < len(lins):
                x = np.maximum(x, 0) if act is torch.nn.ReLU else np.tanh(x)
        assert ref[i][0].dtype == torch.float64
        assert np.abs(ref[i][0].numpy() - x[:, :5]).max() < 1e-12
        assert np.abs(ref[i][1].numpy() - x[:, 5:]).max() < 1e-12
