"""CPU: MlpPolicy -- the packed actor layout of include/mpe_hip.h (MpePolicy), the reference-style action() and the refusals."""
import numpy as np
import pytest
import torch

from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.rollout import MlpPolicy, pack_actor


def mlp(widths, act=torch.nn.ReLU, seed=0):
    torch.manual_seed(seed)
    layers = []
    for k in range(len(widths) - 1):
        layers.append(torch.nn.Linear(widths[k], widths[k + 1]))
        if k + 2 < len(widths):
            layers.append(act())
    return torch.nn.Sequential(*layers)


@pytest.mark.parametrize("widths", [[18, 5], [18, 32, 5], [18, 64, 64, 5], [7, 16, 40, 5]])
def test_packing_layout(widths):
    m = mlp(widths)
    flat = pack_actor(m).numpy()
    assert flat.size % 16 == 0
    lins = [l for l in m if isinstance(l, torch.nn.Linear)]
    off = 0
    for k, lin in enumerate(lins):
        n_in = lin.in_features if k == 0 else 64
        n_out = 8 if k + 1 == len(lins) else 64
        W = flat[off:off + n_in * n_out].reshape(n_in, n_out)
        off += n_in * n_out
        b = flat[off:off + n_out]
        off += n_out
        want = np.zeros((n_in, n_out), np.float32)
        want[:lin.in_features, :lin.out_features] = lin.weight.detach().numpy().T
        assert np.array_equal(W, want)
        assert np.array_equal(b[:lin.out_features], lin.bias.detach().numpy()) and not b[lin.out_features:].any()
    assert not flat[off:].any()


def test_shared_actor_is_packed_once():
    m = mlp([10, 64, 5])
    pol = MlpPolicy(m)
    w, desc = pol.pack([10, 10, 10], "cpu", "greedy", 0)
    assert w.numel() == pack_actor(m).numel()
    assert [desc.offset[i] for i in range(3)] == [0, 0, 0]
    assert [desc.n_layers[i] for i in range(3)] == [2, 2, 2] and list(desc.width[0])[:3] == [10, 64, 5]
    w2, d2 = MlpPolicy([mlp([10, 5]), mlp([12, 5], seed=1)]).pack([10, 12], "cpu", "sample", 3)
    assert d2.offset[1] == pack_actor(mlp([10, 5])).numel() and d2.mode == _abi.MPE_POLICY_SAMPLE and d2.seed == 3


@pytest.mark.parametrize("act", [torch.nn.ReLU, torch.nn.Tanh])
def test_action_matches_numpy(act):
    mods = [mlp([6, 64, 64, 5], act, seed=1), mlp([4, 32, 5], act, seed=2)]
    pol = MlpPolicy(mods)
    rs = np.random.RandomState(0)
    obs = [rs.randn(300, 6).astype(np.float32), rs.randn(300, 4).astype(np.float32)]
    f = np.maximum if act is torch.nn.ReLU else (lambda x, _: np.tanh(x))
    for mode in ("greedy", "softmax"):
        rows = pol.action([torch.as_tensor(o) for o in obs], mode=mode)
        for i, m in enumerate(mods):
            x = obs[i].astype(np.float64)
            lins = [l for l in m if isinstance(l, torch.nn.Linear)]
            for k, lin in enumerate(lins):
                x = x @ lin.weight.detach().numpy().T.astype(np.float64) + lin.bias.detach().numpy()
                if k + 1 < len(lins):
                    x = f(x, 0.0)
            p = np.exp(x - x.max(1, keepdims=True))
            p /= p.sum(1, keepdims=True)
            if mode == "softmax":
                assert np.abs(rows[i].numpy() - p).max() < 1e-5
            else:
                assert np.array_equal(rows[i].numpy(), np.eye(5, dtype=np.float32)[x.argmax(1)])
    s = pol.action([torch.as_tensor(o) for o in obs], mode="sample", generator=torch.Generator().manual_seed(0))
    assert all(float(r.sum()) == 300 for r in s)


@pytest.mark.parametrize("bad,what", [
    (torch.nn.Sequential(torch.nn.Linear(6, 64), torch.nn.ReLU(), torch.nn.Linear(32, 5)), "takes 32 inputs"),
    (torch.nn.Sequential(torch.nn.Linear(6, 64), torch.nn.Sigmoid(), torch.nn.Linear(64, 5)), "unsupported layer"),
    (torch.nn.Sequential(torch.nn.Linear(6, 65), torch.nn.ReLU(), torch.nn.Linear(65, 5)), "hidden width 65"),
    (torch.nn.Sequential(torch.nn.Linear(6, 4)), "gives 4 outputs"),
    (torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.ReLU(), torch.nn.Linear(8, 8), torch.nn.ReLU(), torch.nn.Linear(8, 8),
                         torch.nn.ReLU(), torch.nn.Linear(8, 5)), "4 Linear layers"),
])
def test_refused_by_name(bad, what):
    with pytest.raises(_abi.MpeError, match=what):
        MlpPolicy(bad)


def test_input_width_mismatch_refused():
    with pytest.raises(_abi.MpeError, match="takes 6 inputs, its observation has 18"):
        MlpPolicy(mlp([6, 5])).pack([18], "cpu", "greedy", 0)
