"""On-policy minibatches on the device: mpe_adv_stats and mpe_onpolicy_batch bit-equal to the NumPy restatements of
THE ADVANTAGE STATISTICS RULE and THE MINIBATCH RULE (tests/_onpolicy_batch_ref.py) over the sweep's shapes, Minibatches end to end
behind PolicyLoop.run(values=) and gae, and {adv_stats, batch} inside a HIP graph with a device epoch counter.  mpe_adv_stats also
runs at N = T * B = 1 048 578 (257 chunks): its second launch stages the chunks' partials 256 at a time, and this is the one shape
that takes a second piece.  Every index of
both kernels was walked on the CPU under AddressSanitizer first
(tests/test_onpolicy_batch_cpu.py::test_host_walk_every_block_job_and_lane_under_the_sanitizers)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.onpolicy import Minibatches, Values, adv_stats, gae
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop

import _onpolicy_batch_ref as R

pytestmark = pytest.mark.gpu

_REF = {}


def _case(shape):
    """the synthetic trajectory and the restatement's statistics, computed once per shape and left unchanged"""
    key = (shape[0], shape[1], shape[2], tuple(shape[3]), shape[4])
    if key not in _REF:
        tr = {"adv": R.make_adv(shape)} if shape in R.STATS_SHAPES else R.make_traj(shape)
        stats = R.adv_stats(tr["adv"])
        for x in list(tr.values()) + [stats]:
            if x is not None:
                x.setflags(write=False)
        _REF[key] = (tr, stats)
    return _REF[key]


# ---- the kernel sweep at the ABI --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES + R.STATS_SHAPES, ids=R.SHAPE_IDS + R.STATS_IDS)
def test_adv_stats_kernel_sweep(shape):
    """the workspace zeroed and poisoned.  The last shape has N = T * B = 1 048 578, 257 chunks: k_adv_finish stages a second piece --
    one chunk of two elements -- into the LDS arrays its lanes have just added from."""
    tr, stats = _case(shape)
    dt = R.device_traj({"adv": tr["adv"]})
    for poison in (False, True):
        rc, got, canary_ok = R.run_stats(dt, shape, poison=poison)
        assert rc == 0 and canary_ok
        assert R.same_bits(got, stats), (shape, poison, got, stats)


@pytest.mark.parametrize("shape", R.SHAPES, ids=R.SHAPE_IDS)
def test_onpolicy_batch_kernel_sweep(shape):
    T, A, B, widths, dim_c, M = shape
    tr, stats = _case(shape)
    dt = R.device_traj(tr)
    d_stats = torch.as_tensor(np.array(stats), device=dt["adv"].device)
    N = T * B
    orders = {}
    for epoch, with_stats, with_logp in ((3, True, True), (4, False, False)):
        order = orders[epoch] = R.perm(N, R.SEED, epoch).astype(np.int64)
        seen = []
        for first, m in R.minibatches(N, M):
            got = R.run_batch(dt, shape, first, m, R.SEED, epoch, stats=d_stats if with_stats else None, want_logp=with_logp,
                              want_joint=with_stats)
            assert got["rc"] == 0, got["error"]
            assert got["canary_ok"], (shape, first, "a canary row behind an output was written")
            want = R.batch(tr, shape, order[first:first + m], stats if with_stats else None)
            if not with_logp:
                want["logp"] = None
                assert got["logp_untouched"], "logp is absent: nothing may be written for it"
            if not with_stats:
                want["joint"] = None
            else:
                assert R.same_bits(got["joint"], np.concatenate(got["obs"], axis=1))      # the per-agent blocks side by side
            assert R.first_difference(got, want) is None, (shape, epoch, first, R.first_difference(got, want))
            seen.append(got["idx"])
        assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(N))      # the minibatches partition the trajectory
    assert N < 3 or not np.array_equal(orders[3], orders[4])                    # two epochs differ


def test_epoch_add_is_read_on_the_device():
    shape = R.SHAPES[1]
    T, A, B, widths, dim_c, M = shape
    tr, stats = _case(shape)
    dt = R.device_traj(tr)
    add = torch.tensor([2 ** 32 + 1], dtype=torch.int64, device=dt["adv"].device)
    got = R.run_batch(dt, shape, 0, M, R.SEED, 4, epoch_add=add)
    assert got["rc"] == 0 and np.array_equal(got["idx"], R.perm(T * B, R.SEED, 2 ** 32 + 5).astype(np.int64)[:M])


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _mlp(n_in, n_out, hidden=16):
    return nn.Sequential(nn.Linear(n_in, hidden), nn.Tanh(), nn.Linear(hidden, n_out)).cuda()


def _check_batch_against_the_trajectory(mb, batch, traj, g, stats):
    t, b = batch.t.cpu().numpy(), batch.b.cpu().numpy()
    assert np.array_equal(t * mb.B + b, batch.idx.cpu().numpy())
    tt, bb = torch.as_tensor(t, device=mb.device), torch.as_tensor(b, device=mb.device)
    for i in range(mb.A):
        rows = torch.stack([traj.obs_in[int(t[r])][i][int(b[r])] for r in range(batch.M)])
        assert torch.equal(batch.obs_n[i], rows), ("obs", i)
        assert torch.equal(batch.act[i], traj.act[tt, i, bb]), ("act", i)
        assert torch.equal(batch.ret[i], g.ret[tt, i, bb]) and torch.equal(batch.val[i], traj.val[tt, i, bb]), i
        if traj.logp is not None:
            assert torch.equal(batch.logp[i], traj.logp[tt, i, bb]), ("logp", i)
        if traj.utter is not None:
            assert torch.equal(batch.utter[i], traj.utter[tt, i, bb]), ("utter", i)
        raw = g.adv[tt, i, bb].cpu().numpy()
        want = R.normalise(raw, stats[i]) if stats is not None else raw
        assert R.same_bits(batch.adv[i].cpu().numpy(), want), ("adv", i)
    if batch.joint_obs is not None:
        assert torch.equal(batch.joint_obs, torch.cat(batch.obs_n, dim=1))


def test_end_to_end_simple_spread():
    torch.manual_seed(3)
    env = mpe.make_env("simple_spread", batch_size=7, seed=1)
    pi = Actors(env, [_mlp(18, 5) for _ in range(3)], mode="sample", seed=2, logp=True)
    loop = PolicyLoop(env, pi, episode_len=5)
    V = Values(env, [_mlp(18, 1) for _ in range(3)])
    traj = loop.run(12, values=V)
    g = gae(traj, 0.95, 0.9)
    mb = Minibatches(traj, g, 20, seed=9, joint=True)
    torch.cuda.synchronize()
    stats = mb.stats.cpu().numpy()
    assert R.same_bits(stats, R.adv_stats(g.adv.cpu().numpy())) and R.same_bits(adv_stats(g).cpu().numpy(), stats)
    assert len(mb) == 5 and (mb.N, mb.widths, mb.dim_c) == (84, [18, 18, 18], 0)
    seen, sizes = [], []
    for batch in mb.epoch(1):
        assert np.array_equal(batch.idx.cpu().numpy(), R.perm(84, 9, 1).astype(np.int64)[len(seen) * 20:len(seen) * 20 + batch.M])
        _check_batch_against_the_trajectory(mb, batch, traj, g, stats)
        seen.append(batch.idx.cpu().numpy())
        sizes.append(batch.M)
    assert sizes == [20, 20, 20, 20, 4] and np.array_equal(np.sort(np.concatenate(seen)), np.arange(84))
    assert [b.M for b in mb.epoch(2, drop_last=True)] == [20] * 4
    assert mb.batch(1, 0) is mb.batch(2, 0)      # one set of output tensors per M
    raw = Minibatches(traj, g, 84, seed=9, normalise=False)
    assert raw.stats is None and raw.batch(0, 0).joint_obs is None
    _check_batch_against_the_trajectory(raw, raw.batch(0, 0), traj, g, None)
    with pytest.raises(_abi.MpeError, match="Minibatches.batch: k = 5"):
        mb.batch(0, 5)


def test_end_to_end_utterances_and_no_logp():
    torch.manual_seed(3)
    env = mpe.make_env("simple_reference", batch_size=6, seed=11)
    widths = [int(env._obs_off[i + 1] - env._obs_off[i]) for i in range(env.n)]
    pi = Actors(env, [_mlp(d, 5 + env.world.dim_c) for d in widths], mode="sample", seed=5)
    loop = PolicyLoop(env, pi, episode_len=4)
    V = Values(env, [_mlp(d, 1) for d in widths])
    traj = loop.run(6, values=V)
    assert traj.utter is not None and traj.logp is None
    g = gae(traj, 0.95, 0.9)
    mb = Minibatches(traj, g, 36, seed=1)
    batch = mb.batch(0, 0)
    torch.cuda.synchronize()
    assert batch.logp is None and batch.utter.shape == (env.n, 36, env.world.dim_c) and mb.dim_c == env.world.dim_c
    assert float(traj.utter.abs().sum()) > 0
    _check_batch_against_the_trajectory(mb, batch, traj, g, mb.stats.cpu().numpy())


# ---- inside a HIP graph -----------------------------------------------------------------------------------------------------------
def test_stats_and_batch_in_a_graph_with_an_epoch_counter():
    shape = R.SHAPES[3]
    T, A, B, widths, dim_c, M = shape
    tr, stats = _case(shape)
    dt = R.device_traj(tr)
    dev = dt["adv"].device

    class Traj(object):
        pass
    traj = Traj()
    traj.obs_in_flat, traj.act, traj.utter, traj.logp, traj.val, traj.obs_widths = dt["obs_in"], dt["act"], None, dt["logp"], dt["val"], widths
    from multiagent_particle_envs_amd.onpolicy import GaeResult
    g = GaeResult(dt["adv"], dt["ret"])
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mb = Minibatches(traj, g, M, seed=R.SEED, joint=True, epoch_counter=counter)      # the code objects outside the capture
        out = mb.batch(7, 1)
        out.adv.zero_()
        out.idx.zero_()
        mb.stats.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            mb.restats()
            assert mb.batch(7, 1) is out
    torch.cuda.current_stream().wait_stream(s)

    def got():
        torch.cuda.synchronize()
        return {"idx": out.idx.cpu().numpy(), "obs": [o.cpu().numpy() for o in out.obs_n], "act": out.act.cpu().numpy(), "utter": None,
                "logp": out.logp.cpu().numpy(), "adv": out.adv.cpu().numpy(), "ret": out.ret.cpu().numpy(), "val": out.val.cpu().numpy(),
                "joint": out.joint_obs.cpu().numpy()}

    def want(epoch, trj, st):
        return R.batch(trj, shape, R.perm(T * B, R.SEED, epoch).astype(np.int64)[M:2 * M], st)
    graph.replay()
    first = got()
    assert R.first_difference(first, want(7, tr, stats)) is None
    counter.add_(1)                                                  # bumped on the device: the next replay is epoch 8's shuffle
    graph.replay()
    second = got()
    assert R.first_difference(second, want(8, tr, stats)) is None and not np.array_equal(first["idx"], second["idx"])
    adv2 = (np.array(tr["adv"]) * np.float32(-0.5) + np.float32(1.25)).astype(np.float32)
    dt["adv"].copy_(torch.as_tensor(adv2, device=dev))               # rewritten in place: the graph reads the same tensor
    graph.replay()
    third = got()
    stats2 = R.adv_stats(adv2)
    assert not R.same_bits(stats2, stats) and R.same_bits(mb.stats.cpu().numpy(), stats2)
    tr2 = dict(tr, adv=adv2)
    assert R.first_difference(third, want(8, tr2, stats2)) is None


def test_example_runs_with_minibatches():
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "ppo_spread.py"), "--worlds", "16", "--updates", "2", "--epochs", "2",
                        "--minibatch", "96"], capture_output=True, text=True, cwd=root, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2
    for l in lines:
        assert np.isfinite(l["policy_loss"]) and np.isfinite(l["value_loss"]) and np.isfinite(l["mean_return"])
