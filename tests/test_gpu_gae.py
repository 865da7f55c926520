"""On-policy returns on the device: mpe_gae bit-equal to the NumPy restatement of THE GAE RULE (tests/_gae_ref.py) over
the sweep's shapes and inputs, Values against fp64 with per-agent pointers and widths, PolicyLoop.run(values=) end to end, and
gae_tensors inside a HIP graph.  Every index of the kernel was walked on the CPU under AddressSanitizer first
(tests/test_gae_cpu.py::test_host_walk_every_lane_under_the_sanitizers)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.onpolicy import Values, gae, gae_tensors
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop

import _gae_ref as G
import _td_target_ref as T

pytestmark = pytest.mark.gpu

_REF = {}


def _case(shape, kind):
    """inputs and the restatement's outputs, computed once per (shape, kind) and left unchanged"""
    key = (tuple(shape), kind)
    if key not in _REF:
        rew, done, val, boot = G.make_inputs(shape, kind)
        adv, ret = G.gae(rew, done, val, boot, G.GAMMA, G.LAM, shape[3], shape[4])
        for x in (rew, done, val, boot, adv, ret):
            x.setflags(write=False)
        _REF[key] = (rew, done, val, boot, adv, ret)
    return _REF[key]


# ---- the kernel sweep -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("shape", G.SHAPES, ids=G.SHAPE_IDS)
def test_gae_kernel_sweep(shape, kind):
    Tn, A, B, L, p = shape
    rew, done, val, boot, adv, ret = _case(shape, kind)
    out = G.run_abi(rew, done, val, boot, G.GAMMA, G.LAM, L, p)
    assert out["rc"] == 0, out["error"]
    assert out["canary_ok"], (shape, kind, "a store landed behind the last row")
    assert G.same_bits(out["adv"], adv), (shape, kind, "adv")
    assert G.same_bits(out["ret"], ret), (shape, kind, "ret")
    if kind == "nonfinite":
        own = done != 0
        assert np.isfinite(out["adv"]).all() and G.same_bits(out["adv"][own], (rew - val)[own])
    # adv only, ret only: the same bits
    a = G.run_abi(rew, done, val, boot, G.GAMMA, G.LAM, L, p, want=("adv",))
    r = G.run_abi(rew, done, val, boot, G.GAMMA, G.LAM, L, p, want=("ret",))
    assert a["rc"] == 0 and r["rc"] == 0 and a["canary_ok"] and r["canary_ok"] and a["ret"] is None and r["adv"] is None
    assert G.same_bits(a["adv"], adv) and G.same_bits(r["ret"], ret)
    if B % 4 == 0:      # the scalar path on the shape the 16-byte path just ran: the same bits
        s = G.run_abi(rew, done, val, boot, G.GAMMA, G.LAM, L, p, misalign=True)
        assert s["rc"] == 0 and s["canary_ok"] and G.same_bits(s["adv"], adv) and G.same_bits(s["ret"], ret)


# ---- Values -----------------------------------------------------------------------------------------------------------------------
def _mlp(D, n_out, hidden=(64, 64)):
    mods, k = [], D
    for h in hidden:
        mods += [nn.Linear(k, h), nn.ReLU()]
        k = h
    return nn.Sequential(*(mods + [nn.Linear(k, n_out)])).cuda()


def _over_bar(v, ref64):
    v, ref64 = v.cpu().numpy(), ref64.cpu().numpy()
    return float((np.abs(v - ref64) / (T.Q_BAR * np.maximum(1, np.abs(ref64)))).max())


def test_values_per_agent_pointers_and_widths(record_parity):
    torch.manual_seed(0)
    env = mpe.make_env("simple_tag", batch_size=5, seed=1)
    widths = [int(env._obs_off[i + 1] - env._obs_off[i]) for i in range(env.n)]
    assert len(set(widths)) == 2
    V = Values(env, [_mlp(d, 1) for d in widths])
    obs_n = env.reset()
    v = V.v(obs_n)
    assert v.shape == (env.n, 5)
    m = _over_bar(v, V.reference(obs_n))
    print("Values.v simple_tag: worst |v - v64| / bar %.3f" % m)
    assert m < 1.0
    record_parity("gae_values_decentralised", {"worst_error_over_bar": m, "bar": "1e-5 * max(1, |v|)"})
    # critic i fed agent i's block alone, Critics-style (one pointer for the whole set): the same bits
    wts, aset = V.pack(env.world.device)
    for i in range(env.n):
        one = _abi.MpeActorSet()
        one.n_agents, one.mode, one.weights = env.n, _abi.MPE_POLICY_VALUE, wts.data_ptr()
        for j in range(env.n):
            one.offset[j], one.n_layers[j], one.activation[j] = aset.offset[i], aset.n_layers[i], aset.activation[i]
            for l in range(4):
                one.width[j][l] = aset.width[i][l]
        q = torch.zeros((env.n, 5), dtype=torch.float32, device=env.world.device)
        _abi.check(_abi.lib().mpe_critic_q(C.byref(one), (C.c_void_p * env.n)(*([obs_n[i].data_ptr()] * env.n)), 5, q.data_ptr(), None, None,
                                           _abi.raw_stream(env.world.device)), "mpe_critic_q")
        assert all(torch.equal(q[j], v[i]) for j in range(env.n)), i
    # out=, freeze / unfreeze as Critics'
    mine = torch.zeros((env.n, 5), dtype=torch.float32, device=env.world.device)
    assert V.v(obs_n, out=mine) is mine and torch.equal(mine, v)
    V.freeze()
    with torch.no_grad():
        V.modules[1][4].bias[0] += 0.5
    assert torch.equal(V.v(obs_n), mine)
    V.unfreeze()
    v2 = V.v(obs_n)
    assert not torch.equal(v2[1], mine[1]) and torch.equal(v2[0], mine[0])


def test_values_centralised(record_parity):
    torch.manual_seed(1)
    env = mpe.make_env("simple_spread", batch_size=7, seed=1)
    V = Values(env, [_mlp(54, 1) for _ in range(3)], centralised=True)
    obs_n = env.reset()
    v = V.v(obs_n)
    m = _over_bar(v, V.reference(obs_n))
    print("Values.v centralised simple_spread: worst |v - v64| / bar %.3f" % m)
    assert v.shape == (3, 7) and m < 1.0
    record_parity("gae_values_centralised", {"worst_error_over_bar": m, "bar": "1e-5 * max(1, |v|)"})


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _loop(values_seed=5):
    torch.manual_seed(3)
    env = mpe.make_env("simple_spread", batch_size=7, seed=1)
    pi = Actors(env, [_mlp(18, 5) for _ in range(3)], mode="sample", seed=2, logp=True)
    loop = PolicyLoop(env, pi, episode_len=5)
    torch.manual_seed(values_seed)
    V = Values(env, [_mlp(18, 1) for _ in range(3)])
    return env, pi, loop, V


def test_end_to_end(record_parity):
    env, pi, loop, V = _loop()
    before = [o.clone() for o in loop.run(3, record=False)[0]]      # three steps first: the trajectory starts at phase 3
    traj = loop.run(12, values=V)
    torch.cuda.synchronize()
    assert (traj.episode_len, traj.episode_phase) == (5, 3) and loop.t == 15
    assert traj.val.shape == (12, 3, 7) and traj.boot.shape == (3, 3, 7) and len(traj.obs_in) == 12
    enders = [t for t in range(12) if G.ends(t, 12, 5, 3)]
    assert enders == [1, 6, 11]
    restarts, inside = 0, 0
    for t in range(12):
        if (3 + t) % 5 == 0:      # the loop restarted every world in front of this step: decided on the reset's observation
            want = [o.clone() for o in loop.device_reset((3 + t) // 5)]
            restarts += 1
        else:
            want = before if t == 0 else traj.obs[t - 1]
            inside += 1
        assert all(torch.equal(a, b) for a, b in zip(traj.obs_in[t], want)), t
        assert torch.equal(traj.val[t], V.v(traj.obs_in[t])), t
    assert (restarts, inside) == (2, 10)
    for k, t in enumerate(enders):
        assert torch.equal(traj.boot[k], V.v(traj.obs[t])), (k, t)
    for t in (2, 7):              # ... and the reset's observation is NOT what the truncated step bootstraps from
        assert not torch.equal(traj.obs_in[t][0], traj.obs[t - 1][0])
    g = gae(traj, 0.95, 0.9)
    adv, ret = G.gae(traj.rew.cpu().numpy(), traj.done.cpu().numpy(), traj.val.cpu().numpy(), traj.boot.cpu().numpy(), 0.95, 0.9, 5, 3)
    assert G.same_bits(g.adv.cpu().numpy(), adv) and G.same_bits(g.ret.cpu().numpy(), ret)
    again = gae(traj, 0.95, 0.9, out=g)
    assert again is g and G.same_bits(g.adv.cpu().numpy(), adv)
    record_parity("gae_end_to_end", {"steps": 12, "segments": 3, "restart_steps": restarts, "steps_inside_an_episode": inside,
                                     "values_bit_equal": 12, "boots_bit_equal": 3, "adv_ret_bit_equal_elements": int(adv.size)})


def test_values_leave_the_rollout_alone():
    env_a, pi_a, loop_a, V = _loop()
    env_b, pi_b, loop_b, _ = _loop()
    with_v, without = loop_a.run(12, values=V), loop_b.run(12)
    torch.cuda.synchronize()
    for name in ("act", "rew", "done", "obs_flat", "logp"):
        assert torch.equal(getattr(with_v, name), getattr(without, name)), name
    assert not hasattr(without, "val") and not hasattr(without, "obs_in")


# ---- inside a HIP graph -----------------------------------------------------------------------------------------------------------
def test_gae_tensors_in_a_graph():
    shape = G.SHAPES[3]
    Tn, A, B, L, p = shape
    rew, done, val, boot, adv, ret = _case(shape, "random")
    dev = torch.device("cuda", torch.cuda.current_device())
    d_rew, d_val, d_boot = (torch.as_tensor(np.array(x), device=dev) for x in (rew, val, boot))
    d_done = torch.as_tensor(np.array(done), device=dev).bool()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = gae_tensors(d_rew, d_done, d_val, d_boot, G.GAMMA, G.LAM, L, p)      # the code object outside the capture
        out.adv.zero_()
        out.ret.zero_()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            gae_tensors(d_rew, d_done, d_val, d_boot, G.GAMMA, G.LAM, L, p, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    assert G.same_bits(out.adv.cpu().numpy(), adv) and G.same_bits(out.ret.cpu().numpy(), ret)
    rew2 = (np.array(rew) * np.float32(-0.5) + np.float32(0.25)).astype(np.float32)
    d_rew.copy_(torch.as_tensor(rew2, device=dev))      # rewritten in place: the graph reads the same tensor
    g.replay()
    torch.cuda.synchronize()
    adv2, ret2 = G.gae(rew2, done, val, boot, G.GAMMA, G.LAM, L, p)
    assert not G.same_bits(adv2, adv)
    assert G.same_bits(out.adv.cpu().numpy(), adv2) and G.same_bits(out.ret.cpu().numpy(), ret2)


def test_example_runs():
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "ppo_spread.py"), "--worlds", "16", "--updates", "2", "--epochs", "1"],
                       capture_output=True, text=True, cwd=root, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2
    for l in lines:
        assert np.isfinite(l["policy_loss"]) and np.isfinite(l["value_loss"]) and np.isfinite(l["mean_return"])
