"""The step server's state at rest: a served step leaves its state in HBM only when nobody may read it race-free before the next
step overwrites it -- that is, not when the next step of the launch is already commanded.  What a commander can observe must not
change: the state after the last commanded step of a burst (the server then waits for its next doorbell), the state after a
timeout, and the per-workgroup completion flags, which never claim a step whose outputs are not all in memory.

Each check runs on the dual-role server (a physics and a rows wave per agent, up to 1.5 workgroups per CU) and on the single-role
one (beyond that)."""
import time

import pytest
import torch

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd.rollout import RandomRollout, StepServer

pytestmark = pytest.mark.gpu


def dual_max_workgroups():
    return torch.cuda.get_device_properties(0).multi_processor_count * 3 // 2


def batch_for(role):
    """A ragged batch served by the dual-role kernel, or one just past its limit (the single-role kernel)."""
    B = 4096 + 21 if role == "dual" else 64 * dual_max_workgroups() + 37
    assert ((B + 63) // 64 <= dual_max_workgroups()) == (role == "dual")
    return B


def launched_steps(B, T, EP, ring):
    """T steps of simple_spread through the per-step launches: -> (move ring, per step: obs rows, rew, done, pos, vel)."""
    env = mpe.make_env("simple_spread", batch_size=B, seed=3)
    rr = RandomRollout(env, episode_len=EP, pool=ring, regenerate=False)
    out = []
    for _ in range(T):
        o = rr.enqueue(1)
        torch.cuda.synchronize()
        out.append(([x.clone() for x in o.obs_n], o.rew.clone(), o.done.clone(), env.world.pos.clone(), env.world.vel.clone()))
    return rr.pool_t.clone(), out


def outputs_equal(srv, g, step):
    o_s, r_s, d_s = srv.outputs(g)
    return all(torch.equal(a, b) for a, b in zip(o_s, step[0])) and torch.equal(r_s, step[1]) and torch.equal(d_s, step[2])


@pytest.mark.parametrize("role", ["dual", "single"])
def test_state_after_a_burst_that_ends_mid_episode(role):
    """Bursts of commands rung ahead, each ending inside an episode: after wait() the state in HBM is the launched steps' state at
    the burst's last step, though the steps inside the burst left theirs on chip."""
    B, T, EP, ring = batch_for(role), 40, 25, 8
    moves, ref = launched_steps(B, T, EP, ring)
    env = mpe.make_env("simple_spread", batch_size=B, seed=3)
    srv = StepServer(env, moves, slots=T, episode_len=EP, timeout_s=20.0)
    srv.start(T)
    done = 0
    for n in (7, 11, 13, 9):
        srv.ring(n)
        srv.wait()
        torch.cuda.current_stream().synchronize()
        done += n
        assert int(srv.status.item()) == 0
        last = ref[done - 1]
        assert torch.equal(env.world.pos, last[3]) and torch.equal(env.world.vel, last[4]), "state after step %d" % (done - 1)
        time.sleep(0.01)
    srv.join()
    torch.cuda.synchronize()
    srv.check()
    for g in range(T):
        assert outputs_equal(srv, g, ref[g]), "outputs of step %d" % g


@pytest.mark.parametrize("role", ["dual", "single"])
def test_timeout_after_steps_rung_ahead(role):
    """k steps of a launch of T rung ahead at once, then silence: after the timeout the outputs and the state are those of step
    k - 1, and the blocks of the steps nobody commanded are untouched."""
    B, T, k, EP, ring = batch_for(role), 8, 5, 25, 8
    moves, ref = launched_steps(B, T, EP, ring)
    env = mpe.make_env("simple_spread", batch_size=B, seed=3)
    srv = StepServer(env, moves, slots=T, episode_len=EP, timeout_s=0.2)
    srv.blocks.obs_flat.fill_(float("nan"))
    srv.blocks.rew.fill_(float("nan"))
    srv.blocks.done.fill_(True)
    torch.cuda.synchronize()
    srv.start(T)
    srv.ring(k)
    srv.join()
    torch.cuda.synchronize()
    assert int(srv.status.item()) == 1 and int(srv.flag.min()) == k and int(srv.flag.max()) == k
    for g in range(k):
        assert outputs_equal(srv, g, ref[g]), "outputs of step %d" % g
    for g in range(k, T):
        o_s, r_s, d_s = srv.outputs(g)
        assert all(bool(torch.isnan(o).all()) for o in o_s), "block %d: rows written for a step nobody commanded" % g
        assert bool(torch.isnan(r_s).all()) and bool(d_s.all()), "block %d: rewards / dones written" % g
    assert torch.equal(env.world.pos, ref[k - 1][3]) and torch.equal(env.world.vel, ref[k - 1][4])


@pytest.mark.parametrize("role", ["dual", "single"])
def test_flags_never_run_ahead_of_the_outputs(role):
    """With more steps commanded than waited for, the flags are sampled while the server runs on: every step below the smallest
    flag has all its outputs in memory, equal to the launched step's."""
    B, T, EP, ring = batch_for(role), 48, 25, 8
    moves, ref = launched_steps(B, T, EP, ring)
    env = mpe.make_env("simple_spread", batch_size=B, seed=3)
    srv = StepServer(env, moves, slots=T, episode_len=EP, timeout_s=20.0)
    srv.start(T)
    srv.ring(6)
    checked = 0
    for g in range(1, T + 1):
        if srv.commanded < T:
            srv.ring(1)                  # one step more commanded than waited for, at least
        srv.wait(g)
        torch.cuda.current_stream().synchronize()
        f = int(srv.flag.min())          # (read first: the blocks below are read after it)
        assert f >= g, "wait(%d) returned with the smallest flag at %d" % (g, f)
        for s in range(checked, f):
            assert outputs_equal(srv, s, ref[s]), "flag %d claims step %d, whose outputs are not the launched ones" % (f, s)
        checked = max(checked, f)
    srv.join()
    torch.cuda.synchronize()
    srv.check()
    assert checked == T
    assert torch.equal(env.world.pos, ref[-1][3]) and torch.equal(env.world.vel, ref[-1][4])
