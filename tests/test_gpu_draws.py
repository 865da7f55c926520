"""GPU: every entry point of csrc/mpe_rng.hip against the NumPy Philox restatement (oracle/philox.py) at the counter and shape edges
of tests/_draws_ref.py -- called through the C ABI with bare descriptors, every output buffer between two sentinel bands that are
checked after every call, every comparison `np.array_equal`.  tests/test_oracle_philox.py shows on the CPU that each row's
expectation changes when the counter word the row names is dropped.

The last test runs the fused rollouts (whose moves, words and resets are drawn IN the kernels) against their stepwise restatement
at the same edges (tests/test_gpu_rollout.py's comparison).  The stepwise side draws through the entry points, which the tests
above pin to the restatement at these very counters: together the two make the fused kernels' draws independently checked."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _draws_ref as D  # noqa: E402
from multiagent_particle_envs_amd import _abi  # noqa: E402
from oracle import philox  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 256                                  # sentinel ELEMENTS in front of and behind every output (>= 256 bytes for every dtype)
FILL = {torch.float32: -777.25, torch.int32: -777, torch.uint8: 0xA5}
RECORDS = []


class Guarded(object):
    """n live elements between two sentinel bands; the device gets the address of the live part"""

    def __init__(self, n, dtype):
        self.n, self.fill = int(n), FILL[dtype]
        self.full = torch.full((self.n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.live = self.full[GUARD:GUARD + self.n]

    @property
    def ptr(self):
        return self.live.data_ptr()

    def numpy(self, *shape):
        """the live part (after a synchronising copy), the bands asserted untouched"""
        host = self.full.cpu().numpy()
        assert (host[:GUARD] == self.fill).all(), "the band in FRONT of the buffer was written"
        assert (host[GUARD + self.n:] == self.fill).all(), "the band BEHIND the buffer was written"
        return host[GUARD:GUARD + self.n].reshape(shape)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bare_desc(A, L, pops=()):
    d = _abi.MpeScenarioDesc()
    d.kind, d.n_agents, d.n_landmarks = _abi.MPE_SCN_GENERIC, A, L
    for e in range(A + L):
        d.mass[e] = 1.0
    d.n_choices = len(pops)
    for k, n in enumerate(pops):
        d.choice_pop[k] = n
    return d


class State(object):
    """pos [E][2][B], vel [E][2][B] (the rows behind the agents' must stay as they are), choice [K][B]: all guarded"""

    def __init__(self, B, A, L, K):
        self.B, self.A, self.E, self.K = B, A, A + L, K
        self.pos, self.vel = Guarded(self.E * 2 * B, torch.float32), Guarded(self.E * 2 * B, torch.float32)
        self.choice = Guarded(K * B, torch.int32) if K else None
        self.bufs = _abi.MpeBuffers()
        self.bufs.pos, self.bufs.vel = self.pos.ptr, self.vel.ptr
        self.bufs.choice = self.choice.ptr if K else None

    def read(self):
        out = {"pos": self.pos.numpy(self.E, 2, self.B), "vel": self.vel.numpy(self.E, 2, self.B)}
        if self.K:
            out["choice"] = self.choice.numpy(self.K, self.B)
        return out


def check_state(got, want, A, mask=None):
    """reset worlds: the restatement's positions and picks, agents' velocities zero; the others and the landmarks' velocity rows:
    the sentinel"""
    B = got["pos"].shape[2]
    m = np.ones(B, bool) if mask is None else mask.astype(bool)
    assert np.array_equal(got["pos"][:, :, m], want["pos"][:, :, m])
    assert (got["pos"][:, :, ~m] == FILL[torch.float32]).all()
    assert (got["vel"][:A][:, :, m] == 0.0).all() and not np.signbit(got["vel"][:A][:, :, m]).any()
    assert (got["vel"][:A][:, :, ~m] == FILL[torch.float32]).all()
    assert (got["vel"][A:] == FILL[torch.float32]).all()
    if "choice" in got:
        assert np.array_equal(got["choice"][:, m], want["choice"][:, m])
        assert (got["choice"][:, ~m] == FILL[torch.int32]).all()


def masks(B, seed):
    half = (np.random.RandomState(seed).rand(B) < 0.5).astype(np.uint8)
    if B > 1:
        half[0], half[-1] = 1, 0
    return [("none", None), ("half", half), ("zeros", np.zeros(B, np.uint8))]


@pytest.fixture(scope="module", autouse=True)
def edge_record():
    """With MPE_DRAWS_RECORD=<file> in the environment: per case its name, shapes, counters and pass / fail, written there when the
    module is done (profiles/draws_edges.json is such a record); without it nothing is written."""
    yield
    path = os.environ.get("MPE_DRAWS_RECORD")
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "bar": "equality with oracle/philox.py; sentinel bands untouched",
                   "cases": RECORDS}, f, indent=1)


class recorded(object):
    def __init__(self, entry, row):
        self.rec = {"entry_point": entry}
        self.rec.update({k: (list(v) if isinstance(v, tuple) else v) for k, v in row.items()})

    def __enter__(self):
        return self

    def __exit__(self, kind, exc, tb):
        self.rec["passed"] = kind is None
        RECORDS.append(self.rec)
        return False


# ---- mpe_random_actions / mpe_random_actions_block --------------------------------------------------------------------------------
def run_moves(row, want_act, want_ids, single_step=None):
    """one call -> (act [T, A, B, 5] or None, ids [T, A, B] or None); single_step s: mpe_random_actions at step0 + s (T = 1)"""
    B, A = row["B"], row["A"]
    T = 1 if single_step is not None else row["T"]
    act = Guarded(T * A * B * 5, torch.float32) if want_act else None
    ids = Guarded(T * A * B, torch.int32) if want_ids else None
    L_ = _abi.lib()
    if single_step is None:
        _abi.check(L_.mpe_random_actions_block(act.ptr if act else None, ids.ptr if ids else None, A, B, row["seed"], row["t"], T, row["off"], stream()))
    else:
        _abi.check(L_.mpe_random_actions(act.ptr if act else None, ids.ptr if ids else None, A, B, row["seed"],
                                         (row["t"] + single_step) & D.M64, row["off"], stream()))
    return (act.numpy(T, A, B, 5) if act else None), (ids.numpy(T, A, B) if ids else None)


def check_moves(act, ids, want):
    if ids is not None:
        assert np.array_equal(ids, want)
    if act is not None:      # exactly one 1.0 per row, at the id; 0.0 elsewhere (positive zeros: the bit pattern)
        assert np.array_equal(act.view(np.uint32), philox.one_hot(want).view(np.uint32))


@pytest.mark.parametrize("row", D.MOVES, ids=D.ids(D.MOVES))
def test_random_actions_against_the_restatement(row):
    with recorded("mpe_random_actions(_block)", row):
        want = D.gpu_expect("moves", row)["ids"]
        assert want.min() >= 0 and want.max() <= 4
        for want_act, want_ids in ((False, True), (True, False), (True, True)):
            act, ids = run_moves(row, want_act, want_ids)
            check_moves(act, ids, want)
            for s in range(row["T"]):      # every step of a block is the single-step call at step0 + s
                act1, ids1 = run_moves(row, want_act, want_ids, single_step=s)
                check_moves(act1, ids1, want[s:s + 1])


# ---- mpe_reset ---------------------------------------------------------------------------------------------------------------------
def run_reset(row, mask, lr=None, prog=None):
    st = State(row["B"], row["A"], row["L"], len(row["pops"]))
    d = bare_desc(row["A"], row["L"], row["pops"])
    m = None if mask is None else torch.as_tensor(mask, device="cuda")
    mptr = None if m is None else C.c_void_p(m.data_ptr())
    if prog is None:
        _abi.check(_abi.lib().mpe_reset(C.byref(d), C.byref(st.bufs), row["B"], mptr, lr, row["seed"], row["t"], row["off"], stream()))
    else:
        _abi.check(_abi.lib().mpe_reset_rows(C.byref(d), C.byref(st.bufs), C.byref(prog), row["B"], mptr, 1.0 if lr is None else lr, row["seed"],
                                             row["t"], row["off"], stream()))
    return st.read()


@pytest.mark.parametrize("row", D.RESETS, ids=D.ids(D.RESETS))
def test_reset_against_the_restatement(row):
    with recorded("mpe_reset", row):
        want = D.gpu_expect("resets", row)
        for k, n in enumerate(row["pops"]):
            assert want["choice"][k].min() >= 0 and want["choice"][k].max() < n
        for _, mask in masks(row["B"], 3):
            check_state(run_reset(row, mask, lr=row["lr"]), want, row["A"], mask)


# ---- mpe_reset_random_actions_block ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", D.RESET_MOVES, ids=D.ids(D.RESET_MOVES))
def test_reset_with_the_block_of_moves_against_the_restatement(row):
    """State and picks == mpe_reset(mask = NULL) at `episode`, moves == mpe_random_actions_block, both == the restatement.  The reset
    rides on the first quad of the first step only: its draws are a function of (seed, world, episode, entity), so a later quad or
    step that reset again could only show by writing somewhere else or by drawing with ITS step in the episode's place -- the bands
    and the landmarks' velocity rows cover the first, and every row's episode differs from every step of its block (shown below:
    the restatement at episode = step0 + s is another placement), which covers the second."""
    B, A, T = row["B"], row["A"], row["T"]
    with recorded("mpe_reset_random_actions_block", row):
        want = D.gpu_expect("reset_moves", row)
        for s in range(T):
            other = philox.reset_positions(row["seed"], B, (row["t"] + s) & D.M64, A, row["L"], row["lr"], world_offset=row["off"])
            assert not np.array_equal(other.transpose(1, 2, 0), want["pos"])
        d = bare_desc(A, row["L"], row["pops"])
        for want_act, want_ids in ((True, True), (False, True), (True, False)):
            st = State(B, A, row["L"], len(row["pops"]))
            act = Guarded(T * A * B * 5, torch.float32) if want_act else None
            ids = Guarded(T * A * B, torch.int32) if want_ids else None
            _abi.check(_abi.lib().mpe_reset_random_actions_block(C.byref(d), C.byref(st.bufs), B, row["lr"], row["ep"], act.ptr if act else None,
                                                                 ids.ptr if ids else None, row["seed"], row["t"], T, row["off"], stream()))
            got = st.read()
            check_state(got, want, A)
            check_moves(act.numpy(T, A, B, 5) if act else None, ids.numpy(T, A, B) if ids else None, want["ids"])
            # ... and the two launches it stands for, on the device
            two = run_reset(dict(row, t=row["ep"]), None, lr=row["lr"])
            for k in got:
                assert np.array_equal(got[k].view(np.uint32), two[k].view(np.uint32)), k
            act2, ids2 = run_moves(row, want_act, want_ids)
            check_moves(act2, ids2, want["ids"])


# ---- mpe_reset_rows ----------------------------------------------------------------------------------------------------------------
def box_program(on):
    p = _abi.MpeRowProgram()
    p.reset_boxes = 1 if on else 0
    for e, box in enumerate(D.BOXES):
        for k in range(4):
            p.reset_box[e][k] = box[k]
    return p


@pytest.mark.parametrize("row", D.BOX_RESETS, ids=D.ids(D.BOX_RESETS))
def test_reset_rows_with_boxes_against_the_restatement(row):
    with recorded("mpe_reset_rows", row):
        want = D.gpu_expect("box_resets", row)
        lo = np.array([[b[0], b[2]] for b in D.BOXES], np.float32)[:, :, None]
        assert (want["pos"] >= lo).all()                 # (the restatement itself stays in the boxes' lower ends)
        for _, mask in masks(row["B"], 4):
            check_state(run_reset(row, mask, prog=box_program(True)), want, row["A"], mask)
        # reset_boxes = 0: the call is mpe_reset (the boxes in the struct are not read)
        plain = D.gpu_expect("resets", dict(row, lr=0.9))
        for _, mask in masks(row["B"], 5)[:2]:
            got = run_reset(row, mask, lr=0.9, prog=box_program(False))
            check_state(got, plain, row["A"], mask)
            same = run_reset(row, mask, lr=0.9)
            for k in got:
                assert np.array_equal(got[k].view(np.uint32), same[k].view(np.uint32)), k


# ---- mpe_random_comm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", D.COMMS, ids=D.ids(D.COMMS))
def test_random_comm_against_the_restatement(row):
    B, A, T, dim_c = row["B"], row["A"], row["T"], row["dim_c"]
    with recorded("mpe_random_comm", row):
        want = D.gpu_expect("comms", row)["ids"]                        # [T, speaking agents, B]
        assert want.min() >= 0 and want.max() < dim_c
        comm = Guarded(T * A * B * dim_c, torch.float32)
        _abi.check(_abi.lib().mpe_random_comm(comm.ptr, A, B, dim_c, row["speakers"], row["seed"], row["t"], T, row["off"], stream()))
        got = comm.numpy(T, A, B, dim_c)
        k = 0
        for i in range(A):
            if (row["speakers"] >> i) & 1:
                assert np.array_equal(got[:, i].view(np.uint32), philox.one_hot(want[:, k], dim_c).view(np.uint32)), i
                k += 1
            else:                                                       # a silent agent's rows keep what they held
                assert (got[:, i] == FILL[torch.float32]).all(), i
        for s in range(T):                                              # each step of the block is the T = 1 call at step0 + s
            one = Guarded(A * B * dim_c, torch.float32)
            _abi.check(_abi.lib().mpe_random_comm(one.ptr, A, B, dim_c, row["speakers"], row["seed"], (row["t"] + s) & D.M64, 1, row["off"], stream()))
            assert np.array_equal(one.numpy(A, B, dim_c).view(np.uint32), got[s].view(np.uint32))


# ---- mpe_episode_tick --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_steps,clear", [(0, 0), (0, 1), (7, 0), (7, 1), (1, 1)])
def test_episode_tick_against_four_lines_of_numpy(max_steps, clear):
    B, A = 130, 3
    row = dict(name="tick-max%d-clear%d" % (max_steps, clear), B=B, A=A, max_steps=max_steps, clear_finished=clear)
    with recorded("mpe_episode_tick", row):
        rs = np.random.RandomState(11)
        step0 = rs.randint(0, max(max_steps, 3), size=B).astype(np.int32)
        step0[:4] = [max_steps - 2, max_steps - 1, max_steps, 0]          # below, at and past the horizon (past: a counter set by hand)
        step0[-2:] = [max_steps - 1, max_steps - 2]                        # ... in the second workgroup too (B = 130: two worlds of it)
        done0 = (rs.rand(A, B) < 0.3).astype(np.uint8)
        step, done = Guarded(B, torch.int32), Guarded(A * B, torch.uint8)
        step.live.copy_(torch.as_tensor(step0))
        done.live.copy_(torch.as_tensor(done0.reshape(-1)))
        _abi.check(_abi.lib().mpe_episode_tick(step.ptr, done.ptr, A, B, max_steps, clear, stream()))
        c = step0 + 1
        over = (c >= max_steps) if max_steps > 0 else np.zeros(B, bool)
        want_step = np.where(over & bool(clear), 0, c).astype(np.int32)
        want_done = done0 | over[None, :].astype(np.uint8)
        assert np.array_equal(step.numpy(B), want_step)
        assert np.array_equal(done.numpy(A, B), want_done)
        assert max_steps == 0 or over.any() and not over.all()


# ---- the draws the fused kernels make themselves, at the same edges ----------------------------------------------------------------
EDGE_OFFSET, EDGE_STEP0 = 2 ** 32 - 64, 2 ** 32 - 2
# per kernel family the smallest B and T of tests/test_gpu_rollout.py's list; episode length 1 (a reset at every step: the episode
# number crosses 2^32 with the step) where that file already runs the family so
# (the last column: what mpe_wide_plan must answer for the rollout, so that the row runs the kernel it is named for)
IN_KERNEL = [("narrow", "simple_spread", {"num_agents": 4}, 200, 9, 4, None),
             ("comm-k_split", "simple_crypto", {}, 200, 9, 4, None),
             ("k_multi", "simple_spread", {"num_agents": 8}, 130, 11, 1, (_abi.MPE_WIDE_MULTI8,)),
             ("k_wave", "simple_spread", {"num_agents": 100}, 9, 5, 2, (_abi.MPE_WIDE_WAVE,)),
             ("k_duo", "simple_spread", {"num_agents": 64}, 37, 6, 1, (_abi.MPE_WIDE_DUO_ROLL,))]


@pytest.mark.parametrize("family,name,kw,B,T,ep,plans", IN_KERNEL, ids=[c[0] for c in IN_KERNEL])
def test_in_kernel_draws_at_the_counter_edges(family, name, kw, B, T, ep, plans):
    """mpe_rollout_random == T x { mpe_reset; mpe_random_actions; mpe_random_comm; mpe_step } at world_offset = 2^32 - 64 with the
    steps crossing 2^32 (and, where B <= 64 leaves the batch below the carry, once more at 2^32 - 4 so that it straddles it).  The
    right-hand side's draws are the entry points the tests above hold to the restatement at these counters, so equality here is an
    independent check of the moves, words, placements and picks drawn inside k_split, k_multi, k_wave and k_duo_roll."""
    import multiagent_particle_envs_amd as mpe
    import test_gpu_rollout as tg

    def make(seed):
        return mpe.make_env(name, batch_size=B, seed=seed, **kw)
    row = dict(name="fused-" + family, scenario=name, kw=kw, B=B, T=T, episode_len=ep, t=EDGE_STEP0,
               off=[EDGE_OFFSET] + ([2 ** 32 - 4] if B <= 64 else []))
    with recorded("mpe_rollout_random", row):
        if plans is not None:
            env = make(0)
            env._ensure_buffers()
            assert _abi.wide_plan(env._desc, env._sets[0].bufs, B, True, True, True)[0] in plans
        for off in row["off"]:
            tg.fused_rollout_equals_stepwise(make, B, T, ep, offset=off, step0=EDGE_STEP0)


def test_in_kernel_draws_of_a_row_program_with_boxes_at_the_counter_edges():
    """The Yard of tests/test_rowspec.py (per-entity boxes, one pick): mpe_rollout_rows, whose restarts are drawn in the kernel, ==
    the per-step launches, whose restarts are mpe_reset_rows and whose moves are mpe_random_actions_block -- worlds straddling 2^32,
    steps crossing it, a restart every second step."""
    import multiagent_particle_envs_amd as mpe
    from multiagent_particle_envs_amd.core import World
    from multiagent_particle_envs_amd.rollout import RandomRollout, Trajectory
    import test_rowspec as tr
    boxes = [(-0.25, 0.25, -0.25, 0.25)] * 3 + [(0.2, 0.9, -0.9, 0.9)] * 3

    class Yard(tr.Corral):
        device_reset = True
        arena = 0.95

        def reset_boxes(self, world):
            return boxes

        def reset_world(self, world, mask=None, seeds=None):
            idx = world.reset_boxes(boxes, mask, choices=[3], seeds=seeds)
            if world.choice_i32 is not None:
                world.choice_i32[0].copy_(World.merge_choice(world.choice_i32[0].long(), idx[:, 0].to(world.device), mask).to(torch.int32))

    B, T, EP = 129, 7, 2

    def make():
        sc = Yard()
        w = sc.make_world(batch_size=B)
        w.seed = 21
        w.world_offset = EDGE_OFFSET
        sc.reset_world(w)
        env = mpe.MultiAgentEnv(w, sc.reset_world, sc.reward, sc.observation, compile_program=False)
        env.scenario = sc
        return env
    row = dict(name="fused-rows-yard", B=B, T=T, episode_len=EP, off=EDGE_OFFSET, t=EDGE_STEP0)
    with recorded("mpe_rollout_rows", row):
        a, b = make(), make()
        assert a._prog.struct.reset_boxes == 1
        assert torch.equal(a.world.pos, b.world.pos)
        ra, rb = RandomRollout(a, episode_len=EP, pool=4, regenerate=True), RandomRollout(b, episode_len=EP, pool=4, regenerate=True)
        ra.t = rb.t = EDGE_STEP0
        traj = Trajectory(b, T)
        rb.fused(T, traj)
        for t in range(T):
            out = ra.enqueue(1)
            for i in range(a.n):
                assert torch.equal(traj.obs[t][i], out.obs_n[i]) and torch.equal(traj.rew[t][i], out.reward_n[i]), (t, i)
        torch.cuda.synchronize()
        assert torch.equal(a.world.pos, b.world.pos) and torch.equal(a.world.vel, b.world.vel)
        assert torch.equal(a.world.choice_i32, b.world.choice_i32)
