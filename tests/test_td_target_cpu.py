"""CPU-only checks of the TD-target path (no GPU, no launch): the case table of tests/test_gpu_td_target.py held to
the cap and tolerance conditions of tests/test_actor_ref_cpu.py, the joint-row and y restatements of tests/_td_target_ref.py
against torch and fp64, what fp32 alone costs a critic, the Python side's joint layout against ReplayBuffer's, and every refusal
that needs no device."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.learner import Critics, TdTargets
from multiagent_particle_envs_amd.policy import Actors
from multiagent_particle_envs_amd.replay import NStepReplayBatch, ReplayBatch, ReplayBuffer

import _actor_ref as R
import _td_target_ref as T


@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_case_cap_and_tolerance_conditions(name):
    """the two conditions of test_actor_ref_cpu.test_case_cap_and_tolerance_conditions, on this table"""
    c = T.CASES[T.CASE_NAMES.index(name)]
    assert c["seed"] == 0
    agents, obs = R.build_case(c)
    for mode in ("greedy", "sample"):
        refs = R.case_refs(c, mode, agents, obs)
        checked = sum(ref["z"].shape[0] for ref in refs for d in ref["heads"] if d is not None)
        inband = sum(int((~d["ok"]).sum()) for ref in refs for d in ref["heads"] if d is not None)
        assert inband <= 0.5 * R.CAP * checked, "%s %s: %d of %d rows inside the band" % (name, mode, inband, checked)
        for i, (a, ref) in enumerate(zip(agents, refs)):
            f32 = R.ref_f32(a["layers"], a["act"], a["movable"], a["speaks"], c["dim_c"], obs[i],
                            chosen=[d["chosen"] if d is not None else None for d in ref["heads"]])
            assert np.isfinite(f32["z"]).all()
            assert (np.abs(f32["z"] - ref["z"]).max(axis=1) < R.BAND * ref["scale"]).all(), (name, i, "fp32 logits")
            for h, d in enumerate(ref["heads"]):
                if d is not None:
                    assert (np.abs(f32["heads"][h]["p"] - d["p"]).max(axis=1) < R.BAND * d["scale"]).all(), (name, i, h, "fp32 softmax")
            assert (np.abs(f32["logp"] - ref["logp"]) < R.logp_bar(ref)).all(), (name, i, "fp32 logp")


def test_case_table_is_the_one_stated():
    by = {c["name"]: c for c in T.CASES}
    assert [(c["B"], c["world_offset"]) for c in T.CASES] == [(1, 0), (63, 0), (65, 0), (257, 5), (300, 0), (130, 0)]
    assert T.case_layout(by["wide_joint346_M130"])[1] == 346 > _abi.MPE_ACTOR_MAX_INPUT
    assert [s["D"] for s in by["tag_M300"]["specs"]] == [16, 16, 16, 14] and by["tag_M300"]["specs"][3]["hidden"] == (64,)
    assert [(s["D"], s["movable"], s["speaks"]) for s in by["speaker_listener_M65"]["specs"]] == [(3, 0, 1), (11, 1, 0)]
    assert [(s["D"], s["hidden"]) for s in by["both_heads_M257_off5"]["specs"]] == [(33, (33, 32)), (2, ())]


@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_joint_rows_restatement_is_the_cat_of_the_parts(name):
    c = T.CASES[T.CASE_NAMES.index(name)]
    _, obs = R.build_case(c)
    rs = np.random.RandomState(5)
    A, M, dc = len(obs), c["B"], c["dim_c"]
    moves = rs.uniform(0, 1, (A, M, R.MOVE)).astype(np.float32)
    utter = rs.uniform(0, 1, (A, M, dc)).astype(np.float32) if dc else None
    mv, sp = [s["movable"] for s in c["specs"]], [s["speaks"] for s in c["specs"]]
    parts = [torch.as_tensor(o) for o in obs]
    for i in range(A):
        if mv[i]:
            parts.append(torch.as_tensor(moves[i]))
        if sp[i]:
            parts.append(torch.as_tensor(utter[i]))
    want = torch.cat(parts, dim=1).numpy()
    got = T.joint_rows(obs, moves, utter, mv, sp, dc)
    assert got.shape == (M, T.case_layout(c)[1]) and got.tobytes() == want.tobytes()


def _actor(D, n_out):
    return nn.Sequential(nn.Linear(D, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, n_out))


@pytest.mark.parametrize("name", ["simple_spread", "simple_speaker_listener", "simple_tag", "simple_world_comm"])
def test_actors_joint_layout_is_the_replay_buffers(name):
    env = mpe.make_env(name, batch_size=4, device="cpu")
    buf = ReplayBuffer(env, 2)
    pi = Actors(env, [_actor(D, n) for D, n in zip(buf.obs_widths, buf.n_act)], mode="softmax")
    assert pi.joint_width == buf.joint_width and pi.off == buf.off
    off, width, cm, cu = T.joint_layout(buf.obs_widths, buf.movable, buf.speaks, buf.dim_c)
    assert (off, width) == (buf.off, buf.joint_width) and pi.col_move == cm and pi.col_utter == cu
    # ReplayBatch.joint's columns, from the buffer's own fields: per agent n_act[i] columns, the move row first
    col = buf.off[-1]
    for i in range(buf.A):
        assert pi.col_move[i] == (col if buf.movable[i] else None)
        assert pi.col_utter[i] == ((col + 5 * buf.movable[i]) if buf.speaks[i] else None)
        col += buf.n_act[i]
    assert col == pi.joint_width
    if width <= _abi.MPE_ACTOR_MAX_INPUT:
        assert Critics(env, _actor(width, 1)).joint_width == width


def test_y_rule_restatement():
    rs = np.random.RandomState(3)
    A, M = 3, 4096
    ret, q = (rs.standard_normal((A, M)) * 10).astype(np.float32), (rs.standard_normal((A, M)) * 30).astype(np.float32)
    disc = (0.95 ** rs.randint(1, 6, M)).astype(np.float32)
    done = (rs.uniform(size=(A, M)) < 0.3).astype(np.uint8)
    for discount, gamma in ((disc, None), (None, 0.95)):
        y = T.y_rule(ret, done, q, discount, gamma)
        assert y.dtype == np.float32
        d64 = np.broadcast_to(disc.astype(np.float64)[None] if gamma is None else np.float64(np.float32(gamma)), q.shape)
        y64 = ret.astype(np.float64) + d64 * (1.0 - done) * q.astype(np.float64)
        # two roundings: the product to float32 (half an ulp of |d q|), then the sum (half an ulp of |y|)
        bar = 2.0 ** -24 * (np.abs(d64 * q) + np.abs(y64)) * 1.001 + 1e-45
        assert (np.abs(y - y64) <= bar).all()
        assert (y[done != 0] == ret[done != 0]).all()
    # a select: done hides a non-finite q exactly; without done it shows
    q2 = q.copy()
    q2[0, ::2], q2[1, ::2], q2[2, ::2] = np.inf, np.nan, -np.inf
    y = T.y_rule(ret, done, q2, disc)
    assert y[done != 0].tobytes() == ret[done != 0].tobytes()
    live = (done == 0)
    live[:, 1::2] = False
    assert not np.isfinite(y[live]).any()
    assert T.same_floats(y, T.y_rule(ret, done, q2, disc)) and not T.same_floats(y, ret)


@pytest.mark.parametrize("shape", T.CRITIC_SHAPES, ids=T.CRITIC_IDS)
def test_fp32_critic_against_fp64(shape):
    critics, rows = T.build_critics(shape)
    assert rows.shape == (shape[2], shape[0]) and all(l[-1][0].shape[0] == 1 for l in critics)
    worst = 0.0
    for layers in critics:
        q64, q32 = T.critic_q(layers, rows, np.float64), T.critic_q(layers, rows, np.float32)
        assert q32.dtype == np.float32
        worst = max(worst, float((np.abs(q32 - q64) / (T.Q_BAR * np.maximum(1, np.abs(q64)))).max()))
    print("fp32 critic %s: worst error / bar %.3f" % (shape, worst))
    assert worst < 1.0
    m = R.as_module(critics[0], R.RELU, torch.float64)
    with torch.no_grad():
        assert np.allclose(m(torch.as_tensor(rows).double())[:, 0].numpy(), T.critic_q(critics[0], rows, np.float64), rtol=0, atol=1e-12)


# ---- refusals that need no device ---------------------------------------------------------------------------------------------
FAKE = 4096      # a non-NULL, 16-byte aligned pointer value nothing dereferences: every call below is refused before a launch


def _err():
    return _abi.lib().mpe_last_error().decode()


def _actor_set(mode="greedy"):
    c = T.CASES[T.CASE_NAMES.index("both_heads_M257_off5")]
    agents, _ = R.build_case(c)
    aset, _ = R.make_set(agents, c["dim_c"], mode, 0)
    aset.weights = FAKE
    return aset, len(agents), T.case_layout(c)[1]


def _rows_call(aset, A, **kw):
    a = dict(ptrs=(C.c_void_p * A)(*([FAKE] * A)), M=7, moves=FAKE, utter=FAKE, ids=None, logp=None, logits=None, joint=FAKE, stride=64)
    a.update(kw)
    return _abi.lib().mpe_actor_act_rows(C.byref(aset), a["ptrs"], a["M"], 0, 0, a["moves"], a["utter"], a["ids"], a["logp"], a["logits"],
                                         a["joint"], a["stride"], None)


def test_act_rows_refusals():
    aset, A, width = _actor_set()
    assert width == 53
    assert _rows_call(aset, A, stride=width - 1) == -1 and "joint_stride" in _err() and "joint width 53" in _err()
    assert _rows_call(aset, A, joint=FAKE + 2, stride=width) == -1 and "joint is not 4-byte aligned" in _err()
    assert _rows_call(aset, A, moves=None, joint=None) == -1 and "moves and joint are both NULL" in _err()
    # ... and what mpe_actor_act refuses
    assert _rows_call(aset, A, M=-1) == -1 and "M = -1" in _err()
    assert _rows_call(aset, A, ptrs=None) == -1 and "obs_ptrs is NULL" in _err()
    assert _rows_call(aset, A, ptrs=(C.c_void_p * A)(FAKE, None)) == -1 and "obs_ptrs[1] is NULL" in _err()
    assert _rows_call(aset, A, logits=FAKE + 4) == -1 and "logits is not 16-byte aligned" in _err()
    aset.weights = FAKE + 4
    assert _rows_call(aset, A) == -1 and "weights" in _err()
    aset.weights = None
    assert _rows_call(aset, A) == -1 and "weights" in _err()
    aset.weights = FAKE
    aset.width[0][3] = 8
    assert _rows_call(aset, A) == -1 and "the last layer gives 8 outputs" in _err()
    aset.width[0][3] = 9
    aset.n_agents = 17
    assert _rows_call(aset, A) == -2 and "MPE_ACTOR_MAX_AGENTS" in _err()
    assert _abi.lib().mpe_actor_act_rows(None, None, 1, 0, 0, None, None, None, None, None, None, 0, None) == -1 and "set is NULL" in _err()
    # M == 0: nothing to do, no launch
    aset.n_agents = A
    assert _rows_call(aset, A, M=0, stride=width) == 0


def _critic_set(A=3, W=69):
    critics = [R.make_layers(np.random.RandomState(i), W, (64, 64), 1) for i in range(A)]
    aset, _ = T.make_critic_set(critics)
    aset.weights = FAKE
    return aset


def _td(ret=FAKE, done=FAKE, discount=None, gamma=0.95):
    td = _abi.MpeTdTarget()
    td.ret, td.done, td.discount, td.gamma = ret, done, discount, gamma
    return td


def _q_call(aset, A=3, ptrs=0, M=5, q=FAKE, td=None, y=None):
    ptrs = (C.c_void_p * A)(*([FAKE] * A)) if ptrs == 0 else ptrs
    return _abi.lib().mpe_critic_q(C.byref(aset), ptrs, M, q, C.byref(td) if td is not None else None, y, None)


def test_value_mode_is_the_critic_entrys_alone():
    L = _abi.lib()
    assert _abi.MPE_POLICY_VALUE == 3 and _abi.MPE_ABI_VERSION == 4
    aset = _critic_set()
    ptrs = (C.c_void_p * 3)(FAKE, FAKE, FAKE)
    want = "mode 3 (MPE_POLICY_GREEDY / SAMPLE / SOFTMAX)"
    assert L.mpe_actor_act(C.byref(aset), ptrs, 5, 0, 0, FAKE, None, None, None, None, None) == -1 and _err() == "mpe_actor_act: " + want
    assert L.mpe_actor_act_rows(C.byref(aset), ptrs, 5, 0, 0, FAKE, None, None, None, None, None, 0, None) == -1
    assert _err() == "mpe_actor_act_rows: " + want
    assert L.mpe_actor_supported(C.byref(aset), 5) == -1 and _err() == "mpe_actor_supported: " + want
    # an unknown mode is refused in the same words
    aset.mode = 7
    assert L.mpe_actor_act(C.byref(aset), ptrs, 5, 0, 0, FAKE, None, None, None, None, None) == -1
    assert _err() == "mpe_actor_act: mode 7 (MPE_POLICY_GREEDY / SAMPLE / SOFTMAX)"
    # the critic entry takes nothing else
    for mode in (0, 1, 2, 7):
        aset.mode = mode
        assert _q_call(aset) == -1 and "MPE_POLICY_VALUE" in _err()


def test_critic_q_refusals():
    aset = _critic_set()
    aset.width[1][3] = 2
    assert _q_call(aset) == -1 and "agent 1: the last layer gives 2 outputs" in _err()
    aset.width[1][3] = 1
    aset.movable[2] = 1
    assert _q_call(aset) == -1 and "agent 2: movable = 1, speaks = 0" in _err()
    aset.movable[2], aset.speaks[0] = 0, 1
    assert _q_call(aset) == -1 and "agent 0: movable = 0, speaks = 1" in _err()
    aset.speaks[0], aset.dim_c = 0, 2
    assert _q_call(aset) == -1 and "dim_c = 2" in _err()
    aset.dim_c = 0
    aset.width[0][0] = 257
    assert _q_call(aset) == -2 and "input width 257 > MPE_ACTOR_MAX_INPUT" in _err()
    aset.width[0][0] = 69
    assert _q_call(aset, q=None) == -1 and "q is NULL" in _err()
    assert _q_call(aset, q=FAKE + 2) == -1 and "q is NULL or not 4-byte aligned" in _err()
    assert _q_call(aset, ptrs=None) == -1 and "in_ptrs is NULL" in _err()
    assert _q_call(aset, ptrs=(C.c_void_p * 3)(FAKE, FAKE, None)) == -1 and "in_ptrs[2] is NULL" in _err()
    assert _q_call(aset, M=-2) == -1 and "M = -2" in _err()
    assert _q_call(aset, td=_td(), y=None) == -1 and "td is given and y is NULL" in _err()
    assert _q_call(aset, td=None, y=FAKE) == -1 and "y is given and td is NULL" in _err()
    assert _q_call(aset, td=_td(ret=None), y=FAKE) == -1 and "td->ret is NULL" in _err()
    assert _q_call(aset, td=_td(done=None), y=FAKE) == -1 and "td->done is NULL" in _err()
    for g in (float("nan"), float("inf"), -float("inf")):
        assert _q_call(aset, td=_td(gamma=g), y=FAKE) == -1 and "gamma" in _err() and "not finite" in _err()
    for bad in (dict(td=_td(), y=FAKE + 1), dict(td=_td(ret=FAKE + 2), y=FAKE), dict(td=_td(discount=FAKE + 3), y=FAKE)):
        assert _q_call(aset, **bad) == -1 and "4-byte aligned" in _err()
    aset.weights = FAKE + 8
    assert _q_call(aset) == -1 and "weights" in _err()
    aset.weights = FAKE
    # M == 0 returns 0 without a launch, as B == 0 does (with a discount, a non-finite gamma is not read)
    assert _q_call(aset, M=0) == 0
    assert _q_call(aset, M=0, td=_td(discount=FAKE, gamma=float("nan")), y=FAKE) == 0
    assert _abi.lib().mpe_sizeof_td_target() == C.sizeof(_abi.MpeTdTarget)


def _spread(device="cpu"):
    env = mpe.make_env("simple_spread", batch_size=4, device=device)
    pi = Actors(env, [_actor(18, 5) for _ in range(3)], mode="softmax")
    return env, pi


def test_python_refusals_arrive_as_mpe_errors():
    env, pi = _spread()
    assert pi.joint_width == 69
    # Critics
    with pytest.raises(_abi.MpeError, match="takes 70 inputs, the joint row has 69"):
        Critics(env, _actor(70, 1))
    with pytest.raises(_abi.MpeError, match=r"Critics: the last Linear layer gives 2 outputs \(need 1\)"):
        Critics(env, [_actor(69, 1), _actor(69, 2), _actor(69, 1)])
    with pytest.raises(_abi.MpeError, match="2 critics for 3 agents"):
        Critics(env, [_actor(69, 1), _actor(69, 1)])
    with pytest.raises(_abi.MpeError, match="Critics: hidden width 65"):
        Critics(env, nn.Sequential(nn.Linear(69, 65), nn.ReLU(), nn.Linear(65, 1)))
    wide = mpe.make_env("simple_spread", batch_size=4, device="cpu", num_agents=10)
    assert ReplayBuffer(wide, 2).joint_width > _abi.MPE_ACTOR_MAX_INPUT
    with pytest.raises(_abi.MpeError, match="MPE_ACTOR_MAX_INPUT = 256"):
        Critics(wide, _actor(ReplayBuffer(wide, 2).joint_width, 1))
    cr = Critics(env, [_actor(69, 1) for _ in range(3)])
    with pytest.raises(_abi.MpeError, match=r"Critics.q: rows is a contiguous float32 \[M, 69\]"):
        cr.q(torch.zeros(5, 70))
    with pytest.raises(_abi.MpeError, match="Critics.q: rows"):
        cr.q(torch.zeros(5, 69, dtype=torch.float64))
    with pytest.raises(_abi.MpeError, match="Critics.q: rows"):
        cr.q(torch.zeros(69, 5).t())
    wts, aset = cr.pack()
    assert aset.mode == _abi.MPE_POLICY_VALUE and aset.dim_c == 0 and [aset.width[i][3] for i in range(3)] == [1, 1, 1]
    assert wts.numel() == 3 * ((69 + 1) * 64 + 65 * 64 + 65 * 16) and Critics(env, cr.modules[0]).pack()[0].numel() == wts.numel() // 3
    assert cr.reference(torch.zeros(5, 69)).shape == (3, 5)
    # act_rows
    obs = [torch.zeros(6, 18) for _ in range(3)]
    with pytest.raises(_abi.MpeError, match="Actors.act_rows: 2 observation blocks for 3 agents"):
        pi.act_rows(obs[:2])
    with pytest.raises(_abi.MpeError, match=r"obs_n\[1\] is a contiguous float32 \[6, 18\]"):
        pi.act_rows([obs[0], torch.zeros(5, 18), obs[2]])
    with pytest.raises(_abi.MpeError, match=r"obs_n\[2\] is a contiguous float32"):
        pi.act_rows([obs[0], obs[1], torch.zeros(6, 18, dtype=torch.float64)])
    with pytest.raises(_abi.MpeError, match=r"joint is True or a contiguous float32 \[6, >= 69\]"):
        pi.act_rows(obs, joint=torch.zeros(6, 68))
    with pytest.raises(_abi.MpeError, match="joint is True or a contiguous"):
        pi.act_rows(obs, joint=torch.zeros(5, 69))
    # TdTargets
    with pytest.raises(_abi.MpeError, match="TdTargets: actors is an Actors"):
        TdTargets(cr, cr)
    with pytest.raises(_abi.MpeError, match="TdTargets: critics is a Critics"):
        TdTargets(pi, pi)
    env2, _ = _spread()
    with pytest.raises(_abi.MpeError, match="different envs"):
        TdTargets(pi, Critics(env2, _actor(69, 1)))
    td = TdTargets(pi, cr)
    with pytest.raises(_abi.MpeError, match="batch is a ReplayBatch"):
        td.compute({"rew": None})
    one, nstep = ReplayBatch(), NStepReplayBatch()
    for b in (one, nstep):
        b.rew, b._done_u8 = torch.zeros(3, 6), torch.zeros(3, 6, dtype=torch.uint8)
    nstep.ret, nstep.discount = torch.zeros(3, 6), torch.zeros(6)
    with pytest.raises(_abi.MpeError, match="gamma is required for a one-step batch"):
        td.compute(one)
    with pytest.raises(_abi.MpeError, match="gamma = nan is not finite"):
        td.compute(one, gamma=float("nan"))
    with pytest.raises(_abi.MpeError, match="an n-step batch carries its own discount"):
        td.compute(nstep, gamma=0.95)
    assert td.t == 0      # (a refused call does not advance the draw key)
    assert mpe.Critics is Critics and mpe.TdTargets is TdTargets and mpe.Actors is Actors
