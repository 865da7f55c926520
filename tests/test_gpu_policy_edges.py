"""GPU: the fused policy rollout (mpe_rollout_policy: k_split<..., POL = true>, csrc/mpe_split.hip) at its edges -- every
instantiation of kPolicyTable x every path of pol_logits x both activations, hidden widths below 64, a mixed and a shared actor
set, batch, episode and counter edges, customised constants, an immovable agent, known answers, a poisoned world and the C entry
point's corners -- every case of tests/_policy_edges.py, which names what each one is aimed at; tests/test_policy_edges_cpu.py
holds that table to its own conditions on the CPU first.

Per run: a PolicyTrajectory one block longer than T whose every buffer is pre-filled with a canary -- block T must come back
bit-unchanged.  Decisions against _actor_ref.ref_decide (NumPy fp64) on the recorded decision inputs under _actor_ref's bars
(softmax rows within 1e-5 * max(1, max|z|), indices and one-hot rows exact outside the band, logp within logp_bar, rows inside the
band counted and at most 0.1 % of the rows checked + 1, per sweep); the decision inputs against the previous step's rows (bit for
bit) or the fp64 oracle's observation of the reset draws (1e-5); the step itself by replaying the recorded rows through step_many
(bit for bit; that path is golden-checked in test_gpu_server_oracle.py), or -- at the counter edges, where step_many cannot
follow -- against the fp64 oracle stepped once from the GPU's own previous state with the GPU's own row (1e-5)."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _actor_ref as R  # noqa: E402
import _policy_edges as PE  # noqa: E402
from _parity_util import close, guard_ok, np_, set_choices  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd import _abi  # noqa: E402
from multiagent_particle_envs_amd.rollout import MlpPolicy, PolicyRollout, PolicyTrajectory, step_many  # noqa: E402

pytestmark = pytest.mark.gpu
T = PE.T
_TALLY = {}


# ---- envs, actors, runs -----------------------------------------------------------------------------------------------------------------
def make_env(case, customise=True):
    """make_env's steps (make_env.py), with the case's constants assigned on the world before the env is built"""
    name, kw, _ = PE.SHAPES[case.shape]
    sc = mpe.scenarios.load(name + ".py").Scenario()
    w = sc.make_world(batch_size=case.B, **kw)
    w.seed, w.rng_mode = case.world_seed, "device"
    if customise and case.custom is not None:
        PE.customise_world(case, w)
    sc.reset_world(w)
    env = mpe.MultiAgentEnv(w, sc.reset_world, getattr(sc, "reward", None), getattr(sc, "observation", None))
    env.scenario = sc
    w.world_offset = case.world_offset
    for i in case.immovable:      # an env is built around movable agents: switched off on the live env (the step re-reads the constants)
        w.agents[i].movable = False
    return env


def start(env, case):
    pos, vel, choice = PE.initial_state(case)
    env.world.set_state(pos, vel)
    set_choices(env, choice)
    return pos, vel, choice


def modules(env, layers, acts, shared=False):
    if shared:
        return R.as_module(layers[0], acts[0]).to(env.world.device)
    return [R.as_module(l, a).to(env.world.device) for l, a in zip(layers, acts)]


def canary_traj(env, blocks=T + 1):
    tr = PolicyTrajectory(env, blocks, record_inputs=True, logp=True)
    for x in (tr.act, tr.obs_in_flat, tr.logp, tr.obs_flat, tr.rew):
        x.fill_(PE.CANARY_F)
    tr.done.fill_(True)
    return tr


def canary_intact(tr, n=T):
    per = tr.obs_flat.numel() // tr.T
    tail = (tr.act[n:], tr.logp[n:], tr.rew[n:], tr.obs_flat[n * per:], tr.obs_in_flat[n * per:])
    return all(bool((x == PE.CANARY_F).all()) for x in tail) and bool(tr.done[n:].all())


def new_rollout(env, case, mods, mode):
    roll = PolicyRollout(env, MlpPolicy(mods), mode=mode, episode_len=case.episode_len, seed=case.world_seed, policy_seed=case.policy_seed)
    roll.t = case.step0
    return roll


def run_case(env, case, mods, mode):
    """from the case's start state: one run(T) into a canary trajectory -> (trajectory, final (pos, vel))"""
    start(env, case)
    tr = canary_traj(env)
    new_rollout(env, case, mods, mode).run(T, trajectory=tr, record_inputs=True)
    torch.cuda.synchronize()
    assert canary_intact(tr), (case.id, mode, "block T of the trajectory was written")
    assert not bool(tr.done[:T].any()), (case.id, mode, "done rows the launch did not write")
    for name in ("act", "rew"):
        assert not bool((getattr(tr, name)[:T] == PE.CANARY_F).any()), (case.id, mode, name, "rows the launch did not write")
    if mode == "sample":
        assert not bool((tr.logp[:T] == PE.CANARY_F).any()), (case.id, "logp rows the launch did not write")
    else:
        assert bool((tr.logp == PE.CANARY_F).all()), (case.id, mode, "logp written outside sample mode")
    return tr, env.world.get_state()


def same_bits(a, b):
    a, b = np.ascontiguousarray(np_(a)), np.ascontiguousarray(np_(b))
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return a.shape == b.shape and np.array_equal(a, b)


def tally_of(sweep, record_parity):
    t = _TALLY.setdefault(sweep, {"tally": R.Tally(), "f32": {"softmax": 0.0, "logp": 0.0, "logits": 0.0}, "logit_diff": 0.0})

    def done():
        rep = t["tally"].report()
        rep["worst_error_over_bar"].pop("logits")      # (the fused kernel has no logits output)
        rep["worst_logit_difference_error_over_two_bars_from_softmax_rows"] = t["logit_diff"]
        rep["ref_f32_worst_error_over_bar_same_rows"] = dict(t["f32"])
        record_parity("policy_edges_" + sweep, rep)
        print("policy edges, %s so far: %s" % (sweep, rep))
        assert t["tally"].inband <= R.CAP * t["tally"].checked + 1, (sweep, "rows inside the band")
    return t, done


# ---- the three comparisons ----------------------------------------------------------------------------------------------------------------
def check_decisions(case, mode, tr, layers, acts, t, with_logp=None):
    """1. every step's and agent's rows (and logp: sample mode, or with_logp) against ref_decide on the recorded decision input"""
    act = np_(tr.act[:T])
    with_logp = mode == "sample" if with_logp is None else with_logp
    lp = np_(tr.logp[:T])
    for k in range(T):
        gt = case.step0 + k
        for i in range(len(layers)):
            obs = np_(tr.obs_in[k][i])
            ref = R.ref_decide(layers[i], acts[i], 1, 0, 0, obs, mode, case.policy_seed, gt, i, case.world_offset)
            got = PE.compare(act[k, i], lp[k, i] if with_logp else None, ref, mode)
            assert not got["bad"].any(), (case.id, mode, "step %d agent %d" % (k, i), got["why"])
            tl = t["tally"]
            tl.checked += case.B
            tl.inband += got["inband"]
            tl.worst["softmax"] = max(tl.worst["softmax"], got["softmax"])
            tl.worst["logp"] = max(tl.worst["logp"], got["logp"])
            p32, lp32, z32 = PE.f32_cost(layers[i], acts[i], obs, ref, mode)
            f = t["f32"]
            f["softmax"], f["logits"] = max(f["softmax"], p32), max(f["logits"], z32)
            if mode == "sample":
                f["logp"] = max(f["logp"], lp32)
            if mode == "softmax":      # the logits as far as a softmax row shows them: differences to the top logit, where p >= 1e-2
                d = ref["heads"][0]
                a = act[k, i].astype(np.float64)
                top = d["greedy"][:, None]
                with np.errstate(divide="ignore", invalid="ignore"):
                    dz = np.log(a) - np.log(np.take_along_axis(a, top, 1))
                    want = d["z"] - np.take_along_axis(d["z"], top, 1)
                    e = np.where(d["p"] >= 1e-2, np.abs(dz - want) / (2 * R.BAND * d["scale"][:, None]), 0.0)
                t["logit_diff"] = max(t["logit_diff"], float(e.max()))


def oracle_obs(case, state):
    orc = PE.oracle_of(case)
    PE.set_oracle(orc, *state)
    return orc.observe()


def check_inputs(case, mode, tr):
    """2. obs_in[t] is step t - 1's rows bit for bit, or -- at an episode start, and at step 0 -- the fp64 oracle's observation of
    the reset draws (of the start state) within 1e-5"""
    A = len(PE.obs_widths(case))
    for k in range(T):
        gt = case.step0 + k
        if PE.is_restart(case, gt) or k == 0:
            want = oracle_obs(case, PE.restart_state(case, gt // case.episode_len) if PE.is_restart(case, gt) else PE.initial_state(case))
            for i in range(A):
                close(np_(tr.obs_in[k][i]), want[i], what="%s %s obs_in[%d][%d]" % (case.id, mode, k, i))
        else:
            for i in range(A):
                assert same_bits(tr.obs_in[k][i], tr.obs[k - 1][i]), (case.id, mode, k, i, "obs_in is not the previous step's row")


def check_replay(case, mode, tr, final):
    """3. the recorded rows through step_many on a second env: obs, rew, done and the final state bit for bit"""
    env2 = make_env(case)
    start(env2, case)
    outs = step_many(env2, tr.act[:T].contiguous(), episode_len=case.episode_len, seed=case.world_seed)
    torch.cuda.synchronize()
    for k in range(T):
        o, r, d = outs[k]
        for i in range(env2.n):
            assert same_bits(tr.obs[k][i], o[i]), (case.id, mode, k, i, "obs")
        assert same_bits(tr.rew[k], r) and torch.equal(tr.done[k], d), (case.id, mode, k)
    p2, v2 = env2.world.get_state()
    assert same_bits(final[0], p2) and same_bits(final[1], v2), (case.id, mode, "final state")


def check_stepwise(case, mode, env, mods, tr, final):
    """3. where step_many cannot follow (counter edges): T run(1) calls, after each the state, rows and rewards against the fp64
    oracle stepped once from the GPU's own previous state (at a restart: from the reset draws) with the GPU's own row, at 1e-5,
    rewards within 1e-5 of a contact threshold left out (guard_ok); and the one run(T) equals the T run(1) calls bit for bit.
    -> worlds in which an immovable agent was in contact with another at some step"""
    spec = PE.case_spec(case)
    pos, vel, choice = start(env, case)
    roll = new_rollout(env, case, mods, mode)
    orc = PE.oracle_of(case)
    touched = np.zeros(case.B, bool)
    for k in range(T):
        gt = case.step0 + k
        if PE.is_restart(case, gt):
            pos, vel, choice = PE.restart_state(case, gt // case.episode_len)
        one = roll.run(1, record_inputs=True)
        torch.cuda.synchronize()
        PE.set_oracle(orc, pos, vel, choice)
        for i in case.immovable:
            for j in range(spec.n_agents):
                if j != i and spec.collide[i] and spec.collide[j]:
                    touched |= np.sqrt(((orc.pos[:, i] - orc.pos[:, j]) ** 2).sum(-1)) < spec.size[i] + spec.size[j]
        obs, rew, _, _ = orc.step(np_(one.act[0]).astype(np.float64))
        pos, vel = env.world.get_state()
        what = "%s step %d " % (case.id, k)
        close(pos, orc.pos, what=what + "pos")
        close(vel, orc.vel, what=what + "vel")
        ok = guard_ok(spec, orc.pos)
        for i in range(spec.n_agents):
            close(np_(one.obs[0][i]), obs[i], what=what + "obs%d" % i)
            close(np_(one.rew[0, i])[ok], rew[i][ok], what=what + "rew%d" % i)
        assert same_bits(one.act[0], tr.act[k]) and same_bits(one.logp[0], tr.logp[k]) and same_bits(one.rew[0], tr.rew[k]), (case.id, k)
        for i in range(spec.n_agents):
            assert same_bits(one.obs[0][i], tr.obs[k][i]) and same_bits(one.obs_in[0][i], tr.obs_in[k][i]), (case.id, k, i)
    assert same_bits(pos, final[0]) and same_bits(vel, final[1]), (case.id, "run(T) and T x run(1) end in different states")
    return touched


# ---- the case sweep -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", PE.CASE_IDS)
def test_case_against_fp64(cid, record_parity):
    """Immovable agent (immovable_agent1): the host layer takes the env; the agent's state stays bit-unchanged, its decisions are
    written and correct (comparison 1 runs over every agent), and the others collide with it (the oracle's step, and the replay)."""
    case = PE.BY_ID[cid]
    env = make_env(case)
    layers, acts = PE.case_layers(case)
    mods = modules(env, layers, acts, case.shared)
    t, done = tally_of(case.sweep, record_parity)
    for mode in case.modes:
        tr, final = run_case(env, case, mods, mode)
        check_decisions(case, mode, tr, layers, acts, t)
        check_inputs(case, mode, tr)
        if case.counter_edge or case.immovable:
            if mode == "sample":
                touched = check_stepwise(case, mode, env, mods, tr, final)
                if case.immovable:
                    print("%s: %d worlds with the immovable agent in contact" % (cid, int(touched.sum())))
                    assert touched.any(), "no world in which the others collide with the immovable agent"
        if not case.counter_edge:
            check_replay(case, mode, tr, final)
        if case.immovable:
            p0, v0, _ = PE.initial_state(case)
            for i in case.immovable:
                assert same_bits(final[0][:, i], p0[:, i]) and same_bits(final[1][:, i], v0[:, i]), "an immovable agent's state changed"
    done()


@pytest.mark.parametrize("cid", [c.id for c in PE.CASES if c.custom is not None])
def test_constants_assigned_on_a_live_env(cid):
    """the same constants assigned attribute by attribute on an env that was built with the scenario's own and has already
    rolled out: the next run re-reads them and is the run of the env built around them, bit for bit"""
    case = PE.BY_ID[cid]
    layers, acts = PE.case_layers(case)
    built = make_env(case)
    want, want_final = run_case(built, case, modules(built, layers, acts), "sample")
    live = make_env(case, customise=False)
    mods = modules(live, layers, acts)
    before, _ = run_case(live, case, mods, "sample")
    assert not same_bits(before.rew[:T], want.rew[:T]), "the constants change nothing the rollout shows"
    PE.customise_world(case, live.world)
    got, final = run_case(live, case, mods, "sample")
    for name in ("act", "logp", "rew", "done", "obs_flat", "obs_in_flat"):
        assert same_bits(getattr(got, name), getattr(want, name)), (cid, name)
    assert same_bits(final[0], want_final[0]) and same_bits(final[1], want_final[1])


@pytest.mark.parametrize("shape", ["spread3", "push"])
@pytest.mark.parametrize("L", [2, 3, 8])
def test_launch_splits(L, shape):
    """run(3); run(1); run(3) == run(7) bit for bit: the launch boundaries fall before, on and after a restart"""
    case = dataclasses.replace(PE.BY_ID["batch_%s_B65" % shape], episode_len=L, B=130)
    env = make_env(case)
    layers, acts = PE.case_layers(case)
    mods = modules(env, layers, acts)
    whole, final = run_case(env, case, mods, "sample")
    start(env, case)
    roll = new_rollout(env, case, mods, "sample")
    parts = [roll.run(n, record_inputs=True) for n in (3, 1, 3)]
    torch.cuda.synchronize()
    for name in ("act", "logp", "rew", "done", "obs_flat", "obs_in_flat"):
        got = torch.cat([getattr(p, name) for p in parts])
        assert same_bits(got, getattr(whole, name)[:got.shape[0]]), (L, shape, name)
    p, v = env.world.get_state()
    assert same_bits(p, final[0]) and same_bits(v, final[1])


# ---- known answers (simple_spread 3, B = 65, episode_len = 1: every decision input is known before the run) ----------------------------------
def known_run(case, layers, acts, mode):
    env = make_env(case)
    tr, _ = run_case(env, case, modules(env, layers, acts), mode)
    return np_(tr.act[:T]), np_(tr.logp[:T]), tr


def test_zero_last_layer_equal_biases(record_parity):
    """every logit is 0.5: greedy picks index 0 in every world; the softmax rows are exactly 0.2f; the sample pick is the fp32
    rule's -- c_0 = p_0, c_j = c_{j-1} + p_j in float32, the first j <= 3 with u < c_j, else 4 -- outside |0.2 (j + 1) - u| <= 1e-5;
    logp = log 0.2 within 2e-6"""
    case, layers, acts = PE.known_equal_logits()
    act, _, _ = known_run(case, layers, acts, "greedy")
    assert (act[..., 0] == 1).all() and (act[..., 1:] == 0).all()
    act, _, _ = known_run(case, layers, acts, "softmax")
    assert (act.view(np.uint32) == np.float32(0.2).view(np.uint32)).all()
    act, logp, _ = known_run(case, layers, acts, "sample")
    cj = np.cumsum(np.full(4, 0.2, np.float32), dtype=np.float32)
    inband = 0
    for k in range(T):
        for i in range(3):
            u = R.draw_u(R.STREAM_POLICY, case.policy_seed, case.B, k, i, case.world_offset)
            want = np.minimum((cj[None, :].astype(np.float64) <= u[:, None]).sum(axis=1), 4)
            ok = (np.abs(0.2 * np.arange(1, 5)[None, :] - u[:, None]) > 1e-5).all(axis=1)
            inband += int((~ok).sum())
            a = act[k, i]
            assert (a.sum(axis=1) == 1).all() and (a.max(axis=1) == 1).all()
            assert np.array_equal(a.argmax(axis=1)[ok], want[ok]), (k, i)
    assert len(np.unique(act.argmax(axis=-1))) == 5
    assert float(np.abs(logp.astype(np.float64) - np.log(0.2)).max()) <= 2e-6
    assert inband <= R.CAP * act[..., 0].size + 1
    record_parity("policy_edges_known_equal_logits", {"rows_checked": int(act[..., 0].size), "rows_in_band": inband,
                                                      "worst_logp_error": float(np.abs(logp.astype(np.float64) - np.log(0.2)).max())})


def test_saturated_tanh(record_parity):
    """first layers scaled so that every hidden pre-activation is beyond 50 in magnitude on the reference: exp2 overflows (or is
    0) inside the Tanh; the decisions stay finite and within the bars"""
    case, layers, acts, _ = PE.known_saturated_tanh()
    t, done = tally_of("known_saturated_tanh", record_parity)
    for mode in PE.MODE_NAMES:
        act, logp, tr = known_run(case, layers, acts, mode)
        assert np.isfinite(act).all() and (mode != "sample" or np.isfinite(logp).all())
        for k in range(T):
            for i in range(3):
                W, b = layers[i][0]
                pre = np_(tr.obs_in[k][i]).astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64)
                assert np.abs(pre).min() > 50, (k, i)
        check_decisions(case, mode, tr, layers, acts, t)
    done()


def test_very_large_logits(record_parity):
    """last layers scaled so that the reference's top-two margin is beyond 200: exactly one-hot softmax rows, greedy == sample ==
    argmax, logp of the chosen index 0 within 2e-6, no NaN"""
    case, layers, acts, _ = PE.known_large_logits()
    runs = {mode: known_run(case, layers, acts, mode) for mode in PE.MODE_NAMES}
    for k in range(T):
        for i in range(3):
            ref = R.ref_decide(layers[i], acts[i], 1, 0, 0, np_(runs["greedy"][2].obs_in[k][i]), "greedy", 0, k, i, 0)
            top = np.sort(ref["z"], axis=1)
            assert (top[:, -1] - top[:, -2]).min() > 200, (k, i)
            want = np.eye(5, dtype=np.float32)[ref["heads"][0]["greedy"]]
            for mode in PE.MODE_NAMES:      # (episode_len = 1: the three runs decide on the same inputs)
                assert np.array_equal(runs[mode][0][k, i], want), (mode, k, i)
    logp = runs["sample"][1]
    assert not np.isnan(logp).any() and float(np.abs(logp).max()) <= 2e-6
    record_parity("policy_edges_known_large_logits", {"rows_checked": int(3 * logp.size), "worst_logp_error": float(np.abs(logp).max())})


@pytest.mark.parametrize("mode", ["greedy", "sample", "softmax"])
def test_a_poisoned_world_stays_alone(mode):
    """one world per wave with a NaN agent position: every other world's rows, observations, rewards and final state are what
    the clean run gives, bit for bit; the poisoned worlds' action rows are still rows (one-hot: they sum to 1)"""
    case = dataclasses.replace(PE.BY_ID["mixed_set"], episode_len=0)      # (a restart would redraw the poisoned position)
    layers, acts = PE.case_layers(case)
    env = make_env(case)
    mods = modules(env, layers, acts)
    clean, clean_final = run_case(env, case, mods, mode)
    sick = [5, 70, 129]
    pos, vel, choice = PE.initial_state(case)
    pos = pos.copy()
    pos[sick, 1] = np.nan
    env.world.set_state(pos, vel)
    tr = canary_traj(env)
    new_rollout(env, case, mods, mode).run(T, trajectory=tr, record_inputs=True)
    torch.cuda.synchronize()
    assert canary_intact(tr)
    keep = np.ones(case.B, bool)
    keep[sick] = False
    for i in range(3):      # the poison did reach every actor of those worlds, and those worlds alone
        seen = np.isnan(np_(tr.obs_in[0][i])).any(axis=1)
        assert seen[sick].all() and not seen[keep].any(), i
    assert same_bits(np_(tr.act[:T])[:, :, keep], np_(clean.act[:T])[:, :, keep])
    assert same_bits(np_(tr.rew[:T])[:, :, keep], np_(clean.rew[:T])[:, :, keep])
    if mode == "sample":
        assert same_bits(np_(tr.logp[:T])[:, :, keep], np_(clean.logp[:T])[:, :, keep])
    for k in range(T):
        for i in range(3):
            assert same_bits(np_(tr.obs[k][i])[keep], np_(clean.obs[k][i])[keep]), (k, i)
    p, v = env.world.get_state()
    assert same_bits(p[keep], clean_final[0][keep]) and same_bits(v[keep], clean_final[1][keep])
    if mode != "softmax":
        a = np_(tr.act[:T])[:, :, sick]
        assert (a.sum(axis=-1) == 1).all() and (a.max(axis=-1) == 1).all() and ((a == 0) | (a == 1)).all()


# ---- the C entry point ------------------------------------------------------------------------------------------------------------------------
def abi_run(env, case, mods, mode, record=True, logp=True, relayout=None):
    """mpe_rollout_policy called directly -> (rc, canary trajectory).  relayout(weights, pol) -> the weights tensor to hand over"""
    start(env, case)
    roll = new_rollout(env, case, mods, mode)
    tr = canary_traj(env)
    weights, pol = MlpPolicy(mods).pack(roll.obs_widths, env.world.device, mode, case.policy_seed)
    if relayout is not None:
        weights = relayout(weights, pol)
        pol.weights = weights.data_ptr()
    rc = _abi.lib().mpe_rollout_policy(C.byref(roll._desc), C.byref(tr.bufs), C.byref(pol), case.B, T, case.episode_len, roll._lr,
                                       case.world_seed, case.step0, case.world_offset, 1, tr.act.data_ptr(),
                                       tr.obs_in_flat.data_ptr() if record else None, tr.logp.data_ptr() if logp else None,
                                       _abi.raw_stream(env.world.device))
    torch.cuda.synchronize()
    del weights
    return rc, tr


def test_greedy_with_logp_out(record_parity):
    """PolicyRollout never passes logp_out in GREEDY mode; the entry point allows it: log softmax at the argmax, within logp_bar"""
    case = PE.BY_ID["mixed_set"]
    env = make_env(case)
    layers, acts = PE.case_layers(case)
    rc, tr = abi_run(env, case, modules(env, layers, acts), "greedy")
    assert rc == 0, _abi.lib().mpe_last_error()
    assert canary_intact(tr) and not bool((tr.logp[:T] == PE.CANARY_F).any())
    t, done = tally_of("abi_greedy_logp", record_parity)
    check_decisions(case, "greedy", tr, layers, acts, t, with_logp=True)
    done()


def test_sample_without_recording_gives_the_same_bits():
    case = PE.BY_ID["mixed_set"]
    env = make_env(case)
    layers, acts = PE.case_layers(case)
    mods = modules(env, layers, acts)
    rc, a = abi_run(env, case, mods, "sample")
    assert rc == 0, _abi.lib().mpe_last_error()
    rc, b = abi_run(env, case, mods, "sample", record=False)
    assert rc == 0, _abi.lib().mpe_last_error()
    assert bool((b.obs_in_flat == PE.CANARY_F).all()), "obs_in written although obs_in_out was NULL"
    for name in ("act", "logp", "rew", "obs_flat"):
        assert same_bits(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize("mode", ["sample", "softmax"])
def test_relaid_out_weights(mode):
    """MlpPolicy.pack's blob re-laid out -- the actors in reverse order with 16 k floats of NaN in front of, between and behind
    them, pol.offset[i] rewritten: the rollout is the contiguous blob's bit for bit (pol.off[i] is what is read, and nothing
    outside an actor's own packed size)"""
    case = PE.BY_ID["mixed_set"]
    env = make_env(case)
    layers, acts = PE.case_layers(case)
    mods = modules(env, layers, acts)
    rc, want = abi_run(env, case, mods, mode, logp=mode != "softmax")
    assert rc == 0, _abi.lib().mpe_last_error()

    def relayout(weights, pol):
        A = 3
        offs = [int(pol.offset[i]) for i in range(A)]
        sizes = np.diff(offs + [weights.numel()]).tolist()
        assert offs == sorted(offs) and all(s > 0 and s % 16 == 0 for s in sizes), (offs, sizes)
        for i, lay in enumerate(layers):      # the packed size of each actor, restated: (in + 1) * wide per layer, 8 wide at the end
            n = sum((W.shape[1] if k == 0 else 64) + 1 for k, (W, _) in enumerate(lay[:-1])) * 64 if len(lay) > 1 else 0
            n += ((lay[-1][0].shape[1] if len(lay) == 1 else 64) + 1) * 8
            assert sizes[i] == n + (-n) % 16, (i, sizes[i], n)
        parts, at = [], 0
        for k, i in enumerate(reversed(range(A))):
            gap = 16 * (k + 1)
            parts.append(torch.full((gap,), float("nan"), device=weights.device))
            at += gap
            parts.append(weights[offs[i]:offs[i] + sizes[i]])
            pol.offset[i] = at
            at += sizes[i]
        parts.append(torch.full((64,), float("nan"), device=weights.device))
        return torch.cat(parts).contiguous()
    rc, got = abi_run(env, case, mods, mode, logp=mode != "softmax", relayout=relayout)
    assert rc == 0, _abi.lib().mpe_last_error()
    assert canary_intact(got)
    for name in ("act", "logp", "rew", "done", "obs_flat", "obs_in_flat"):
        assert same_bits(getattr(got, name), getattr(want, name)), name
