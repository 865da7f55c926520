"""TD targets on the device: mpe_actor_act_rows against the fp64 restatement of tests/_actor_ref.py and its joint rows
against the rule of include/mpe_hip.h, mpe_critic_q against fp64, against the merged actor kernel's logit 0 and against the y rule,
and the Python path (Actors.act_rows, Critics, TdTargets) end to end behind a replay buffer, eagerly and inside a HIP graph.

Margins measured on an MI355X (worst error / bar; record_parity keys td_target_*; DESIGN.md 2.14's table): act_rows 8 820 rows, 0 in
the band, logits 0.016, softmax 0.005, logp 0.012; critic q 0.026; end to end action columns 0.003, q_next 0.008."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd.learner import Critics, TdTargets
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop
from multiagent_particle_envs_amd.replay import PrioritizedReplayBuffer, ReplayBuffer

import _actor_ref as R
import _td_target_ref as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE_NAMES = ("greedy", "softmax", "sample")
_TALLY = R.Tally()
_WORST = {}


def _margin(key, m):
    _WORST[key] = max(_WORST.get(key, 0.0), float(m))
    return _WORST[key]


# ---- mpe_actor_act_rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("name", T.CASE_NAMES)
def test_act_rows_case(name, mode, record_parity):
    c = T.CASES[T.CASE_NAMES.index(name)]
    agents, obs = R.build_case(c)
    seed, t, off, dc = c["draw_seed"], c["t"], c["world_offset"], c["dim_c"]
    out = T.run_rows_abi(agents, dc, obs, mode, seed, t, off)
    assert out["rc"] == 0, out["error"]
    assert out["canary_ok"], (name, "a store landed behind the last row")
    for k in ("moves", "utter", "logp", "logits"):
        if out[k] is not None:
            assert not (out[k] == R.CANARY_F).any(), (name, k, "rows the launch did not write")
    assert not (out["ids"] == R.CANARY_I).any()
    before = (_TALLY.checked, _TALLY.inband)
    for i, a in enumerate(agents):
        ref = R.ref_decide(a["layers"], a["act"], a["movable"], a["speaks"], dc, obs[i], mode, seed, t, i, off)
        R.check_agent(out, i, ref, mode, _TALLY, "%s %s" % (name, mode))
    assert _TALLY.inband - before[1] <= R.CAP * (_TALLY.checked - before[0]) + 1, (name, mode, "rows inside the band")
    # the joint rows: the rule applied to this launch's own rows, bit for bit; the stride tail untouched
    width = out["width"]
    mv, sp = [a["movable"] for a in agents], [a["speaks"] for a in agents]
    assert width == T.case_layout(c)[1] and out["joint"].shape == (c["B"], width + T.JOINT_TAIL)
    want = T.joint_rows(obs, out["moves"], out["utter"], mv, sp, dc)
    assert out["joint"][:, :width].tobytes() == want.tobytes(), (name, mode, "joint rows")
    assert (out["joint"][:, width:] == R.CANARY_F).all(), (name, mode, "a column at or beyond the joint width was written")
    # without joint: the same rows; without moves / utter: the same joint
    plain = T.run_rows_abi(agents, dc, obs, mode, seed, t, off, joint=False)
    assert plain["rc"] == 0 and plain["canary_ok"] and plain["joint"] is None
    for k in ("moves", "utter", "logp", "ids"):
        assert (out[k] is None and plain[k] is None) or out[k].tobytes() == plain[k].tobytes(), (name, mode, k)
    only = T.run_rows_abi(agents, dc, obs, mode, seed, t, off, moves=False)
    assert only["rc"] == 0 and only["canary_ok"] and only["moves"] is None and only["utter"] is None
    assert only["joint"].tobytes() == out["joint"].tobytes(), (name, mode, "joint without moves")
    rep = _TALLY.report()
    record_parity("td_target_act_rows", rep)
    print("act_rows so far: %s" % rep)


def _mlp(D, n_out, hidden=(64, 64)):
    mods, k = [], D
    for h in hidden:
        mods += [nn.Linear(k, h), nn.ReLU()]
        k = h
    return nn.Sequential(*(mods + [nn.Linear(k, n_out)])).cuda()


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_act_rows_equals_act(mode):
    torch.manual_seed(0)
    env = mpe.make_env("simple_spread", batch_size=70)
    env.world.world_offset = 1234
    pi = Actors(env, [_mlp(18, 5) for _ in range(3)], mode=mode, seed=5, logp=(mode != "softmax"), ids=True, logits=True)
    obs_n = env.reset()
    for t in (0, 7):
        a = pi.act(obs_n, t).clone()
        b = pi.act_rows(obs_n, t, row_offset=env.world.world_offset, joint=True)
        assert torch.equal(a, b) and pi.joint_rows.shape == (70, 69)
        assert torch.equal(pi.ids, pi.rows.ids) and torch.equal(pi.logits, pi.rows.logits)
        if pi.logp is not None:
            assert torch.equal(pi.logp, pi.rows.logp)
        assert torch.equal(pi.joint_rows, torch.cat(list(obs_n) + [b[i] for i in range(3)], dim=1))
        assert torch.equal(a, pi.moves), "act_rows wrote act()'s own buffers"
    if mode == "sample":      # the row offset is the draw key
        c = pi.act_rows(obs_n, 7, row_offset=0).clone()
        assert not torch.equal(c, a)


# ---- mpe_critic_q ---------------------------------------------------------------------------------------------------------------
def _td_inputs(A, M, seed):
    rs = np.random.RandomState(seed)
    ret = (rs.standard_normal((A, M)) * 3).astype(np.float32)
    done = (rs.uniform(size=(A, M)) < 0.4).astype(np.uint8)
    done[:, 0] = (1, 0, 1)[:A] if M == 1 else done[:, 0]
    disc = (0.95 ** rs.randint(1, 4, M)).astype(np.float32)
    return ret, done, disc


@pytest.mark.parametrize("shape", T.CRITIC_SHAPES, ids=T.CRITIC_IDS)
def test_critic_q(shape, record_parity):
    critics, rows = T.build_critics(shape)
    A, M = len(critics), shape[2]
    ret, done, disc = _td_inputs(A, M, 1)
    out = T.run_critic_abi(critics, rows, dict(ret=ret, done=done, discount=disc))
    assert out["rc"] == 0, out["error"]
    assert out["canary_ok"] and not (out["q"] == R.CANARY_F).any() and not (out["y"] == R.CANARY_F).any()
    q64 = np.stack([T.critic_q(l, rows, np.float64) for l in critics])
    m = float((np.abs(out["q"] - q64) / (T.Q_BAR * np.maximum(1, np.abs(q64)))).max())
    print("critic %s: worst |q - q64| / bar %.3f" % (shape, m))
    assert m < 1.0
    record_parity("td_target_critic_q", {"worst_error_over_bar": _margin("q", m), "bar": "1e-5 * max(1, |q|)"})
    # the merged kernel as the yardstick: the same packed weights declared as one-logit utterance heads
    agents = [{"layers": l, "act": R.RELU, "movable": 0, "speaks": 1} for l in critics]
    act = R.run_abi(agents, 1, [rows] * A, "softmax", 0, 0, 0, want=("utter", "logits"))
    assert act["rc"] == 0, act["error"]
    assert out["q"].tobytes() == act["logits"][:, :, 0].tobytes(), "q is not the merged kernel's logit 0"
    # y: the rule on the launch's own q, with a discount row and with gamma alone
    assert T.same_floats(out["y"], T.y_rule(ret, done, out["q"], disc))
    g = T.run_critic_abi(critics, rows, dict(ret=ret, done=done, discount=None, gamma=0.95))
    assert g["rc"] == 0 and g["canary_ok"] and g["q"].tobytes() == out["q"].tobytes()
    assert T.same_floats(g["y"], T.y_rule(ret, done, g["q"], None, 0.95))
    if M > 1:
        assert not T.same_floats(g["y"], out["y"])
    # no td: q alone, the same
    q_only = T.run_critic_abi(critics, rows)
    assert q_only["rc"] == 0 and q_only["y"] is None and q_only["q"].tobytes() == out["q"].tobytes()
    # done rows behind a non-finite q: critic 0's last bias is +inf, critic 1's NaN
    bad = [list(l) for l in critics]
    bad[0][-1] = (bad[0][-1][0], np.array([np.inf], np.float32))
    bad[1][-1] = (bad[1][-1][0], np.array([np.nan], np.float32))
    nf = T.run_critic_abi(bad, rows, dict(ret=ret, done=done, discount=disc))
    assert nf["rc"] == 0 and nf["canary_ok"]
    assert np.isinf(nf["q"][0]).all() and np.isnan(nf["q"][1]).all() and nf["q"][2].tobytes() == out["q"][2].tobytes()
    assert T.same_floats(nf["y"], T.y_rule(ret, done, nf["q"], disc))
    d = done != 0
    assert nf["y"][d].tobytes() == ret[d].tobytes(), "done did not hide a non-finite q"
    assert not np.isfinite(nf["y"][:2][~d[:2]]).any()


def test_critic_q_one_shared_module():
    """joint width 69, one packed critic behind all three agents (equal offsets)"""
    critics, rows = T.build_critics(T.CRITIC_SHAPES[2])
    from multiagent_particle_envs_amd import _abi
    import ctypes as C
    aset, blob = T.make_critic_set(critics[:1] * 3)
    one = blob[:blob.size // 3].copy()
    for i in range(3):
        aset.offset[i] = 0
    dev = torch.device("cuda", torch.cuda.current_device())
    wts, x = torch.as_tensor(one, device=dev), torch.as_tensor(rows, device=dev)
    aset.weights = wts.data_ptr()
    q = torch.full((3 * 65 + R.CANARY_ROWS,), R.CANARY_F, device=dev)
    rc = _abi.lib().mpe_critic_q(C.byref(aset), (C.c_void_p * 3)(*([x.data_ptr()] * 3)), 65, q.data_ptr(), None, None, _abi.raw_stream(dev))
    assert rc == 0, _abi.lib().mpe_last_error()
    torch.cuda.synchronize()
    host = q.cpu().numpy()
    assert (host[3 * 65:] == R.CANARY_F).all()
    got = host[:3 * 65].reshape(3, 65)
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()
    q64 = T.critic_q(critics[0], rows, np.float64)
    assert (np.abs(got[0] - q64) <= T.Q_BAR * np.maximum(1, np.abs(q64))).all()


# ---- the Python path, end to end ------------------------------------------------------------------------------------------------
def _learner(prioritized=False, batch_size=7, shared_critic=False):
    torch.manual_seed(3)
    env = mpe.make_env("simple_spread", batch_size=batch_size, seed=1)
    pi = Actors(env, [_mlp(18, 5) for _ in range(3)], mode="sample", seed=2)
    loop = PolicyLoop(env, pi, episode_len=5)
    buf = (PrioritizedReplayBuffer if prioritized else ReplayBuffer)(env, 8, seed=4)
    mu_t = Actors(env, [_mlp(18, 5) for _ in range(3)], mode="softmax", logits=True)
    q_t = Critics(env, _mlp(69, 1) if shared_critic else [_mlp(69, 1) for _ in range(3)])
    return env, loop, buf, mu_t, q_t, TdTargets(mu_t, q_t)


def _check_compute(batch, td, mu_t, q_t, y, disc, gamma, record_parity):
    jn = td.joint_next_act
    assert jn.shape == (130, 69) and td.q_next.shape == (3, 130) and y.shape == (3, 130) and y is td.y
    assert torch.equal(jn[:, :54], batch.joint_next)
    assert all(torch.equal(jn[:, 18 * i:18 * i + 18], batch.next_obs_n[i]) for i in range(3))
    # the target actors' softmax rows against fp64, the critics against fp64 on the kernel's own rows
    ref = mu_t.reference(batch.next_obs_n)
    worst = 0.0
    for i in range(3):
        z = ref[i][0].cpu().numpy()
        p = np.exp(z - z.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        bar = R.BAND * np.maximum(1, np.abs(z).max(axis=1))
        got = jn[:, 54 + 5 * i:59 + 5 * i].cpu().numpy().astype(np.float64)
        worst = max(worst, float((np.abs(got - p).max(axis=1) / bar).max()))
    assert worst < 1.0, ("target actors' action columns", worst)
    q64 = q_t.reference(jn).cpu().numpy()
    mq = float((np.abs(td.q_next.cpu().numpy() - q64) / (T.Q_BAR * np.maximum(1, np.abs(q64)))).max())
    assert mq < 1.0, ("q_next", mq)
    ret = (batch.ret if disc is not None else batch.rew).cpu().numpy()
    want = T.y_rule(ret, batch._done_u8.cpu().numpy(), td.q_next.cpu().numpy(), disc.cpu().numpy() if disc is not None else None, gamma)
    assert T.same_floats(y.cpu().numpy(), want)
    record_parity("td_target_end_to_end", {"action_columns_error_over_bar": _margin("e2e_act", worst),
                                           "q_next_error_over_bar": _margin("e2e_q", mq)})


@pytest.mark.parametrize("kind", ["nstep", "one_step", "prioritized"])
def test_end_to_end(kind, record_parity):
    env, loop, buf, mu_t, q_t, td = _learner(prioritized=(kind == "prioritized"))
    loop.run(12, record=False, replay=buf)
    if kind == "one_step":
        batch = buf.sample(130, joint=True)
        y = td.compute(batch, gamma=0.95)
        _check_compute(batch, td, mu_t, q_t, y, None, 0.95, record_parity)
    else:
        batch = buf.sample(130, joint=True, n_step=3, gamma=0.95, episode_len=5)
        y = td.compute(batch)
        _check_compute(batch, td, mu_t, q_t, y, batch.discount, None, record_parity)
    assert td.t == 1
    if kind == "prioritized":
        q = Critics(env, [_mlp(69, 1) for _ in range(3)]).q(batch.joint)
        buf.update_td(batch.idx, y[0] - q[0])
        torch.cuda.synchronize()
        pr = buf.priorities.reshape(-1)[batch.idx]
        assert torch.isfinite(pr).all() and float(pr.min()) > 0


def test_in_place_weight_updates_are_seen_until_freeze():
    env, loop, buf, mu_t, q_t, td = _learner()
    loop.run(12, record=False, replay=buf)
    batch = buf.sample(130, joint=True, n_step=3, gamma=0.95, episode_len=5)
    y0 = td.compute(batch, t=0).clone()
    assert torch.equal(td.compute(batch, t=0), y0)
    with torch.no_grad():
        q_t.modules[1][4].bias[0] += 0.5
    y1 = td.compute(batch, t=0).clone()
    assert not torch.equal(y1[1], y0[1]) and torch.equal(y1[0], y0[0]) and torch.equal(y1[2], y0[2])
    with torch.no_grad():
        mu_t.modules[0][4].bias[2] += 1.0
    y2 = td.compute(batch, t=0).clone()
    assert not torch.equal(y2, y1)
    mu_t.freeze()
    q_t.freeze()
    with torch.no_grad():
        q_t.modules[1][4].bias[0] += 0.5
        mu_t.modules[0][4].bias[2] += 1.0
    assert torch.equal(td.compute(batch, t=0), y2)
    mu_t.unfreeze()
    q_t.unfreeze()
    assert not torch.equal(td.compute(batch, t=0), y2)


def test_push_sample_compute_in_one_graph():
    env, loop, buf, mu_t, q_t, td = _learner()
    loop.run(12, record=False, replay=buf)
    loop.pi.freeze()
    mu_t.freeze()
    q_t.freeze()
    kw = dict(joint=True, n_step=3, gamma=0.95, episode_len=5)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    t0, count0, draw0 = loop.t, buf.count, 100
    with torch.cuda.stream(s):
        head = buf.head.clone()
        state = (env.world.pos.clone(), env.world._vel_all.clone(), [o.clone() for o in loop.obs_n], loop.obs_n, env._flip)
        for _ in range(2):      # code objects and allocations outside the capture
            loop.step(replay=buf)
            td.compute(buf.sample(130, draw=draw0, **kw), t=9)
        buf.head.copy_(head)
        env.world.pos.copy_(state[0])
        env.world._vel_all.copy_(state[1])
        for dst, src in zip(state[3], state[2]):
            dst.copy_(src)
        loop.t, loop.obs_n, env._flip, buf.count = t0, state[3], state[4], count0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            loop.step(replay=buf)
            batch = buf.sample(130, draw=draw0, **kw)
            y = td.compute(batch, t=9)
    torch.cuda.current_stream().wait_stream(s)
    seen = []
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        buf.count = count0 + k + 1
        got, idx = y.clone(), batch.idx.clone()
        assert int(buf.head) == buf.count
        want = td.compute(buf.gather(idx, **kw), t=9)
        assert torch.equal(got, want), "replay %d" % k
        seen.append(got)
    assert not torch.equal(seen[0], seen[1]) or not torch.equal(seen[1], seen[2])


def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "maddpg_spread.py"), "--worlds", "16", "--batch", "64", "--updates", "2"],
                       capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    import json
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2
    for l in lines:
        assert np.isfinite(l["critic_loss"]) and np.isfinite(l["actor_loss"])
