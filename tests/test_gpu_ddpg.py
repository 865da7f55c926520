"""The off-policy update's device pieces on the GPU: mpe_td_loss and mpe_polyak BIT-EQUAL to the float32 restatements
of tests/_ddpg_ref.py on every shape; mpe_policy_rows against joint's bits outside the windows, the actor kernel's own softmax bits
inside, sentinels behind row M; mpe_policy_rows_grad, ActorLoss and the losses within the project's parity bound (4 x float32 torch
autograd's deviation from the float64 restatement on this GPU, floor 2 ulps); the prioritized buffer's wiring; a whole MADDPG update
captured as ONE HIP graph; and the example's --device-update mode.

mpe_td_loss also runs where its second launch (k_ddpg_finish, the PPO head's two loops over the chunks' partials) takes a second piece
and a second trip of a piece's load: (L32, 16385), (L22, 87297) and (L22, 131073), bit-equal like every other shape.

Recorded on an MI355X: profiles/ddpg_parity.json (tools/ddpg_parity.py)."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.learner import (ActorLoss, Critics, RowsLayout, TdLoss, TdTargets, policy_rows_grad_tensors,
                                                  policy_rows_tensors, td_loss_tensors)
from multiagent_particle_envs_amd.optim import DeviceAdam, PolyakTargets
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop
from multiagent_particle_envs_amd.replay import PrioritizedReplayBuffer, ReplayBuffer
from multiagent_particle_envs_amd.train import Trainable, mlp_dinput_tensors, mlp_grad_tensors

import _ddpg_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -777.25
PAD = 64      # sentinel floats (256 bytes: the 16-byte alignment stays) in front of and behind a buffer
LAYOUT_IDS = sorted(R.LAYOUTS)
PARITY = {}   # name -> the largest deviation / bound seen (tools/ddpg_parity.py writes it out)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _t(a):
    return torch.tensor(np.asarray(a), device=_dev())


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _u32(t):
    return t.detach().cpu().numpy().reshape(-1).view(np.uint32)


def _layout(lay):
    return RowsLayout(lay.W, lay.dim_c, lay.col, lay.movable, lay.speaks)


def _note(name, dev, bound):
    PARITY[name] = max(PARITY.get(name, 0.0), dev / bound if bound > 0 else 0.0)
    print("%s: ours %.3e bound %.3e" % (name, dev, bound))


@pytest.fixture(scope="module", autouse=True)
def _parity_out():
    yield
    if os.environ.get("MPE_DDPG_PARITY_OUT"):      # tools/ddpg_parity.py
        with open(os.environ["MPE_DDPG_PARITY_OUT"], "w") as f:
            f.write(json.dumps({"device": torch.cuda.get_device_name(0), "largest_fraction_of_bound": max(PARITY.values()) if PARITY else None,
                                "fraction_of_bound": PARITY}) + "\n")


# ---- THE TD LOSS RULE ----------------------------------------------------------------------------------------------------------------
# The second launch (k_ddpg_finish: the PPO head's loops over the chunks' partials) past each loop's first trip: pieces of 6144 / (6 A)
# chunks, a piece of one agent loaded 8 x 256 doubles at a trip.  A = 16, 65 chunks in pieces of 64: a second piece of one chunk of
# one row; A = 2, 342 chunks in one piece of 2052 doubles per agent: a second trip of the load; A = 2, 513 chunks in pieces of 512: a
# second piece.
TD_SECOND_TRIPS = [(16385, "L32"), (87297, "L22"), (131073, "L22")]


@pytest.mark.parametrize("M,name", [(M, name) for M in R.ROWS for name in LAYOUT_IDS] + TD_SECOND_TRIPS)
def test_td_loss_bit_equal_to_the_restatement(M, name):
    """with and without the weights; the A [M] blocks at their own addresses; a second run gives the same bits"""
    lay = R.LAYOUTS[name]
    x = R.make_inputs(lay, M)
    q_n, y, w = [_t(x["q"][i]) for i in range(lay.A)], _t(x["y"]), _t(x["w"])
    for weights, wn in ((w, x["w"]), (None, None)):
        want = R.td_loss32(x["q"], x["y"], wn)
        res = td_loss_tensors(q_n, y, weights)
        first = [t.clone() for t in (res.dq, res.td_abs, res.stats, res.loss)]
        assert td_loss_tensors(q_n, y, weights, out=res) is res
        for got, a, k in zip((res.dq, res.td_abs, res.stats), first, ("dq", "td_abs", "stats")):
            assert np.array_equal(_u32(got), want[k].reshape(-1).view(np.uint32)), (k, weights is not None)
            assert torch.equal(_bits(got), _bits(a))
        assert _u32(res.loss)[0] == want["loss"].view(np.uint32)


def test_td_loss_nan_reaches_td_abs_and_autograd():
    """a NaN in d reaches td_abs whichever agent holds it; TdLoss's backward is grad_output x dq; a stale backward is refused"""
    lay, M = R.LAYOUTS["L69"], 257
    x = R.make_inputs(lay, M)
    for agent, row in ((0, 3), (1, 100), (2, 256)):
        x["q"][agent, row] = np.nan
    want = R.td_loss32(x["q"], x["y"], None)
    res = td_loss_tensors([_t(x["q"][i]) for i in range(3)], _t(x["y"]))
    got = res.td_abs.cpu().numpy()
    assert np.isnan(got[[3, 100, 256]]).all() and np.isnan(got).sum() == 3
    keep = ~np.isnan(got)
    assert np.array_equal(got[keep].view(np.uint32), want["td_abs"][keep].view(np.uint32))
    x = R.make_inputs(lay, M)
    head = TdLoss()
    q_n = [_t(x["q"][i]).requires_grad_() for i in range(3)]
    loss = head(q_n, _t(x["y"]), _t(x["w"]))
    (3.0 * loss).backward()
    want = R.td_loss32(x["q"], x["y"], x["w"])
    assert _u32(loss)[0] == want["loss"].view(np.uint32) and head.last.td_abs.shape == (M,) and loss.stats is head.last.stats
    for i in range(3):
        assert np.array_equal(q_n[i].grad.cpu().numpy(), np.float32(3.0) * want["dq"][i])
    stale = head(q_n, _t(x["y"]))
    head(q_n, _t(x["y"]))
    with pytest.raises(_abi.MpeError, match="TdLoss: backward\\(\\) of a loss whose buffers a later forward"):
        stale.backward()


# ---- THE POLYAK RULE -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.POLYAK_N)
def test_polyak_bit_equal_to_the_restatement(n):
    """every tau, by value and through tau_ptr; two sets in one launch; sentinels around the targets intact; padding stays +0.0"""
    dev, L_ = _dev(), _abi.lib()
    import ctypes as C
    rs = np.random.RandomState(n)
    xs = [rs.standard_normal(k).astype(np.float32) for k in (n, 48)]
    ws = [rs.standard_normal(k).astype(np.float32) for k in (n, 48)]
    for a in xs + ws:
        a[-5:] = 0.0
    tau_dev = torch.zeros(1, dtype=torch.float32, device=dev)
    for tau in R.POLYAK_TAU:
        for by_ptr in (False, True):
            tg = []
            for x in xs:
                t = torch.full((PAD + x.size + PAD,), SENTINEL, dtype=torch.float32, device=dev)
                t[PAD:PAD + x.size] = _t(x)
                tg.append(t)
            on = [_t(w) for w in ws]
            c = _abi.MpePolyak()
            c.n_sets, c.tau, c.tau_ptr = 2, float("nan") if by_ptr else tau, tau_dev.data_ptr() if by_ptr else None
            tau_dev.fill_(float(np.float32(tau)))
            for k in range(2):
                c.set[k].target, c.set[k].online, c.set[k].n = tg[k].data_ptr() + 4 * PAD, on[k].data_ptr(), xs[k].size
            _abi.check(L_.mpe_polyak(C.byref(c), _abi.raw_stream(dev)), "mpe_polyak")
            for k in range(2):
                got = tg[k].cpu().numpy()
                assert np.all(got[:PAD] == SENTINEL) and np.all(got[PAD + xs[k].size:] == SENTINEL)
                assert np.array_equal(got[PAD:PAD + xs[k].size].view(np.uint32), R.polyak32(xs[k], ws[k], tau).view(np.uint32)), (n, tau, by_ptr, k)
                assert np.array_equal(on[k].cpu().numpy().view(np.uint32), ws[k].view(np.uint32))


# ---- THE POLICY ROWS RULE ------------------------------------------------------------------------------------------------------------
def _rows_padded(lay, M, x, unaligned=False):
    """one launch into over-allocated outputs: sentinels in front of row 0 and behind row M -> (the A [M, W] views, the raw tensors)"""
    dev = _dev()
    off = 1 if unaligned else 0
    raw = [torch.full((PAD + off + M * lay.W + PAD,), SENTINEL, dtype=torch.float32, device=dev) for _ in range(lay.A)]
    out = [r[PAD + off:PAD + off + M * lay.W].view(M, lay.W) for r in raw]
    got = policy_rows_tensors(_layout(lay), _t(x["joint"]), [_t(z) for z in x["logits"]], out=out)
    assert all(a is b for a, b in zip(got, out))
    return out, raw


@pytest.mark.parametrize("name", LAYOUT_IDS)
@pytest.mark.parametrize("M", R.ROWS)
def test_policy_rows_outside_inside_and_beyond(M, name):
    """outside the windows joint's bits (a NaN payload included); inside p within LOGP_TOL on log p; no float in front of row 0 or
    behind row M touched, at a 16-byte aligned base and 4 bytes off it, both writing the same bits; two runs bit-equal"""
    lay = R.LAYOUTS[name]
    x = R.make_inputs(lay, M)
    R.check_logits(lay, x)
    runs = []
    for unaligned in (False, True, False):
        out, raw = _rows_padded(lay, M, x, unaligned)
        off = 1 if unaligned else 0
        for r in raw:
            h = r.cpu().numpy()
            assert np.all(h[:PAD + off] == SENTINEL) and np.all(h[PAD + off + M * lay.W:] == SENTINEL)
        runs.append([o.cpu().numpy().copy() for o in out])
    assert R.outside_equal(lay, runs[0], x)
    dev = R.logp_deviation(lay, runs[0], x)
    _note("rows_logp", dev, R.LOGP_TOL)
    assert dev <= R.LOGP_TOL
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", LAYOUT_IDS)
def test_policy_rows_same_bits_at_any_position(name):
    """a row depends on that row alone: M = 65 against rows 960.. of M = 1025"""
    lay = R.LAYOUTS[name]
    x = R.make_inputs(lay, 1025)
    tail = dict(joint=np.ascontiguousarray(x["joint"][960:]), logits=[np.ascontiguousarray(z[960:]) for z in x["logits"]])
    whole, _ = _rows_padded(lay, 1025, x)
    part, _ = _rows_padded(lay, 65, tail)
    for a, b in zip(whole, part):
        assert torch.equal(_bits(a[960:]), _bits(b))


ENVS = {"simple_spread": "L69", "simple_speaker_listener": "L22", "simple_reference": "L72"}


def _mlp(D, n_out, act=nn.ReLU):
    return nn.Sequential(nn.Linear(D, 64), act(), nn.Linear(64, 64), act(), nn.Linear(64, n_out)).cuda()


@pytest.mark.parametrize("scenario", sorted(ENVS))
def test_policy_rows_window_is_the_actor_kernels(scenario):
    """On the actor launch's own logits the windows carry the very bits Actors(mode="softmax").act_rows(joint=True) writes, and the
    env's joint layout is the synthetic one of the sweeps"""
    torch.manual_seed(1)
    env = mpe.make_env(scenario, batch_size=8, seed=3)
    lay = R.LAYOUTS[ENVS[scenario]]
    w = env.world
    n_out = [5 * bool(a.movable) + (int(w.dim_c) if not a.silent else 0) for a in w.agents]
    widths = [int(env._obs_off[i + 1] - env._obs_off[i]) for i in range(len(w.agents))]
    pi = Actors(env, [_mlp(D, n) for D, n in zip(widths, n_out)], mode="softmax", logits=True)
    mine = RowsLayout.of(pi)
    assert (mine.W, mine.dim_c, mine.col, mine.movable, mine.speaks, mine.n) == (lay.W, lay.dim_c, lay.col, lay.movable, lay.speaks, lay.n)
    M = 65
    obs_n = [4.0 * torch.randn((M, D), device=_dev()) for D in widths]
    pi.act_rows(obs_n, joint=True)
    theirs = pi.joint_rows.clone()
    logits_n = [pi.rows.logits[i, :, :n].clone(memory_format=torch.contiguous_format) for i, n in enumerate(n_out)]
    joint = torch.randn((M, mine.W), device=_dev())
    rows = policy_rows_tensors(pi, joint, logits_n)
    for i, (c, n) in enumerate(zip(mine.col, mine.n)):
        assert torch.equal(_bits(rows[i][:, c:c + n]), _bits(theirs[:, c:c + n])), (scenario, i)
        keep = torch.ones(mine.W, dtype=torch.bool, device=_dev())
        keep[c:c + n] = False
        assert torch.equal(_bits(rows[i][:, keep]), _bits(joint[:, keep]))


# ---- THE POLICY ROWS GRADIENT RULE -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg_coef", [0.0, 1e-3])
@pytest.mark.parametrize("name", LAYOUT_IDS)
@pytest.mark.parametrize("M", R.ROWS)
def test_policy_rows_grad_within_the_parity_bound(M, name, reg_coef):
    """ld = n_i (the packed window) and ld = W (a full-row gradient read in place), stats present and absent: dlogits, the stats
    and the loss against the float64 restatement, bound from float32 torch autograd on this GPU; the window's source and the stats
    change no bit of dlogits; no float behind a dlogits block written"""
    lay = R.LAYOUTS[name]
    x = R.make_inputs(lay, M)
    mine = _layout(lay)
    zs, q = [_t(z) for z in x["logits"]], _t(x["q"])
    full = [_t(g) for g in x["G"]]
    inplace = [g[:, c:c + n] for g, c, n in zip(full, lay.col, lay.n)]
    packed = [g.contiguous() for g in inplace]
    ref = R.rows_grad64(lay, x, reg_coef, q=x["q"])
    bound = R.bounds(R.grad_deviations(lay, R.torch_rows(lay, x, reg_coef, torch.float32, device=_dev(), q=x["q"]), ref))
    a = policy_rows_grad_tensors(mine, zs, packed, reg_coef, q=q)
    first, at = a.grads.clone(), 0
    for n in lay.n:      # the floats between the blocks (each starts at a multiple of 4) are not written
        end = at + (M * n + 3) // 4 * 4
        assert not a.grads[at + M * n:end].any()
        at = end
    assert torch.equal(_bits(policy_rows_grad_tensors(mine, zs, packed, reg_coef, q=q, out=a).grads), _bits(first))
    b = policy_rows_grad_tensors(mine, zs, inplace, reg_coef, q=q)
    c = policy_rows_grad_tensors(mine, zs, packed, reg_coef)
    for i in range(lay.A):
        assert torch.equal(_bits(a.dlogits_n[i]), _bits(b.dlogits_n[i])) and torch.equal(_bits(a.dlogits_n[i]), _bits(c.dlogits_n[i]))
    assert torch.equal(_bits(a.stats), _bits(b.stats)) and torch.equal(_bits(a.loss), _bits(b.loss))
    assert not c.stats.any() and not c.loss.any()      # without stats the second launch is skipped: nothing is written
    out = dict(dlogits=[g.cpu().numpy() for g in a.dlogits_n], stats=a.stats.cpu().numpy(), loss=float(a.loss))
    for k, (dev, _) in R.grad_deviations(lay, out, ref).items():
        _note("grad_" + k, dev, bound[k])
        assert dev <= bound[k], (name, M, reg_coef, k, dev, bound[k])
    assert np.all(out["stats"][:, [3, 4, 5, 7]] == 0)


# ---- ActorLoss -------------------------------------------------------------------------------------------------------------------------
def _spread(batch_size=16, act=nn.Tanh):
    torch.manual_seed(11)
    env = mpe.make_env("simple_spread", batch_size=batch_size, seed=2)
    mu = [_mlp(18, 5, act) for _ in range(3)]
    qs = [_mlp(69, 1, act) for _ in range(3)]
    return env, mu, qs


def _example_actor_loss(mu, qs, obs_n, joint, col, reg_coef):
    """examples/maddpg_spread.py's formula, on modules and tensors of any dtype"""
    loss = 0.0
    for i in range(3):
        z = mu[i](obs_n[i])
        j = joint.clone()
        j[:, col[i]:col[i] + 5] = F.softmax(z, dim=1)
        loss = loss - qs[i](j)[:, 0].mean() + reg_coef * (z ** 2).mean()
    return loss


@pytest.mark.parametrize("reg_coef", [0.0, 1e-3])
def test_actor_loss_parameter_gradients_against_float64_autograd(reg_coef):
    """simple_spread, M = 65, Tanh nets: every actor parameter's gradient against float64 autograd of the example's formula, within
    max(4 x float32 torch autograd on this GPU, 2 ulps of the tensor's largest magnitude); the loss likewise"""
    env, mu, qs = _spread()
    M = 65
    obs_n = [torch.randn((M, 18), device=_dev()) for _ in range(3)]
    joint = torch.randn((M, 69), device=_dev())
    pi = Trainable(Actors(env, mu, mode="softmax", logits=True))
    critics = Critics(env, qs)
    head = ActorLoss(pi.net, critics, reg_coef)
    loss = head(pi(obs_n), joint)
    loss.backward()
    assert loss.stats.shape == (3, 8) and head.last.dlogits_n[0].shape == (M, 5)
    col = pi.net.col_move
    grads = {}
    for dtype in (torch.float64, torch.float32):
        m2, q2 = [copy.deepcopy(m).to(dtype) for m in mu], [copy.deepcopy(m).to(dtype) for m in qs]
        for m in m2:
            m.zero_grad()
        l2 = _example_actor_loss(m2, q2, [o.to(dtype) for o in obs_n], joint.to(dtype), col, reg_coef)
        l2.backward()
        grads[dtype] = ([p.grad.double().cpu().numpy() for m in m2 for p in m.parameters()], float(l2))
    ours = [p.grad.double().cpu().numpy() for m in mu for p in m.parameters()]
    (ref, lref), (t32, l32) = grads[torch.float64], grads[torch.float32]
    for k, (a, t, r) in enumerate(zip(ours, t32, ref)):
        dev, bound = float(np.abs(a - r).max()), max(4 * float(np.abs(t - r).max()), 2 * float(np.spacing(np.float32(np.abs(r).max()))))
        _note("actor_loss_param_grad", dev, bound)
        assert dev <= bound, (k, dev, bound)
    dev, bound = abs(float(loss) - lref), max(4 * abs(l32 - lref), 2 * float(np.spacing(np.float32(abs(lref)))))
    _note("actor_loss_loss", dev, bound)
    assert dev <= bound
    assert all(p.grad is None for m in qs for p in m.parameters())      # the critics are a constant of the loss


# ---- prioritized replay ----------------------------------------------------------------------------------------------------------------
def test_prioritized_replay_takes_td_abs_back():
    """sample -> weights(beta) -> TdLoss -> update_td(batch.idx, loss_head.last.td_abs): the stored priorities are (|td| + eps)^alpha
    of the reference, to float32 rounding of the power"""
    env, mu, qs = _spread(batch_size=7, act=nn.ReLU)
    loop = PolicyLoop(env, Actors(env, mu, mode="sample", seed=2), episode_len=5)
    buf = PrioritizedReplayBuffer(env, 8, seed=4, alpha=0.6, eps=1e-6)
    loop.run(12, record=False, replay=buf)
    td = TdTargets(Actors(env, [copy.deepcopy(m) for m in mu], mode="softmax"), Critics(env, [copy.deepcopy(m) for m in qs]))
    batch = buf.sample(130, joint=True, n_step=3, gamma=0.95, episode_len=5)
    y = td.compute(batch)
    q_train, head = Trainable(Critics(env, qs)), TdLoss()
    q = q_train(batch.joint)
    w = batch.weights(0.4).contiguous()
    loss = head(q, y, w)
    loss.backward()
    buf.update_td(batch.idx, head.last.td_abs)
    torch.cuda.synchronize()
    qh, yh, wh = np.stack([t.detach().cpu().numpy() for t in q]), y.cpu().numpy(), w.cpu().numpy()
    want = R.td_loss32(qh, yh, wh)
    assert np.array_equal(_u32(head.last.td_abs), want["td_abs"].view(np.uint32)) and _u32(loss)[0] == want["loss"].view(np.uint32)
    idx = batch.idx.cpu().numpy()
    ref = {}
    for j, t in zip(idx, np.abs(qh.astype(np.float64) - yh).max(axis=0)):      # the largest where several samples name one transition
        ref[int(j)] = max(ref.get(int(j), 0.0), (t + 1e-6) ** 0.6)
    pr = buf.priorities.reshape(-1).cpu().numpy()
    for j, p in ref.items():
        assert abs(pr[j] - p) <= 4 * np.spacing(np.float32(p)), (j, pr[j], p)
    assert all(p.grad is not None for p in q_train.parameters())


# ---- a whole update as ONE graph ---------------------------------------------------------------------------------------------------------
def test_whole_update_as_one_graph():
    """{sample, TdTargets.compute, critic update with DeviceAdam, actor update with DeviceAdam, PolyakTargets.step} captured as ONE
    HIP graph (one stream) and replayed three times: the weights, the moments, the optimiser states and the target buffers are
    bit-equal to the same three updates run eager"""
    env, mu0, qs0 = _spread(batch_size=7, act=nn.ReLU)
    dev, M = _dev(), 130
    loop = PolicyLoop(env, Actors(env, [copy.deepcopy(m) for m in mu0], mode="sample", seed=2), episode_len=5)
    buf = ReplayBuffer(env, 8, seed=4)
    loop.run(12, record=False, replay=buf)
    kw = dict(joint=True, n_step=3, gamma=0.95, episode_len=5)

    def build():
        mu, qs = [copy.deepcopy(m) for m in mu0], [copy.deepcopy(m) for m in qs0]
        pi, Q = Actors(env, mu, mode="softmax", logits=True), Critics(env, qs)
        pi_t, Q_t = Actors(env, [copy.deepcopy(m) for m in mu], mode="softmax"), Critics(env, [copy.deepcopy(m) for m in qs])
        opt_q, opt_mu = DeviceAdam([Q], lr=1e-2), DeviceAdam([pi], lr=1e-2)
        pol = PolyakTargets([(pi, pi_t), (Q, Q_t)], 0.05)
        z_n = [torch.zeros((M, 5), dtype=torch.float32, device=dev) for _ in range(3)]
        dout = torch.full((M,), -1.0 / M, dtype=torch.float32, device=dev)
        return dict(pi=pi, Q=Q, td=TdTargets(pi_t, Q_t), opt_q=opt_q, opt_mu=opt_mu, pol=pol, z_n=z_n, dout=dout, lay=RowsLayout.of(pi), out={})

    def update(s):
        batch = buf.sample(M, draw=100, **kw)
        y = s["td"].compute(batch, t=9)
        o = s["out"]
        # critics
        q = s["Q"].q(batch.joint)
        o["td"] = td_loss_tensors([q[i] for i in range(3)], y, out=o.get("td"))
        s["opt_q"].step([mlp_grad_tensors(s["Q"], batch.joint, [o["td"].dq[i] for i in range(3)])])
        # actors, against the critics just updated
        s["pi"].act_rows(batch.obs_n)
        for i in range(3):
            s["z_n"][i].copy_(s["pi"].rows.logits[i, :, :5])
        o["rows"] = policy_rows_tensors(s["lay"], batch.joint, s["z_n"], out=o.get("rows"))
        qa = s["Q"].q(o["rows"])
        g = mlp_dinput_tensors(s["Q"], o["rows"], [s["dout"]] * 3, cols=[(c, 5) for c in s["lay"].col])
        o["grad"] = policy_rows_grad_tensors(s["lay"], s["z_n"], g, 1e-3, q=qa, out=o.get("grad"))
        s["opt_mu"].step([mlp_grad_tensors(s["pi"], batch.obs_n, o["grad"].dlogits_n)])
        s["pol"].step()

    def state(s):
        return s["opt_q"].weights + s["opt_q"].m + s["opt_q"].v + [s["opt_q"].state] + s["opt_mu"].weights + s["opt_mu"].m + s["opt_mu"].v + \
            [s["opt_mu"].state] + s["pol"].weights

    eager = build()
    start = [t.clone() for t in state(eager)]
    for _ in range(3):
        update(eager)
    torch.cuda.synchronize()
    g_ = build()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        before = [t.clone() for t in state(g_)]
        update(g_)      # the code objects and the buffers outside the capture
        for t, b in zip(state(g_), before):
            t.copy_(b)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            update(g_)
    torch.cuda.current_stream().wait_stream(stream)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert g_["opt_q"].t == 3 == eager["opt_q"].t and g_["opt_mu"].t == 3 == eager["opt_mu"].t
    for a, b in zip(state(g_), state(eager)):
        assert torch.equal(_bits(a), _bits(b))
    assert not any(torch.equal(a, b) for a, b in zip(state(eager)[:1] + state(eager)[-2:], start[:1] + start[-2:]))
    # the target nets read the updated buffers; write_back() brings the modules along
    g_["pol"].write_back()
    fresh = Critics(env, g_["td"].critics.modules)
    rows = torch.randn((9, 69), device=dev)
    assert torch.equal(_bits(fresh.q(rows)), _bits(g_["td"].critics.q(rows)))
    g_["td"].critics.unfreeze()
    with pytest.raises(_abi.MpeError, match=r"PolyakTargets.step: pairs\[1\]'s target net no longer reads the live buffer"):
        g_["pol"].step()


def test_polyak_targets_hard_update_and_refusals():
    env, mu, qs = _spread(batch_size=4, act=nn.ReLU)
    Q, Q_t = Critics(env, qs), Critics(env, [copy.deepcopy(m) for m in qs])
    with pytest.raises(_abi.MpeError, match=r"PolyakTargets: pairs\[0\]'s online net is not attached"):
        PolyakTargets([(Q, Q_t)], 0.01)
    with pytest.raises(_abi.MpeError, match=r"PolyakTargets: pairs\[0\]: the target net holds the online net's module objects"):
        PolyakTargets([(Q, Critics(env, qs))], 0.01)
    opt = DeviceAdam([Q], lr=0.1)
    with pytest.raises(_abi.MpeError, match="PolyakTargets: tau = 1.5"):
        PolyakTargets([(Q, Q_t)], 1.5)
    Q_t.freeze()
    with pytest.raises(_abi.MpeError, match=r"PolyakTargets: pairs\[0\]'s target net is already frozen"):
        PolyakTargets([(Q, Q_t)], 0.01)
    Q_t.unfreeze()
    with pytest.raises(_abi.MpeError, match=r"PolyakTargets: pairs\[0\]: the target's packed layout differs"):
        PolyakTargets([(Q, Critics(env, _mlp(69, 1)))], 0.01)
    tau = torch.tensor([1.0], device=_dev())
    pol = PolyakTargets([(Q, Q_t)], 0.01, tau_tensor=tau)
    opt.weights[0].mul_(1.5)
    assert not torch.equal(pol.weights[0], opt.weights[0])
    pol.step()      # tau_tensor = 1: the online bits
    assert torch.equal(_bits(pol.weights[0]), _bits(opt.weights[0]))
    opt.weights[0].mul_(0.5)
    pol.hard_update()
    assert torch.equal(_bits(pol.weights[0]), _bits(opt.weights[0]))
    before = [p.detach().clone() for m in Q_t.modules for p in m.parameters()]
    pol.release()
    assert Q_t.attached() is None and not any(torch.equal(a, p.detach()) for a, p in zip(before, [p for m in Q_t.modules for p in m.parameters()]))


# ---- the example -----------------------------------------------------------------------------------------------------------------------
def test_example_runs_with_device_update():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "maddpg_spread.py"), "--worlds", "16", "--batch", "64", "--updates", "2",
                        "--device-update"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2
    for l in lines:
        assert np.isfinite(l["critic_loss"]) and np.isfinite(l["actor_loss"])
