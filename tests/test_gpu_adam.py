"""mpe_adam_step and DeviceAdam on the GPU: the host walk's shapes at the ABI, BIT-EQUAL to the float32 restatement of
THE ADAM RULE (tests/_adam_ref.py) with sentinels around every buffer; the skip and lr_ptr; {gradient copy-in, step} as a replayed
HIP graph; the nets' forwards reading the live buffer; a PolicyLoop graph captured ONCE that follows an update; three whole PPO
updates against a float64 chain within the project's bar (4 x float32 torch's deviation on this GPU, floor 2 ulps of the block's
largest magnitude); and the device half of a minibatch update, optimiser included, as one graph.

Whole update, recorded on an MI355X: see profiles/adam_parity.json (tools/adam_parity.py)."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.onpolicy import Minibatches, PpoLoss, Values, gae, ppo_loss_tensors
from multiagent_particle_envs_amd.optim import DeviceAdam
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop
from multiagent_particle_envs_amd.netset import module_views as _module_views
from multiagent_particle_envs_amd.train import MlpGradResult, Trainable, mlp_grad_tensors

import _adam_ref as R
import _mlp_grad_ref as G
import _ppo_loss_ref as P

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
PAD = 64      # sentinel floats (256 bytes: the 16-byte alignment stays) in front of and behind every buffer


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    """bit equality; a NaN equals a NaN (its payload is not part of the rule: only a skipped step's norm and partial hold one)"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and R.same_bits(np.where(nan, 0, a), np.where(nan, 0, b))


def _abi_run(cfg, sets, grads, lr_values=None):
    """len(grads[0]) mpe_adam_step calls on sentinel-padded w, m, v, state and work -> (sets, per step (state, work), intact)"""
    dev, L_ = _dev(), _abi.lib()
    ns = [s["w"].size for s in sets]

    def padded(src, dtype=torch.float32):
        t = torch.full((PAD + src.size + PAD,), SENTINEL, dtype=dtype, device=dev)
        t[PAD:PAD + src.size] = torch.tensor(src, device=dev)
        return t
    c = _abi.MpeAdam()
    c.lr, c.beta1, c.beta2, c.eps, c.weight_decay, c.max_grad_norm = (cfg[k] for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "max_grad_norm"))
    c.n_sets = len(sets)
    lr_dev = torch.zeros(1, dtype=torch.float32, device=dev)
    c.lr_ptr = lr_dev.data_ptr() if lr_values is not None else None
    bufs, gbufs = [], []
    for k, s in enumerate(sets):
        b = {name: padded(s[name]) for name in ("w", "m", "v")}
        g = torch.zeros(ns[k], dtype=torch.float32, device=dev)
        bufs.append(b)
        gbufs.append(g)
        q = c.set[k]
        q.weights, q.m, q.v, q.grad, q.n = (b["w"].data_ptr() + 4 * PAD, b["m"].data_ptr() + 4 * PAD, b["v"].data_ptr() + 4 * PAD, g.data_ptr(), ns[k])
        assert all(p % 16 == 0 for p in (q.weights, q.m, q.v, q.grad))
    P_ = int(L_.mpe_adam_work(C.byref(c)))
    assert P_ == sum(R.tiles_of(ns))
    state = padded(R.fresh_state(), torch.float64)
    work = torch.full((PAD + P_ + PAD,), SENTINEL, dtype=torch.float64, device=dev)
    log = []
    for t in range(len(grads[0])):
        for g, gs in zip(gbufs, grads):
            g.copy_(torch.tensor(gs[t], device=dev))
        if lr_values is not None:
            lr_dev.fill_(float(np.float32(lr_values[t])))
        _abi.check(L_.mpe_adam_step(C.byref(c), state.data_ptr() + 8 * PAD, work.data_ptr() + 8 * PAD, _abi.raw_stream(dev)), "mpe_adam_step")
        log.append((state[PAD:PAD + R.STATE_DOUBLES].cpu().numpy(), work[PAD:PAD + P_].cpu().numpy()))
    torch.cuda.synchronize()
    intact, out = True, []
    for b, n in zip(bufs, ns):
        d = {}
        for name, t in b.items():
            x = t.cpu().numpy()
            intact = intact and bool(np.all(x[:PAD] == SENTINEL) and np.all(x[PAD + n:] == SENTINEL))
            d[name] = x[PAD:PAD + n].copy()
        out.append(d)
    for t, n in ((state, R.STATE_DOUBLES), (work, P_)):
        x = t.cpu().numpy()
        intact = intact and bool(np.all(x[:PAD] == SENTINEL) and np.all(x[PAD + n:] == SENTINEL))
    return out, log, intact


def _equals_ref(cfg, sets, grads, lr_values=None):
    want, wlog = R.run_ref(cfg, sets, grads, lr_values=lr_values)
    got, glog, intact = _abi_run(cfg, sets, grads, lr_values)
    assert intact
    ns = [s["w"].size for s in sets]
    for t, ((gs, gw), (ws, ww)) in enumerate(zip(glog, wlog)):
        assert _same(gs, ws), ("state", ns, t, gs, ws)
        assert _same(gw, ww), ("work", ns, t)
    for k, (g, w) in enumerate(zip(got, want)):
        for name in ("w", "m", "v"):
            assert R.same_bits(g[name], w[name]), (name, ns, k, int((g[name] != w[name]).sum()))
    return got, glog


BOTH = dict(R.CFG, lr=1e-2, weight_decay=0.01, max_grad_norm=0.5)


@pytest.mark.parametrize("ns", R.SHAPES, ids=R.SHAPE_IDS)
def test_abi_bit_equal_to_the_restatement(ns):
    """three steps per shape, plain Adam and AdamW with an active clip; gradient magnitudes 1e-22 .. 1e3 (g * g denormal in places:
    a flush in the kernel would show here, and here alone); sentinels intact; padding +0.0f; a second run gives the same bits"""
    sets, grads = R.make_sets(ns, seed=len(ns) * 1000 + ns[0])
    _equals_ref(R.CFG, sets, grads)
    got, log = _equals_ref(BOTH, sets, grads)
    assert log[-1][0][3] == R.STEPS and log[-1][0][8] == 0 and 0 < log[-1][0][7] < 1
    for s, g in zip(sets, got):
        for name in ("w", "m", "v"):
            assert not g[name][s["pad"]].view(np.uint32).any(), (name, ns)
    again, alog, intact = _abi_run(BOTH, sets, grads)
    assert intact and all(R.same_bits(a[k], b[k]) for a, b in zip(again, got) for k in ("w", "m", "v"))
    assert all(R.same_bits(a[0], b[0]) and R.same_bits(a[1], b[1]) for a, b in zip(alog, log))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_nonfinite_gradient_skips_the_step(bad):
    """(the NaN is DATA: a skipped step stores nothing to w, m or v, and nothing faults)"""
    sets, grads = R.make_sets((6416, 16, 20000), seed=11)
    poisoned = grads[2][1].copy()
    poisoned[17000] = bad
    grads[2][1] = poisoned
    _, log = _equals_ref(dict(R.CFG, max_grad_norm=0.5), sets, grads)
    assert [int(s[3]) for s, _ in log] == [1, 1, 2] and [int(s[8]) for s, _ in log] == [0, 1, 1]
    assert log[1][0][7] == 0.0 and not np.isfinite(log[1][0][6])


def test_lr_ptr_changed_between_steps_is_followed():
    sets, grads = R.make_sets((1040,), seed=3)
    cfg = dict(R.CFG, lr=float("nan"), weight_decay=0.01)
    got, _ = _equals_ref(cfg, sets, grads, lr_values=[1e-2, 0.0, 3e-3])
    fixed, _ = R.run_ref(dict(cfg, lr=1e-2), sets, grads)
    assert not R.same_bits(got[0]["w"], fixed[0]["w"])


# ---- the host layer ----------------------------------------------------------------------------------------------------------------
def _mlp(n_out, hidden=(64, 64), act=nn.Tanh):
    mods, k = [], 18
    for h in hidden:
        mods += [nn.Linear(k, h), act()]
        k = h
    return nn.Sequential(*(mods + [nn.Linear(k, n_out)])).cuda()


def _mixed(n_out):
    """18-33-n Tanh, 18-64-64-n ReLU, 18-64-64-n Tanh"""
    return [_mlp(n_out, (33,)), _mlp(n_out, (64, 64), nn.ReLU), _mlp(n_out)]


def _fake_grad(net, seed, scale=1.0):
    """an MlpGradResult whose packed gradient is N(0, scale) on the modules' entries and +0.0 on the padding"""
    g = MlpGradResult()
    n = int(net.pack(_dev())[0].numel())
    mask = torch.zeros(n, dtype=torch.float32, device=_dev())
    for views in _module_views(net, mask)[0]:
        for w, b in views:
            w.fill_(1.0)
            b.fill_(1.0)
    gen = torch.Generator(device="cpu").manual_seed(seed)
    g.packed = (torch.randn(n, generator=gen) * scale).to(_dev()) * mask
    g.M, g.work, g.modules, g.shape = 0, None, None, None
    return g


def test_forwards_read_the_live_buffer():
    """after step(), act() / v() rows are bit-equal to those of FRESH sets built over the modules after write_back(); a shared
    sampling set follows; the modules' own parameters do not move before write_back(); release() thaws"""
    torch.manual_seed(3)
    env = mpe.make_env("simple_spread", batch_size=64, seed=5)
    pm, vm = _mixed(5), _mixed(1)
    pi, V = Actors(env, pm, mode="greedy", logits=True), Values(env, vm)
    behaviour = Actors(env, pm, mode="sample", seed=9, logp=True)
    before = [p.detach().clone() for m in pm + vm for p in m.parameters()]
    opt = DeviceAdam([pi, V], lr=0.05, weight_decay=0.01, max_grad_norm=0.5)
    assert opt.share(pi, behaviour) is behaviour and pi._frozen[0] is opt.weights[0] and behaviour._frozen[0] is opt.weights[0]
    obs_n = env.reset()
    stale = [t.clone() for t in (pi.act(obs_n, 3), pi.logits, V.v(obs_n))]
    opt.step([_fake_grad(pi, 1), _fake_grad(V, 2)])
    live = [t.clone() for t in (pi.act(obs_n, 3), pi.logits, V.v(obs_n), behaviour.act(obs_n, 3), behaviour.logp)]
    assert not torch.equal(live[1], stale[1]) and not torch.equal(live[2], stale[2])
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, [p for m in pm + vm for p in m.parameters()]))
    assert (opt.t, opt.skipped) == (1, 0) and 0 < opt.clip_coef < 1 and opt.grad_norm > 0.5
    opt.write_back()
    assert not any(torch.equal(a, p.detach()) for a, p in zip(before, [p for m in pm + vm for p in m.parameters()]))
    pi2, V2 = Actors(env, pm, mode="greedy", logits=True), Values(env, vm)
    b2 = Actors(env, pm, mode="sample", seed=9, logp=True)
    fresh = [t.clone() for t in (pi2.act(obs_n, 3), pi2.logits, V2.v(obs_n), b2.act(obs_n, 3), b2.logp)]
    for a, b in zip(live, fresh):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(pi2.pack(_dev())[0]), _bits(opt.weights[0]))      # the padding of the live buffer is still +0.0f
    sd = opt.state_dict()
    opt.step([_fake_grad(pi, 3), _fake_grad(V, 4)])
    moved = opt.weights[0].clone()
    opt.load_state_dict(sd)
    assert opt.t == 1 and torch.equal(_bits(opt.weights[0]), _bits(sd["weights"][0])) and not torch.equal(moved, opt.weights[0])
    opt.release()
    assert pi._frozen is None and V._frozen is None and behaviour._frozen is None


def test_graph_of_copy_in_and_step_replayed_three_times():
    """{fresh gradient copy-in, opt.step} captured once: three replays equal three eager steps bit for bit; t advances on the device"""
    torch.manual_seed(4)
    env = mpe.make_env("simple_spread", batch_size=64, seed=5)
    nets = lambda: (Actors(env, pm, mode="greedy", logits=True), Values(env, vm))      # noqa: E731
    pm, vm = _mixed(5), _mixed(1)
    srcs = [[_fake_grad(n, 10 * t + k).packed for k, n in enumerate(nets())] for t in range(3)]
    kw = dict(lr=0.01, weight_decay=0.01, max_grad_norm=0.5)
    eager = DeviceAdam(list(nets()), **kw)
    ge = [_fake_grad(n, 0) for n in eager.nets]
    for t in range(3):
        for g, s in zip(ge, srcs[t]):
            g.packed.copy_(s)
        eager.step(ge)
    opt = DeviceAdam(list(nets()), **kw)
    gg = [_fake_grad(n, 0) for n in opt.nets]
    feed = [torch.zeros_like(s) for s in srcs[0]]
    s_ = torch.cuda.Stream()
    s_.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s_):
        start = opt.state_dict()
        opt.step(gg)      # the code objects outside the capture
        opt.load_state_dict(start)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s_):
            for g, f in zip(gg, feed):
                g.packed.copy_(f)
            opt.step(gg)
    torch.cuda.current_stream().wait_stream(s_)
    for t in range(3):
        for f, s in zip(feed, srcs[t]):
            f.copy_(s)
        graph.replay()
    torch.cuda.synchronize()
    assert opt.t == 3 == eager.t
    for a, b in zip(opt.weights + opt.m + opt.v + [opt.state], eager.weights + eager.m + eager.v + [eager.state]):
        assert torch.equal(_bits(a), _bits(b))


def test_a_captured_policy_loop_follows_an_update():
    """PolicyLoop.capture(5) taken ONCE; its replay behind an opt.step equals an eager 5-step loop over fresh Actors built from the
    written-back modules, from the same start state and step count"""
    torch.manual_seed(5)
    pm = _mixed(5)
    env = mpe.make_env("simple_spread", batch_size=64, seed=5)
    pi = Actors(env, pm, mode="sample", seed=9)
    opt = DeviceAdam([pi], lr=0.05)
    loop = PolicyLoop(env, pi, episode_len=5)
    graph = loop.capture(5)
    assert pi._frozen[0] is opt.weights[0]      # capture() did not freeze a snapshot over the live buffer
    graph.replay()
    torch.cuda.synchronize()
    first = env.world.pos.clone()
    opt.step([_fake_grad(pi, 7)])
    loop.t = 0
    graph.replay()
    torch.cuda.synchronize()
    second = env.world.pos.clone()
    assert not torch.equal(first, second)
    opt.write_back()
    env2 = mpe.make_env("simple_spread", batch_size=64, seed=5)
    loop2 = PolicyLoop(env2, Actors(env2, pm, mode="sample", seed=9), episode_len=5)
    loop2.run(5, record=False)
    torch.cuda.synchronize()
    assert loop2.t == loop.t == 5 and torch.equal(_bits(env2.world.pos), _bits(second))
    assert torch.equal(_bits(env2.world._vel_all), _bits(env.world._vel_all))


# ---- the whole update --------------------------------------------------------------------------------------------------------------
KW = dict(clip=0.2, value_clip=0.2, vf_coef=0.5, ent_coef=0.01)
ADAM = dict(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.5)
NET = G.Net(18, (64, 64), 5, "tanh", True)


@pytest.fixture(scope="module")
def spread():
    """simple_spread, B = 64, T = 5: a recorded trajectory, its returns and minibatches of all 320 rows"""
    torch.manual_seed(7)
    env = mpe.make_env("simple_spread", batch_size=64, seed=2)
    pm, vm = [_mlp(5) for _ in range(3)], [_mlp(1) for _ in range(3)]
    actors, values = Actors(env, pm, mode="sample", seed=4, logp=True, logits=True), Values(env, vm)
    traj = PolicyLoop(env, actors, episode_len=5).run(5, values=values)
    g = gae(traj, 0.95, 0.9)
    counter = torch.zeros(1, dtype=torch.int64, device=g.adv.device)
    return dict(env=env, pm=pm, vm=vm, traj=traj, g=g, counter=counter)


def _params64(mods):
    """per module [(W [in, out], b)] float64 NumPy, the layout of tests/_mlp_grad_ref.py"""
    return [[(l.weight.detach().double().cpu().numpy().T.copy(), l.bias.detach().double().cpu().numpy().copy()) for l in m if isinstance(l, nn.Linear)]
            for m in mods]


def _out64(net, params, x):
    hs, _ = G.forward64(net, params, x)
    return hs[-1] @ params[-1][0] + params[-1][1]


def _chain64(spread, batches):
    """the float64 chain: the float64 restatements of the loss, the gradient and THE ADAM RULE (imported, not edited)"""
    case = P.Case("spread_B64_T5", [P.MOVER] * 3, 0, 320, 0, **KW)
    vnet = NET._replace(n_out=1)
    pp, vp = _params64(spread["pm"]), _params64(spread["vm"])
    flat = lambda ps: np.concatenate([a.reshape(-1) for p in ps for Wb in p for a in Wb])      # noqa: E731
    sets = [dict(w=flat(pp), m=None, v=None), dict(w=flat(vp), m=None, v=None)]
    for s in sets:
        s["m"], s["v"] = np.zeros_like(s["w"]), np.zeros_like(s["w"])

    def views(s):
        out, at = [], 0
        for _ in range(3):
            p = []
            for k_in, k_out in ((18, 64), (64, 64), (64, s)):
                W = at, at + k_in * k_out
                p.append((W, (W[1], W[1] + k_out), (k_in, k_out)))
                at = W[1] + k_out
            out.append(p)
        return out
    state = R.fresh_state()
    cfg = dict(R.CFG, lr=ADAM["lr"], max_grad_norm=ADAM["max_grad_norm"])
    for b in batches:
        obs = [o.astype(np.float64) for o in b["obs"]]
        cur = []
        for s, n_out in zip(sets, (5, 1)):
            cur.append([[(s["w"][W[0]:W[1]].reshape(shape), s["w"][bb[0]:bb[1]]) for W, bb, shape in p] for p in views(n_out)])
        x = dict(logits=[_out64(NET, cur[0][i], obs[i]) for i in range(3)], values=[_out64(vnet, cur[1][i], obs[i])[:, 0] for i in range(3)],
                 act=b["act"], utter=None, adv=b["adv"], ret=b["ret"], val_old=b["val"], logp_old=b["logp"])
        r = P.rule64(case, x)
        for s, net, ps, douts in ((sets[0], NET, cur[0], r["dlogits"]), (sets[1], vnet, cur[1], [r["dvalues"][i][:, None] for i in range(3)])):
            g = [G.agent_grads64(net, ps[i], obs[i], douts[i]) for i in range(3)]
            s["g"] = np.concatenate([a.reshape(-1) for gi in g for dWb in gi for a in dWb])
        R.step(cfg, sets, state, dtype=np.float64)
    return [[s["w"][lo:hi] for p in views(n_out) for W, bb, _ in p for lo, hi in (W, bb)] for s, n_out in zip(sets, (5, 1))]


def _torch32(spread, batches):
    """the float32 torch path on this GPU: torch modules, autograd, clip_grad_norm_ and torch.optim.Adam"""
    case = P.Case("spread_B64_T5", [P.MOVER] * 3, 0, 320, 0, **KW)
    pm, vm = [copy.deepcopy(m) for m in spread["pm"]], [copy.deepcopy(m) for m in spread["vm"]]
    params = [p for m in pm + vm for p in m.parameters()]
    opt = torch.optim.Adam(params, lr=ADAM["lr"], betas=ADAM["betas"], eps=ADAM["eps"])
    for b in batches:
        t = {k: torch.tensor(v, device=_dev()) for k, v in b.items() if k != "obs"}
        obs = [torch.tensor(o, device=_dev()) for o in b["obs"]]
        loss = P.torch_loss_terms(case, [pm[i](obs[i]) for i in range(3)], [vm[i](obs[i]) for i in range(3)], t["act"], None, t["logp"], t["adv"],
                                  t["ret"], t["val"])[0]
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, ADAM["max_grad_norm"])
        opt.step()
    return pm, vm


def _tensors(mods):
    """per module per Linear: W as [in, out] flattened, then b -- the order of _chain64's result"""
    return [a for m in mods for l in m if isinstance(l, nn.Linear)
            for a in (l.weight.detach().double().cpu().numpy().T.reshape(-1), l.bias.detach().double().cpu().numpy())]


def test_three_whole_updates_against_the_float64_chain(spread):
    """Minibatches -> Trainable -> PpoLoss -> DeviceAdam (clip 0.5), three updates on three epochs' minibatches of one trajectory.
    Every parameter tensor: |ours - float64 chain| <= max(4 x |float32 torch on this GPU - float64 chain|, 2 ulps of the tensor's
    largest magnitude)."""
    env = spread["env"]
    pm, vm = [copy.deepcopy(m) for m in spread["pm"]], [copy.deepcopy(m) for m in spread["vm"]]
    tp, tv = Trainable(Actors(env, pm, mode="sample", seed=4, logits=True)), Trainable(Values(env, vm))
    opt = DeviceAdam([tp, tv], **ADAM)
    head = PpoLoss(env, **KW)
    mb = Minibatches(spread["traj"], spread["g"], 320, seed=6)
    batches = []
    for u in range(3):
        b = mb.batch(u, 0)
        batches.append(dict(obs=[o.cpu().numpy().copy() for o in b.obs_n], act=b.act.cpu().numpy().copy(), logp=b.logp.cpu().numpy().copy(),
                            adv=b.adv.cpu().numpy().copy(), ret=b.ret.cpu().numpy().copy(), val=b.val.cpu().numpy().copy()))
        head(tp(b.obs_n), tv(b.obs_n), b).backward()
        assert tp.last_grad is not None and tv.last_grad is not None
        opt.step()
        assert tp.last_grad is None and tv.last_grad is None
    with pytest.raises(_abi.MpeError, match=r"DeviceAdam.step: nets\[0\].last_grad is None"):
        opt.step()
    assert (opt.t, opt.skipped) == (3, 0)
    assert all(p.grad is not None for p in tp.parameters())      # (the autograd path is untouched: .grad is still filled)
    opt.write_back()
    ref = _chain64(spread, batches)
    t32 = _torch32(spread, batches)
    rows, worst = [], 0.0
    for name, ours, theirs, want in (("actors", pm, t32[0], ref[0]), ("values", vm, t32[1], ref[1])):
        for k, (a, t, r) in enumerate(zip(_tensors(ours), _tensors(theirs), want)):
            dev, dt = float(np.abs(a - r).max()), float(np.abs(t - r).max())
            bound = max(4 * dt, 2 * float(np.spacing(np.float32(np.abs(r).max()))))
            rows.append(dict(block="%s_module%d_layer%d_%s" % (name, k // 6, (k % 6) // 2, "Wb"[k % 2]), kernel=dev, torch_float32=dt, bound=bound,
                             largest_magnitude=float(np.abs(r).max())))
            worst = max(worst, dev / bound)
            print("%s: ours %.3e torch %.3e bound %.3e" % (rows[-1]["block"], dev, dt, bound))
    if os.environ.get("MPE_ADAM_PARITY_OUT"):      # tools/adam_parity.py
        with open(os.environ["MPE_ADAM_PARITY_OUT"], "w") as f:
            f.write(json.dumps({"device": torch.cuda.get_device_name(0), "updates": 3, "largest_fraction_of_bound": worst, "blocks": rows}) + "\n")
    for r in rows:
        assert r["kernel"] <= r["bound"], r


def test_device_half_of_an_update_as_one_graph(spread):
    """{batch, both forwards, ppo_loss_tensors, both mlp_grad_tensors, opt.step} captured as ONE HIP graph; two replays (the epoch
    counter bumped between them) are bit-equal to two eager updates"""
    env, counter, dev = spread["env"], spread["counter"], _dev()
    M = 96

    def build():
        pm, vm = [copy.deepcopy(m) for m in spread["pm"]], [copy.deepcopy(m) for m in spread["vm"]]
        pi, V = Actors(env, pm, mode="sample", seed=4, logits=True), Values(env, vm)
        return pi, V, DeviceAdam([pi, V], **ADAM), Minibatches(spread["traj"], spread["g"], M, seed=6, epoch_counter=counter)

    def update(pi, V, opt, mb, z_n, out=None):
        b = mb.batch(3, 1)
        pi.act_rows(b.obs_n)
        for i in range(3):
            z_n[i].copy_(pi.rows.logits[i, :, :5])
        v = V.v(b.obs_n)
        res = ppo_loss_tensors(z_n, [v[i] for i in range(3)], b.act, b.utter, b.logp, b.adv, b.ret, b.val, movable=[True] * 3,
                               speaks=[False] * 3, dim_c=0, out=out, **KW)
        opt.step([mlp_grad_tensors(pi, b.obs_n, res.dlogits_n), mlp_grad_tensors(V, b.obs_n, [res.dvalues[i] for i in range(3)])])
        return res
    counter.zero_()
    try:
        pi, V, eager, mb = build()
        z_n = [torch.zeros((M, 5), dtype=torch.float32, device=dev) for _ in range(3)]
        for _ in range(2):
            update(pi, V, eager, mb, z_n)
            counter.add_(1)
        counter.zero_()
        pi, V, opt, mb = build()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            start = opt.state_dict()
            res = update(pi, V, opt, mb, z_n)      # the code objects and the buffers outside the capture
            opt.load_state_dict(start)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s):
                assert update(pi, V, opt, mb, z_n, res) is res
        torch.cuda.current_stream().wait_stream(s)
        for _ in range(2):
            graph.replay()
            counter.add_(1)
        torch.cuda.synchronize()
        assert opt.t == 2 == eager.t
        for a, b in zip(opt.weights + opt.m + opt.v + [opt.state], eager.weights + eager.m + eager.v + [eager.state]):
            assert torch.equal(_bits(a), _bits(b))
        assert not torch.equal(opt.weights[0], start["weights"][0])
    finally:
        counter.zero_()
