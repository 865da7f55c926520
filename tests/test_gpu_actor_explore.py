"""mpe_actor_act_explore on the GPU: the epsilon-greedy actor launch against THE EXPLORATION RULE restated on the
SAMPLE draws' own bits (tests/_q_loss_ref.py on tests/_actor_ref.py's Philox block).  Moves, utterances and ids are bit-equal to the
rule applied to the greedy choice of the same launch's logits; logp is bit-equal where it can be restated without a transcendental
(an agent with one head: the greedy launch's logp is minus the head's log-sum-exp, exactly) and within the project's 2e-6 of the
float64 log-softmax of the launch's own logits where an agent has two heads.  epsilon = 0 is mpe_actor_act in every output bit,
epsilon = 1 explores everywhere, world_offset and step move the draws as SAMPLE's do, and a closed loop with epsilon > 0 pushes the
rows that were played."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

import multiagent_particle_envs_amd as mpe
from multiagent_particle_envs_amd import _abi
from multiagent_particle_envs_amd.policy import Actors, PolicyLoop
from multiagent_particle_envs_amd.replay import ReplayBuffer

import _actor_ref as AR
import _q_loss_ref as R

pytestmark = pytest.mark.gpu
MOVE = 5
# (D, movable, speaks) per agent and dim_c: simple_spread N = 3, simple_speaker_listener, simple_reference
LAYOUTS = {
    "spread3": ([(18, 1, 0)] * 3, 0),
    "speaker_listener": ([(3, 0, 1), (11, 1, 0)], 3),
    "reference": ([(21, 1, 1)] * 2, 10),
}
BATCHES = (1, 63, 64, 65, 255, 256, 257)
EPSILONS = (0.0, 2.0 ** -16, 0.5, 1.0)
SEED = 0x1234567887654321


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _case(name, B):
    specs, dim_c = LAYOUTS[name]
    rs = np.random.RandomState(50 + B)
    agents, obs = [], []
    for D, mv, sp in specs:
        agents.append({"layers": AR.make_layers(rs, D, (64, 64), MOVE * mv + dim_c * sp, wscale=3.0), "act": AR.TANH, "movable": mv, "speaks": sp})
        obs.append(rs.uniform(-1, 1, (B, D)).astype(np.float32))
    return agents, obs, dim_c


class _Set(object):
    """a hand-built GREEDY set and its observations on the device"""

    def __init__(self, agents, obs, dim_c):
        dev = _dev()
        self.agents, self.dim_c, self.A, self.B = agents, dim_c, len(agents), int(obs[0].shape[0])
        self.aset, blob = AR.make_set(agents, dim_c, "greedy", SEED)
        self.wts = torch.as_tensor(blob, device=dev)
        self.aset.weights = self.wts.data_ptr()
        self.obs = [torch.cat([torch.as_tensor(o).reshape(-1), torch.zeros(64)]).to(dev) for o in obs]

    def run(self, epsilon, t, world_offset, B=None, row0=0):
        """epsilon None: mpe_actor_act.  Rows row0 .. row0 + B of the observations.  -> dict of NumPy outputs"""
        dev, A, dc = _dev(), self.A, self.dim_c
        B = self.B if B is None else B
        ptrs = (C.c_void_p * A)(*[o.data_ptr() + 4 * row0 * int(a["layers"][0][0].shape[1]) for o, a in zip(self.obs, self.agents)])
        o = dict(moves=torch.full((A, B, MOVE), -7.0, device=dev), utter=torch.full((A, B, dc), -7.0, device=dev) if dc else None,
                 ids=torch.full((2, A, B), -7, dtype=torch.int32, device=dev), logp=torch.full((A, B), -7.0, device=dev),
                 logits=torch.full((A, B, 16), -7.0, device=dev))
        out = [o[k].data_ptr() if o[k] is not None else None for k in ("moves", "utter", "ids", "logp", "logits")]
        L_ = _abi.lib()
        if epsilon is None:
            _abi.check(L_.mpe_actor_act(C.byref(self.aset), ptrs, B, int(t), int(world_offset), *out, _abi.raw_stream(dev)), "mpe_actor_act")
        else:
            _abi.check(L_.mpe_actor_act_explore(C.byref(self.aset), ptrs, B, int(t), int(world_offset), float(epsilon), *out,
                                                _abi.raw_stream(dev)), "mpe_actor_act_explore")
        torch.cuda.synchronize()
        return {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}


def _heads(agent, dim_c):
    """[(head number, first logit, logits, the stream of its draws)] of an agent"""
    out = []
    if agent["movable"]:
        out.append((0, 0, MOVE, AR.STREAM_POLICY))
    if agent["speaks"]:
        out.append((1, MOVE if agent["movable"] else 0, dim_c, AR.STREAM_POLICY_COMM))
    return out


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check_against_rule(s, greedy, got, epsilon, t, world_offset, tag):
    """`got` (an exploring launch) against the rule applied to `greedy` (mpe_actor_act on the same rows) -> the explored share"""
    E, B = R.explore_E(epsilon), greedy["moves"].shape[1]
    assert _same(got["logits"], greedy["logits"]), tag
    explored_n = total = 0
    for i, agent in enumerate(s.agents):
        heads = _heads(agent, s.dim_c)
        z = greedy["logits"][i]
        lp32, lp64 = None, np.zeros(B)
        for h, k0, n, stream in heads:
            bits = R.head_bits(stream, SEED, B, t, i, world_offset)
            chosen, explored = R.explore_pick(bits, n, E, greedy["ids"][h, i])
            explored_n, total = explored_n + int(explored.sum()), total + B
            if E == 65536:
                assert explored.all() and np.array_equal(chosen, ((bits & 0xFFFF).astype(np.int64) * n) >> 16)
            assert np.array_equal(got["ids"][h, i], chosen), tag + (i, h, "ids")
            rows = np.zeros((B, n), np.float32)
            rows[np.arange(B), chosen] = 1.0
            assert _same((got["utter"] if h else got["moves"])[i], rows), tag + (i, h, "rows")
            zh = z[:, k0:k0 + n]
            zm = zh.max(axis=1)
            if len(heads) == 1:      # logp = (z[chosen] - zm) - L, and the greedy launch's logp is 0 - L: L = -logp exactly
                lp32 = (zh[np.arange(B), chosen] - zm) - (-greedy["logp"][i])
            s64 = zh.astype(np.float64) - zm[:, None]
            lp64 += s64[np.arange(B), chosen] - np.log(np.exp(s64).sum(axis=1))
        for h in (0, 1):
            if h not in [x[0] for x in heads]:
                assert (got["ids"][h, i] == -1).all() and ((got["utter"] if h else got["moves"]) is None or
                                                            not (got["utter"] if h else got["moves"])[i].any()), tag + (i, h)
        if lp32 is not None:
            assert _same(got["logp"][i], lp32.astype(np.float32)), tag + (i, "logp bits")
        bar = 2e-6 + 4 * np.spacing(np.float32(np.abs(lp64).max()))      # the project's bar on the exp / log intrinsics, and the adds' rounding
        assert np.abs(got["logp"][i] - lp64).max() <= bar, tag + (i, "logp", float(np.abs(got["logp"][i] - lp64).max()))
    return explored_n / total


@pytest.mark.parametrize("name", sorted(LAYOUTS))
@pytest.mark.parametrize("B", BATCHES)
def test_explore_bit_equal_to_the_rule(B, name):
    """every epsilon at every batch edge: epsilon = 0 is mpe_actor_act bit for bit; the others are the rule on the draws of (seed,
    world_offset + b, step, agent); epsilon = 1 chooses ((b & 0xffff) * n) >> 16 everywhere"""
    s = _Set(*_case(name, B))
    t, wo = 3, 777
    greedy = s.run(None, t, wo)
    for eps in EPSILONS:
        got = s.run(eps, t, wo)
        if eps == 0.0:
            for k, v in greedy.items():
                assert v is None or _same(got[k], v), (name, B, k)
        share = _check_against_rule(s, greedy, got, eps, t, wo, (name, B, eps))
        assert share == (0.0 if eps == 0.0 else 1.0 if eps == 1.0 else share)
    if B >= 255:      # (at 0.5 the explored share of >= 510 head draws lies within 5 binomial sigma)
        share = _check_against_rule(s, greedy, s.run(0.5, t, wo), 0.5, t, wo, (name, B, 0.5))
        n = B * sum(len(_heads(a, s.dim_c)) for a in s.agents)
        assert abs(share - 0.5) <= 5 * np.sqrt(0.25 / n)


def test_world_offset_and_step_move_the_draws_as_samples_do():
    """world = world_offset + b: rows 65.. of a launch at offset 1000 are a launch of those rows at offset 1065; a step beyond 2^32
    and a world beyond 2^32 reach the counter's high words; another step draws other bits"""
    s = _Set(*_case("reference", 130))
    for t, wo in ((3, 1000), (2 ** 32 + 5, 2 ** 33 + 1000)):
        whole, part = s.run(0.5, t, wo), s.run(0.5, t, wo + 65, B=65, row0=65)
        for k in ("moves", "utter", "logp", "logits"):
            assert _same(whole[k][:, 65:], part[k]), (t, k)
        assert np.array_equal(whole["ids"][:, :, 65:], part["ids"])
        greedy = s.run(None, t, wo)
        _check_against_rule(s, greedy, whole, 0.5, t, wo, ("offset", t))
    a, b = s.run(0.5, 3, 1000), s.run(0.5, 4, 1000)
    assert not np.array_equal(a["ids"], b["ids"]) and _same(a["logits"], b["logits"])


def _mlp(D, n_out):
    return nn.Sequential(nn.Linear(D, 64), nn.Tanh(), nn.Linear(64, n_out)).cuda()


def test_actors_epsilon_and_the_loop_push_the_rows_played():
    """Actors(mode="greedy", epsilon=...): epsilon = 0 is the greedy act() bit for bit; a schedule is an assignment; another mode
    refuses it; act_rows stays greedy; and PolicyLoop.run(replay=buf) with epsilon > 0 pushes the very rows the rule plays on the
    observation each step was decided on"""
    torch.manual_seed(5)
    env = mpe.make_env("simple_spread", batch_size=70, seed=3)
    nets = [_mlp(18, 5) for _ in range(3)]
    pi = Actors(env, nets, mode="greedy", seed=9, ids=True, epsilon=0.0)
    plain = Actors(env, nets, mode="greedy", seed=9, ids=True)
    obs_n = [torch.randn((70, 18), device=_dev()) for _ in range(3)]
    m0 = plain.act(obs_n, 4).clone()
    assert torch.equal(pi.act(obs_n, 4).view(torch.int32), m0.view(torch.int32))
    pi.epsilon = 1.0
    m1, ids1 = pi.act(obs_n, 4).clone(), pi.ids.clone()
    assert not torch.equal(m1, m0)
    for i in range(3):
        bits = R.head_bits(AR.STREAM_POLICY, 9, 70, 4, i, int(env.world.world_offset))
        assert np.array_equal(ids1[0, i].cpu().numpy(), ((bits & 0xFFFF).astype(np.int64) * 5) >> 16)
    assert torch.equal(pi.act_rows(obs_n, 4).view(torch.int32), m0.view(torch.int32))      # targets are greedy
    with pytest.raises(_abi.MpeError, match="Actors: epsilon = 0.3 with mode 'sample'"):
        Actors(env, nets, mode="sample", epsilon=0.3)
    pi.epsilon = 1.5
    with pytest.raises(_abi.MpeError, match=r"Actors.act: epsilon = 1.5 \(a number in \[0, 1\]\)"):
        pi.act(obs_n, 4)
    # the closed loop: an epsilon schedule of one assignment per run, 3 + 3 steps of an episode of 6
    pi.epsilon = 0.5
    loop, buf = PolicyLoop(env, pi, episode_len=6), ReplayBuffer(env, 8, seed=1)
    a = loop.run(3, replay=buf)
    pi.epsilon = 0.25
    b = loop.run(3, replay=buf)
    torch.cuda.synchronize()
    played = torch.cat([a.act, b.act])
    assert torch.equal(buf.act[:6].view(torch.int32), played.view(torch.int32))
    obs = a.obs + b.obs
    explored = 0
    for t in range(1, 6):      # (step 0 was decided on the reset's observation, which the trajectory does not hold)
        E = R.explore_E(0.5 if t < 3 else 0.25)
        plain.act(obs[t - 1], t)
        for i in range(3):
            bits = R.head_bits(AR.STREAM_POLICY, 9, 70, t, i, int(env.world.world_offset))
            chosen, ex = R.explore_pick(bits, 5, E, plain.ids[0, i].cpu().numpy())
            explored += int((chosen != plain.ids[0, i].cpu().numpy()).sum())
            assert np.array_equal(played[t, i].argmax(dim=1).cpu().numpy(), chosen), (t, i)
            assert bool(((played[t, i] == 0) | (played[t, i] == 1)).all()) and bool((played[t, i].sum(dim=1) == 1).all())
    assert explored > 0      # rows that are not the greedy choice were played, and pushed
