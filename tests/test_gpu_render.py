"""MultiAgentEnv.render(mode='rgb_array') on the device (`mpe_render`, csrc/mpe_render.hip) against the NumPy restatement of
the rendering rule (tests/_render_ref.py): byte for byte, except on knife-edge pixels (sigma within
1e-6 of a coverage threshold), which must stay under 0.01 % of the pixels."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_ref as R  # noqa: E402

import multiagent_particle_envs_amd as mpe  # noqa: E402
from multiagent_particle_envs_amd import _abi  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINE = ["simple", "simple_adversary", "simple_crypto", "simple_push", "simple_reference", "simple_speaker_listener",
        "simple_spread", "simple_tag", "simple_world_comm"]


def _random_state(env, seed, scale=1.1):
    w = env.world
    rs = np.random.RandomState(seed)
    pos = rs.uniform(-scale, scale, size=(env.batch_size, len(w.entities), 2)).astype(np.float32)
    w.set_state(pos)
    return pos


def _host_pos(env):
    return env.world.pos.permute(2, 0, 1).contiguous().cpu().numpy()      # [B, E, 2]


def _cameras(env):
    if env.shared_viewer:
        return [-1]
    return [env.world.entities.index(a) for a in env.agents]


def _check(env, frames, S, worlds=None, pos=None):
    """frames: what env.render returned (per viewer [K, S, S, 3]) for the worlds `worlds` (None: all).  Every pixel that differs
    must be a knife-edge one, and they must stay under 0.01 % of the pixels."""
    idx = np.arange(env.batch_size) if worlds is None else np.asarray(worlds)
    pos = _host_pos(env) if pos is None else pos
    ref, knife = R.render_frames(pos[idx], R.env_sizes(env), R.env_colours(env)[idx], S, _cameras(env))
    got = torch.stack(frames).cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.uint8
    bad = (got != ref).any(axis=-1)
    assert not (bad & ~knife).any(), "%d pixels differ off the knife edge, first at %s" % (
        int((bad & ~knife).sum()), np.argwhere(bad & ~knife)[:3].tolist())
    assert bad.sum() <= 1e-4 * bad.size, int(bad.sum())
    return got, knife


@pytest.mark.parametrize("name", NINE)
def test_builtin_scenarios_match_the_rule(name):
    env = mpe.make_env(name, batch_size=64)
    env.reset()                                   # per-world picks -> goal colours
    _random_state(env, 11)
    frames = env.render("rgb_array", size=96)
    assert len(frames) == 1 and frames[0].shape == (64, 96, 96, 3) and frames[0].dtype == torch.uint8
    assert frames[0].device == env.world.device
    got, knife = _check(env, frames, 96)
    assert (got != 255).any()                     # something was drawn
    assert knife.sum() < 1e-4 * knife.size, int(knife.sum())


def test_one_viewer_per_agent():
    env = mpe.make_env("simple_tag", batch_size=16)
    env.shared_viewer = False
    _random_state(env, 3)
    frames = env.render("rgb_array", size=64)
    assert len(frames) == env.n and all(f.shape == (16, 64, 64, 3) for f in frames)
    _check(env, frames, 64)
    # each view is centred on its agent: the agent's own disc covers the middle pixels
    for v, f in enumerate(frames):
        assert (f[:, 31:33, 31:33] != 255).all()


def test_sixty_four_agents_overlapping():
    env = mpe.make_env("simple_spread", batch_size=16, num_agents=64)
    _random_state(env, 5, scale=1.0)
    frames = env.render("rgb_array", size=256)
    _check(env, frames, 256)


def test_world_selection():
    env = mpe.make_env("simple_spread", batch_size=32)
    _random_state(env, 7)
    full = env.render("rgb_array", size=48)[0]
    assert torch.equal(env.render("rgb_array", worlds=5, size=48)[0], full[5:6])
    assert torch.equal(env.render("rgb_array", worlds=[3, 0, 31, -1], size=48)[0], full[[3, 0, 31, 31]])
    t = torch.tensor([9, 1, 30], device=env.world.device)
    assert torch.equal(env.render("rgb_array", worlds=t, size=48)[0], full[[9, 1, 30]])
    assert torch.equal(env.render("rgb_array", worlds=slice(2, 20, 3), size=48)[0], full[2:20:3])
    for bad in (32, -33, [0, 32], torch.tensor([40], device=env.world.device)):
        with pytest.raises(IndexError):
            env.render("rgb_array", worlds=bad, size=48)


def test_single_world_mode_returns_numpy_frames():
    env = mpe.make_env("simple_spread")
    out = env.render("rgb_array")
    assert isinstance(out, list) and len(out) == 1
    img = out[0]
    assert isinstance(img, np.ndarray) and img.shape == (700, 700, 3) and img.dtype == np.uint8
    pos = _host_pos(env)
    ref, knife = R.render_frame(pos[0], R.env_sizes(env), R.env_colours(env)[0], 700)
    bad = (img != ref).any(axis=-1)
    assert not (bad & ~knife).any(), int((bad & ~knife).sum())


def test_colours_follow_device_resets():
    from multiagent_particle_envs_amd.rollout import RandomRollout
    env = mpe.make_env("simple_adversary", batch_size=64)
    env.reset()
    RandomRollout(env, episode_len=25).fused(50)     # in-launch resets: new goals drawn on the device
    assert env._scenario_state_stale
    frames = env.render("rgb_array", size=64)
    goal = env.world.choice_i32[0].cpu().numpy()
    assert len(set(goal.tolist())) > 1
    rgba = R.env_colours(env)
    A = len(env.world.agents)
    green = np.array([0.15, 0.65, 0.15], np.float32)
    for b in range(env.batch_size):
        for l in range(len(env.world.landmarks)):
            assert np.array_equal(rgba[b, A + l, :3], green) == (l == goal[b])
    _check(env, frames, 64)


def test_render_is_read_only():
    envs = [mpe.make_env("simple_spread", batch_size=64) for _ in range(2)]
    for e in envs:
        _random_state(e, 13, scale=1.0)
    rs = np.random.RandomState(1)
    for t in range(4):
        act = torch.as_tensor(np.eye(5, dtype=np.float32)[rs.randint(0, 5, size=(3, 64))]).cuda()
        outs = []
        for i, e in enumerate(envs):
            obs, rew, _, _ = e.step(act)
            if i == 0:
                frames = e.render("rgb_array", size=64)       # between the steps of env 0 only
            outs.append((torch.stack([o.clone() for o in obs]), torch.stack([r.clone() for r in rew]), e.world.pos.clone(),
                         e.world.vel.clone()))
        for a, b in zip(*outs):
            assert torch.equal(a, b)
        _check(envs[0], frames, 64, pos=outs[0][2].permute(2, 0, 1).cpu().numpy())


def test_entities_partly_outside_the_view_are_clipped():
    env = mpe.make_env("simple_spread", batch_size=8)
    pos = _random_state(env, 17, scale=0.5)
    pos[:, 3] = (1.02, 0.0)                        # landmark 0 (size 0.05) straddles the right edge
    env.world.set_state(pos)
    got, _ = _check(env, env.render("rgb_array", size=100), 100)
    assert (got[0, :, 49:51, 99] != 255).any(axis=-1).all()     # its visible part reaches the last column
    assert (got[0, :, 49:51, 0] == 255).all()                    # ... and does not wrap to the first


def test_refusals():
    env = mpe.make_env("simple_spread", batch_size=4)
    with pytest.raises(NotImplementedError):
        env.render()
    with pytest.raises(ValueError, match="unknown mode"):
        env.render("video")
    env.world.landmarks[1].color = None
    with pytest.raises(ValueError, match="landmark 1"):
        env.render("rgb_array", size=32)
    ref = mpe.make_env(os.path.join(ROOT, "tests", "refstyle", "convoy.py"), batch_size=4, traced=False)
    with pytest.raises(NotImplementedError, match="colours"):
        ref.render("rgb_array")


def test_odd_size_tail_and_many_small_frames():
    """size 9: 81 pixels per frame, so a block spans many frames and the last 16-pixel run is partial -- the bytes behind
    the frames stay untouched."""
    import ctypes as C
    env = mpe.make_env("simple_tag", batch_size=7)
    _random_state(env, 19, scale=0.9)
    frames = env.render("rgb_array", size=9)
    _check(env, frames, 9)
    n = 7 * 9 * 9 * 3
    buf = torch.full((n + 256,), 7, dtype=torch.uint8, device=env.world.device)
    w = env.world
    rgba = torch.as_tensor(R.env_colours(env)[0], device=w.device).contiguous()     # constant colours: [E, 4]
    a = _abi.MpeRenderArgs()
    a.pos, a.B, a.K, a.n_entities = w.pos.data_ptr(), 7, 7, len(w.entities)
    a.rgba, a.rgba_world_stride, a.n_viewers, a.size, a.out = rgba.data_ptr(), 0, 1, 9, buf.data_ptr()
    desc = w.scenario_desc(_abi.MPE_SCN_GENERIC)
    _abi.check(_abi.lib().mpe_render(C.byref(desc), C.byref(a), _abi.raw_stream(w.device)), "mpe_render")
    assert torch.equal(buf[:n].view(1, 7, 9, 9, 3)[0], frames[0])
    assert buf[n:].eq(7).all()
