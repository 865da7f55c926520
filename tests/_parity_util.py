"""Helpers shared by the GPU parity tests (test_gpu_parity.py, test_f3_scenarios.py, test_gpu_server_oracle.py): the per-element
bar, the guard band of the strict-< outputs, and the golden files' per-world picks / comm state / action rows."""
import os

import numpy as np
import torch

TOL = 1e-5


def close(a, b, tol=TOL, what=""):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert np.all(err <= tol), "%s: max scaled err %.3e at %s" % (what, err.max(), np.unravel_index(err.argmax(), err.shape))
    return float(err.max()) if err.size else 0.0


def np_(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


MASKED = {}   # test -> most worlds the guard band masked (asserted <= 1 % wherever it is used)


def guard_ok(spec, pos64, margin=1e-6, max_frac=0.01):
    """True per world where no counted pair is within `margin` of its collision threshold.  Fails when the band masks
    more than `max_frac` of the worlds (min. one world): a check that masks everything would pass vacuously."""
    ok = _guard_ok(spec, pos64, margin)
    n_masked = int((~ok).sum())
    assert n_masked <= max(1, max_frac * len(ok)), "guard band masks %d of %d worlds" % (n_masked, len(ok))
    key = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::")[-1]
    MASKED[key] = max(MASKED.get(key, 0), n_masked)
    return ok


def _guard_ok(spec, pos64, margin):
    A = spec.n_agents
    size = np.asarray(spec.size)
    ok = np.ones(pos64.shape[0], bool)

    def near(i_idx, j_idx, thr):
        d = pos64[:, i_idx, None, :] - pos64[:, None, j_idx, :]
        dist = np.sqrt((d ** 2).sum(-1))
        return (np.abs(dist - thr[None]) < margin).any(axis=(1, 2))
    ag = list(range(A))
    if spec.name == "simple_spread":
        ok &= ~near(ag, ag, size[ag][:, None] + size[ag][None, :])
        lm = list(range(A, spec.n_entities))
        ok &= ~near(ag, lm, np.full((A, len(lm)), 0.1))
    if spec.name == "simple_tag":
        good = [j for j in ag if not spec.adversary[j]]
        adv = [j for j in ag if spec.adversary[j]]
        ok &= ~near(good, adv, size[good][:, None] + size[adv][None, :])
    return ok


def set_choices(env, choice):
    sc = env.scenario
    if choice.shape[1] == 0:
        return
    if hasattr(sc, "set_choices"):
        sc.set_choices(env.world, torch.as_tensor(choice))
    elif choice.shape[1] == 1:
        sc.set_goal(env.world, torch.as_tensor(choice[:, 0]))
    else:
        sc.set_goal(env.world, torch.as_tensor(choice))


def set_comm(env, g, t):
    for i, agent in enumerate(env.world.agents):
        c = g["c%d" % i][t] if t >= 0 else np.zeros_like(g["c%d" % i][0])
        agent.state.c = torch.as_tensor(c, dtype=torch.float32, device=env.world.device)


def golden_moves_and_words(g, world):
    """A golden's action rows split the way env.step splits them (environment.py:148-190): -> (moves [T, A, W, 5], words
    [T, A, W, dim_c] or None).  Goldens of the three BASELINE scenarios hold `act` [T, W, A, 5]; the f3 ones `act<i>` [T, W, d_i]
    with d_i = [5 if movable] + [dim_c if not silent] -- an immovable agent's move and a silent agent's words are zeros."""
    if "act" in g:
        return np.ascontiguousarray(np.transpose(g["act"], (0, 2, 1, 3)), dtype=np.float32), None
    agents, dc = world.agents, int(world.dim_c)
    T, W = g["act0"].shape[:2]
    moves = np.zeros((T, len(agents), W, 5), np.float32)
    words = np.zeros((T, len(agents), W, dc), np.float32)
    for i, agent in enumerate(agents):
        a, k = g["act%d" % i], 0
        if agent.movable:
            moves[:, i] = a[..., :5]
            k = 5
        if not agent.silent:
            words[:, i] = a[..., k:k + dc]
            k += dc
        assert k == a.shape[-1], (i, k, a.shape)
    return moves, (words if any(not a.silent for a in agents) else None)
