"""The n-step rule of mpe_replay_sample_nstep / mpe_replay_gather_nstep (include/mpe_hip.h) restated in Python
integers and NumPy float32 on top of _replay_ref.NumpyRing (TEST INFRASTRUCTURE).  Every float32 operation is wrapped in
np.float32(...), in the order the header fixes, so every comparison against this is equality: bits() for floats."""
import numpy as np

import _replay_ref as R

MAX_NSTEP = 16
SEVENTH = np.float32(1.0) / np.float32(7.0)
CAUSES = ("done", "cut", "n", "head")


def coded32(t, field, agent, B, cols):
    """_replay_ref.coded for t < 32: the integer ((((t * 8 + field) * 8 + agent) * 128 + world) * 32 + col), below 2^23, so exact
    in float32 and different for every (t, field, agent, world, col)."""
    assert 0 <= t < 32 and agent < 8 and B <= 128 and cols <= 32
    w = np.arange(B, dtype=np.int64)[:, None]
    c = np.arange(cols, dtype=np.int64)[None, :]
    return (((((t * 8 + R.FIELDS[field]) * 8 + agent) * 128 + w) * 32) + c).astype(np.float32)


def sparse_done(t, A, B):
    """done(t, i, w) = (5 t + 3 w + 7 i) % 29 == 0: a world sees an agent done at about one step in ten."""
    return np.array([[(5 * t + 3 * w + 7 * i) % 29 == 0 for w in range(B)] for i in range(A)])


def sparse_step(t, B, widths, dim_c):
    """_replay_ref.coded_step with the sparse done rule and rewards coded * float32(1 / 7) (rounded: no exact products, so the
    order of the roundings in ret matters): (obs_n, moves, utter, next_obs_n, rew [A,B], done [A,B] bool)."""
    A = len(widths)
    obs = [coded32(t, "obs", i, B, widths[i]) for i in range(A)]
    nxt = [coded32(t, "next_obs", i, B, widths[i]) for i in range(A)]
    moves = np.stack([coded32(t, "act", i, B, 5) for i in range(A)])
    utter = np.stack([coded32(t, "utter", i, B, dim_c) for i in range(A)]) if dim_c else np.zeros((A, B, 0), np.float32)
    rew = np.stack([(coded32(t, "rew", i, B, 1)[:, 0] * SEVENTH).astype(np.float32) for i in range(A)])
    return obs, moves, utter, nxt, rew, sparse_done(t, A, B)


def chain_returns(rews, gamma):
    """rews: the m float32 rewards of one agent's chain -> (ret, discount), each operation rounded to float32 on its own:
    d_0 = 1, ret = r_0; d_k = d_{k-1} * gamma, ret = ret + d_k * r_k; discount = d_{m-1} * gamma."""
    gamma = np.float32(gamma)
    d, ret = np.float32(1.0), np.float32(rews[0])
    for r in rews[1:]:
        d = np.float32(d * gamma)
        ret = np.float32(ret + np.float32(d * np.float32(r)))
    return ret, np.float32(d * gamma)


def walk(ring, j, n, L=0, p=0):
    """The chain of transition j -> (j as used, m, last, cause): cause is the first of CAUSES that stopped the walk."""
    S, B, h = ring.S, ring.B, ring.count
    assert 1 <= n <= MAX_NSTEP and L >= 0 and 0 <= p < max(L, 1) and h >= 1
    if not 0 <= j < ring.n_valid():
        j = 0
    slot, world = divmod(j, B)
    ahead = (h - 1 - slot) % S
    g = h - 1 - ahead
    k = 0
    while True:
        assert k < n and k <= ahead      # the step is used
        if ring.done[(slot + k) % S, :, world].any():
            cause = "done"
        elif L > 0 and (g + k + 1 + p) % L == 0:
            cause = "cut"
        elif k + 1 == n:
            cause = "n"
        elif k == ahead:
            cause = "head"
        else:
            k += 1
            continue
        break
    m = k + 1
    return j, m, ((slot + m - 1) % S) * B + world, cause


def nstep(ring, idx, n, gamma, L=0, p=0):
    """What the n-step launch returns for the transitions idx (Python ints) -> a dict: the fields of NumpyRing.gather (obs_n, act,
    utter, rew at idx; next_obs_n, done at `last`), ret [A,M] and discount [M] float32, n_used [M] int32, last [M] int64, and
    cause: each sample's stop cause."""
    S, B, A = ring.S, ring.B, ring.A
    walks = [walk(ring, int(j), n, L, p) for j in idx]
    used, last = [w[0] for w in walks], [w[2] for w in walks]
    out = ring.gather(used)
    at_last = ring.gather(last)
    out["next_obs_n"], out["done"] = at_last["next_obs_n"], at_last["done"]
    M = len(walks)
    ret, disc = np.zeros((A, M), np.float32), np.zeros(M, np.float32)
    for c, (j, m, _, _) in enumerate(walks):
        slot, world = divmod(j, B)
        for i in range(A):
            ret[i, c], disc[c] = chain_returns([ring.rew[(slot + k) % S, i, world] for k in range(m)], gamma)
    out.update(ret=ret, discount=disc, n_used=np.array([w[1] for w in walks], np.int32), last=np.array(last, np.int64),
               cause=[w[3] for w in walks], idx=used)
    return out
