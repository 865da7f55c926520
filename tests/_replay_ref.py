"""The replay buffer restated in NumPy and Python integers (TEST INFRASTRUCTURE): the ring of include/mpe_hip.h (MpeReplay) as
plain arrays, and the draw rule of mpe_replay_sample on oracle.philox.philox4x32_10.  Both kernels only move data, so every
comparison against this is equality."""
import numpy as np

from oracle.philox import philox4x32_10

STREAM_REPLAY = 0x5245504C      # "REPL"
M32 = 0xFFFFFFFF


def draw_words(seed, draw, M):
    """-> (hi, lo) uint32 arrays [M]: sample k's two words of Philox block k >> 1 -- (x, y) for an even k, (z, w) for an odd one."""
    k = np.arange(M, dtype=np.uint64)
    blk = k >> np.uint64(1)
    c0 = blk & np.uint64(M32)
    c1 = (blk >> np.uint64(32)) ^ np.uint64((draw >> 32) & M32)
    c2 = np.zeros(M, np.uint64)
    c3 = np.full(M, (STREAM_REPLAY ^ (draw & M32)) & M32, np.uint64)
    o = philox4x32_10(c0, c1, c2, c3, seed & M32, (seed >> 32) & M32)
    odd = (k & np.uint64(1)).astype(bool)
    return np.where(odd, o[2], o[0]), np.where(odd, o[3], o[1])


def draw_indices(seed, draw, M, n_valid):
    """Transition indices [M] (Python ints): j = (u * n_valid) >> 64 with u = hi << 32 | lo."""
    hi, lo = draw_words(seed, draw, M)
    return [(((int(h) << 32) | int(l)) * int(n_valid)) >> 64 for h, l in zip(hi, lo)]


class NumpyRing(object):
    """obs / next_obs: per slot a list of [B, D_i]; act [S,A,B,5]; utter [S,A,B,dim_c]; rew [S,A,B]; done [S,A,B] bool."""

    def __init__(self, S, B, widths, dim_c):
        A = len(widths)
        self.S, self.B, self.A, self.widths, self.dim_c, self.count = S, B, A, list(widths), dim_c, 0
        self.obs = [[np.zeros((B, d), np.float32) for d in widths] for _ in range(S)]
        self.next_obs = [[np.zeros((B, d), np.float32) for d in widths] for _ in range(S)]
        self.act = np.zeros((S, A, B, 5), np.float32)
        self.utter = np.zeros((S, A, B, dim_c), np.float32)
        self.rew = np.zeros((S, A, B), np.float32)
        self.done = np.zeros((S, A, B), bool)

    def push(self, obs_n, moves, utter, next_obs_n, rew, done):
        s = self.count % self.S
        for i in range(self.A):
            self.obs[s][i][...] = obs_n[i]
            self.next_obs[s][i][...] = next_obs_n[i]
        self.act[s], self.rew[s], self.done[s] = moves, rew, done
        if self.dim_c:
            self.utter[s] = utter
        self.count += 1

    def n_valid(self):
        return min(self.count, self.S) * self.B

    def gather(self, idx):
        """-> dict of the fields at transitions idx (slot = j // B, world = j % B), shaped as mpe_replay_sample's outputs."""
        sl = [j // self.B for j in idx]
        wd = [j % self.B for j in idx]
        A = self.A
        out = {"obs_n": [np.stack([self.obs[s][i][w] for s, w in zip(sl, wd)]) for i in range(A)],
               "next_obs_n": [np.stack([self.next_obs[s][i][w] for s, w in zip(sl, wd)]) for i in range(A)],
               "act": np.stack([self.act[sl, i, wd] for i in range(A)]),
               "utter": np.stack([self.utter[sl, i, wd] for i in range(A)]),
               "rew": np.stack([self.rew[sl, i, wd] for i in range(A)]),
               "done": np.stack([self.done[sl, i, wd] for i in range(A)])}
        return out


FIELDS = {"obs": 0, "next_obs": 1, "act": 2, "utter": 3, "rew": 4}


def coded(t, field, agent, B, cols):
    """[B, cols] float32 whose element (world, col) is the integer ((((t * 8 + field) * 8 + agent) * 128 + world) * 32 + col): below
    2^21 for t < 8, agent < 8, B <= 128, cols <= 32, so exact in float32 and different for every (t, field, agent, world, col)."""
    assert t < 8 and agent < 8 and B <= 128 and cols <= 32
    w = np.arange(B, dtype=np.int64)[:, None]
    c = np.arange(cols, dtype=np.int64)[None, :]
    return (((((t * 8 + FIELDS[field]) * 8 + agent) * 128 + w) * 32) + c).astype(np.float32)


def coded_step(t, B, widths, dim_c):
    """One synthetic step: (obs_n, moves [A,B,5], utter [A,B,dim_c], next_obs_n, rew [A,B], done [A,B] bool)."""
    A = len(widths)
    obs = [coded(t, "obs", i, B, widths[i]) for i in range(A)]
    nxt = [coded(t, "next_obs", i, B, widths[i]) for i in range(A)]
    moves = np.stack([coded(t, "act", i, B, 5) for i in range(A)])
    utter = np.stack([coded(t, "utter", i, B, dim_c) for i in range(A)]) if dim_c else np.zeros((A, B, 0), np.float32)
    rew = np.stack([coded(t, "rew", i, B, 1)[:, 0] for i in range(A)])
    done = np.array([[(t + 2 * i + w) % 3 == 0 for w in range(B)] for i in range(A)])
    return obs, moves, utter, nxt, rew, done
