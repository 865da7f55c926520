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
    """obs / next_obs: per slot a list of [B, D_i]; act [S,A,B,5]; utter [S,A,B,dim_c]; rew [S,A,B]; done [S,A,B] bool.  Any S, B,
    widths and dim_c.  The float fields are stored and gathered through their uint32 views, so every bit pattern (NaN payloads,
    denormals, -0.0) comes back as it went in; compare them with bits()."""

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
            _store(self.obs[s][i], obs_n[i])
            _store(self.next_obs[s][i], next_obs_n[i])
        _store(self.act[s], moves)
        _store(self.rew[s], rew)
        self.done[s] = done
        if self.dim_c:
            _store(self.utter[s], utter)
        self.count += 1

    def n_valid(self):
        return min(self.count, self.S) * self.B

    def gather(self, idx):
        """-> dict of the fields at transitions idx (slot = j // B, world = j % B), shaped as mpe_replay_sample's outputs."""
        sl = [j // self.B for j in idx]
        wd = [j % self.B for j in idx]
        A = self.A
        act, utter, rew = self.act.view(np.uint32), self.utter.view(np.uint32), self.rew.view(np.uint32)
        out = {"obs_n": [np.stack([self.obs[s][i].view(np.uint32)[w] for s, w in zip(sl, wd)]).view(np.float32) for i in range(A)],
               "next_obs_n": [np.stack([self.next_obs[s][i].view(np.uint32)[w] for s, w in zip(sl, wd)]).view(np.float32)
                              for i in range(A)],
               "act": np.stack([act[sl, i, wd] for i in range(A)]).view(np.float32),
               "utter": np.stack([utter[sl, i, wd] for i in range(A)]).view(np.float32),
               "rew": np.stack([rew[sl, i, wd] for i in range(A)]).view(np.float32),
               "done": np.stack([self.done[sl, i, wd] for i in range(A)])}
        return out


def _store(dst, src):
    """float32 -> float32 as 32-bit integers: no float ever passes through an arithmetic unit, a NaN keeps its payload."""
    dst.view(np.uint32)[...] = np.ascontiguousarray(src, dtype=np.float32).view(np.uint32)


def bits(x):
    """A float32 array (or a torch tensor's .cpu().numpy()) as int32: what np.array_equal compares where the data holds NaNs."""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


FIELDS = {"obs": 0, "next_obs": 1, "act": 2, "utter": 3, "rew": 4, "done": 5}


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


ODD = 0x9E3779B1      # an odd multiplier: c -> c * ODD mod 2^32 is a bijection of the 32-bit patterns
SPECIALS = (0x7FC00001, 0xFFC12345, 0x00000001, 0x80000000, 0x7F800000)      # two NaNs with payloads, a denormal, -0.0, +inf


def _counter(t, field, agent, B, cols):
    """[B, cols] uint64: ((t * 8 + field) * 16 + agent) * 2^20 + world * cols + col -- below 2^32 and different for every
    (t, field, agent, world, col) while t < 32, agent < 16 and B * cols <= 2^20 (a row of 4096 floats for 256 worlds)."""
    assert 0 <= t < 32 and 0 <= agent < 16 and B * cols <= 2 ** 20
    e = np.arange(B * cols, dtype=np.uint64).reshape(B, cols)
    return np.uint64(((t * 8 + FIELDS[field]) * 16 + agent) << 20) + e


def bit_patterns(t, field, agent, B, cols):
    """[B, cols] float32 whose every element is a different 32-bit pattern: the counter times ODD mod 2^32, so floats of every
    exponent, NaNs among them."""
    u = ((_counter(t, field, agent, B, cols) * np.uint64(ODD)) & np.uint64(M32)).astype(np.uint32)
    return u.view(np.float32)


def _force_specials(t, field, blocks):
    """SPECIALS into five consecutive elements of one step's whole field (its agents' blocks in agent order, as the ring lays
    them out), ONCE per field: at its very first elements for step 0's obs, and five elements further on for every next
    (step, field), so that in a ring of few worlds no agent's row is nothing but SPECIALS in every slot and field.  Everything
    else stays distinct: T steps of a field of n floats hold at least T * (n - 5) different patterns."""
    n = sum(b.size for b in blocks)
    k = min(len(SPECIALS), n)
    start = (5 * (t * 8 + FIELDS[field])) % (n - k + 1)
    flat = [b.reshape(-1).view(np.uint32) for b in blocks]      # (views: the blocks are contiguous)
    for j in range(k):
        e = start + j
        for f in flat:
            if e < f.size:
                f[e] = SPECIALS[j]
                break
            e -= f.size


def distinct_patterns(arrays):
    """How many different 32-bit patterns the float32 arrays hold between them."""
    return len(np.unique(np.concatenate([np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).reshape(-1) for a in arrays])))


def bits_step(t, A, B, widths, dim_c):
    """coded_step without its size limits and with every float a bit pattern of its own, but for five SPECIALS per field
    (_force_specials): (obs_n, moves [A,B,5], utter [A,B,dim_c], next_obs_n, rew [A,B], done [A,B] bool).  done is bit 13 of the
    same mixed counter."""
    assert len(widths) == A
    obs = [bit_patterns(t, "obs", i, B, widths[i]) for i in range(A)]
    nxt = [bit_patterns(t, "next_obs", i, B, widths[i]) for i in range(A)]
    moves = np.stack([bit_patterns(t, "act", i, B, 5) for i in range(A)])
    utter = np.stack([bit_patterns(t, "utter", i, B, dim_c) for i in range(A)]) if dim_c else np.zeros((A, B, 0), np.float32)
    rew = np.stack([bit_patterns(t, "rew", i, B, 1)[:, 0] for i in range(A)])
    for field, blocks in (("obs", obs), ("next_obs", nxt), ("act", [moves]), ("utter", [utter]), ("rew", [rew])):
        if sum(b.size for b in blocks):
            _force_specials(t, field, blocks)
    done = np.stack([(((_counter(t, "done", i, B, 1)[:, 0] * np.uint64(ODD)) >> np.uint64(13)) & np.uint64(1)).astype(bool)
                     for i in range(A)])
    return obs, moves, utter, nxt, rew, done
