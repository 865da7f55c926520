"""Prioritized replay restated in NumPy (TEST INFRASTRUCTURE): the sum tree, the push, update and draw rules of include/mpe_hip.h
(MpeReplayPrio) in float32 / float64 arithmetic and oracle.philox.  The kernels add non-negative floats in one fixed order, so
every comparison against this is equality."""
import numpy as np

from oracle.philox import philox4x32_10

FANOUT = 16
PRIO_MIN, PRIO_MAX = np.float32(2.0 ** -40), np.float32(2.0 ** 40)
STREAM_REPLAY_PRIO = 0x5250524F      # "RPRO"
M32 = 0xFFFFFFFF


def level_sizes(n_leaves):
    """[n_0, n_1, ..]: n_0 = n_leaves, n_l = ceil(n_{l-1} / 16), down to the level of one node."""
    n, out = int(n_leaves), []
    while True:
        out.append(n)
        if n == 1:
            return out
        n = -(-n // FANOUT)


def layout(n_leaves):
    """-> (level offsets off[0..levels] in floats, each level padded to a multiple of 16; the float count)."""
    off = [0]
    for n in level_sizes(n_leaves):
        off.append(off[-1] + -(-n // FANOUT) * FANOUT)
    return off, off[-1]


def clamp(p):
    """A stored priority: into [2^-40, 2^40], a NaN to 2^-40."""
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(p >= PRIO_MIN, np.where(p <= PRIO_MAX, p, PRIO_MAX), PRIO_MIN).astype(np.float32)


def pair_sum(children):
    """[n, 16] float32 -> [n]: (c0 + c1), (c2 + c3), ... then pairs of those, four rounds."""
    v = np.asarray(children, dtype=np.float32)
    for _ in range(4):
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def build(leaves):
    """The levels of the tree over `leaves`: a list of float32 arrays, each padded with zeros to a multiple of 16."""
    sizes = level_sizes(len(leaves))
    levels = []
    cur = np.asarray(leaves, dtype=np.float32)
    for l, n in enumerate(sizes):
        pad = np.zeros(-(-n // FANOUT) * FANOUT, np.float32)
        pad[:n] = cur
        levels.append(pad)
        if l + 1 < len(sizes):
            cur = pair_sum(pad.reshape(-1, FANOUT))
    return levels


def flat(levels):
    """The levels one after another: the device allocation."""
    return np.concatenate(levels)


def prio_bits(seed, draw, M):
    """The 24 bits of samples 0..M-1 of draw number `draw`: the top 24 of the word pair of the replay draw's counter layout
    (sample k: block k >> 1, (x, y) for an even k, (z, w) for an odd one) on STREAM_REPLAY_PRIO -> the top 24 bits of the first word."""
    k = np.arange(M, dtype=np.uint64)
    blk = k >> np.uint64(1)
    c0 = blk & np.uint64(M32)
    c1 = (blk >> np.uint64(32)) ^ np.uint64((draw >> 32) & M32)
    c2 = np.zeros(M, np.uint64)
    c3 = np.full(M, (STREAM_REPLAY_PRIO ^ (draw & M32)) & M32, np.uint64)
    o = philox4x32_10(c0, c1, c2, c3, seed & M32, (seed >> 32) & M32)
    odd = (k & np.uint64(1)).astype(bool)
    return (np.where(odd, o[2], o[0]) >> np.uint32(8)).astype(np.uint32)


def draw(levels, M, r):
    """The stratified descent for the 24-bit values r [M] -> (idx int64 [M], prio float32 [M], total float32, how many times the
    last-child rule fired -- counted per (sample, level))."""
    top = len(levels) - 1
    total = np.float32(levels[top][0])
    k = np.arange(M, dtype=np.float64)
    r = (np.asarray(r).astype(np.int64) & 0xFFFFFF).astype(np.float64)
    x = ((k + r * 2.0 ** -24) / np.float64(M) * np.float64(total)).astype(np.float32)
    node = np.zeros(M, np.int64)
    val = np.full(M, total, np.float32)
    fired = 0
    rows = np.arange(M)
    for l in range(top, 0, -1):
        ch = levels[l - 1].reshape(-1, FANOUT)[node]      # [M, 16]
        acc = np.zeros(M, np.float32)
        pick = np.full(M, -1, np.int64)
        acc_pick = np.zeros(M, np.float32)
        last = np.zeros(M, np.int64)
        acc_last = np.zeros(M, np.float32)
        for c in range(FANOUT):
            nxt = (acc + ch[:, c]).astype(np.float32)
            open_ = pick < 0
            hit = open_ & (x < nxt)
            pick[hit], acc_pick[hit] = c, acc[hit]
            pos = open_ & ~hit & (ch[:, c] > 0)
            last[pos], acc_last[pos] = c, acc[pos]
            acc = nxt
        none = pick < 0
        fired += int(none.sum())
        pick[none], acc_pick[none] = last[none], acc_last[none]
        x = (x - acc_pick).astype(np.float32)
        val = ch[rows, pick]
        node = node * FANOUT + pick
    return node, val.astype(np.float32), total, fired


class PrioTree(object):
    """The priorities of an S x B ring and their tree: leaves [S * B] float32 (0 = never pushed), pmax, head (pushes so far)."""

    def __init__(self, S, B):
        self.S, self.B, self.n = S, B, S * B
        self.leaves = np.zeros(self.n, np.float32)
        self.pmax = np.float32(1.0)
        self.head = 0

    def push(self):
        """mpe_replay_prio_push, then the ring push's head += 1."""
        s = self.head % self.S
        self.leaves[s * self.B: (s + 1) * self.B] = self.pmax
        self.head += 1

    def update(self, idx, prio):
        v = clamp(prio)
        new = {}
        for j, p in zip(np.asarray(idx, dtype=np.int64).tolist(), v.tolist()):
            if 0 <= j < self.n and self.leaves[j] != 0:
                new[j] = max(new.get(j, 0.0), p)
        for j, p in new.items():
            self.leaves[j] = np.float32(p)
            self.pmax = max(self.pmax, np.float32(p))

    def levels(self):
        return build(self.leaves)

    def tree(self):
        return flat(self.levels())

    def n_valid(self):
        return min(self.head, self.S) * self.B

    def draw(self, M, seed=0, draw_no=0, u24=None):
        """-> (idx, prio, total, fired); u24: the caller's bits [M] instead of the drawn ones."""
        r = prio_bits(seed, draw_no, M) if u24 is None else np.asarray(u24)
        return draw(self.levels(), M, r)


def find_last_child_case(seed=0, tries=100000):
    """A seeded search: 16 priorities whose pairwise total exceeds their sequential float32 sum -> the float32 [16] array."""
    rs = np.random.RandomState(seed)
    for _ in range(tries):
        p = (2.0 ** rs.randint(-3, 4, size=16) * (1.0 + rs.rand(16))).astype(np.float32)
        seq = np.float32(0)
        for c in p:
            seq = np.float32(seq + c)
        if pair_sum(p[None, :])[0] > seq:
            return p
    raise AssertionError("no such leaf set in %d tries" % tries)
