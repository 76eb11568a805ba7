"""The position sampler of the heatmap mutual-information loss, restated in numpy: Philox4x32-10
and the per-row procedure of posu_heatmap_mi_sample (include/posu.h), written from the definition
and independently of csrc/mi_sample.hip.  It is the specification the kernel is held to, bit for
bit; the distribution tests (tests/test_heatmap_mi_sampler_host.py) run on it.

Row k's draw is a function of (seed, call, k) and of that row's inputs only.  Its random words are
those of the Philox blocks with counter (b, k, call low, call high), b = 0, 1, 2, ..., key (seed low,
seed high), taken in output order; bounded(w, n) = (w * n) >> 32 maps a word to [0, n)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57      # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85      # the Weyl constants added to the key between rounds
MASK = 0xFFFFFFFF
MAX_DRAWS_PER_SLOT = 64              # outside draws per position before the deterministic fill


def philox4x32_10(counter, key):
    """Ten rounds on a counter of four and a key of two 32-bit words: four 32-bit words."""
    c0, c1, c2, c3 = [int(c) & MASK for c in counter]
    k0, k1 = [int(k) & MASK for k in key]
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
    return c0, c1, c2, c3


def bounded(w, n):
    return (int(w) * int(n)) >> 32


class Words:
    """The word stream of row k: blocks 0, 1, 2, ... in output order."""

    def __init__(self, seed, call, k):
        self.key = (seed & MASK, (seed >> 32) & MASK)
        self.tail = (int(k) & MASK, call & MASK, (call >> 32) & MASK)
        self.block, self.buf, self.used = 0, (), 0

    def next(self):
        if not self.buf:
            self.buf = philox4x32_10((self.block,) + self.tail, self.key)
            self.block += 1
        w, self.buf = self.buf[0], self.buf[1:]
        self.used += 1
        return w


def sizes(radius):
    p = (2 * radius + 1) ** 2
    return p, p // 2, p // 4


def grid_coordinate(v, feat, size):
    """trunc(v / feat + 0.5) in f64, clamped to [0, size - 1]; NaN gives 0."""
    t = np.float64(v) / np.float64(feat) + np.float64(0.5)
    if not t >= 1.0:
        return 0
    if t >= size:
        return size - 1
    return int(t)


def window_of(centre, radius, h, w):
    """The (2 radius + 1)^2 entries around `centre`: the clamped LINEAR index, row-major in (dy, dx)."""
    return [min(max(centre + dy * w + dx, 0), h * w - 1)
            for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]


def sample_row(joint_xy, visible, k, feat_w, feat_h, h, w, radius, seed, call, stats=None):
    """(idx [Q], loc) of row k.  stats: optional dict, receives 'draws' (outside draws made) and
    'filled' (slots the bounded loop left to the deterministic fill)."""
    p, n_in, n_out = sizes(radius)
    hw = h * w
    words = Words(seed, call, k)
    gx = grid_coordinate(joint_xy[0], feat_w, w)
    gy = grid_coordinate(joint_xy[1], feat_h, h)
    w0 = words.next()
    centre = gy * w + gx if visible else bounded(w0, hw)
    window = window_of(centre, radius, h, w)
    perm = list(range(p))
    inside = []
    for t in range(n_in):
        j = t + bounded(words.next(), p - t)
        perm[t], perm[j] = perm[j], perm[t]
        inside.append(window[perm[t]])
    taken = set(window)
    outside, draws = [], 0
    while len(outside) < n_out and draws < MAX_DRAWS_PER_SLOT * n_out:
        q = bounded(words.next(), hw)
        draws += 1
        if q not in taken:
            taken.add(q)
            outside.append(q)
    filled = n_out - len(outside)
    q = 0
    while len(outside) < n_out:      # the lowest free positions, ascending
        if q not in taken:
            taken.add(q)
            outside.append(q)
        q += 1
    if stats is not None:
        stats['draws'], stats['filled'] = draws, filled
    return inside + outside, centre


def sample(joints, vis, joint_idx, feat_w, feat_h, h, w, radius, seed, call, first_row=0, stats=None):
    """joints [B, J, 2] f64, vis [B, J] -> (idx [B, Q] int32, loc [B] int32); row k of the result is
    row first_row + k of the stream.  stats: optional list, one dict per row appended."""
    joints, vis = np.asarray(joints, dtype=np.float64), np.asarray(vis)
    b = joints.shape[0]
    _, n_in, n_out = sizes(radius)
    idx = np.zeros((b, n_in + n_out), dtype=np.int32)
    loc = np.zeros((b,), dtype=np.int32)
    for k in range(b):
        st = {} if stats is not None else None
        idx[k], loc[k] = sample_row(joints[k, joint_idx], vis[k, joint_idx] != 0, first_row + k, feat_w, feat_h, h, w,
                                    radius, seed, call, st)
        if stats is not None:
            stats.append(st)
    return idx, loc
