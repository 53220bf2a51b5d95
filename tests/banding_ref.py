"""numpy restatement of spec PP-BAND-1, written from the
spec's text alone: it shares no code with csrc/banding.hip or
pixpath/banding.py.  Everything is exact integer arithmetic (Python / int64).
"""
import numpy as np

SCALES = 5
BINS = 1024


def ten_bit(x, bitdepth):
    """Step 1."""
    x = np.asarray(x).astype(np.int64)
    return x << 2 if bitdepth == 8 else np.minimum(x, 1023)


def anti_dither(u):
    """Step 2: the rounded mean of a sample, its right, lower and lower-right
    neighbour, the last row and column standing in for what lies outside."""
    r = np.concatenate([u[1:], u[-1:]], axis=0)
    return (u + np.concatenate([u[:, 1:], u[:, -1:]], axis=1) + r +
            np.concatenate([r[:, 1:], r[:, -1:]], axis=1) + 2) >> 2


def box_sum(a, r):
    """Sum of `a` over the (2r + 1)^2 neighbourhood of every position, 0 outside."""
    h, w = a.shape
    p = np.zeros((h + 2 * r + 1, w + 2 * r + 1), dtype=np.int64)
    p[r + 1:r + 1 + h, r + 1:r + 1 + w] = a
    c = p.cumsum(axis=0).cumsum(axis=1)
    n = 2 * r + 1
    return c[n:n + h, n:n + w] - c[:h, n:n + w] - c[n:n + h, :w] + c[:h, :w]


def flat_mask(y0):
    """Step 3."""
    h, w = y0.shape
    right = np.ones((h, w), dtype=bool)
    right[:, :-1] = y0[:, :-1] == y0[:, 1:]
    below = np.ones((h, w), dtype=bool)
    below[:-1] = y0[:-1] == y0[1:]
    z = (right & below).astype(np.int64)
    return (box_sum(z, 3) >= 25).astype(np.int64)


def mode3(y):
    """The most frequent of the nine values around every position (edges
    replicated), the smallest on a tie."""
    h, w = y.shape
    p = np.pad(y, 1, mode="edge")
    nb = np.stack([p[a:a + h, b:b + w] for a in range(3) for b in range(3)])
    cnt = (nb[:, None] == nb[None, :]).sum(axis=1)  # cnt[d]: how often value nb[d] occurs
    best = cnt.max(axis=0)
    return np.where(cnt == best, nb, 1 << 20).min(axis=0)


def levels(x, bitdepth):
    """[(y_s, m_s)] for s = 0 .. 4 of one plane."""
    y = anti_dither(ten_bit(x, bitdepth))
    m = flat_mask(y)
    out = [(y, m)]
    for _ in range(SCALES - 1):
        y, m = mode3(y)[::2, ::2], m[::2, ::2]
        out.append((y, m))
    return out


def contrast(y, m, window, tvi=None):
    """Step 5: Q of every position of one scale."""
    tvi = [1023] * 4 if tvi is None else [int(t) for t in tvi]
    r = window // 2
    w2 = window * window
    h, w = y.shape
    # n_d at (i, j): masked positions of the window whose value is y(i, j) + d.  Per value
    # present in the plane one indicator plane and its box sums.
    counts = {}
    for val in np.unique(y[m == 1]) if (m == 1).any() else []:
        counts[int(val)] = box_sum(((y == val) & (m == 1)).astype(np.int64), r)
    zero = np.zeros((h, w), dtype=np.int64)

    def n_of(d):
        out = np.zeros((h, w), dtype=np.int64)
        for val in counts:
            sel = (y == val - d)  # positions whose v + d is val
            if sel.any():
                out[sel] = counts[val][sel]
        return out
    n0 = n_of(0)
    masked = m == 1
    assert (n0[masked] >= 1).all()
    q = zero.copy()
    for k in range(1, 5):
        ok = masked & (y <= tvi[k - 1])
        for sign in (1, -1):
            nk = n_of(sign * k)
            num = 1024 * k * n0 * nk
            den = np.where(ok, (n0 + nk) * w2, 1)
            q = np.maximum(q, np.where(ok, num // den, 0))
    q = np.where(masked, q, 0)
    assert q.max(initial=0) <= 1023
    return q


def frame_hist(x, bitdepth, window, tvi=None):
    """Step 6: hist [5][1024] (uint32) of one plane."""
    out = np.zeros((SCALES, BINS), dtype=np.uint32)
    for s, (y, m) in enumerate(levels(x, bitdepth)):
        q = contrast(y, m, window, tvi)
        out[s] = np.bincount(q.reshape(-1), minlength=BINS).astype(np.uint32)
        assert int(out[s].sum()) == y.size
    return out


def hist(frames, bitdepth, window, tvi=None):
    """hist [n][5][1024] of a sequence of planes."""
    return np.stack([frame_hist(f, bitdepth, window, tvi) for f in frames])


# ---- synthetic content of the tests (no part of the spec) ----------------------

def content(bitdepth, n, w, h, seed=0):
    """[n, h, w] planes, half banded and half noisy: left of 55 % of the width
    a slanted staircase whose steps are 5 + f samples wide and 1 .. 4 codes high
    (10 bits; one code at 8 bits, which is 4 on the ten-bit scale), changing
    every 8 rows; right of it noise over the whole range, which the mask removes."""
    rng = np.random.default_rng(4000 + seed)
    ii, jj = np.mgrid[0:h, 0:w]
    top = (1 << bitdepth) - 1
    out = np.zeros((n, h, w), dtype=np.uint16 if bitdepth > 8 else np.uint8)
    for f in range(n):
        band = (jj + ii // 3 + f) // (5 + f)
        val = 200 + band * (1 + (ii // 8) % 4) if bitdepth > 8 else 40 + band
        noise = rng.integers(0, top + 1, (h, w))
        out[f] = np.where(jj * 100 < w * 55, np.minimum(val, top), noise)
    return out
