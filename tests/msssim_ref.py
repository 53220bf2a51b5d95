"""numpy fp64 restatement of spec PP-MSSSIM-1, written from the spec
text in the direct 2-D form: block means by reshape, every window as the 121
samples under the outer-product weight.  It shares nothing with the kernel's
separable order (csrc/msssim.hip); `terms_separable` is a second evaluation for
the CPU cross-check, `terms_longdouble` the 121-term one in extended precision."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

SCALES = 5
EXPONENTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window(dtype=np.float64):
    i = np.arange(11, dtype=dtype)
    g = np.exp(-((i - 5) ** 2) / dtype(4.5))
    return g / g.sum()


def level(x, s, dtype=np.float64):
    """Scale s of plane x: the means of its 2^s x 2^s blocks (exact), trailing rows / columns dropped."""
    b = 1 << s
    hs, ws = x.shape[0] >> s, x.shape[1] >> s
    v = x[:hs * b, :ws * b].astype(np.int64).reshape(hs, b, ws, b).sum(axis=(1, 3))
    return v.astype(dtype) / dtype(b * b)


def constants(depth):
    L = float((1 << depth) - 1)
    return (.01 * L) ** 2, (.03 * L) ** 2


def _means(mu_a, mu_b, e_aa, e_bb, e_ab, c1, c2):
    va, vb, cov = e_aa - mu_a * mu_a, e_bb - mu_b * mu_b, e_ab - mu_a * mu_b
    l = (2 * mu_a * mu_b + c1) / (mu_a * mu_a + mu_b * mu_b + c1)
    cs = (2 * cov + c2) / (va + vb + c2)
    return [cs.mean(), (l * cs).mean()]


def terms(a, b, depth, dtype=np.float64):
    """[5][2]: mean cs and mean l * cs of every scale of planes a (reference) and b; NaN without a window."""
    c1, c2 = (dtype(c) for c in constants(depth))
    g = window(dtype)
    W = np.outer(g, g)
    out = np.full((SCALES, 2), np.nan)
    for s in range(SCALES):
        pa, pb = level(a, s, dtype), level(b, s, dtype)
        if min(pa.shape) < 11:
            continue
        f = lambda p: np.einsum("ijkl,kl->ij", sliding_window_view(p, (11, 11)), W)
        out[s] = [float(v) for v in _means(f(pa), f(pb), f(pa * pa), f(pb * pb), f(pa * pb), c1, c2)]
    return out


def terms_longdouble(a, b, depth):
    return terms(a, b, depth, np.longdouble)


def terms_separable(a, b, depth):
    """The same values with the window applied along rows, then along columns."""
    c1, c2 = constants(depth)
    g = window()
    out = np.full((SCALES, 2), np.nan)
    for s in range(SCALES):
        pa, pb = level(a, s), level(b, s)
        if min(pa.shape) < 11:
            continue

        def f(p):
            hpass = sum(g[i] * p[:, i:p.shape[1] - 10 + i] for i in range(11))
            return sum(g[i] * hpass[i:p.shape[0] - 10 + i] for i in range(11))
        out[s] = _means(f(pa), f(pb), f(pa * pa), f(pb * pb), f(pa * pb), c1, c2)
    return out


def pool(t):
    """MS-SSIM of one frame's [5][2] terms, in plain Python floats."""
    if any(math.isnan(v) for row in t for v in row):
        return math.nan
    v = [t[s][0] for s in range(4)] + [t[4][1]]
    r = 1.0
    for x, e in zip(v, EXPONENTS):
        r *= max(float(x), 0.0) ** e
    return r


CONTENTS = ("noise", "small_error", "smooth_noise", "checker1", "checker16", "full_vs_zero")


def content(name, depth, w, h, seed=0):
    """(a, b): two w x h planes of the named content as int64; `depth` 16 means
    the whole uint16 container (stored values past 1023)."""
    rng = np.random.default_rng(seed)
    top = (1 << depth) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "noise":
        return rng.integers(0, top + 1, (h, w)), rng.integers(0, top + 1, (h, w))
    if name == "small_error":
        a = rng.integers(0, top + 1, (h, w))
        return a, np.clip(a + rng.integers(-2, 3, (h, w)), 0, top)
    if name == "smooth_noise":
        a = np.rint(top * (0.5 + 0.4 * np.sin(xx / 37.0) * np.cos(yy / 23.0))).astype(np.int64)
        return a, np.clip(a + rng.integers(-top // 16, top // 16 + 1, (h, w)), 0, top)
    if name in ("checker1", "checker16"):
        n = 1 if name == "checker1" else 16
        a = (((xx // n) + (yy // n)) & 1) * top
        return a, top - a
    if name == "full_vs_zero":
        return np.full((h, w), top, np.int64), np.zeros((h, w), np.int64)
    raise ValueError(name)
