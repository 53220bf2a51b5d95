"""numpy fp64 restatement of spec PP-VIF-1, written from the spec
text in the direct 2-D form: every position's five quantities as the N x N
samples of the `reflect`-padded plane under the outer-product weight.  It
shares nothing with the kernel's separable order (csrc/vif.hip).  The pyramid
uses the same direct form and keeps the even rows and columns.  `separable`
applies the window along rows, then along columns, everywhere the direct form
applies the 2-D one: the same values up to the order of the fp64 sums, fast
enough for a 1920x1080 plane (`terms_separable`, what tools/vif_bench.py
checks the GPU against)."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

SCALES = 4
TAPS = (17, 9, 5, 3)
EPS = 1e-10


def window(s):
    n = TAPS[s]
    sigma = n / 5.0
    g = np.exp(-((np.arange(n, dtype=np.float64) - n // 2) ** 2) / (2.0 * sigma * sigma))
    return g / g.sum()


def exists(p, s):
    return min(p.shape) >= TAPS[s] // 2 + 1


def filt(p, s, separable=False):
    """Plane p under the 2-D window of scale s, mirrored borders: same shape."""
    g = window(s)
    r = TAPS[s] // 2
    q = np.pad(p, r, mode="reflect")
    if separable:
        rows = sum(g[i] * q[:, i:i + p.shape[1]] for i in range(TAPS[s]))
        return sum(g[i] * rows[i:i + p.shape[0]] for i in range(TAPS[s]))
    return np.einsum("ijkl,kl->ij", sliding_window_view(q, (TAPS[s], TAPS[s])), np.outer(g, g))


def levels(x, depth, separable=False):
    """The scales of plane x that exist, as fp64 planes on the 8-bit scale."""
    p = np.asarray(x).astype(np.float64) / float(1 << (depth - 8))
    out = []
    for s in range(SCALES):
        if s:
            p = filt(p, s, separable)[0:2 * (p.shape[0] // 2):2, 0:2 * (p.shape[1] // 2):2]
        if not exists(p, s):
            break
        out.append(p)
    return out


def moments(pa, pb, s, separable=False):
    """sigma1^2, sigma2^2, sigma12 of every position of scale s (clamped as the spec says)."""
    f = lambda p: filt(p, s, separable)
    mu1, mu2 = f(pa), f(pb)
    s1 = np.maximum(f(pa * pa) - mu1 * mu1, 0.0)
    s2 = np.maximum(f(pb * pb) - mu2 * mu2, 0.0)
    s12 = f(pa * pb) - mu1 * mu2
    return s1, s2, s12


def position_terms(s1, s2, s12):
    """num and den of every position from its moments, the spec's steps in order."""
    s1 = s1.copy()
    g = s12 / (s1 + EPS)
    sv = s2 - g * s12
    m = s1 < EPS
    g[m], sv[m], s1[m] = 0.0, s2[m], 0.0
    m = s2 < EPS
    g[m], sv[m] = 0.0, 0.0
    m = g < 0
    sv[m], g[m] = s2[m], 0.0
    sv = np.maximum(sv, EPS)
    g = np.minimum(g, 100.0)
    num = np.log2(1.0 + g * g * s1 / (sv + 2.0))
    den = np.log2(1.0 + s1 / 2.0)
    num[s12 < 0] = 0.0
    m = s1 < 2.0
    num[m] = 1.0 - s2[m] * 4.0 / 65025.0
    den[m] = 1.0
    return num, den


def terms(a, b, depth, separable=False):
    """[4][2]: sum of num and sum of den of every scale of planes a (reference)
    and b; NaN for a scale that does not exist and every later one."""
    out = np.full((SCALES, 2), np.nan)
    la, lb = levels(a, depth, separable), levels(b, depth, separable)
    for s in range(len(la)):
        num, den = position_terms(*moments(la[s], lb[s], s, separable))
        out[s] = [float(num.sum()), float(den.sum())]
    return out


def terms_separable(a, b, depth):
    """The same values with every window applied along rows, then along columns."""
    return terms(a, b, depth, separable=True)


def near_branch(a, b, depth):
    """Per scale, the number of positions that sit on one of the spec's
    branches: sigma1^2 within 1e-6 of 2, sigma1^2 or sigma2^2 within 1e-12 of
    eps, g (before the branches) or sigma12 within 1e-9 of 0.  num jumps there,
    so two correct evaluations may differ by up to 1 per such position: an input
    of a tolerance comparison must have none."""
    la, lb = levels(a, depth), levels(b, depth)
    out = []
    for s in range(len(la)):
        s1, s2, s12 = moments(la[s], lb[s], s)
        g = s12 / (s1 + EPS)
        hit = (np.abs(s1 - 2.0) <= 1e-6) | (np.abs(s1 - EPS) <= 1e-12) | (np.abs(s2 - EPS) <= 1e-12) \
            | (np.abs(g) <= 1e-9) | (np.abs(s12) <= 1e-9)
        out.append(int(hit.sum()))
    return out


def pool(t):
    """(vif_scales [4], vif) of one frame's [4][2] sums, in plain Python floats."""
    scales = []
    for num, den in t:
        scales.append(math.nan if math.isnan(num) or math.isnan(den) else 1.0 if den == 0 else float(num) / float(den))
    if any(math.isnan(v) for v in scales):
        return scales, math.nan
    sn, sd = sum(float(r[0]) for r in t), sum(float(r[1]) for r in t)
    return scales, 1.0 if sd == 0 else sn / sd


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
        return a, np.clip(a + rng.integers(-(top // 32), top // 32 + 1, (h, w)), 0, top)
    if name == "smooth_noise":  # flat enough for sigma1^2 < 2 at places, noisy elsewhere
        a = np.rint(top * (0.5 + 0.4 * np.sin(xx / 37.0) * np.cos(yy / 23.0))).astype(np.int64)
        return a, np.clip(a + rng.integers(-(top // 16), top // 16 + 1, (h, w)), 0, top)
    raise ValueError(name)
