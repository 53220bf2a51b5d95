"""numpy restatement of spec PP-ADM-1, written from the spec text
in the direct 2-D form: every coefficient as the 4 x 4 samples of the
`reflect`-padded level under the outer product of its two filters, the masking
neighbourhoods by sliding_window_view.  It shares nothing with the kernel's
separable order (csrc/adm.hip).  `dtype` selects the arithmetic (float64,
longdouble, float32) and `separable` a rows-then-columns evaluation of the
transform: the three evaluations whose spread sets the bar, and the fp32 one
that must fall outside it."""
import math

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

SCALES = 4
AMPLITUDES = ((0.67234, 0.72709), (0.41317, 0.49428), (0.22727, 0.28688), (0.11792, 0.15214))
NEAR = 1e-9  # distance of the angle from one degree, relative to it, that near_branch reports


def filters(dtype=np.float64):
    t = np.dtype(dtype).type
    r3 = np.sqrt(t(3))
    lo = np.array([1 + r3, 3 + r3, 3 - r3, 1 - r3], dtype=dtype) / (t(4) * np.sqrt(t(2)))
    return lo, np.array([lo[3], -lo[2], lo[1], -lo[0]], dtype=dtype)


def rf(dtype=np.float64):
    """[4][3] contrast sensitivity rf[s][theta] = 1 / Q(s, theta), theta = H, V, D."""
    t = np.dtype(dtype).type
    pi = t(np.pi) if dtype != np.longdouble else np.arctan(t(1)) * t(4)
    r = t(3) * t(1080) * pi / t(180)
    out = np.empty((SCALES, 3), dtype=dtype)
    for s in range(SCALES):
        for th in range(3):
            g = t("0.534") if th == 2 else t(1)
            lg = np.log10(t(2) ** (s + 1) * t("0.401") * g / r)
            q = t(2) * t("0.495") * t(10) ** (t("0.466") * lg * lg) / t(repr(AMPLITUDES[s][th == 2]))
            out[s, th] = t(1) / q
    return out


def cos2(dtype=np.float64):
    t = np.dtype(dtype).type
    if dtype == np.float64:
        return math.cos(math.pi / 180.0) ** 2
    pi = np.arctan(t(1)) * t(4)
    return np.cos(pi / t(180)) ** 2


def margin(n):
    return max(1, (n - 5) // 10)


def exists(p):
    h, w = p.shape
    return min(w, h, (w + 1) // 2, (h + 1) // 2) >= 3


def bands(p, separable=False):
    """(A, H, V, D) of level p: output (i, j) reads rows 2i - 1 .. 2i + 2 and
    columns 2j - 1 .. 2j + 2 of the mirrored level.  H = hi vertically, lo
    horizontally; V = lo vertically, hi horizontally."""
    lo, hi = filters(p.dtype)
    h, w = p.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    q = np.pad(p, ((1, 2), (1, 2)), mode="reflect")
    if separable:  # along the rows first, then down the columns
        def horiz(f):
            return sum(f[k] * q[:, k:k + 2 * wo:2] for k in range(4))

        def vert(x, f):
            return sum(f[k] * x[k:k + 2 * ho:2] for k in range(4))
        L, Hh = horiz(lo), horiz(hi)
        return vert(L, lo), vert(L, hi), vert(Hh, lo), vert(Hh, hi)
    win = sliding_window_view(q, (4, 4))[0:2 * ho:2, 0:2 * wo:2]
    return tuple(np.einsum("ijkl,kl->ij", win, np.outer(fv, fh)) for fv, fh in ((lo, lo), (hi, lo), (lo, hi), (hi, hi)))


def decouple(o, t, c2):
    """(r, a, angle) of the three bands o, t ([3][h][w]: H, V, D)."""
    one, zero = o.dtype.type(1), o.dtype.type(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(o == 0, zero, np.clip(t / np.where(o == 0, one, o), zero, one))
    r = k * o
    a = t - r
    dp = o[0] * t[0] + o[1] * t[1]
    om = o[0] * o[0] + o[1] * o[1]
    tm = t[0] * t[0] + t[1] * t[1]
    angle = (dp >= 0) & (dp * dp >= c2 * om * tm)
    r = np.where(angle, t, r)
    a = np.where(angle, zero, a)
    return r, a, angle


def scale_sums(o, t, s, dtype):
    """The six sums of scale s from its bands o, t ([3][h][w])."""
    w = rf(dtype)[s]
    r, a, _ = decouple(o, t, cos2(dtype))
    hs, ws = o.shape[1:]
    mh, mw = margin(hs), margin(ws)
    ty = np.dtype(dtype).type
    M = np.zeros((hs - 2, ws - 2), dtype=dtype)  # of the positions that have all eight neighbours
    for th in range(3):
        m = np.abs(w[th] * a[th])
        nb = sliding_window_view(m, (3, 3)).sum(axis=(2, 3)) - m[1:-1, 1:-1]
        M = M + (nb / ty(30) + m[1:-1, 1:-1] / ty(15))
    M = M[mh - 1:hs - mh - 1, mw - 1:ws - mw - 1]
    out = []
    for th in range(3):
        x = np.maximum(np.abs(w[th] * r[th])[mh:hs - mh, mw:ws - mw] - M, ty(0))
        out.append((x * x * x).sum())
    for th in range(3):
        y = np.abs(w[th] * o[th])[mh:hs - mh, mw:ws - mw]
        out.append((y * y * y).sum())
    return out


def levels(a, b, depth, dtype=np.float64, separable=False):
    """[(o, t)] of the scales that exist: the H, V, D bands of both planes."""
    ty = np.dtype(dtype).type
    pa, pb = (np.asarray(x).astype(dtype) / ty(1 << (depth - 8)) for x in (a, b))
    out = []
    for s in range(SCALES):
        if not exists(pa):
            break
        ba, bb = bands(pa, separable), bands(pb, separable)
        out.append((np.stack(ba[1:]), np.stack(bb[1:])))
        pa, pb = ba[0], bb[0]
    return out


def terms(a, b, depth, dtype=np.float64, separable=False):
    """[4][6]: the six sums of every scale of planes a (reference) and b; NaN
    for a scale that does not exist and every later one."""
    out = np.full((SCALES, 6), np.nan, dtype=dtype)
    for s, (o, t) in enumerate(levels(a, b, depth, dtype, separable)):
        out[s] = scale_sums(o, t, s, dtype)
    return out


def coef_rounding(s, peak):
    """Bound on the absolute rounding error of an fp64 coefficient of scale s
    from samples of magnitude <= peak (8-bit scale): its level's input is at
    most 2^s peak (the low-pass gain is 2 a level), a coefficient is two dot
    products of four taps (sum |f| = 1.93 each way, four roundings of 2^-53
    each), so 8 * 2^-53 * 1.93^2 * 2^s peak < 32 * 2^-53 * 2^(s + 1) peak with a
    factor 2 to spare."""
    return 32.0 * 2.0 ** -53 * 2.0 ** (s + 1) * peak


def near_branch(a, b, depth):
    """Per scale, the number of positions whose angle test is within reach of
    flipping.  The test compares the angle theta between (o_H, o_V) and (t_H,
    t_V) with one degree; a position counts if |theta - 1 deg| <= NEAR * 1 deg
    + u / |o| + u / |t|, u = coef_rounding: the angle a rounding-level change
    of the coefficients can turn either vector by.  A vector at rounding level
    (a flat or purely diagonal neighbourhood: zero in exact arithmetic) has no
    direction, so such a position always counts.  r and a jump there, so two
    correct evaluations may differ by a whole coefficient per such position:
    an input of a tolerance comparison must have none."""
    out = []
    peak = float(max(np.max(a), np.max(b))) / float(1 << (depth - 8))
    deg = math.pi / 180.0
    for s, (o, t) in enumerate(levels(a, b, depth)):
        u = coef_rounding(s, max(peak, 1.0))
        dp = o[0] * t[0] + o[1] * t[1]
        no, nt = np.hypot(o[0], o[1]), np.hypot(t[0], t[1])
        with np.errstate(divide="ignore", invalid="ignore"):
            theta = np.arccos(np.clip(dp / (no * nt), -1.0, 1.0))
            slack = NEAR * deg + u / no + u / nt
            hit = ~(np.abs(theta - deg) > slack)  # NaN (a zero vector) counts
        out.append(int(hit.sum()))
    return out


def areas(w, h):
    out = []
    for s in range(SCALES):
        ws, hs = (w + 1) // 2, (h + 1) // 2
        if min(w, h, ws, hs) < 3:
            break
        out.append((ws - 2 * margin(ws)) * (hs - 2 * margin(hs)))
        w, h = ws, hs
    return out + [math.nan] * (SCALES - len(out))


def pool(t, w, h):
    """(adm_scales [4], adm2) of one frame's [4][6] sums, in plain Python floats."""
    nums, dens = [], []
    for row, area in zip(t, areas(w, h)):
        c = math.nan if math.isnan(area) else (area / 32.0) ** (1.0 / 3.0)
        nums.append(sum(float(np.cbrt(v)) for v in row[:3]) + 3 * c)
        dens.append(sum(float(np.cbrt(v)) for v in row[3:]) + 3 * c)
    scales = [n / d for n, d in zip(nums, dens)]
    return scales, sum(nums) / sum(dens)


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
    if name == "smooth_noise":  # a dithered smooth reference: flat runs would leave H = V = 0, no direction
        a = np.rint(top * (0.5 + 0.4 * np.sin(xx / 37.0) * np.cos(yy / 23.0))).astype(np.int64)
        a = a + rng.integers(-2, 3, (h, w))
        return a, np.clip(a + rng.integers(-(top // 16), top // 16 + 1, (h, w)), 0, top)
    if name == "blur":  # the detail loss ADM is meant for: a 3 x 3 box blur of noise
        a = rng.integers(0, top + 1, (h, w))
        q = np.pad(a, 1, mode="edge")
        return a, sliding_window_view(q, (3, 3)).sum(axis=(2, 3)) // 9
    if name == "checker":  # inverse 1-pixel checkerboards, each under a little noise of its own: a pure
        # checkerboard has H = V = 0 in exact arithmetic, and the angle test no direction to judge
        a = np.where((xx + yy) & 1, top - top // 8, top // 8)
        n = top // 16 + 1
        return a + rng.integers(-n, n + 1, (h, w)), top - a + rng.integers(-n, n + 1, (h, w))
    raise ValueError(name)
