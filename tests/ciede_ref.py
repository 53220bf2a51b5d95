"""numpy float64 restatement of spec PP-CIEDE-1, vectorised and
written from the spec's text: limited-range BT.709 Y'CbCr -> R'G'B' clipped to
[0, 1] -> linear light (sRGB curve) -> XYZ (D65) over its white -> Lab ->
dE00 (Sharma, Wu, Dalal 2005).  Every step is in the order the spec writes.

``ciede`` also reports how far the nearest sample of its inputs sits from a
branch boundary of the dE00 formula (|h'_1 - h'_2| = 180 degrees, a hue sum of
360 degrees): two correct implementations may take different arms there, so
the tests keep their seeded inputs away from them."""
import numpy as np

RAD = 0.017453292519943295  # pi / 180
DEG = 57.29577951308232     # 180 / pi
P25_7 = 6103515625.0        # 25^7
WHITE = (0.95047, 1.0, 1.08883)
XYZ = ((0.4124564, 0.3575761, 0.1804375), (0.2126729, 0.7151522, 0.0721750), (0.0193339, 0.1191920, 0.9503041))


def _linear(c):
    c = np.minimum(np.maximum(c, 0.0), 1.0)
    return np.where(c <= 0.04045, c / 12.92, np.power((c + 0.055) / 1.055, 2.4))


def _f(t):
    return np.where(t > 216.0 / 24389.0, np.cbrt(t), (24389.0 / 27.0 * t + 16.0) / 116.0)


def lab(Y, U, V, depth):
    """(L, a, b) of code values (arrays of one shape), steps 1 .. 5."""
    s = float(1 << (depth - 8))
    y = (np.asarray(Y, np.float64) - 16.0 * s) / (219.0 * s)
    cb = (np.asarray(U, np.float64) - 128.0 * s) / (224.0 * s)
    cr = (np.asarray(V, np.float64) - 128.0 * s) / (224.0 * s)
    r = _linear(y + 1.5748 * cr)
    g = _linear((y - 0.1873 * cb) - 0.4681 * cr)
    b = _linear(y + 1.8556 * cb)
    f = [_f(((m[0] * r + m[1] * g) + m[2] * b) / wp) for m, wp in zip(XYZ, WHITE)]
    return 116.0 * f[1] - 16.0, 500.0 * (f[0] - f[1]), 200.0 * (f[1] - f[2])


def _pow7(x):
    x2 = x * x
    x4 = x2 * x2
    return (x4 * x2) * x


def _hue(b, a):
    h = np.arctan2(b, a) * DEG
    h = np.where(h < 0.0, h + 360.0, h)
    return np.where((a == 0.0) & (b == 0.0), 0.0, h)


def de00(L1, a1, b1, L2, a2, b2, weights=(1.0, 1.0, 1.0), with_margin=False):
    """dE00 of Lab pairs (arrays of one shape), step 6.  with_margin: also the
    distance in degrees of every pair from the nearest branch boundary (inf for
    a pair with C'_1 C'_2 = 0, which has none)."""
    kL, kC, kH = (float(v) for v in weights)
    L1, a1, b1, L2, a2, b2 = (np.asarray(v, np.float64) for v in (L1, a1, b1, L2, a2, b2))
    C1, C2 = np.sqrt(a1 * a1 + b1 * b1), np.sqrt(a2 * a2 + b2 * b2)
    Cb7 = _pow7((C1 + C2) / 2.0)
    G = 0.5 * (1.0 - np.sqrt(Cb7 / (Cb7 + P25_7)))
    ap1, ap2 = (1.0 + G) * a1, (1.0 + G) * a2
    Cp1, Cp2 = np.sqrt(ap1 * ap1 + b1 * b1), np.sqrt(ap2 * ap2 + b2 * b2)
    h1, h2 = _hue(b1, ap1), _hue(b2, ap2)
    dL, dC = L2 - L1, Cp2 - Cp1
    CC, hs, hd = Cp1 * Cp2, h1 + h2, h2 - h1
    zero = CC == 0.0
    dh = np.where(zero, 0.0, np.where(hd > 180.0, hd - 360.0, np.where(hd < -180.0, hd + 360.0, hd)))
    hb = np.where(zero, hs, np.where(np.abs(h1 - h2) <= 180.0, hs / 2.0,
                                     np.where(hs < 360.0, (hs + 360.0) / 2.0, (hs - 360.0) / 2.0)))
    dH = 2.0 * np.sqrt(CC) * np.sin(dh / 2.0 * RAD)
    Lb, Cb = (L1 + L2) / 2.0, (Cp1 + Cp2) / 2.0
    T = (((1.0 - 0.17 * np.cos((hb - 30.0) * RAD)) + 0.24 * np.cos(2.0 * hb * RAD))
         + 0.32 * np.cos((3.0 * hb + 6.0) * RAD)) - 0.20 * np.cos((4.0 * hb - 63.0) * RAD)
    e = (hb - 275.0) / 25.0
    dth = 30.0 * np.exp(-(e * e))
    Cq7 = _pow7(Cb)
    RC = 2.0 * np.sqrt(Cq7 / (Cq7 + P25_7))
    l50 = (Lb - 50.0) * (Lb - 50.0)
    SL = 1.0 + 0.015 * l50 / np.sqrt(20.0 + l50)
    SC = 1.0 + 0.045 * Cb
    SH = 1.0 + 0.015 * Cb * T
    RT = -np.sin(2.0 * dth * RAD) * RC
    tl, tc, th = dL / (kL * SL), dC / (kC * SC), dH / (kH * SH)
    de = np.sqrt(((tl * tl + tc * tc) + th * th) + RT * tc * th)
    if not with_margin:
        return de
    far = np.abs(np.abs(hd) - 180.0)
    # the hue-sum arm is looked at only where |h'_1 - h'_2| > 180
    far = np.where(np.abs(hd) > 180.0, np.minimum(far, np.abs(hs - 360.0)), far)
    return de, np.where(zero, np.inf, far)


def upsample(c, hsub, vsub, w, h):
    """A chroma plane [..., ch, cw] at the luma positions: [y >> vsub][x >> hsub]."""
    return c[..., (np.arange(h) >> vsub)[:, None], (np.arange(w) >> hsub)[None, :]]


def frame_de(ref, dist, fmt_depth, hsub, vsub, weights=(1.0, 1.0, 1.0)):
    """(dE00 [n, h, w], margin [n, h, w]) of two lists of planes [n, rows, cols] of equal n."""
    h, w = dist[0].shape[-2:]
    s = [(p[0], upsample(p[1], hsub, vsub, w, h), upsample(p[2], hsub, vsub, w, h)) for p in (ref, dist)]
    de, far = de00(*lab(*s[0], fmt_depth), *lab(*s[1], fmt_depth), weights=weights, with_margin=True)
    same = (s[0][0] == s[1][0]) & (s[0][1] == s[1][1]) & (s[0][2] == s[1][2])
    assert (de[same] == 0.0).all()  # the kernel's shortcut changes nothing
    return de, np.where(same, np.inf, far)


def ciede(ref, dist, depth, hsub, vsub, ref_index=None, weights=(1.0, 1.0, 1.0)):
    """(out [n, 2]: sum and max of dE00 per distorted frame, the smallest
    distance in degrees of any sample from a branch boundary) of pp_ciede's
    inputs: lists of three planes [n, rows, cols]."""
    n = dist[0].shape[0]
    idx = np.arange(n) if ref_index is None else np.asarray(ref_index, dtype=np.int64)
    de, far = frame_de([p[idx] for p in ref], dist, depth, hsub, vsub, weights)
    out = np.stack([de.reshape(n, -1).sum(axis=1), de.reshape(n, -1).max(axis=1)], axis=1) if n else np.zeros((0, 2))
    return out, float(far.min()) if far.size else float("inf")
