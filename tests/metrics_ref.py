"""Numpy restatement of spec PP-METRIC-1, written from the spec:
exact int64 sums, fp64 quotients.  The reference the GPU kernel is held to."""
import numpy as np


def plane_sse(a, b):
    """Sum of squared differences over every sample (exact Python int)."""
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


def plane_ssim(a, b, depth):
    """Mean SSIM over the 8x8 windows at stride 4 built from 4x4 block sums;
    NaN when the plane has fewer than 2 x 2 blocks."""
    ph, pw = a.shape
    bw, bh = pw >> 2, ph >> 2
    if bw < 2 or bh < 2:
        return float("nan")
    a = a[:bh * 4, :bw * 4].astype(np.int64).reshape(bh, 4, bw, 4)
    b = b[:bh * 4, :bw * 4].astype(np.int64).reshape(bh, 4, bw, 4)

    def windows(v):  # block sums, then the 2x2 groups of adjacent blocks
        s = v.sum(axis=(1, 3))
        return s[:-1, :-1] + s[:-1, 1:] + s[1:, :-1] + s[1:, 1:]

    s1, s2 = windows(a), windows(b)
    ss, s12 = windows(a * a + b * b), windows(a * b)
    mx = float((1 << depth) - 1)
    c1 = .01 * .01 * mx * mx * 64
    c2 = .03 * .03 * mx * mx * 64 * 63
    vars_ = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    assert vars_.dtype == np.int64 and covar.dtype == np.int64
    v = ((2 * s1 * s2).astype(np.float64) + c1) * ((2 * covar).astype(np.float64) + c2) / (
        ((s1 * s1 + s2 * s2).astype(np.float64) + c1) * (vars_.astype(np.float64) + c2))
    return float(v.mean())


def metrics(ref_planes, dist_planes, depth, ref_index=None):
    """ref_planes / dist_planes: lists of three [N, rows, cols] arrays.
    Returns (sse int64 [N, 3], ssim float64 [N, 3]); dist frame k against ref
    frame ref_index[k] (None: k)."""
    n = dist_planes[0].shape[0]
    idx = range(n) if ref_index is None else [int(i) for i in ref_index]
    sse = np.zeros((n, 3), np.int64)
    ssim = np.zeros((n, 3), np.float64)
    for k, r in enumerate(idx):
        for p in range(3):
            sse[k, p] = plane_sse(ref_planes[p][r], dist_planes[p][k])
            ssim[k, p] = plane_ssim(ref_planes[p][r], dist_planes[p][k], depth)
    return sse, ssim
