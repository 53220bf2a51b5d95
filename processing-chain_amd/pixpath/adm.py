"""Host side of the Additive / Detail-loss Metric (spec PP-ADM-1): the filters,
the contrast sensitivity, the geometry of the scales and the pooling.

pp_adm (ops.adm) gives, per distorted frame and scale, six sums over the
scale's region: the cubes of the masked restored coefficients of H, V, D and
the cubes of the weighted reference coefficients of H, V, D.  This module turns
the 24 values of a frame into adm_scale0..3 and adm2, in the form VMAF uses
(Li, Ngan et al. 2011).  Parity with libvmaf's float_adm is unpinned
(DESIGN.md).
"""
import math

import numpy as np

from .clips import nan_mean

SCALES = 4
SUMS = 6               # per scale: x^3 of H, V, D, then |rf o|^3 of H, V, D
MIN_SIZE = 33          # the smallest width and height with all four scales
# Watson's basis amplitudes of the 9/7 wavelet: [s] = (H and V, D)
AMPLITUDES = ((0.67234, 0.72709), (0.41317, 0.49428), (0.22727, 0.28688), (0.11792, 0.15214))
# kernel geometry (csrc/adm.hip), for tests that place sizes on its seams
TILE_COLS = 254        # kAdmTileCols: coefficient columns of a workgroup's tile (256 lanes less the halo)
WAVE_COLS = 64         # of one wave; the first wave's first lane is the halo
BAND_ROWS = 32         # kAdmBandRows: coefficient rows of a tile
FRAMES_PER_LAUNCH = 256  # kFrameMap (csrc/analysis_host.hpp)


def filters():
    """(lo, hi): the Daubechies-2 analysis pair, fp64."""
    r3 = math.sqrt(3.0)
    lo = np.array([1.0 + r3, 3.0 + r3, 3.0 - r3, 1.0 - r3]) / (4.0 * math.sqrt(2.0))
    return lo, np.array([lo[3], -lo[2], lo[1], -lo[0]])


def rf():
    """[4][3]: rf[s][theta] = 1 / Q(s, theta), theta = H, V, D, fp64."""
    r = 3.0 * 1080.0 * math.pi / 180.0
    out = np.empty((SCALES, 3))
    for s in range(SCALES):
        for th in range(3):
            g = 0.534 if th == 2 else 1.0
            lg = math.log10(2.0 ** (s + 1) * 0.401 * g / r)
            out[s, th] = 1.0 / (2.0 * 0.495 * 10.0 ** (0.466 * lg * lg) / AMPLITUDES[s][th == 2])
    return out


def scale_sizes(w, h):
    """[(w_s, h_s)] of the scales that exist for a w x h plane: a level halves
    its input rounding up, and a scale needs 3 samples each way in its input
    and in its bands; the first missing one ends the list."""
    out = []
    for _ in range(SCALES):
        ws, hs = (w + 1) // 2, (h + 1) // 2
        if min(w, h, ws, hs) < 3:
            break
        out.append((ws, hs))
        w, h = ws, hs
    return out


def margin(n):
    """Coefficients left out on either side of an axis of n: floor(0.1 n - 0.5), at least 1."""
    return max(1, (n - 5) // 10)


def areas(w, h):
    """[4] positions of the region of every scale of a w x h plane; NaN for one that does not exist."""
    out = [math.nan] * SCALES
    for s, (ws, hs) in enumerate(scale_sizes(w, h)):
        out[s] = float((ws - 2 * margin(ws)) * (hs - 2 * margin(hs)))
    return np.array(out)


def pool(terms, w, h):
    """(adm_scales [..., 4], adm2 [...]) of pp_adm's sums ([..., 4, 6]) of
    w x h planes: with c_s = (area_s / 32)^(1/3), num_s = sum over theta of the
    cube roots of the first three sums + 3 c_s, den_s the same of the last
    three; adm_scale_s = num_s / den_s, NaN for a scale that does not exist;
    adm2 = sum num / sum den over the four scales, NaN if any scale is NaN."""
    t = np.asarray(terms, dtype=np.float64)
    if t.shape[-2:] != (SCALES, SUMS):
        raise ValueError("terms must be [..., 4, 6]")
    c = 3.0 * np.cbrt(areas(w, h) / 32.0)
    root = np.cbrt(t)
    num = root[..., 0:3].sum(axis=-1) + c
    den = root[..., 3:6].sum(axis=-1) + c
    with np.errstate(invalid="ignore"):
        return num / den, num.sum(axis=-1) / den.sum(axis=-1)


def summarize(terms, w, h, matched=None):
    """Per-frame arrays ``adm2_y`` (float64 [N]) and ``adm_scales_y`` ([N, 4])
    from pp_adm's output, plus ``mean``: the clip values of both, over the
    frames that have one.  ``matched`` (bool [N]): the other frames have no
    reference frame and are NaN."""
    t = np.array(terms, dtype=np.float64).reshape(-1, SCALES, SUMS)
    if matched is not None:
        t[~np.asarray(matched, dtype=bool)] = np.nan
    scales, adm2 = pool(t, w, h)
    res = {"adm2_y": adm2.reshape(-1), "adm_scales_y": scales.reshape(-1, SCALES)}
    res["mean"] = {"adm2_y": nan_mean(res["adm2_y"]),
                   "adm_scales_y": [nan_mean(res["adm_scales_y"][:, s]) for s in range(SCALES)]}
    return res
