"""Host side of pixel-domain VIF (spec PP-VIF-1): the windows and the pooling.

pp_vif (ops.vif) gives, per distorted frame and scale, the pair (sum num, sum
den) over every sample position of the scale; this module turns the eight
values of a frame into the four per-scale ratios and the combined VIF, in the
form VMAF uses as its vif_scale0..3 features (Sheikh & Bovik 2006).  Parity
with libvmaf's float_vif is unpinned.
"""
import numpy as np

from .clips import nan_mean

SCALES = 4
TAPS = (17, 9, 5, 3)   # filter length of scale s; sigma = taps / 5
MIN_SIZE = 16          # the smallest width and height with all four scales
EPS = 1e-10
SIGMA_NSQ = 2.0
# kernel geometry (csrc/vif.hip), for tests that place sizes on its seams
TILE_COLS = 256        # kVifTileCols: columns of a workgroup's tile, one per lane
WAVE_COLS = 64         # of one wave
BAND_ROWS = 64         # kVifBandRows: rows of a statistics tile
DEC_BAND_ROWS = 32     # kVifDecRows: output rows of a decimation tile (its columns: TILE_COLS)
FRAMES_PER_LAUNCH = 256  # kFrameMap (csrc/analysis_host.hpp)


def window(s):
    """The TAPS[s] normalised weights g[i] = exp(-(i - N//2)^2 / (2 (N/5)^2)) / sum, fp64."""
    n = TAPS[s]
    sigma = n / 5.0
    g = np.exp(-((np.arange(n) - n // 2) ** 2) / (2.0 * sigma * sigma))
    return g / g.sum()


def scale_sizes(w, h):
    """[(w_s, h_s)] of the scales that exist for a w x h plane: w_s = w >> s, and
    a scale needs N_s // 2 + 1 samples each way; the first missing one ends the list."""
    out = []
    for s in range(SCALES):
        ws, hs = w >> s, h >> s
        if ws < TAPS[s] // 2 + 1 or hs < TAPS[s] // 2 + 1:
            break
        out.append((ws, hs))
    return out


def pool(terms):
    """(vif_scales [..., 4], vif [...]) of pp_vif's sums ([..., 4, 2]: num, den):
    vif_scale_s = num_s / den_s (1.0 where den_s == 0), NaN for a scale that
    does not exist; vif = sum num / sum den over the four scales (1.0 where the
    sum of den is 0), NaN if any scale is NaN."""
    t = np.asarray(terms, dtype=np.float64)
    if t.shape[-2:] != (SCALES, 2):
        raise ValueError("terms must be [..., 4, 2]")

    def ratio(num, den):
        zero = den == 0
        with np.errstate(invalid="ignore"):
            return np.where(zero, np.where(np.isnan(num), np.nan, 1.0), num / np.where(zero, 1.0, den))
    return ratio(t[..., 0], t[..., 1]), ratio(t[..., 0].sum(axis=-1), t[..., 1].sum(axis=-1))


def summarize(terms, matched=None):
    """Per-frame arrays ``vif_y`` (float64 [N]) and ``vif_scales_y`` ([N, 4])
    from pp_vif's output, plus ``mean``: the clip values of both, over the
    frames that have one.  ``matched`` (bool [N]): the other frames have no
    reference frame and are NaN."""
    t = np.array(terms, dtype=np.float64).reshape(-1, SCALES, 2)
    if matched is not None:
        t[~np.asarray(matched, dtype=bool)] = np.nan
    scales, vif = pool(t)
    res = {"vif_y": vif.reshape(-1), "vif_scales_y": scales.reshape(-1, SCALES)}
    res["mean"] = {"vif_y": nan_mean(res["vif_y"]),
                   "vif_scales_y": [nan_mean(res["vif_scales_y"][:, s]) for s in range(SCALES)]}
    return res
