"""Host side of MS-SSIM (spec PP-MSSSIM-1): the exponents and the pooling.

pp_ms_ssim (ops.ms_ssim) gives, per distorted frame and scale, the mean of cs
and of l * cs over the scale's 11 x 11 Gaussian windows; this module turns the
ten values of a frame into MS-SSIM after Wang, Simoncelli & Bovik 2003 and
into the Gaussian-window SSIM of scale 0.  Parity with libvmaf's float_ms_ssim
is unpinned.
"""
import numpy as np

from .clips import nan_mean

SCALES = 5
EXPONENTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WINDOW = 11        # kMsTaps: side of the Gaussian window
SIGMA = 1.5
MIN_SIZE = WINDOW << (SCALES - 1)  # 176: the smallest width and height with a window on every scale
# kernel geometry (csrc/msssim.hip), for tests that place sizes on its seams
TILE_COLS = 256    # kMsTileCols: window columns of a workgroup's tile, one per lane
WAVE_COLS = 64     # of one wave
BAND_ROWS = 64     # kMsBandRows: window rows of a tile
FRAMES_PER_LAUNCH = 256  # kFrameMap (csrc/analysis_host.hpp)


def window():
    """The 11 normalised weights g[i] = exp(-(i - 5)^2 / 4.5) / sum, fp64."""
    g = np.exp(-((np.arange(WINDOW) - WINDOW // 2) ** 2) / (2 * SIGMA * SIGMA))
    return g / g.sum()


def pool(terms):
    """MS-SSIM of pp_ms_ssim's per-scale means ([..., 5, 2]: cs, ssim):
    prod_{s<4} max(cs_s, 0)^e_s * max(ssim_4, 0)^e_4.  A negative mean is
    clamped to 0 (the spec's choice where implementations of the paper
    differ); NaN if any scale has no window."""
    t = np.asarray(terms, dtype=np.float64)
    if t.shape[-2:] != (SCALES, 2):
        raise ValueError("terms must be [..., 5, 2]")
    v = np.concatenate([t[..., :SCALES - 1, 0], t[..., SCALES - 1:, 1]], axis=-1)
    bad = np.isnan(t).any(axis=(-2, -1))
    with np.errstate(invalid="ignore"):
        out = np.prod(np.maximum(v, 0.0) ** np.array(EXPONENTS), axis=-1)
    return np.where(bad, np.nan, out)


def summarize(terms, matched=None):
    """Per-frame arrays ``ms_ssim_y``, ``ssim_gauss_y`` (float64 [N]),
    ``cs_scales_y`` and ``ssim_scales_y`` ([N, 5]) from pp_ms_ssim's output,
    plus ``mean``: the clip values of the first two, over the frames that have
    one.  ``matched`` (bool [N]): the other frames have no reference frame and
    are NaN."""
    t = np.array(terms, dtype=np.float64).reshape(-1, SCALES, 2)
    if matched is not None:
        t[~np.asarray(matched, dtype=bool)] = np.nan
    res = {"ms_ssim_y": pool(t).reshape(-1), "ssim_gauss_y": t[:, 0, 1].copy(),
           "cs_scales_y": t[:, :, 0].copy(), "ssim_scales_y": t[:, :, 1].copy()}
    res["mean"] = {key: nan_mean(res[key]) for key in ("ms_ssim_y", "ssim_gauss_y")}
    return res
