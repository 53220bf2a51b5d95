"""Host side of the CIEDE2000 colour difference (spec PP-CIEDE-1): the kernel's
geometry, the pooling of the sums and the clip values.

pp_ciede (ops.ciede) gives, per distorted frame, the sum of the dE00 of every
luma position against its reference frame and the largest of them.  This
module turns the two into the mean colour difference ``delta_e``, the largest
``delta_e_max`` and the score on libvmaf's scale, ``ciede2000`` = min(45 - 20
log10(delta_e), 100), in numpy, importable without a GPU.  The conversion and
the formula (Sharma, Wu, Dalal 2005) are the spec's text; parity with
libvmaf's ``ciede`` feature is unpinned: no libvmaf exists to compare with
(DESIGN.md).
"""
import numpy as np

from .clips import nan_mean

SPEC = "PP-CIEDE-1 (CIEDE2000 of BT.709 limited-range Y'CbCr, nearest chroma, parity with libvmaf unpinned)"
WEIGHTS = (1.0, 1.0, 1.0)   # kL, kC, kH of the CIE
SCORE_CAP = 100.0           # ciede2000 of delta_e = 0 and of every delta_e below 10^-2.75
KEYS = ("delta_e", "delta_e_max", "ciede2000")
# kernel geometry (csrc/ciede.hip), for tests that place sizes on its seams
PIECE_BYTES = 16         # kCiePieceBytes: a lane's piece of a chroma row
LANES = 64               # kCieLanes: chroma pieces a wave, and a workgroup, is wide
WAVES = 4                # kCieWaves: waves of a workgroup, one below the other
WAVE_ROWS = 4            # kCieWaveRows: chroma rows a wave walks
FRAMES_PER_LAUNCH = 256  # kFrameMap (csrc/analysis_host.hpp)


def spans(fmt):
    """(lane, wave, wave_rows, band_rows) of a format in luma samples and
    rows: the columns a lane and a wave (= a workgroup) own, the rows a wave
    and a workgroup own."""
    from . import formats
    f = formats.fmt(fmt)
    lane = (PIECE_BYTES // f.bytes_per_sample) << f.hsub
    return lane, lane * LANES, WAVE_ROWS << f.vsub, (WAVE_ROWS * WAVES) << f.vsub


def parse_weights(text):
    """(kL, kC, kH) of the option text "KL,KC,KH": three positive finite numbers."""
    try:
        v = tuple(float(x) for x in str(text).split(","))
    except ValueError:
        v = ()
    if len(v) != 3 or not all(np.isfinite(x) and x > 0 for x in v):
        raise ValueError("weights must be KL,KC,KH: three positive numbers (got %r)" % (text,))
    return v


def score(delta_e):
    """min(45 - 20 log10(delta_e), 100); 100 for delta_e = 0, NaN for NaN."""
    d = np.asarray(delta_e, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d > 0, np.minimum(45.0 - 20.0 * np.log10(np.where(d > 0, d, 1.0)), SCORE_CAP),
                        np.where(d == 0, SCORE_CAP, np.nan))


def pool(out, w, h):
    """(delta_e [N], delta_e_max [N], ciede2000 [N]) of pp_ciede's [N, 2] (sum,
    max) of w x h frames, float64."""
    t = np.asarray(out, dtype=np.float64).reshape(-1, 2)
    de = t[:, 0] / (float(w) * float(h))
    return de, t[:, 1].copy(), score(de)


def summarize(out, w, h, matched=None):
    """Per-frame arrays ``delta_e``, ``delta_e_max`` and ``ciede2000`` (float64
    [N]) from pp_ciede's output, plus ``mean``: the clip values (the means over
    the frames that have one; ``delta_e_max`` the largest).  ``matched`` (bool
    [N]): the other frames have no reference frame and are NaN."""
    t = np.array(out, dtype=np.float64).reshape(-1, 2)
    if matched is not None:
        t[~np.asarray(matched, dtype=bool)] = np.nan
    res = dict(zip(KEYS, pool(t, w, h)))
    mx = res["delta_e_max"][~np.isnan(res["delta_e_max"])]
    res["mean"] = {"delta_e": nan_mean(res["delta_e"]), "delta_e_max": float(mx.max()) if mx.size else float("nan"),
                   "ciede2000": nan_mean(res["ciede2000"])}
    return res
