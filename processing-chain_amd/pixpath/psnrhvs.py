"""Host side of PSNR-HVS / PSNR-HVS-M (spec PP-HVS-1): the tables, the block
geometry, the pooling of the sums and the clip values.

pp_psnr_hvs (ops.psnr_hvs) gives, per distorted frame and plane, the sums
S_hvs and S_hvsm of the contrast-sensitivity-weighted squared DCT differences
over the plane's 8 x 8 blocks, without and with between-coefficient masking.
This module turns them into ``mse_hvs_*``, ``mse_hvsm_*``, ``psnr_hvs_*`` and
``psnr_hvsm_*`` for ``y``, ``u``, ``v`` and ``all`` in numpy, importable
without a GPU.  The model is the published psnrhvsm definition (Ponomarenko
et al. 2007) and libvmaf's ``psnr_hvs`` feature as recalled; parity with both
is unpinned: neither exists to compare with.
"""
import numpy as np

from .clips import nan_mean

SPEC = ("PP-HVS-1 (PSNR-HVS / PSNR-HVS-M over 8 x 8 DCT blocks, the grey-picture tables on all three planes, "
        "parity with libvmaf's psnr_hvs and with the published psnrhvsm unpinned)")
STEPS = (8, 7)            # the published definition and default; the overlap libvmaf is recalled to use
N = 8                     # a block's rows and columns
PLANES = ("y", "u", "v")
WEIGHTS = (0.8, 0.1, 0.1)  # of mse_y, mse_u, mse_v in mse_all
KINDS = ("hvs", "hvsm")
KEYS = tuple("%s_%s_%s" % (q, kind, name) for q in ("mse", "psnr") for kind in KINDS for name in PLANES + ("all",))
# JPEG Annex K luminance quantisation table
Q = np.array([[16, 11, 10, 16, 24, 40, 51, 61],
              [12, 12, 14, 19, 26, 58, 60, 55],
              [14, 13, 16, 24, 40, 57, 69, 56],
              [14, 17, 22, 29, 51, 87, 80, 62],
              [18, 22, 37, 56, 68, 109, 103, 77],
              [24, 35, 55, 64, 81, 104, 113, 92],
              [49, 64, 78, 87, 103, 121, 120, 101],
              [72, 92, 95, 98, 112, 100, 103, 99]], dtype=np.float64)
# the published six-decimal contrast-sensitivity table: 25.735088 / Q rounded to six decimals everywhere but at
# [0][1], where the publication has 2.339554 and the quotient 2.3395535
CSF = np.array([[1.608443, 2.339554, 2.573509, 1.608443, 1.072295, 0.643377, 0.504610, 0.421887],
                [2.144591, 2.144591, 1.838221, 1.354478, 0.989811, 0.443708, 0.428918, 0.467911],
                [1.838221, 1.979622, 1.608443, 1.072295, 0.643377, 0.451493, 0.372972, 0.459555],
                [1.838221, 1.513829, 1.169777, 0.887417, 0.504610, 0.295806, 0.321689, 0.415082],
                [1.429727, 1.169777, 0.695543, 0.459555, 0.378457, 0.236102, 0.249855, 0.334222],
                [1.072295, 0.735288, 0.467911, 0.402111, 0.317717, 0.247453, 0.227744, 0.279729],
                [0.525206, 0.402111, 0.329937, 0.295806, 0.249855, 0.212687, 0.214459, 0.254803],
                [0.357432, 0.279729, 0.270896, 0.262603, 0.229778, 0.257351, 0.249855, 0.259950]])
MASK = (10.0 / Q) * (10.0 / Q)    # the published masking table to 5e-7
# kernel geometry (csrc/psnrhvs.hip), for tests that place sizes on its seams
BLOCK_LANES = 8          # lanes that own a block
GROUP_BLOCKS = 32        # kHvsGroupBlocks: consecutive blocks of a block row a workgroup owns
FRAMES_PER_LAUNCH = 256  # kFrameMap (csrc/analysis_host.hpp)


def dct_matrix():
    """C[k][n] = c(k) cos((2n + 1) k pi / 16), c(0) = sqrt(1/8), else 1/2: the
    orthonormal 8-point DCT-II; D(X) = C X C^T."""
    k, n = np.arange(N, dtype=np.float64)[:, None], np.arange(N, dtype=np.float64)[None, :]
    c = np.where(k == 0, np.sqrt(1.0 / N), 0.5)
    return c * np.cos((2.0 * n + 1.0) * k * np.pi / 16.0)


def check_step(step):
    if int(step) not in STEPS or int(step) != step:
        raise ValueError("step must be 8 or 7 (got %r)" % (step,))
    return int(step)


def blocks_axis(n, step=8):
    """Blocks along an axis of n samples: origins i step with i step + 8 <= n."""
    return 0 if n < N else (int(n) - N) // check_step(step) + 1


def tile_width(step=8):
    """Samples a workgroup's GROUP_BLOCKS blocks span: the next sample but
    ``step - 8`` more starts the next workgroup's first block."""
    return (GROUP_BLOCKS - 1) * check_step(step) + N


def blocks(fmt, w, h, step=8):
    """The number of blocks of each of the three planes of a w x h frame."""
    from . import formats
    return tuple(blocks_axis(c, step) * blocks_axis(r, step) for r, c in formats.plane_shapes(formats.fmt(fmt), w, h))


def _psnr(mse, peak):
    """10 log10(peak^2 / MSE); NaN (absent) where MSE is 0 or undefined."""
    mse = np.asarray(mse, dtype=np.float64)
    out = np.full(mse.shape, np.nan)
    ok = mse > 0
    out[ok] = 10.0 * np.log10(peak * peak / mse[ok])
    return out


def pool(terms, fmt, w, h, step=8):
    """The per-frame arrays by key (float64 [N]) of pp_psnr_hvs' [N, 3, 2]:
    mse = S / (64 blocks) per plane, NaN for a plane with no block; ``all``
    from 0.8 mse_y + 0.1 (mse_u + mse_v), NaN if any plane has none; psnr = 10
    log10(peak^2 / mse), NaN where mse is 0 or NaN."""
    from . import formats
    t = np.asarray(terms, dtype=np.float64).reshape(-1, 3, 2)
    nb = blocks(fmt, w, h, step)
    peak = float((1 << formats.fmt(fmt).depth) - 1)
    res = {}
    for j, kind in enumerate(KINDS):
        for p, name in enumerate(PLANES):
            res["mse_%s_%s" % (kind, name)] = t[:, p, j] / (64.0 * nb[p]) if nb[p] else np.full(t.shape[0], np.nan)
        y, u, v = (res["mse_%s_%s" % (kind, name)] for name in PLANES)
        res["mse_%s_all" % kind] = WEIGHTS[0] * y + WEIGHTS[1] * (u + v)
        for name in PLANES + ("all",):
            res["psnr_%s_%s" % (kind, name)] = _psnr(res["mse_%s_%s" % (kind, name)], peak)
    return {key: res[key] for key in KEYS}


def summarize(terms, w, h, matched=None, fmt="yuv420p", step=8):
    """pool's per-frame arrays from pp_psnr_hvs' output, plus ``mean``: the clip
    values (the mean MSE over the frames that have one and the PSNR of that
    mean, PP-METRIC-1's rule), ``hvs_step`` and ``hvs_blocks`` (per plane).
    ``matched`` (bool [N]): the other frames have no reference frame and are
    NaN."""
    from . import formats
    t = np.array(terms, dtype=np.float64).reshape(-1, 3, 2)
    if matched is not None:
        t[~np.asarray(matched, dtype=bool)] = np.nan
    res = pool(t, fmt, w, h, step)
    peak = float((1 << formats.fmt(fmt).depth) - 1)
    mean = {}
    for key in KEYS:
        if key.startswith("mse_"):
            mean[key] = nan_mean(res[key])
            mean["psnr_" + key[4:]] = float(_psnr(mean[key], peak))
    mean = {key: mean[key] for key in KEYS}
    mean["hvs_step"] = check_step(step)
    mean["hvs_blocks"] = list(blocks(fmt, w, h, step))
    res["mean"] = mean
    return res
