"""Host side of the banding measure (spec PP-BAND-1): the default window, the
pooling of the contrast-value histograms, the clip values and the banding of
one file.

pp_banding (ops.banding) gives, per shown frame and each of five scales, the
exact histogram of the contrast value Q of the scale's positions.  This module
turns the histograms into the per-frame banding index and the clip values, in
numpy, importable without a GPU.  The measure is modelled on CAMBI (Tandon et
al., PCS 2021) as recalled and defined by the spec's text alone: no display
model, integer contrast values; parity with libvmaf's CAMBI is unpinned
(DESIGN.md).
"""
import os

import numpy as np

SCALES = 5
BINS = 1024
SCALE_WEIGHTS = (16, 8, 4, 2, 1)  # sum 31
TOP_NUM, TOP_DEN = 3, 5           # the share of a scale's positions that is pooled: 0.6
MIN_WINDOW, MAX_WINDOW = 3, 63
# kernel geometry (csrc/banding.hip), for tests that place sizes on its seams
MASK_TILE_ROWS = 32      # kBdMaskRows: rows of a tile of the mask kernel
MASK_TILE_COLS = 64      # kBdMaskCols: its columns
TILE = 32                # kBdTile: rows and columns of a tile of the contrast kernel
CHUNK = 4                # kBdChunk: tiles a workgroup walks before it adds its bins
FRAMES_PER_LAUNCH = 256  # kFrameMap (csrc/analysis_host.hpp)


def default_window(w, h):
    """The window for a w x h plane: 63 at 2160p, 33 at 1080p, never below 3."""
    return 2 * min(max((31 * (int(w) + int(h)) + 3000) // 6000, 1), 31) + 1


def scale_sizes(w, h):
    """[(w_s, h_s)] of the five scales."""
    out = [(int(w), int(h))]
    for _ in range(SCALES - 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def pool(hist):
    """(banding [N], top [N, 5]) of pp_banding's histograms [N, 5, 1024],
    float64: top[k, s] is the mean of the ceil(0.6 n_s) largest Q of scale s
    (n_s = the histogram's sum, the scale's positions) divided by 1024, and
    banding[k] = (16 top_0 + 8 top_1 + 4 top_2 + 2 top_3 + top_4) / 31, in
    [0, 1).  The sums are exact integers; one division per value."""
    hh = np.asarray(hist)
    if hh.ndim == 2:
        hh = hh[None]
    if hh.ndim != 3 or hh.shape[1:] != (SCALES, BINS):
        raise ValueError("hist must be [N, %d, %d]" % (SCALES, BINS))
    n = hh.shape[0]
    top = np.zeros((n, SCALES), dtype=np.float64)
    qrev = np.arange(BINS - 1, -1, -1, dtype=np.int64)
    for k in range(n):
        for s in range(SCALES):
            rev = hh[k, s, ::-1].astype(np.int64)  # bin 1023 first; counts < 2^31, sums < 2^41
            cum = np.cumsum(rev)
            need = (TOP_NUM * int(cum[-1]) + TOP_DEN - 1) // TOP_DEN  # ceil(0.6 total), exact
            if need == 0:
                continue
            i = int(np.searchsorted(cum, need))  # the bin that holds the last position taken
            acc = int((rev[:i] * qrev[:i]).sum()) + (need - (int(cum[i - 1]) if i else 0)) * int(qrev[i])
            top[k, s] = acc / (need * 1024.0)
    weights = np.array(SCALE_WEIGHTS, dtype=np.float64)
    return (top * weights).sum(axis=1) / weights.sum(), top


def summarize(hist):
    """Per-frame ``banding_y`` [N] and ``banding_scales_y`` [N, 5] from
    pp_banding's output for a whole clip, plus ``mean``: the clip values
    ``banding_y`` (mean over frames), ``banding_max_y`` (the largest frame
    value) and ``banding_scales_y`` (five means); NaN for an empty clip."""
    b, top = pool(hist)
    nan = float("nan")
    mean = {"banding_y": float(b.mean()) if b.size else nan,
            "banding_max_y": float(b.max()) if b.size else nan,
            "banding_scales_y": [float(v) for v in top.mean(axis=0)] if b.size else [nan] * SCALES}
    return {"banding_y": b, "banding_scales_y": top, "mean": mean}


def banding_of_file(path, batch=32, window=None, crop=None, crop_from="yuv422p"):
    """PP-BAND-1 of the file ``path`` on its own: ``summarize``'s dict plus
    ``frames``, ``w``, ``h`` and ``window``.  The file is opened as
    stats.stats_of_file opens it (a v210 / UYVY AVI is unpacked on the GPU)
    and streamed ``batch`` frames at a time.  ``window``: default
    default_window of the picture measured.  ``crop``, ``crop_from``: as
    stats_of_file's."""
    import torch

    from . import clips, ops
    with clips.clip_batches(path, max(1, int(batch)), crop, crop_from) as (rd, win, batches):
        w, h = (rd.w, rd.h) if win is None else win[2:]
        window = default_window(w, h) if window is None else int(window)
        outs = [ops.banding(b, window=window) for b in batches]
        torch.cuda.current_stream().synchronize()
    hist = clips.host_array(outs, (SCALES, BINS), np.uint32)
    res = summarize(hist)
    res.update({"frames": int(hist.shape[0]), "w": int(w), "h": int(h), "window": int(window)})
    return res


def report(res, path, per_frame=False):
    """The JSON object `cli banding` prints: the clip values, and with
    per_frame the per-frame lists; NaN becomes null."""
    from .clips import json_value
    mean = res["mean"]
    out = {"file": os.path.basename(path), "frames": int(res["frames"]), "w": int(res["w"]), "h": int(res["h"]),
           "spec": "PP-BAND-1", "window": int(res["window"]),
           "banding_y": json_value(mean["banding_y"]), "banding_max_y": json_value(mean["banding_max_y"]),
           "banding_scales_y": [json_value(v) for v in mean["banding_scales_y"]]}
    if per_frame:
        out["banding_y_frames"] = [json_value(v) for v in res["banding_y"]]
        out["banding_scales_y_frames"] = [[json_value(v) for v in row] for row in res["banding_scales_y"]]
    return out
