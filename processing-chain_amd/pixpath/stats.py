"""Per-frame signal statistics of a clip (spec PP-STATS-1).

What is inside one file: is a SRC really limited-range, is a "10-bit" SRC
8-bit content shifted up, do a 10-bit file's samples carry junk above bit 9,
which frames of a stalled AVPVS are black and which repeat the frame before.
The MI355X makes one pass over the frames the readers already put into HBM
(pp_frame_stats) and returns, per frame and plane, a histogram, the count of
samples outside the container's bins and the sum of absolute differences to
the previous frame; everything reported is host arithmetic on those three
exact integer arrays, in this module, in numpy, importable without a GPU.

The names and definitions are modelled on FFmpeg's vf_signalstats,
vf_blackdetect and vf_freezedetect; parity with FFmpeg is unpinned (no FFmpeg
here; INTEGRATION.md has the recipe that would pin it).  The spec is what the
tests pin.
"""
import math
import os

import numpy as np

from . import formats
from .clips import json_value

PLANES = ("y", "u", "v")
SAD_ABSENT = (1 << 64) - 1  # pp_frame_stats' sad[0] without a previous frame
# kernel geometry (csrc/stats.hip), for tests that place sizes on its seams
LANE_BYTES = 16      # kStLaneBytes: bytes a lane loads per piece
TILE_BYTES = 1024    # kStTileBytes: bytes of a row one tile (one wave load) spans: the row trip
WAVE_ROWS = 16       # kStLaneRows: rows of a tile one wave holds
TILE_ROWS = 64       # kStTileRows: rows of a tile (a band)
FRAMES_PER_WORKGROUP = 16  # kStFrames: frames a workgroup walks with the previous frame in registers

BLACK_PIX_TH = 0.10  # vf_blackdetect's pixel_black_th default
BLACK_PIC_TH = 0.98  # vf_blackdetect's picture_black_ratio_th default

PER_PLANE = ("min", "max", "avg", "low", "high", "dif", "bitdepth", "out_of_range", "over")


def _runs(flags):
    """[first, last] index runs of the true entries."""
    out = []
    for k, v in enumerate(flags):
        if v:
            if out and out[-1][1] == k - 1:
                out[-1][1] = k
            else:
                out.append([k, k])
    return out


def _percentile(cum, target):
    """Per row of cum [N, bins]: the smallest v with cum[v] >= target, NaN if none."""
    hit = cum >= target[:, None]
    return np.where(hit.any(axis=1), hit.argmax(axis=1), np.nan).astype(np.float64)


def summarize(hist, sad, over, fmt, w, h, pix_th=BLACK_PIX_TH, pic_th=BLACK_PIC_TH, histogram=False):
    """Host side of PP-STATS-1.  ``hist`` [N, 3, bins], ``sad`` [N, 3] (or
    None: no differences) and ``over`` [N, 3] as pp_frame_stats returns them
    (sad's sentinel as uint64 2^64-1 or int64 -1), of a clip of planar format
    ``fmt`` and size w x h.  With d the bit depth, s = 2^(d-8) and ``count``
    the samples of the plane, the result holds float64 / integer arrays [N]
    per plane, keys ``<name>_y/u/v``:

      min, max      lowest and highest non-empty bin (NaN: no sample in a bin)
      avg           sum v hist[v] / sum hist, float64 (NaN likewise)
      low, high     the smallest v whose cumulative count is >= rint(0.10 count)
                    resp. rint(0.90 count), rint rounding half to even (NaN
                    where the bins never reach it: samples in ``over``)
      dif           sad / count; NaN where sad is the sentinel or not computed
      bitdepth      set bits of the OR of all non-empty bin indices
      out_of_range  samples below 16 s or above 235 s (luma) / 240 s (chroma),
                    plus ``over``.  Per plane: vf_signalstats' BRNG counts the
                    PIXELS with any component outside, a cross-plane measure
                    this one knowingly differs from
      over          as returned by the kernel

    per frame ``black`` (the share of luma samples <= 16 s + pix_th (235-16) s
    is >= pic_th: vf_blackdetect's pixel_black_th and picture_black_ratio_th,
    defaults 0.10 and 0.98) and ``repeat`` (every plane's sad is 0), and under
    ``clip`` the values of the whole clip: min of min, max of max, mean avg and
    mean dif (over the frames that have one) per plane, the max bitdepth, the
    totals of out_of_range and over, ``black_frames`` and ``repeat_frames`` as
    [first, last] index runs, and with ``histogram`` the per-plane sum of the
    frames' histograms (``histogram_y/u/v``, lists of bins integers)."""
    f = formats.fmt(fmt)
    d = f.depth
    bins = 1 << d
    s = 1 << (d - 8)
    hist = np.asarray(hist).astype(np.int64).reshape(-1, 3, bins)
    n = hist.shape[0]
    over = np.asarray(over).astype(np.int64).reshape(-1, 3)
    if sad is None:
        sadu = np.full((n, 3), SAD_ABSENT, np.uint64)
    else:
        sadu = np.ascontiguousarray(np.asarray(sad).reshape(-1, 3))
        sadu = sadu.view(np.uint64) if sadu.dtype == np.int64 else sadu.astype(np.uint64)
    count = np.array([r * c for r, c in formats.plane_shapes(f, w, h)], dtype=np.int64)
    v = np.arange(bins, dtype=np.int64)
    res = {"frames": int(n)}
    clip = {}
    for p, name in enumerate(PLANES):
        hp = hist[:, p, :]
        tot = hp.sum(axis=1)
        some = tot > 0
        nz = hp > 0
        lo = np.where(some, nz.argmax(axis=1), np.nan).astype(np.float64)
        hi = np.where(some, bins - 1 - nz[:, ::-1].argmax(axis=1), np.nan).astype(np.float64)
        avg = np.where(some, (hp * v).sum(axis=1) / np.where(some, tot, 1).astype(np.float64), np.nan)
        cum = hp.cumsum(axis=1)
        t_lo = np.full(n, np.rint(0.10 * count[p])).astype(np.int64)
        t_hi = np.full(n, np.rint(0.90 * count[p])).astype(np.int64)
        absent = sadu[:, p] == np.uint64(SAD_ABSENT)
        dif = np.where(absent, np.nan, sadu[:, p].astype(np.float64) / float(count[p]))
        used = np.bitwise_or.reduce(np.where(nz, v, 0), axis=1)
        bd = np.array([bin(int(x)).count("1") for x in used], dtype=np.int64)
        top = (235 if p == 0 else 240) * s
        oor = hp[:, :16 * s].sum(axis=1) + hp[:, top + 1:].sum(axis=1) + over[:, p]
        res["min_" + name], res["max_" + name], res["avg_" + name] = lo, hi, avg
        res["low_" + name], res["high_" + name] = _percentile(cum, t_lo), _percentile(cum, t_hi)
        res["dif_" + name], res["bitdepth_" + name] = dif, bd
        res["out_of_range_" + name], res["over_" + name] = oor, over[:, p].copy()

        def nan_or(fn, a):
            a = a[~np.isnan(a)]
            return float(fn(a)) if a.size else float("nan")
        clip["min_" + name], clip["max_" + name] = nan_or(np.min, lo), nan_or(np.max, hi)
        clip["avg_" + name], clip["dif_" + name] = nan_or(np.mean, avg), nan_or(np.mean, dif)
        clip["bitdepth_" + name] = int(bd.max()) if n else 0
        clip["out_of_range_" + name], clip["over_" + name] = int(oor.sum()), int(over[:, p].sum())
        if histogram:
            clip["histogram_" + name] = [int(x) for x in hp.sum(axis=0)]
    thr = 16 * s + float(pix_th) * (235 - 16) * s
    dark = hist[:, 0, :min(bins, int(math.floor(thr)) + 1)].sum(axis=1)
    res["black"] = dark.astype(np.float64) / float(count[0]) >= float(pic_th)
    res["repeat"] = (sadu == 0).all(axis=1)
    clip["black_frames"], clip["repeat_frames"] = _runs(res["black"]), _runs(res["repeat"])
    res["clip"] = clip
    return res


def arrays_of_file(path, batch=32, crop=None, crop_from="yuv422p"):
    """pp_frame_stats over every frame of ``path``: (hist, sad, over, fmt, w, h)
    with numpy arrays [N, 3, bins] int32, [N, 3] uint64, [N, 3] int32 and the
    planar format and size they describe.  The file is opened as `cli metrics`
    opens its inputs (clips.open_clip / read_device: an FFV1 AVI through the
    GPU decoder, a v210 / UYVY AVI unpacked on the GPU to yuv422p10le /
    yuv422p, anything else through io.open_reader) and streamed ``batch``
    frames at a time; the last frame of a batch is the next call's ``prev``,
    so only frame 0 of the file has no difference.  ``crop`` = (w, h): the
    file is a packed CPVS canvas and only the w x h AVPVS picture inside it
    counts, at the offsets the CPVS pad put it (clips.crop_window;
    ``crop_from``: the AVPVS's pixel format) -- without it a letterboxed
    CPVS's bars dominate every statistic."""
    import torch

    from . import clips, ops
    from .frames import FrameBatch
    with clips.clip_batches(path, max(1, int(batch)), crop, crop_from) as (rd, window, batches):
        f = clips.planar_format(rd)
        w, h = (rd.w, rd.h) if window is None else window[2:]
        outs, prev = [], None
        for b in batches:
            outs.append(ops.frame_stats(b, prev=prev))
            prev = FrameBatch(f, w, h, 1, planes=[t[b.n - 1:b.n] for t in b.planes])
        torch.cuda.current_stream().synchronize()
    hist = clips.host_array([o[0] for o in outs], (3, 1 << f.depth), np.int32)
    sad = clips.host_array([o[1] for o in outs], (3,), np.uint64)
    over = clips.host_array([o[2] for o in outs], (3,), np.int32)
    return hist, sad, over, f, int(w), int(h)


def stats_of_file(path, batch=32, crop=None, crop_from="yuv422p", pix_th=BLACK_PIX_TH, pic_th=BLACK_PIC_TH,
                  histogram=False):
    """PP-STATS-1 of the file ``path``: ``summarize`` of ``arrays_of_file``,
    plus ``fmt`` (the name of the planar format analysed), ``w`` and ``h``."""
    hist, sad, over, f, w, h = arrays_of_file(path, batch=batch, crop=crop, crop_from=crop_from)
    res = summarize(hist, sad, over, f, w, h, pix_th=pix_th, pic_th=pic_th, histogram=histogram)
    res.update({"fmt": f.name, "w": w, "h": h})
    return res


def report(res, path, per_frame=False):
    """The JSON object `cli stats` prints: the clip values, and with per_frame
    the per-frame lists (``<name>_<plane>_frames``, ``black``, ``repeat``); NaN
    becomes null."""
    out = {"file": os.path.basename(path), "frames": int(res["frames"]), "spec": "PP-STATS-1"}
    for k in ("fmt", "w", "h"):
        if k in res:
            out[k] = res[k]
    for k, v in res["clip"].items():
        out[k] = v if isinstance(v, list) else json_value(v)
    if per_frame:
        for kind in PER_PLANE:
            for name in PLANES:
                key = "%s_%s" % (kind, name)
                out[key + "_frames"] = [json_value(v) for v in res[key]]
        out["black"] = [bool(v) for v in res["black"]]
        out["repeat"] = [bool(v) for v in res["repeat"]]
    return out
