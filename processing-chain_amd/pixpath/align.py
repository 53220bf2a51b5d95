"""Temporal alignment of a PVS to its SRC (spec PP-ALIGN-1): which reference
frame every distorted frame shows.

The chain makes PVSes with stalls, freezes and black lead-ins (PP-STALL-1);
after the first of them the vf_fps map `cli metrics` pairs frames by is wrong.
Here the map is found from the pictures: the MI355X computes the luma SSE of
every distorted frame against a band of reference frames (pp_frame_sse_band,
ops.sse_band), and ``track`` -- a host rule on those exact integers -- walks a
cursor through the reference.  No reference implementation exists and nobody
has tuned the two settings (``lookahead``, ``min_psnr``) on real PVSes
(DESIGN.md).
"""
import math
import os

import numpy as np

from .clips import clip_pair, json_value, map_entries

# kernel geometry (csrc/align.hip), for tests that place sizes on its seams
LANE_BYTES = 16    # kAlnLaneBytes: bytes a lane loads per piece
TILE_BYTES = 1024  # kAlnTileBytes: a wave's span of a row (64 lanes)
WAVE_ROWS = 16     # kAlnLaneRows: rows of a tile one wave holds
TILE_ROWS = 64     # kAlnTileRows: rows of a unit (4 waves)
GROUP = 4          # kAlnGroup: reference pieces in flight per lane
CHUNK = 32         # kAlnChunk: candidates between two exchanges through LDS
FIRST_PER_LAUNCH = 256  # kFrameMap: `first` entries per launch

ABSENT = np.uint64(0xFFFFFFFFFFFFFFFF)
LOOKAHEAD = 64
MIN_PSNR = 14.0
UNKNOWN_LENGTH = (1 << 31) - 1  # n_ref while the reference's end has not been read


def threshold(w, h, depth, min_psnr):
    """The largest SSE of a match: floor(w h peak^2 10^(-min_psnr / 10)) with
    peak = 2^depth - 1, the product formed in double precision from the exact
    integer w h peak^2."""
    peak = (1 << int(depth)) - 1
    return int(math.floor(float(int(w) * int(h) * peak * peak) * 10.0 ** (-float(min_psnr) / 10.0)))


def track(sse_rows, first, nominal_advance, n_ref, lookahead, min_psnr, w, h, depth, cursor):
    """The host rule of PP-ALIGN-1 over one launch's rows.  ``sse_rows``
    [n, ncand] (uint64, or the int64 view ops.sse_band returns): row k holds the
    SSE of distorted frame k against reference frames first[k] .. first[k] +
    ncand - 1, ABSENT where there is none.  ``nominal_advance`` [n]: d_k, the
    advance of the vf_fps map at each frame.  ``cursor``: the reference index of
    the last matched frame (0 at the start of a clip).

    Frame k's candidates are j in [cursor, min(cursor + lookahead, n_ref)).
    e = their smallest SSE; among the candidates with SSE e the one nearest to
    cursor + d_k wins, then the smaller j.  e <= threshold(): map[k] = j and the
    cursor moves there; otherwise map[k] = -1 and the cursor stays.  A row that
    does not cover its candidates ends the walk: nothing is guessed.

    Returns (map int32 [m], sse int64 [m] (-1 unmatched), cursor) for the
    m <= n rows walked; the caller relaunches rows m.. from the new cursor."""
    rows = np.asarray(sse_rows)
    if rows.dtype != np.uint64:
        rows = np.ascontiguousarray(rows, dtype=np.int64).view(np.uint64)
    rows = rows.reshape(len(first), -1)
    ncand = rows.shape[1]
    thr = threshold(w, h, depth, min_psnr)
    c, lookahead, n_ref = int(cursor), int(lookahead), int(n_ref)
    out_map, out_sse = [], []
    for k in range(rows.shape[0]):
        f0 = int(first[k])
        lo, hi = c, min(c + lookahead, n_ref)
        if hi > lo and (f0 > lo or f0 + ncand < hi):
            break
        best = None
        if hi > lo:
            cand = rows[k, lo - f0:hi - f0]
            ok = cand != ABSENT
            if ok.any():
                e = cand[ok].min()
                js = lo + np.flatnonzero(ok & (cand == e))
                want = c + int(nominal_advance[k])
                j = int(js[np.argmin(np.abs(js - want))])  # argmin: the first, that is the smaller j
                best = (j, int(e))
        if best is not None and best[1] <= thr:
            out_map.append(best[0])
            out_sse.append(best[1])
            c = best[0]
        else:
            out_map.append(-1)
            out_sse.append(-1)
    return np.asarray(out_map, dtype=np.int32), np.asarray(out_sse, dtype=np.int64), c


def events(ref_map, nominal_advance, cursor=0):
    """What a map says happened, walking it as ``track`` did from ``cursor``:
    ``holds``  [first_k, length, ref_index]: runs of matched frames that show the
               reference frame of the matched frame before them although the
               nominal map advances there (d_k >= 1): stalls and freezes;
    ``skips``  [k, from_ref, to_ref]: a matched frame more than d_k past the cursor;
    ``unmatched`` [first_k, length]: runs of -1."""
    holds, skips, unmatched = [], [], []
    c, seen = int(cursor), False
    for k, j in enumerate(int(v) for v in ref_map):
        d = int(nominal_advance[k])
        if j < 0:
            if unmatched and unmatched[-1][0] + unmatched[-1][1] == k:
                unmatched[-1][1] += 1
            else:
                unmatched.append([k, 1])
            continue
        if seen and j == c and d >= 1:
            if holds and holds[-1][0] + holds[-1][1] == k and holds[-1][2] == j:
                holds[-1][1] += 1
            else:
                holds.append([k, 1, j])
        elif j - c > d:
            skips.append([k, c, j])
        c, seen = j, True
    return {"holds": holds, "skips": skips, "unmatched": unmatched}


def nominal_advances(k0, n, in_rate, out_rate):
    """d_k for k in [k0, k0 + n): nom[k] - nom[k-1] of the vf_fps map of a
    reference at ``in_rate`` shown at ``out_rate`` (ops.fps_map, taken from a
    long enough clip: the clamp to a last frame never shows), d_0 = 0."""
    lo = max(int(k0) - 1, 0)
    m = map_entries(lo, int(k0) + int(n) - lo, in_rate, out_rate).astype(np.int64)
    d = np.diff(m, prepend=m[:1])
    return d[int(k0) - lo:]


def band(advances, lookahead):
    """Candidates per row of a launch whose rows all start at the cursor: the
    lookahead plus the advance the nominal map makes over the rows.  That sum
    bounds the cursor's advance only while the clip runs at its nominal rate; a
    skip can pass it, and then ``track`` stops at the first row the band does
    not cover and the rest is launched again from the new cursor."""
    return int(lookahead) + int(np.sum(advances))


def _slice(b, lo, hi=None):
    from .frames import FrameBatch
    hi = b.n if hi is None else hi
    return FrameBatch(b.fmt, b.w, b.h, hi - lo, planes=[t[lo:hi] for t in b.planes])


def align_files(ref_path, dist_path, batch=32, lookahead=LOOKAHEAD, min_psnr=MIN_PSNR, flags="bicubic", crop=None,
                crop_from="yuv422p"):
    """PP-ALIGN-1 of the file ``dist_path`` (the PVS) against ``ref_path`` (the
    SRC).  The pair is opened by clips.clip_pair (packed CPVS and ``crop``
    included; the reference is brought to the distorted clip's size and format
    with ops.Scaler when they differ).  The reference frames [cursor, cursor +
    band) stay resident, frames behind the cursor are dropped
    (clips.ReferenceWindow); every distorted batch is one ops.sse_band launch
    (more only after a skip past the band) followed by ``track``.

    Returns a dict: ``map`` int32 [N] (-1 unmatched), ``sse`` int64 [N] (the
    winning SSE, -1 unmatched), ``advance`` (d_k), ``holds`` / ``skips`` /
    ``unmatched`` (``events``), ``w``, ``h``, ``depth``, ``frames``."""
    import torch

    from . import ops
    batch, lookahead = int(batch), int(lookahead)
    if lookahead < 1:
        raise ValueError("lookahead must be at least 1")
    dev = torch.device("cuda", torch.cuda.current_device())
    maps, sses, advs = [], [], []
    with clip_pair(ref_path, dist_path, batch, flags, crop, crop_from) as (ref, dist, dfmt, dw, dh, dists, window):
        cursor, k0 = 0, 0
        for d in dists:
            adv = nominal_advances(k0, d.n, ref.rate, dist.rate)
            advs.append(adv)
            r = 0
            while r < d.n:
                ncand = band(adv[r:], lookahead)
                window.extend(cursor + ncand, cursor)  # the band resident, the frames behind the cursor dropped
                m = d.n - r
                if window.frames is None:  # an empty reference: nothing can match
                    mp, ws = np.full(m, -1, np.int32), np.full(m, -1, np.int64)
                else:
                    rows = ops.sse_band(window.frames, _slice(d, r), [cursor - window.first] * m, ncand)
                    torch.cuda.current_stream(dev).synchronize()
                    mp, ws, cursor = track(rows.cpu().numpy(), [cursor] * m, adv[r:],
                                           window.count if window.ended else UNKNOWN_LENGTH, lookahead, min_psnr,
                                           dw, dh, dfmt.depth, cursor)
                maps.append(mp)
                sses.append(ws)
                r += len(mp)
            k0 += d.n
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    res = {"map": cat(maps, np.int32), "sse": cat(sses, np.int64), "advance": cat(advs, np.int64),
           "w": int(dw), "h": int(dh), "depth": int(dfmt.depth)}
    res.update(events(res["map"], res["advance"]))
    res["frames"] = int(len(res["map"]))
    return res


def psnr_of(res):
    """Per-frame luma PSNR of the matches of an align_files result: NaN where
    unmatched or identical (MSE 0), as pixpath.metrics."""
    sse = res["sse"].astype(np.float64)
    peak = float((1 << res["depth"]) - 1)
    out = np.full(sse.shape, np.nan)
    ok = sse > 0
    out[ok] = 10.0 * np.log10(peak * peak * res["w"] * res["h"] / sse[ok])
    return out


def report(res, ref_path, dist_path, per_frame=False):
    """The JSON object `cli align` prints."""
    matched = int((res["map"] >= 0).sum())
    adv = res["advance"]
    out = {"ref": os.path.basename(ref_path), "file": os.path.basename(dist_path), "spec": "PP-ALIGN-1",
           "frames": res["frames"], "matched": matched, "unmatched": res["frames"] - matched,
           "unmatched_runs": res["unmatched"], "holds": res["holds"], "skips": res["skips"], "held_frames": int(sum(x[1] for x in res["holds"])),
           "skipped_ref_frames": int(sum(t - f - int(adv[k]) for k, f, t in res["skips"]))}
    if per_frame:
        out["map"] = [int(v) for v in res["map"]]
        out["psnr_y_frames"] = [json_value(v) for v in psnr_of(res)]
    return out
