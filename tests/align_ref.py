"""numpy / Python-int reference of PP-ALIGN-1, written from the
spec's text and independently of pixpath.align: the SSE band a launch of
pp_frame_sse_band must produce, the tracker's rule, and the events."""
import math

import numpy as np

ABSENT = 0xFFFFFFFFFFFFFFFF


def sse_band_ref(dist, ref, first, ncand):
    """dist [nd, h, w], ref [nr, h, w] integer arrays; uint64 [nd, ncand]."""
    dist = np.asarray(dist).astype(np.int64)
    ref = np.asarray(ref).astype(np.int64)
    out = np.empty((dist.shape[0], ncand), np.uint64)
    for k in range(dist.shape[0]):
        for c in range(ncand):
            j = int(first[k]) + c
            if j < 0 or j >= ref.shape[0]:
                out[k, c] = ABSENT
            else:
                d = dist[k] - ref[j]
                out[k, c] = int((d * d).sum())  # <= 2^31 samples * 2^32: int64 holds it
    return out


def threshold_ref(w, h, depth, min_psnr):
    peak = 2 ** depth - 1
    return math.floor(float(w * h * peak * peak) * 10.0 ** (-min_psnr / 10.0))


def track_ref(sse_rows, first, advance, n_ref, lookahead, min_psnr, w, h, depth, cursor):
    """The rule, frame by frame, on Python ints.  Returns (map, sse, cursor)
    lists for the rows walked; stops before a row whose band does not hold
    every candidate."""
    rows = [[int(v) for v in row] for row in np.asarray(sse_rows).astype(np.uint64)]
    thr = threshold_ref(w, h, depth, min_psnr)
    c = cursor
    out_map, out_sse = [], []
    for k, row in enumerate(rows):
        cands = list(range(c, min(c + lookahead, n_ref)))
        if cands and (cands[0] < first[k] or cands[-1] >= first[k] + len(row)):
            break
        vals = {j: row[j - first[k]] for j in cands if row[j - first[k]] != ABSENT}
        if vals:
            e = min(vals.values())
            target = c + int(advance[k])
            j = min((j for j in vals if vals[j] == e), key=lambda j: (abs(j - target), j))
        if vals and e <= thr:
            out_map.append(j)
            out_sse.append(e)
            c = j
        else:
            out_map.append(-1)
            out_sse.append(-1)
    return out_map, out_sse, c


def events_ref(ref_map, advance, cursor=0):
    holds, skips, unmatched = [], [], []
    c, matched_before = cursor, False
    k, n = 0, len(ref_map)
    while k < n:
        j = int(ref_map[k])
        if j < 0:
            e = k
            while e < n and ref_map[e] < 0:
                e += 1
            unmatched.append([k, e - k])
            k = e
            continue
        if matched_before and j == c and advance[k] >= 1:
            e = k
            while e < n and ref_map[e] == j and advance[e] >= 1:
                e += 1
            holds.append([k, e - k, j])
            k = e
            continue
        if j - c > advance[k]:
            skips.append([k, c, j])
        c, matched_before = j, True
        k += 1
    return {"holds": holds, "skips": skips, "unmatched": unmatched}


def walk(track, dist, ref, advance, batch, lookahead, min_psnr, depth):
    """A clip through ``track`` (track_ref or pixpath.align.track) the way
    PP-ALIGN-1 launches it: ``batch`` distorted frames at a time, every row's
    band starting at the cursor and lookahead + (the rows' nominal advance)
    wide, the rest of a batch launched again from the new cursor when a row
    does not cover its candidates.  Returns (map, sse, launches)."""
    dist, ref = np.asarray(dist), np.asarray(ref)
    h, w = dist.shape[1:]
    out_map, out_sse, launches, c = [], [], 0, 0
    for k0 in range(0, len(dist), batch):
        d = dist[k0:k0 + batch]
        adv = list(advance[k0:k0 + batch])
        r = 0
        while r < len(d):
            ncand = lookahead + int(sum(adv[r:]))
            m = len(d) - r
            rows = sse_band_ref(d[r:], ref, [c] * m, ncand)
            launches += 1
            mp, ss, c = track(rows, [c] * m, adv[r:], len(ref), lookahead, min_psnr, w, h, depth, c)
            assert len(mp) >= 1
            out_map += [int(v) for v in mp]
            out_sse += [int(v) for v in ss]
            r += len(mp)
    return out_map, out_sse, launches
