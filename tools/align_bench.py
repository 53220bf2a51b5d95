#!/usr/bin/env python3
"""Time pp_frame_sse_band (PP-ALIGN-1) on one MI355X with HIP events, next to
what the library offered before it: one pp_metrics call per candidate offset.

Shape: --frames (600) frames of 1920x1080, 8-bit (yuv420p) and 10-bit
(yuv420p10le), distorted = reference + bounded noise, walked as
pixpath.align walks a clip at equal rates: --batch (32) distorted frames per
launch, every row's band starting at the batch's first frame and --band (96)
candidates wide (candidates past the reference's end are absent).
  new       one ops.sse_band launch per batch, luma only
  baseline  per batch, one ops.metrics call per candidate that exists, with
            ref_index = first + c: the distorted batch read once per offset,
            SSIM and both chroma planes computed along
Both run in this process on the same buffers; a pass over the clip is timed
as a whole (events around all its launches), --iters passes after --warmup
(the baseline: --base-iters).  Before timing, the two paths are compared once:
sse[:, c] must equal pp_metrics' plane-0 SSE for every batch and candidate of
the first and the last batch.  Prints one JSON line; a measurement, not a
gate; it fails without a GPU.

  python tools/align_bench.py [--frames 600] [--out profiles/align/NAME.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "processing-chain_amd"))


def timed(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"avg_ms": round(sum(ms) / len(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "passes": len(ms)}


def one_depth(fmt, a, dev):
    import numpy as np
    import torch

    from pixpath import ops
    from pixpath.frames import FrameBatch
    w, h, n = 1920, 1080, a.frames
    ten = fmt.endswith("10le")
    lo, hi = (64, 941) if ten else (16, 236)
    ref, dist = FrameBatch(fmt, w, h, n, device=dev), FrameBatch(fmt, w, h, n, device=dev)
    for p in range(3):
        rp, dp = (t.planes[p].view(torch.int16) if ten else t.planes[p] for t in (ref, dist))
        for k in range(n):  # frame by frame: no batch-sized temporaries
            r = torch.randint(lo, hi, rp[k].shape, dtype=torch.int16, device=dev)
            rp[k].copy_(r)
            dp[k].copy_((r + torch.randint(-8, 9, r.shape, dtype=torch.int16, device=dev)).clamp_(0, 1023 if ten else 255))
    torch.cuda.synchronize()
    batches = [(k0, min(a.batch, n - k0)) for k0 in range(0, n, a.batch)]
    cut = lambda k0, m: FrameBatch(fmt, w, h, m, planes=[t[k0:k0 + m] for t in dist.planes])
    parts = [(k0, m, cut(k0, m), min(a.band, n - k0)) for k0, m in batches]  # (first, frames, batch, candidates that exist)
    keep = {}

    def new_pass():
        for k0, m, d, _ in parts:
            keep["new"] = ops.sse_band(ref, d, [k0] * m, a.band)

    def base_pass():
        for k0, m, d, live in parts:
            for c in range(live):
                keep["base"] = ops.metrics(ref, d, ref_index=np.full(m, k0 + c, np.int32))

    # the two paths agree (first and last batch, every candidate)
    for k0, m, d, live in (parts[0], parts[-1]):
        got = ops.sse_band(ref, d, [k0] * m, a.band)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        for c in range(a.band):
            if c < live:
                sse, _ = ops.metrics(ref, d, ref_index=np.full(m, k0 + c, np.int32))
                torch.cuda.synchronize()
                if not np.array_equal(got[:, c], sse.cpu().numpy()[:, 0]):
                    raise SystemExit("align_bench: %s batch %d candidate %d differs from pp_metrics" % (fmt, k0, c))
            elif not (got[:, c] == -1).all():
                raise SystemExit("align_bench: %s batch %d candidate %d should be absent" % (fmt, k0, c))
    new = timed(new_pass, a.warmup, a.iters)
    base = timed(base_pass, 1, a.base_iters)
    cands = sum(m * live for _, m, _, live in parts)
    es = 2 if ten else 1
    return {"fmt": fmt, "new": new, "baseline": base, "baseline_over_new": round(base["avg_ms"] / new["avg_ms"], 2),
            "launches_new": len(parts), "calls_baseline": sum(live for *_, live in parts),
            "frame_pairs": cands, "luma_bytes_compared": cands * w * h * es, "agree": True}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--band", type=int, default=96)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--base-iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("align_bench: no GPU visible (a timing needs the MI355X)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(910)
    res = {"tool": "align_bench", "device": torch.cuda.get_device_name(0), "w": 1920, "h": 1080, "frames": a.frames,
           "batch": a.batch, "band": a.band, "warmup": a.warmup,
           "timer": "HIP events around one pass over the clip: every pp_frame_sse_band launch (align_kernel + "
                    "align_finalize) / every pp_metrics call (metrics_kernel + metrics_finalize) of the pass",
           "depths": [one_depth(f, a, dev) for f in ("yuv420p", "yuv420p10le")]}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
