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
import sys

import callbench


def one_depth(fmt, a, dev):
    import numpy as np
    import torch

    from pixpath import ops
    from pixpath.frames import FrameBatch
    w, h, n = callbench.W, callbench.H, a.frames
    ten = fmt.endswith("10le")
    ref, dist = callbench.noise_pair(fmt, n, dev)
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
    new = callbench.timed(new_pass, a.warmup, a.iters, count="passes")
    base = callbench.timed(base_pass, 1, a.base_iters, count="passes")
    cands = sum(m * live for _, m, _, live in parts)
    es = 2 if ten else 1
    return {"fmt": fmt, "new": new, "baseline": base, "baseline_over_new": round(base["avg_ms"] / new["avg_ms"], 2),
            "launches_new": len(parts), "calls_baseline": sum(live for *_, live in parts),
            "frame_pairs": cands, "luma_bytes_compared": cands * w * h * es, "agree": True}


def main(argv=None):
    ap = callbench.parser(600, 2, 10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--band", type=int, default=96)
    ap.add_argument("--base-iters", type=int, default=3)
    a = ap.parse_args(argv)
    dev = callbench.require_gpu("align_bench", seed=910)
    res = callbench.header(
        "align_bench", a, ("w", "h", "frames", "batch", "band", "warmup"),
        timer="HIP events around one pass over the clip: every pp_frame_sse_band launch (align_kernel + "
              "align_finalize) / every pp_metrics call (metrics_kernel + metrics_finalize) of the pass",
        depths=[one_depth(f, a, dev) for f in ("yuv420p", "yuv420p10le")])
    callbench.emit(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
