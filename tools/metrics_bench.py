#!/usr/bin/env python3
"""Time pp_metrics (PP-METRIC-1) on one MI355X with HIP events.

Shape: --frames (600) frames of 1920x1080 yuv422p10le against a second such
batch (reference + bounded noise).  Algorithmic traffic = both batches read
once = 2 x frames x 8,294,400 B (9.95 GB at 600 frames).  Prints one JSON
line: avg / min / max launch time over --iters (>= 20) timed launches after
--warmup, `frac` = bytes / time / 8 TB/s (the HBM peak), and in the same run
siti_kernel's time on the luma of one of the two batches with its own bytes
and fraction: the in-repo yardstick for a read-only pass.  A measurement, not a
gate; it fails without a GPU.

  python tools/metrics_bench.py [--frames 600] [--out profiles/metrics/NAME.json]
"""
import sys

import callbench


def main(argv=None):
    ap = callbench.parser(600, 3, 20)
    a = ap.parse_args(argv)
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    dev = callbench.require_gpu("metrics_bench", seed=910)
    import torch
    from pixpath import formats, ops
    from pixpath.frames import FrameBatch
    fmt, w, h, n = "yuv422p10le", callbench.W, callbench.H, a.frames
    ref, dist = FrameBatch(fmt, w, h, n, device=dev), FrameBatch(fmt, w, h, n, device=dev)
    for p in range(3):
        r16, d16 = ref.planes[p].view(torch.int16), dist.planes[p].view(torch.int16)
        for k in range(n):  # frame by frame: no batch-sized temporaries
            r16[k].random_(64, 941)
            d16[k].copy_((r16[k] + torch.randint(-8, 9, r16[k].shape, dtype=torch.int16, device=dev)).clamp_(0, 1023))
    torch.cuda.synchronize()
    out = {}

    def run_metrics():
        out["m"] = ops.metrics(ref, dist)

    m_ms = callbench.times(run_metrics, a.warmup, a.iters)
    luma = ref.planes[0]

    def run_siti():
        out["s"] = ops.siti(luma, 10)

    s_ms = callbench.times(run_siti, a.warmup, a.iters)
    fb = formats.frame_bytes(fmt, w, h)
    res = callbench.header("metrics_bench", a, ("fmt",) + callbench.HEAD + ("iters",), fmt=fmt,
                           timer="HIP events around one pp_metrics call (metrics_kernel + metrics_finalize) / "
                                 "one pp_siti call (siti_kernel + siti_finalize)",
                           pp_metrics=callbench.throughput(m_ms, 2 * n * fb),
                           pp_siti_luma=callbench.throughput(s_ms, n * w * h * 2))
    res["metrics_vs_siti_per_byte"] = round(res["pp_metrics"]["GBps"] / res["pp_siti_luma"]["GBps"], 3)
    sse, ssim = out["m"]
    res["check"] = {"sse_sum": int(sse.sum().item()), "ssim_mean_y": float(ssim[:, 0].mean().item())}
    callbench.emit(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
