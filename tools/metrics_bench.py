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
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "processing-chain_amd"))

HBM_PEAK = 8.0e12  # B/s


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
    return ms


def stats(ms, nbytes):
    avg = sum(ms) / len(ms)
    return {"avg_launch_ms": round(avg, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "bytes": nbytes, "GBps": round(nbytes / avg / 1e6, 1), "frac": round(nbytes / (avg * 1e-3) / HBM_PEAK, 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench: no GPU visible (a timing needs the MI355X)")
    from pixpath import formats, ops
    from pixpath.frames import FrameBatch
    fmt, w, h, n = "yuv422p10le", 1920, 1080, a.frames
    dev = torch.device("cuda", 0)
    torch.manual_seed(910)
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

    m_ms = timed(run_metrics, a.warmup, a.iters)
    luma = ref.planes[0]

    def run_siti():
        out["s"] = ops.siti(luma, 10)

    s_ms = timed(run_siti, a.warmup, a.iters)
    fb = formats.frame_bytes(fmt, w, h)
    res = {"tool": "metrics_bench", "device": torch.cuda.get_device_name(0), "fmt": fmt, "w": w, "h": h, "frames": n,
           "warmup": a.warmup, "iters": a.iters, "timer": "HIP events around one pp_metrics call "
           "(metrics_kernel + metrics_finalize) / one pp_siti call (siti_kernel + siti_finalize)",
           "pp_metrics": stats(m_ms, 2 * n * fb), "pp_siti_luma": stats(s_ms, n * w * h * 2)}
    res["metrics_vs_siti_per_byte"] = round(res["pp_metrics"]["GBps"] / res["pp_siti_luma"]["GBps"], 3)
    sse, ssim = out["m"]
    res["check"] = {"sse_sum": int(sse.sum().item()), "ssim_mean_y": float(ssim[:, 0].mean().item())}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
