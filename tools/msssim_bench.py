#!/usr/bin/env python3
"""Time pp_ms_ssim (PP-MSSSIM-1) on one MI355X with HIP events, next to
pp_metrics on the same buffers in the same process.

Shape: --frames (600) frames of 1920x1080, 8-bit (yuv420p) and 10-bit
(yuv420p10le), distorted = reference + bounded noise.
  ms_ssim   one ops.ms_ssim call over the clip's luma (both pyramids, the
            window kernel and the finalize of every launch)
  metrics   one ops.metrics call over the same batches (PSNR / block SSIM of
            all three planes): the box-to-box spread cancels in the ratio
Before timing, the GPU values of the first and the last frame are compared
with a CPU evaluation (numpy fp64, window applied along rows then columns) at
1e-9.  The kernel is bound by fp64 arithmetic, so next to the time the json
records the fp64 instructions the algorithm needs (an FMA counted once:
33 products + 55 FMAs along the rows, 55 FMAs along the columns and about 27
for l and cs with their two divisions = 170 per window), their rate, and that
rate's share of the vector fp64 issue rate (256 CUs x 4 SIMDs x 16 lanes a
clock x 2.4 GHz = 39.3e12 instructions/s, i.e. the 78.6 TFLOPS peak counted in
FMAs).  Prints one JSON line; a measurement, not a gate; it fails without a GPU.

  python tools/msssim_bench.py [--frames 600] [--out profiles/msssim/NAME.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "processing-chain_amd"))

INSTR_PER_WINDOW = 170
FP64_ISSUE_RATE = 256 * 4 * 16 * 2.4e9


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
            "launches": len(ms)}


def cpu_terms(a, b, depth):
    """PP-MSSSIM-1 of two luma planes in numpy fp64: [5][2]."""
    import numpy as np
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / 4.5)
    g /= g.sum()
    L = float((1 << depth) - 1)
    c1, c2 = (.01 * L) ** 2, (.03 * L) ** 2
    out = np.full((5, 2), np.nan)
    for s in range(5):
        n = 1 << s
        hs, ws = a.shape[0] >> s, a.shape[1] >> s
        if min(hs, ws) < 11:
            continue
        pa, pb = (x[:hs * n, :ws * n].astype(np.int64).reshape(hs, n, ws, n).sum(axis=(1, 3)) / float(n * n) for x in (a, b))

        def f(p):
            rows = sum(g[i] * p[:, i:ws - 10 + i] for i in range(11))
            return sum(g[i] * rows[i:hs - 10 + i] for i in range(11))
        ma, mb, aa, bb, ab = f(pa), f(pb), f(pa * pa), f(pb * pb), f(pa * pb)
        l = (2 * ma * mb + c1) / (ma * ma + mb * mb + c1)
        cs = (2 * (ab - ma * mb) + c2) / ((aa - ma * ma) + (bb - mb * mb) + c2)
        out[s] = [cs.mean(), (l * cs).mean()]
    return out


def one_depth(fmt, a, dev):
    import numpy as np
    import torch

    from pixpath import ops
    from pixpath.frames import FrameBatch
    w, h, n = 1920, 1080, a.frames
    ten = fmt.endswith("10le")
    depth = 10 if ten else 8
    lo, hi = (64, 941) if ten else (16, 236)
    ref, dist = FrameBatch(fmt, w, h, n, device=dev), FrameBatch(fmt, w, h, n, device=dev)
    for p in range(3):
        rp, dp = (t.planes[p].view(torch.int16) if ten else t.planes[p] for t in (ref, dist))
        for k in range(n):  # frame by frame: no batch-sized temporaries
            r = torch.randint(lo, hi, rp[k].shape, dtype=torch.int16, device=dev)
            rp[k].copy_(r)
            dp[k].copy_((r + torch.randint(-8, 9, r.shape, dtype=torch.int16, device=dev)).clamp_(0, 1023 if ten else 255))
    torch.cuda.synchronize()
    keep = {}

    def ms_pass():
        keep["ms"] = ops.ms_ssim(ref, dist)

    def met_pass():
        keep["met"] = ops.metrics(ref, dist)

    ms_pass()
    torch.cuda.synchronize()
    got = keep["ms"].cpu().numpy()
    worst = 0.0
    for k in (0, n - 1):
        ya, yb = (t.view(0)[k].cpu().numpy() for t in (ref, dist))
        worst = max(worst, float(np.abs(got[k] - cpu_terms(ya, yb, depth)).max()))
    if not worst <= 1e-9:
        raise SystemExit("msssim_bench: %s differs from the CPU evaluation by %.3e" % (fmt, worst))
    ms = timed(ms_pass, a.warmup, a.iters)
    met = timed(met_pass, a.warmup, a.iters)
    windows = n * sum(((w >> s) - 10) * ((h >> s) - 10) for s in range(5))
    rate = windows * INSTR_PER_WINDOW / (ms["avg_ms"] * 1e-3)
    return {"fmt": fmt, "ms_ssim": ms, "metrics": met, "ms_ssim_over_metrics": round(ms["avg_ms"] / met["avg_ms"], 2),
            "windows": windows, "fp64_instr_per_window": INSTR_PER_WINDOW, "fp64_instr_per_s": float("%.4g" % rate),
            "share_of_fp64_issue_rate": round(rate / FP64_ISSUE_RATE, 3), "cpu_check_max_abs": worst}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("msssim_bench: no GPU visible (a timing needs the MI355X)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(910)
    res = {"tool": "msssim_bench", "device": torch.cuda.get_device_name(0), "w": 1920, "h": 1080, "frames": a.frames,
           "warmup": a.warmup,
           "timer": "HIP events around one call over the clip: every launch of pp_ms_ssim (pyramids, msssim_kernel, "
                    "msssim_finalize) / of pp_metrics (metrics_kernel + metrics_finalize, three planes)",
           "fp64_issue_rate_per_s": FP64_ISSUE_RATE,
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
