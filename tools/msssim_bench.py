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
with the tests' numpy fp64 restatement in its rows-then-columns form
(tests/msssim_ref.py: terms_separable) at 1e-9.  The kernel is bound by fp64
arithmetic, so next to the time the json records the fp64 instructions the algorithm needs (an FMA counted once:
33 products + 55 FMAs along the rows, 55 FMAs along the columns and about 27
for l and cs with their two divisions = 170 per window), their rate, and that
rate's share of the vector fp64 issue rate (256 CUs x 4 SIMDs x 16 lanes a
clock x 2.4 GHz = 39.3e12 instructions/s, i.e. the 78.6 TFLOPS peak counted in
FMAs).  Prints one JSON line; a measurement, not a gate; it fails without a GPU.

  python tools/msssim_bench.py [--frames 600] [--out profiles/msssim/NAME.json]
"""
import sys

import callbench

INSTR_PER_WINDOW = 170


def one_depth(fmt, a, dev):
    import numpy as np
    import torch

    import msssim_ref
    from pixpath import ops
    w, h, n = callbench.W, callbench.H, a.frames
    depth = 10 if fmt.endswith("10le") else 8
    ref, dist = callbench.noise_pair(fmt, n, dev)
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
        worst = max(worst, float(np.abs(got[k] - msssim_ref.terms_separable(ya, yb, depth)).max()))
    if not worst <= 1e-9:
        raise SystemExit("msssim_bench: %s differs from the CPU evaluation by %.3e" % (fmt, worst))
    ms = callbench.timed(ms_pass, a.warmup, a.iters)
    met = callbench.timed(met_pass, a.warmup, a.iters)
    windows = n * sum(((w >> s) - 10) * ((h >> s) - 10) for s in range(5))
    rate = windows * INSTR_PER_WINDOW / (ms["avg_ms"] * 1e-3)
    return {"fmt": fmt, "ms_ssim": ms, "metrics": met, "ms_ssim_over_metrics": round(ms["avg_ms"] / met["avg_ms"], 2),
            "windows": windows, "fp64_instr_per_window": INSTR_PER_WINDOW, "fp64_instr_per_s": float("%.4g" % rate),
            "share_of_fp64_issue_rate": round(rate / callbench.FP64_ISSUE_RATE, 3), "cpu_check_max_abs": worst}


def main(argv=None):
    ap = callbench.parser(600, 3, 20)
    a = ap.parse_args(argv)
    dev = callbench.require_gpu("msssim_bench", seed=910)
    res = callbench.header(
        "msssim_bench", a,
        timer="HIP events around one call over the clip: every launch of pp_ms_ssim (pyramids, msssim_kernel, "
              "msssim_finalize) / of pp_metrics (metrics_kernel + metrics_finalize, three planes)",
        fp64_issue_rate_per_s=callbench.FP64_ISSUE_RATE,
        depths=[one_depth(f, a, dev) for f in ("yuv420p", "yuv420p10le")])
    callbench.emit(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
