#!/usr/bin/env python3
"""Time pp_vif (PP-VIF-1) on one MI355X with HIP events, next to pp_ms_ssim
and pp_metrics on the same buffers in the same process.

Shape: --frames (600) frames of 1920x1080, 8-bit (yuv420p) and 10-bit
(yuv420p10le), distorted = reference + bounded noise.
  vif       one ops.vif call over the clip's luma (three decimations, four
            statistics kernels and the finalize of every launch)
  ms_ssim   one ops.ms_ssim call over the same luma
  metrics   one ops.metrics call over the same batches (all three planes)
The box-to-box spread cancels in the ratios.  Before timing, the GPU sums of
the first frame are compared with the tests' numpy fp64 restatement in its
rows-then-columns form (tests/vif_ref.py: terms_separable) at 1e-7 relative,
after checking that no position of that frame sits on one of the spec's
branches (vif_ref.near_branch).
The kernels are bound by fp64 arithmetic, so next to the time the json records
the fp64 instructions the algorithm needs per position of a scale of N taps (an
FMA counted once: 3 N products + 5 N FMAs along the rows, 5 N FMAs along the
columns, and about 200 for the position's arithmetic with its three IEEE
divisions and two log2: 13 N + 200), their rate, and that rate's share of the
vector fp64 issue rate (256 CUs x 4 SIMDs x 16 lanes a clock x 2.4 GHz =
39.3e12 instructions/s).  The same count for pp_ms_ssim is 170 per window.
Prints one JSON line; a measurement, not a gate; it fails without a GPU.

  python tools/vif_bench.py [--frames 600] [--out profiles/vif/NAME.json]
"""
import sys

import callbench

TAPS = (17, 9, 5, 3)
INSTR_POSITION = 200
MS_INSTR_PER_WINDOW = 170


def one_depth(fmt, a, dev):
    import numpy as np
    import torch

    import vif_ref
    from pixpath import ops
    w, h, n = callbench.W, callbench.H, a.frames
    depth = 10 if fmt.endswith("10le") else 8
    ref, dist = callbench.noise_pair(fmt, n, dev)
    keep = {}

    def vif_pass():
        keep["vif"] = ops.vif(ref, dist)

    def ms_pass():
        keep["ms"] = ops.ms_ssim(ref, dist)

    def met_pass():
        keep["met"] = ops.metrics(ref, dist)

    vif_pass()
    torch.cuda.synchronize()
    got = keep["vif"].cpu().numpy()
    ya, yb = (t.view(0)[0].cpu().numpy() for t in (ref, dist))
    want, near = vif_ref.terms_separable(ya, yb, depth), sum(vif_ref.near_branch(ya, yb, depth))
    if near:
        raise SystemExit("vif_bench: %d positions of the checked frame sit on a branch: use another seed" % near)
    worst = float(np.abs(got[0] / want - 1).max())
    if not worst <= 1e-7:
        raise SystemExit("vif_bench: %s differs from the CPU evaluation by %.3e relative" % (fmt, worst))
    if np.isnan(got).any():
        raise SystemExit("vif_bench: NaN in the result")
    vf = callbench.timed(vif_pass, a.warmup, a.iters)
    ms = callbench.timed(ms_pass, a.warmup, a.iters)
    met = callbench.timed(met_pass, a.warmup, a.iters)
    positions = [n * (w >> s) * (h >> s) for s in range(4)]
    instr = sum(p * (13 * TAPS[s] + INSTR_POSITION) for s, p in enumerate(positions))
    rate = instr / (vf["avg_ms"] * 1e-3)
    ms_instr = n * sum(((w >> s) - 10) * ((h >> s) - 10) for s in range(5)) * MS_INSTR_PER_WINDOW
    return {"fmt": fmt, "vif": vf, "ms_ssim": ms, "metrics": met,
            "vif_over_ms_ssim": round(vf["avg_ms"] / ms["avg_ms"], 2), "vif_over_metrics": round(vf["avg_ms"] / met["avg_ms"], 2),
            "positions": positions, "fp64_instr": instr, "fp64_instr_over_ms_ssim": round(instr / ms_instr, 2),
            "fp64_instr_per_s": float("%.4g" % rate), "share_of_fp64_issue_rate": round(rate / callbench.FP64_ISSUE_RATE, 3),
            "ms_ssim_share_of_fp64_issue_rate": round(ms_instr / (ms["avg_ms"] * 1e-3) / callbench.FP64_ISSUE_RATE, 3),
            "cpu_check_max_rel": worst}


def main(argv=None):
    ap = callbench.parser(600, 3, 20)
    a = ap.parse_args(argv)
    dev = callbench.require_gpu("vif_bench", seed=910)
    res = callbench.header(
        "vif_bench", a,
        timer="HIP events around one call over the clip: every launch of pp_vif (vif_decimate x 3, vif_stat x 4, "
              "vif_finalize) / of pp_ms_ssim / of pp_metrics (three planes)",
        fp64_issue_rate_per_s=callbench.FP64_ISSUE_RATE, fp64_instr_per_position="13 * taps + %d" % INSTR_POSITION,
        depths=[one_depth(f, a, dev) for f in ("yuv420p", "yuv420p10le")])
    callbench.emit(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
