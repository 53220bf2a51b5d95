#!/usr/bin/env python3
"""Time pp_ciede (PP-CIEDE-1) on one MI355X with HIP events, next to pp_vif and
pp_metrics on the same buffers in the same process.

Shape: --frames (600) frames of 1920x1080, yuv420p and yuv422p10le, three
kinds of content:
  noise      reference and distorted clip independent uniform noise: every
             position runs the whole maths
  smooth     a diagonal ramp against itself with the chroma planes moved by 3
             code values: every position runs the maths, few take the dark
             (linear) segments
  identical  a clip against a copy of itself: every position takes the
             equal-samples shortcut, the call is its loads
  ciede      one ops.ciede call over the clip (ciede_kernel and ciede_finalize
             of every launch)
  vif        one ops.vif call over the same luma (noise content)
  metrics    one ops.metrics call over the same batches (noise content)
The box-to-box spread cancels in the ratios.  Before timing, the GPU sums of
the first two frames of every content are compared with the numpy restatement
(tests/ciede_ref.py) at 1e-9 relative.  Next to the time the json records the
fp64 instructions of the kernel's per-position body counted in its disassembly
(FP64_INSTR_POSITION: v_*_f64 of ciede_kernel, all but about 14 of them in the
body; a static count, so an upper bound on what a position executes: the
linear segments of the transfer curve and of f(t) skip a pow or a cbrt), the
rate that count gives and its share of the vector fp64 issue rate (256 CUs x 4
SIMDs x 16 lanes a clock x 2.4 GHz = 39.3e12 instructions/s).
Prints one JSON line; a measurement, not a gate; it fails without a GPU.

  python tools/ciede_bench.py [--frames 600] [--out profiles/ciede/NAME.json]
"""
import sys

import callbench

FP64_INSTR_POSITION = 2452  # 2466 v_*_f64 in ciede_kernel's disassembly less the 14 of the reduction
W, H = callbench.W, callbench.H


def fill(kind, fmt, n, dev):
    """(ref, dist) FrameBatches of one content, made on the device frame by frame."""
    import torch

    from pixpath.frames import FrameBatch
    ten = fmt.endswith("10le")
    s = 4 if ten else 1
    ref, dist = FrameBatch(fmt, W, H, n, device=dev), FrameBatch(fmt, W, H, n, device=dev)
    for p in range(3):
        rp, dp = (t.planes[p].view(torch.int16) if ten else t.planes[p] for t in (ref, dist))
        rows, cols = rp.shape[1:]
        lo, hi = (16 * s, (236 if p == 0 else 241) * s)
        ramp = (torch.arange(rows, device=dev)[:, None] * 3 + torch.arange(cols, device=dev)[None, :] * 2)
        for k in range(n):  # frame by frame: no batch-sized temporaries
            if kind == "smooth":
                r = (lo + (ramp + 5 * k) % (hi - lo)).to(torch.int16)
                d = r + (3 if p else 0)
            else:
                r = torch.randint(lo, hi, (rows, cols), dtype=torch.int16, device=dev)
                d = r if kind == "identical" else torch.randint(lo, hi, (rows, cols), dtype=torch.int16, device=dev)
            rp[k].copy_(r)
            dp[k].copy_(d)
    torch.cuda.synchronize()
    return ref, dist


def check(fmt, ref, dist, got):
    """The first two frames' sums and maxima against the restatement; the worst relative error."""
    import numpy as np

    import ciede_ref
    from pixpath import formats
    f = formats.fmt(fmt)
    planes = [[t.view(p)[:2].cpu().numpy() for p in range(3)] for t in (ref, dist)]
    want, _ = ciede_ref.ciede(planes[0], planes[1], f.depth, f.hsub, f.vsub)
    if not np.array_equal(want == 0, got[:2] == 0):
        raise SystemExit("ciede_bench: %s: zero sums differ from the restatement" % fmt)
    worst = float(np.abs(got[:2][want > 0] / want[want > 0] - 1).max()) if (want > 0).any() else 0.0
    if not worst <= 1e-9 or np.isnan(got).any():
        raise SystemExit("ciede_bench: %s differs from the restatement by %.3e relative" % (fmt, worst))
    return worst


def one_format(fmt, a, dev):
    import torch

    from pixpath import formats, ops
    n = a.frames
    res = {"fmt": fmt}
    for kind in ("noise", "smooth", "identical"):
        ref, dist = fill(kind, fmt, n, dev)
        keep = {}

        def ciede_pass():
            keep["ciede"] = ops.ciede(ref, dist, fmt)

        ciede_pass()
        torch.cuda.synchronize()
        got = keep["ciede"].cpu().numpy()
        worst = check(fmt, ref, dist, got)
        t = callbench.timed(ciede_pass, a.warmup, a.iters)
        px = n * W * H
        entry = {"ciede": t, "ns_per_pixel": round(t["avg_ms"] * 1e6 / px, 4), "restatement_max_rel": worst,
                 "mean_delta_e": float(got[:, 0].mean() / (W * H))}
        if kind != "identical":
            rate = px * FP64_INSTR_POSITION / (t["avg_ms"] * 1e-3)
            entry["fp64_instr_per_s_upper"] = float("%.4g" % rate)
            entry["share_of_fp64_issue_rate_upper"] = round(rate / callbench.FP64_ISSUE_RATE, 3)
        else:
            es = 2 if fmt.endswith("10le") else 1
            traffic = 2 * n * sum(r * c for r, c in formats.plane_shapes(fmt, W, H)) * es
            entry["algorithmic_bytes"] = traffic
            entry["tb_per_s"] = round(traffic / (t["avg_ms"] * 1e-3) / 1e12, 3)
        if kind == "noise":
            vf = callbench.timed(lambda: keep.__setitem__("vif", ops.vif(ref, dist)), a.warmup, a.iters)
            met = callbench.timed(lambda: keep.__setitem__("met", ops.metrics(ref, dist)), a.warmup, a.iters)
            entry.update({"vif": vf, "metrics": met, "ciede_over_vif": round(t["avg_ms"] / vf["avg_ms"], 3),
                          "ciede_over_metrics": round(t["avg_ms"] / met["avg_ms"], 2)})
            res["vif_ms"], res["metrics_ms"] = vf["avg_ms"], met["avg_ms"]
        else:
            entry.update({"ciede_over_vif": round(t["avg_ms"] / res["vif_ms"], 3),
                          "ciede_over_metrics": round(t["avg_ms"] / res["metrics_ms"], 2)})
        res[kind] = entry
        del ref, dist, keep
        torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = callbench.parser(600, 2, 10)
    a = ap.parse_args(argv)
    dev = callbench.require_gpu("ciede_bench", seed=910)
    res = callbench.header(
        "ciede_bench", a,
        timer="HIP events around one call over the clip: every launch of pp_ciede (ciede_kernel, ciede_finalize) "
              "/ of pp_vif (luma) / of pp_metrics (three planes)",
        fp64_issue_rate_per_s=callbench.FP64_ISSUE_RATE, fp64_instr_per_position_static=FP64_INSTR_POSITION,
        formats=[one_format(f, a, dev) for f in ("yuv420p", "yuv422p10le")])
    callbench.emit(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
