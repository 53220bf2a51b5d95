#!/usr/bin/env python3
"""Time pp_adm (PP-ADM-1) on one MI355X with HIP events, next to pp_vif and
pp_metrics on the same buffers in the same process.

Shape: --frames (600) frames of 1920x1080, 8-bit (yuv420p) and 10-bit
(yuv420p10le), distorted = reference + bounded noise.
  adm       one ops.adm call over the clip's luma (four fused scale kernels
            and the finalize of every launch)
  vif       one ops.vif call over the same luma
  metrics   one ops.metrics call over the same batches (all three planes)
The box-to-box spread cancels in the ratios.  Before timing, the GPU sums of
the first frame are compared with the tests' numpy fp64 restatement in its
rows-then-columns form (tests/adm_ref.py: terms with separable=True) at 1e-7
relative, after checking that no position of that frame has its angle test
within reach of flipping (adm_ref.near_branch).  Next to the time the json records the fp64
instructions the algorithm needs per coefficient position (an FMA counted
once): 32 along the rows (two new input rows x two planes x two filters x four
taps), 32 down the columns (four bands x two planes x four taps), and about 140
for the decoupling (three IEEE divisions of about 30 each, the angle test, the
products with rf), the threshold and the six cubes: 204; their rate, and that
rate's share of the vector fp64 issue rate (256 CUs x 4 SIMDs x 16 lanes a
clock x 2.4 GHz = 39.3e12 instructions/s).  The same count for pp_vif is
13 N + 200 per position of an N-tap scale.
Prints one JSON line; a measurement, not a gate; it fails without a GPU.

  python tools/adm_bench.py [--frames 600] [--out profiles/adm/NAME.json]
"""
import sys

import callbench

INSTR_POSITION = 204
VIF_TAPS = (17, 9, 5, 3)


def one_depth(fmt, a, dev):
    import numpy as np
    import torch

    import adm_ref
    from pixpath import adm, ops
    w, h, n = callbench.W, callbench.H, a.frames
    ten = fmt.endswith("10le")
    depth = 10 if ten else 8
    ref, dist = callbench.noise_pair(fmt, n, dev)
    keep = {}

    def adm_pass():
        keep["adm"] = ops.adm(ref, dist)

    def vif_pass():
        keep["vif"] = ops.vif(ref, dist)

    def met_pass():
        keep["met"] = ops.metrics(ref, dist)

    adm_pass()
    torch.cuda.synchronize()
    got = keep["adm"].cpu().numpy()
    ya, yb = (t.view(0)[0].cpu().numpy() for t in (ref, dist))
    want, near = adm_ref.terms(ya, yb, depth, separable=True), sum(adm_ref.near_branch(ya, yb, depth))
    if near:
        raise SystemExit("adm_bench: %d positions of the checked frame sit on the angle branch: use another seed" % near)
    worst = float(np.abs(got[0] / want - 1).max())
    if not worst <= 1e-7:
        raise SystemExit("adm_bench: %s differs from the CPU evaluation by %.3e relative" % (fmt, worst))
    if np.isnan(got).any():
        raise SystemExit("adm_bench: NaN in the result")
    ad = callbench.timed(adm_pass, a.warmup, a.iters)
    vf = callbench.timed(vif_pass, a.warmup, a.iters)
    met = callbench.timed(met_pass, a.warmup, a.iters)
    positions = [n * ws * hs for ws, hs in adm.scale_sizes(w, h)]
    instr = sum(positions) * INSTR_POSITION
    rate = instr / (ad["avg_ms"] * 1e-3)
    vif_instr = sum(n * (w >> s) * (h >> s) * (13 * VIF_TAPS[s] + 200) for s in range(4))
    # bytes that must move: both planes read once, the A bands of levels 0 .. 2 written and read once
    es = 2 if ten else 1
    traffic = n * 2 * (w * h * es + 2 * 8 * sum(ws * hs for ws, hs in adm.scale_sizes(w, h)[:3]))
    return {"fmt": fmt, "adm": ad, "vif": vf, "metrics": met,
            "adm_over_vif": round(ad["avg_ms"] / vf["avg_ms"], 3), "adm_over_metrics": round(ad["avg_ms"] / met["avg_ms"], 2),
            "positions": positions, "fp64_instr": instr, "fp64_instr_over_vif": round(instr / vif_instr, 3),
            "fp64_instr_per_s": float("%.4g" % rate), "share_of_fp64_issue_rate": round(rate / callbench.FP64_ISSUE_RATE, 3),
            "vif_share_of_fp64_issue_rate": round(vif_instr / (vf["avg_ms"] * 1e-3) / callbench.FP64_ISSUE_RATE, 3),
            "algorithmic_bytes": traffic, "tb_per_s": round(traffic / (ad["avg_ms"] * 1e-3) / 1e12, 3),
            "cpu_check_max_rel": worst}


def main(argv=None):
    ap = callbench.parser(600, 3, 20)
    a = ap.parse_args(argv)
    dev = callbench.require_gpu("adm_bench", seed=910)
    res = callbench.header(
        "adm_bench", a,
        timer="HIP events around one call over the clip: every launch of pp_adm (adm_scale x 4, adm_finalize) "
              "/ of pp_vif / of pp_metrics (three planes)",
        fp64_issue_rate_per_s=callbench.FP64_ISSUE_RATE, fp64_instr_per_position=INSTR_POSITION,
        depths=[one_depth(f, a, dev) for f in ("yuv420p", "yuv420p10le")])
    callbench.emit(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
