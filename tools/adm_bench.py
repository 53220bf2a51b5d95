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
the first frame are compared with a CPU evaluation (numpy fp64, the filters
applied along rows then columns on the `reflect`-padded levels) at 1e-7
relative, after checking that no position of that frame has its angle test
within 1e-10 relative of flipping.  Next to the time the json records the fp64
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
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "processing-chain_amd"))

INSTR_POSITION = 204
VIF_TAPS = (17, 9, 5, 3)
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
    """PP-ADM-1 of two luma planes in numpy fp64: ([4][6] sums, positions near the angle branch)."""
    import numpy as np

    from pixpath import adm
    lo, hi = adm.filters()
    rf = adm.rf()
    cos2 = math.cos(math.pi / 180.0) ** 2

    def bands(p):
        h, w = p.shape
        ho, wo = (h + 1) // 2, (w + 1) // 2
        q = np.pad(p, ((1, 2), (1, 2)), mode="reflect")
        horiz = lambda f: sum(f[k] * q[:, k:k + 2 * wo:2] for k in range(4))
        vert = lambda x, f: sum(f[k] * x[k:k + 2 * ho:2] for k in range(4))
        L, Hh = horiz(lo), horiz(hi)
        return vert(L, lo), np.stack([vert(L, hi), vert(Hh, lo), vert(Hh, hi)])

    pa, pb = (x.astype(np.float64) / float(1 << (depth - 8)) for x in (a, b))
    out, near = np.full((4, 6), np.nan), 0
    for s, (ws, hs) in enumerate(adm.scale_sizes(a.shape[1], a.shape[0])):
        (pa, o), (pb, t) = bands(pa), bands(pb)
        k = np.where(o == 0, 0.0, np.clip(t / np.where(o == 0, 1.0, o), 0.0, 1.0))
        r = k * o
        d = t - r
        dp, om, tm = o[0] * t[0] + o[1] * t[1], o[0] * o[0] + o[1] * o[1], t[0] * t[0] + t[1] * t[1]
        lhs, rhs = dp * dp, cos2 * om * tm
        near += int(((dp >= 0) & (np.abs(lhs - rhs) <= 1e-10 * np.maximum(lhs, rhs))).sum())
        angle = (dp >= 0) & (lhs >= rhs)
        r, d = np.where(angle, t, r), np.where(angle, 0.0, d)
        m = sum(np.abs(rf[s, th] * d[th]) for th in range(3))
        box = sum(m[i:hs - 2 + i, j:ws - 2 + j] for i in range(3) for j in range(3)) - m[1:-1, 1:-1]
        M = box / 30.0 + m[1:-1, 1:-1] / 15.0
        mh, mw = adm.margin(hs), adm.margin(ws)
        M = M[mh - 1:hs - mh - 1, mw - 1:ws - mw - 1]
        cut = lambda x: x[mh:hs - mh, mw:ws - mw]
        out[s] = [(np.maximum(cut(np.abs(rf[s, th] * r[th])) - M, 0.0) ** 3).sum() for th in range(3)] \
            + [(cut(np.abs(rf[s, th] * o[th])) ** 3).sum() for th in range(3)]
    return out, near


def one_depth(fmt, a, dev):
    import numpy as np
    import torch

    from pixpath import adm, ops
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
    want, near = cpu_terms(ya, yb, depth)
    if near:
        raise SystemExit("adm_bench: %d positions of the checked frame sit on the angle branch: use another seed" % near)
    worst = float(np.abs(got[0] / want - 1).max())
    if not worst <= 1e-7:
        raise SystemExit("adm_bench: %s differs from the CPU evaluation by %.3e relative" % (fmt, worst))
    if np.isnan(got).any():
        raise SystemExit("adm_bench: NaN in the result")
    ad = timed(adm_pass, a.warmup, a.iters)
    vf = timed(vif_pass, a.warmup, a.iters)
    met = timed(met_pass, a.warmup, a.iters)
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
            "fp64_instr_per_s": float("%.4g" % rate), "share_of_fp64_issue_rate": round(rate / FP64_ISSUE_RATE, 3),
            "vif_share_of_fp64_issue_rate": round(vif_instr / (vf["avg_ms"] * 1e-3) / FP64_ISSUE_RATE, 3),
            "algorithmic_bytes": traffic, "tb_per_s": round(traffic / (ad["avg_ms"] * 1e-3) / 1e12, 3),
            "cpu_check_max_rel": worst}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("adm_bench: no GPU visible (a timing needs the MI355X)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(910)
    res = {"tool": "adm_bench", "device": torch.cuda.get_device_name(0), "w": 1920, "h": 1080, "frames": a.frames,
           "warmup": a.warmup,
           "timer": "HIP events around one call over the clip: every launch of pp_adm (adm_scale x 4, adm_finalize) "
                    "/ of pp_vif / of pp_metrics (three planes)",
           "fp64_issue_rate_per_s": FP64_ISSUE_RATE, "fp64_instr_per_position": INSTR_POSITION,
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
