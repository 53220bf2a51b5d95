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
the first frame are compared with a CPU evaluation (numpy fp64, windows applied
along rows then columns on the `reflect`-padded planes) at 1e-7 relative, after
checking that no position of that frame sits on one of the spec's branches.
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
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "processing-chain_amd"))

TAPS = (17, 9, 5, 3)
INSTR_POSITION = 200
MS_INSTR_PER_WINDOW = 170
FP64_ISSUE_RATE = 256 * 4 * 16 * 2.4e9
EPS = 1e-10


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
    """PP-VIF-1 of two luma planes in numpy fp64: ([4][2] sums, positions on a branch)."""
    import numpy as np

    def filt(p, s):
        n = TAPS[s]
        g = np.exp(-((np.arange(n) - n // 2) ** 2) / (2.0 * (n / 5.0) ** 2))
        g /= g.sum()
        q = np.pad(p, n // 2, mode="reflect")
        rows = sum(g[i] * q[:, i:i + p.shape[1]] for i in range(n))
        return sum(g[i] * rows[i:i + p.shape[0]] for i in range(n))

    pa, pb = (x.astype(np.float64) / float(1 << (depth - 8)) for x in (a, b))
    out, near = np.full((4, 2), np.nan), 0
    for s in range(4):
        if s:
            pa, pb = (filt(p, s)[0:2 * (p.shape[0] // 2):2, 0:2 * (p.shape[1] // 2):2] for p in (pa, pb))
        if min(pa.shape) < TAPS[s] // 2 + 1:
            break
        mu1, mu2 = filt(pa, s), filt(pb, s)
        s1 = np.maximum(filt(pa * pa, s) - mu1 * mu1, 0.0)
        s2 = np.maximum(filt(pb * pb, s) - mu2 * mu2, 0.0)
        s12 = filt(pa * pb, s) - mu1 * mu2
        g = s12 / (s1 + EPS)
        near += int(((np.abs(s1 - 2.0) <= 1e-6) | (np.abs(s1 - EPS) <= 1e-12) | (np.abs(s2 - EPS) <= 1e-12)
                     | (np.abs(g) <= 1e-9) | (np.abs(s12) <= 1e-9)).sum())
        sv = s2 - g * s12
        m = s1 < EPS
        g[m], sv[m], s1[m] = 0.0, s2[m], 0.0
        m = s2 < EPS
        g[m], sv[m] = 0.0, 0.0
        m = g < 0
        sv[m], g[m] = s2[m], 0.0
        sv = np.maximum(sv, EPS)
        g = np.minimum(g, 100.0)
        num = np.log2(1.0 + g * g * s1 / (sv + 2.0))
        den = np.log2(1.0 + s1 / 2.0)
        num[s12 < 0] = 0.0
        m = s1 < 2.0
        num[m] = 1.0 - s2[m] * 4.0 / 65025.0
        den[m] = 1.0
        out[s] = [num.sum(), den.sum()]
    return out, near


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
    want, near = cpu_terms(ya, yb, depth)
    if near:
        raise SystemExit("vif_bench: %d positions of the checked frame sit on a branch: use another seed" % near)
    worst = float(np.abs(got[0] / want - 1).max())
    if not worst <= 1e-7:
        raise SystemExit("vif_bench: %s differs from the CPU evaluation by %.3e relative" % (fmt, worst))
    if np.isnan(got).any():
        raise SystemExit("vif_bench: NaN in the result")
    vf = timed(vif_pass, a.warmup, a.iters)
    ms = timed(ms_pass, a.warmup, a.iters)
    met = timed(met_pass, a.warmup, a.iters)
    positions = [n * (w >> s) * (h >> s) for s in range(4)]
    instr = sum(p * (13 * TAPS[s] + INSTR_POSITION) for s, p in enumerate(positions))
    rate = instr / (vf["avg_ms"] * 1e-3)
    ms_instr = n * sum(((w >> s) - 10) * ((h >> s) - 10) for s in range(5)) * MS_INSTR_PER_WINDOW
    return {"fmt": fmt, "vif": vf, "ms_ssim": ms, "metrics": met,
            "vif_over_ms_ssim": round(vf["avg_ms"] / ms["avg_ms"], 2), "vif_over_metrics": round(vf["avg_ms"] / met["avg_ms"], 2),
            "positions": positions, "fp64_instr": instr, "fp64_instr_over_ms_ssim": round(instr / ms_instr, 2),
            "fp64_instr_per_s": float("%.4g" % rate), "share_of_fp64_issue_rate": round(rate / FP64_ISSUE_RATE, 3),
            "ms_ssim_share_of_fp64_issue_rate": round(ms_instr / (ms["avg_ms"] * 1e-3) / FP64_ISSUE_RATE, 3),
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
        raise SystemExit("vif_bench: no GPU visible (a timing needs the MI355X)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(910)
    res = {"tool": "vif_bench", "device": torch.cuda.get_device_name(0), "w": 1920, "h": 1080, "frames": a.frames,
           "warmup": a.warmup,
           "timer": "HIP events around one call over the clip: every launch of pp_vif (vif_decimate x 3, vif_stat x 4, "
                    "vif_finalize) / of pp_ms_ssim / of pp_metrics (three planes)",
           "fp64_issue_rate_per_s": FP64_ISSUE_RATE, "fp64_instr_per_position": "13 * taps + %d" % INSTR_POSITION,
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
