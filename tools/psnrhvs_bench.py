#!/usr/bin/env python3
"""Time pp_psnr_hvs (PP-HVS-1) on one MI355X with HIP events, next to pp_adm,
pp_ciede and pp_metrics on the same buffers in the same process.

Shape: --frames (600) frames of 1920x1080, yuv420p and yuv422p10le, block
steps 8 and 7, three kinds of content:
  noise      reference and distorted clip independent uniform noise
  smooth     a diagonal ramp against itself moved by 3 code values
  identical  a clip against a copy of itself: every sum is exactly 0
  psnr_hvs   one ops.psnr_hvs call over the clip (hvs_kernel and hvs_finalize
             of every launch)
  adm        one ops.adm call over the same luma (noise content)
  ciede      one ops.ciede call over the same batches (noise content)
  metrics    one ops.metrics call over the same batches (noise content)
The kernel has no data-dependent path, so the three contents should cost the
same; the tool measures that rather than assuming it.  The box-to-box spread
cancels in the ratios.  Before timing, the GPU sums of the first frame of
every content, format and step are compared with the numpy restatement
(tests/psnrhvs_ref.py): S_hvs at 1e-9 relative, S_hvsm within 1e-9 of S_hvs.
Next to the time the json records the fp64 instructions a block takes by the
static count of the disassembly (FP64_INSTR_LANE v_*_f64 in hvs_kernel, which
is straight-line code, times the 8 lanes of a block), the rate that gives and
its share of the vector fp64 issue rate (256 CUs x 4 SIMDs x 16 lanes a clock
x 2.4 GHz = 39.3e12 instructions/s).
Prints one JSON line; a measurement, not a gate; it fails without a GPU.

  python tools/psnrhvs_bench.py [--frames 600] [--out profiles/psnrhvs/NAME.json]
"""
import sys

import callbench

FP64_INSTR_LANE = 470  # v_*_f64 in hvs_kernel<uint8_t, true>'s disassembly (profiles/psnrhvs/kernel_resources.md)
FP64_INSTR_BLOCK = 8 * FP64_INSTR_LANE
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
                d = r + 3
            else:
                r = torch.randint(lo, hi, (rows, cols), dtype=torch.int16, device=dev)
                d = r if kind == "identical" else torch.randint(lo, hi, (rows, cols), dtype=torch.int16, device=dev)
            rp[k].copy_(r)
            dp[k].copy_(d)
    torch.cuda.synchronize()
    return ref, dist


def check(fmt, step, ref, dist, got):
    """The first frame's sums against the restatement; the worst differences (S_hvs relative, S_hvsm over S_hvs)."""
    import numpy as np

    import psnrhvs_ref
    planes = [[t.view(p)[:1].cpu().numpy() for p in range(3)] for t in (ref, dist)]
    want = psnrhvs_ref.psnr_hvs(planes[0], planes[1], step)
    g = got[:1]
    if np.isnan(g).any() or not np.array_equal(want[..., 0] == 0, g[..., 0] == 0) or (g[want[..., 0] == 0] != 0).any():
        raise SystemExit("psnrhvs_bench: %s step %d: zero sums differ from the restatement" % (fmt, step))
    nz = want[..., 0] > 0
    rel = float(np.abs(g[..., 0][nz] / want[..., 0][nz] - 1).max()) if nz.any() else 0.0
    relm = float((np.abs(g[..., 1][nz] - want[..., 1][nz]) / want[..., 0][nz]).max()) if nz.any() else 0.0
    if not (rel <= 1e-9 and relm <= 1e-9):
        raise SystemExit("psnrhvs_bench: %s step %d differs from the restatement by %.3e / %.3e" % (fmt, step, rel, relm))
    return rel, relm


def one_format(fmt, a, dev):
    import torch

    from pixpath import formats, ops, psnrhvs
    from pixpath.clips import json_value
    n = a.frames
    res = {"fmt": fmt}
    for kind in ("noise", "smooth", "identical"):
        ref, dist = fill(kind, fmt, n, dev)
        keep = {}
        entry = {}
        for step in psnrhvs.STEPS:
            def hvs_pass():
                keep["hvs"] = ops.psnr_hvs(ref, dist, step=step)

            hvs_pass()
            torch.cuda.synchronize()
            got = keep["hvs"].cpu().numpy()
            rel, relm = check(fmt, step, ref, dist, got)
            t = callbench.timed(hvs_pass, a.warmup, a.iters)
            nblk = n * sum(psnrhvs.blocks(fmt, W, H, step))
            rate = nblk * FP64_INSTR_BLOCK / (t["avg_ms"] * 1e-3)
            pooled = psnrhvs.summarize(got, W, H, None, fmt, step)["mean"]
            es = 2 if fmt.endswith("10le") else 1
            traffic = 2 * n * sum(r * c for r, c in formats.plane_shapes(fmt, W, H)) * es
            entry["step%d" % step] = {
                "psnr_hvs": t, "blocks": nblk, "ns_per_block": round(t["avg_ms"] * 1e6 / nblk, 4),
                "restatement_max_rel_hvs": rel, "restatement_max_hvsm_over_hvs": relm,
                "psnr_hvs_all": json_value(pooled["psnr_hvs_all"]), "psnr_hvsm_all": json_value(pooled["psnr_hvsm_all"]),
                "fp64_instr_per_s": float("%.4g" % rate), 
                "share_of_fp64_issue_rate": round(rate / callbench.FP64_ISSUE_RATE, 3),
                "algorithmic_bytes": traffic, "tb_per_s": round(traffic / (t["avg_ms"] * 1e-3) / 1e12, 3)}
        if kind == "noise":
            for name, fn in (("adm", lambda: ops.adm(ref, dist)), ("ciede", lambda: ops.ciede(ref, dist, fmt)),
                             ("metrics", lambda: ops.metrics(ref, dist))):
                entry[name] = callbench.timed(lambda fn=fn: keep.__setitem__("o", fn()), a.warmup, a.iters)
                res[name + "_ms"] = entry[name]["avg_ms"]
        for step in psnrhvs.STEPS:
            e = entry["step%d" % step]
            for name in ("adm", "ciede", "metrics"):
                e["psnr_hvs_over_" + name] = round(e["psnr_hvs"]["avg_ms"] / res[name + "_ms"], 3)
        res[kind] = entry
        del ref, dist, keep
        torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = callbench.parser(600, 2, 10)
    a = ap.parse_args(argv)
    dev = callbench.require_gpu("psnrhvs_bench", seed=910)
    res = callbench.header(
        "psnrhvs_bench", a,
        timer="HIP events around one call over the clip: every launch of pp_psnr_hvs (hvs_kernel, hvs_finalize) "
              "/ of pp_adm (luma) / of pp_ciede and pp_metrics (three planes)",
        fp64_issue_rate_per_s=callbench.FP64_ISSUE_RATE, fp64_instr_per_block_static=FP64_INSTR_BLOCK,
        formats=[one_format(f, a, dev) for f in ("yuv420p", "yuv422p10le")])
    callbench.emit(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
