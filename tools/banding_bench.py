#!/usr/bin/env python3
"""Time pp_banding (PP-BAND-1) on one MI355X with HIP events, next to
pp_ms_ssim and pp_frame_stats on the same buffers in the same process.

Shape: --frames (600) frames of 1920x1080 luma, 8-bit (yuv420p) and 10-bit
(yuv420p10le), at the default window (33), on three contents:
  banded    a slanted staircase, one code every 24 samples: every position is
            masked and walks its whole window (the contrast kernel's worst case)
  noise     noise over the legal range: every position unmasked, no window work
  constant  one value: every position masked, every Q in bin 0 (the
            histogram's hard case) and every window walked
  banding   one ops.banding call over the clip's luma (clear, banding_prep,
            four banding_down and banding_contrast of every launch)
  ms_ssim   one ops.ms_ssim call of the clip against itself (five scales too)
  stats     one ops.frame_stats call over the same batch (three planes)
The box-to-box spread cancels in the ratios.  Before timing, the GPU
histograms of the first frames are compared with the numpy restatement
(tests/banding_ref.py) for equality; its seconds per frame on one thread are
recorded: it is the only other implementation that exists.
Prints one JSON line; a measurement, not a gate; it fails without a GPU.

  python tools/banding_bench.py [--frames 600] [--out profiles/banding/NAME.json]
"""
import sys
import time

import callbench

CHECKED = 2  # frames compared with the restatement per content and depth
CONTENTS = ("banded", "noise", "constant")


def fill(src, content, ten, dev):
    import torch
    n, h, w = src.view(0).shape
    lo, hi = (64, 941) if ten else (16, 236)
    ii = torch.arange(h, device=dev, dtype=torch.int32)[:, None]
    jj = torch.arange(w, device=dev, dtype=torch.int32)[None, :]
    for p in range(3):
        sp = src.planes[p].view(torch.int16) if ten else src.planes[p]
        for k in range(n):  # frame by frame: no batch-sized temporaries
            if p or content == "constant":
                sp[k].fill_(512 if ten else 128)
            elif content == "noise":
                sp[k].copy_(torch.randint(lo, hi, sp[k].shape, dtype=torch.int16, device=dev))
            else:
                sp[k].copy_((lo + 40 + (jj + ii // 3 + k) // 24 % 150).to(torch.int16))
    torch.cuda.synchronize()


def one(fmt, content, a, dev):
    import numpy as np
    import torch

    import banding_ref
    from pixpath import banding, ops
    from pixpath.frames import FrameBatch
    w, h, n = callbench.W, callbench.H, a.frames
    ten = fmt.endswith("10le")
    depth = 10 if ten else 8
    window = banding.default_window(w, h)
    src = FrameBatch(fmt, w, h, n, device=dev)
    fill(src, content, ten, dev)
    keep = {}

    def banding_pass():
        keep["banding"] = ops.banding(src)

    def ms_pass():
        keep["ms"] = ops.ms_ssim(src, src)

    def stats_pass():
        keep["stats"] = ops.frame_stats(src)

    banding_pass()
    torch.cuda.synchronize()
    got = keep["banding"][:CHECKED].cpu().numpy()
    luma = src.view(0)[:CHECKED].cpu().numpy()
    t0 = time.perf_counter()
    want = banding_ref.hist(luma, depth, window)
    ref_s = (time.perf_counter() - t0) / CHECKED
    if not np.array_equal(got, want):
        raise SystemExit("banding_bench: %s %s differs from the restatement" % (fmt, content))
    val = banding.summarize(keep["banding"].cpu().numpy())["mean"]
    bd = callbench.timed(banding_pass, a.warmup, a.iters)
    ms = callbench.timed(ms_pass, a.warmup, a.iters)
    st = callbench.timed(stats_pass, a.warmup, a.iters)
    return {"fmt": fmt, "content": content, "window": window, "banding_y": val["banding_y"], "banding": bd,
            "ms_ssim": ms, "stats": st, "us_per_frame": round(bd["avg_ms"] * 1e3 / n, 2),
            "banding_over_ms_ssim": round(bd["avg_ms"] / ms["avg_ms"], 3),
            "banding_over_stats": round(bd["avg_ms"] / st["avg_ms"], 3),
            "restatement_s_per_frame": round(ref_s, 3), "cpu_check_frames": CHECKED, "cpu_check": "equal"}


def main(argv=None):
    ap = callbench.parser(600, 2, 10)
    a = ap.parse_args(argv)
    dev = callbench.require_gpu("banding_bench", seed=910)
    res = callbench.header(
        "banding_bench", a,
        timer="HIP events around one call over the clip: every launch of pp_banding / of pp_ms_ssim (the clip "
              "against itself) / of pp_frame_stats (three planes, histograms)",
        runs=[one(f, c, a, dev) for f in ("yuv420p", "yuv420p10le") for c in CONTENTS])
    callbench.emit(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
