#!/usr/bin/env python3
"""Time pp_frame_stats (PP-STATS-1) on one MI355X with HIP events.

Shape: --frames (600) frames of 1920x1080 as yuv422p10le and as yuv420p, three
contents each:
  noise     uniform over the legal range (64..940 / 64..960; 16..235 / 16..240)
  smooth    the FFV1 bench's moving gradients plus +-4 (8-bit: +-1) noise
  constant  Y 64 / C 512 (8-bit: Y 16 / C 128): every sample of a plane in one
            bin, the histogram's hard case and this tool's normal one
For each: avg / min / max / median time of one pp_frame_stats call (stat_kernel
+ stat_finalize) with and without `sad`, over --iters (>= 20) timed calls after
--warmup, and in the same process on the same buffers pp_frame_adler32 (the
yardstick: it reads the same bytes once and has no contention) and pp_siti on
the 10-bit luma.  The calls are taken in turn so that drift hits all alike.
`bytes` are algorithmic: every sample once (the histograms, 600 x 3 x 1024 x 4 B
= 7.4 MB, are not counted); `frac` = bytes / avg time / 8 TB/s (the HBM peak).
Reported per content: the ratio of pp_frame_adler32's time to pp_frame_stats'
(1.0 = as fast as the yardstick), and constant against noise.  Frames 0 and 1
of every buffer are compared with numpy before anything is timed.  A
measurement, not a gate; it fails without a GPU.

  python tools/stats_bench.py [--frames 600] [--out profiles/stats/NAME.json]
"""
import os
import sys

import callbench

CONTENTS = ("noise", "smooth", "constant")


def fill(batch, content, seed):
    """Frame by frame: no batch-sized temporaries."""
    import torch
    dev = batch.device
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    ten = batch.fmt.depth == 10
    s = 4 if ten else 1
    for p in range(3):
        v = batch.view(p)
        yy = torch.arange(v.shape[1], device=dev, dtype=torch.int32).view(-1, 1)
        xx = torch.arange(v.shape[2], device=dev, dtype=torch.int32).view(1, -1)
        for k in range(batch.n):
            if content == "noise":
                t = torch.randint(16 * s, (235 if p == 0 else 240) * s + 1, v.shape[1:], generator=g, device=dev,
                                  dtype=torch.int32)
            elif content == "smooth":
                a = 4 if ten else 1
                noise = torch.randint(-a, a + 1, v.shape[1:], generator=g, device=dev, dtype=torch.int32)
                t = ((xx * (p + 1) + yy * 2 + 3 * k) % (200 * s) + 25 * s + noise).clamp(16 * s, 235 * s)
            else:
                t = torch.full(v.shape[1:], (16 if p == 0 else 128) * s, device=dev, dtype=torch.int32)
            v[k].copy_(t.to(v.dtype))


def verify(batch):
    import numpy as np
    import torch
    from pixpath import ops
    from pixpath.frames import FrameBatch
    two = FrameBatch(batch.fmt, batch.w, batch.h, 2, planes=[t[:2] for t in batch.planes])
    hist, sad, over = ops.frame_stats(two)
    torch.cuda.synchronize()
    hist, sad = hist.cpu().numpy(), sad.cpu().numpy()
    bins = 1 << batch.fmt.depth
    for p in range(3):
        a = two.view(p).cpu().numpy().astype(np.int64)
        for k in range(2):
            if not np.array_equal(np.bincount(a[k].reshape(-1), minlength=bins), hist[k, p]):
                raise SystemExit("stats_bench: histogram of frame %d plane %d differs from numpy" % (k, p))
        if int(np.abs(a[1] - a[0]).sum()) != int(sad[1, p]):
            raise SystemExit("stats_bench: sad of plane %d differs from numpy" % p)
    if over.cpu().numpy().any():
        raise SystemExit("stats_bench: samples above the container")


def main(argv=None):
    ap = callbench.parser(600, 3, 20)
    ap.add_argument("--contents", default=",".join(CONTENTS))
    a = ap.parse_args(argv)
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    dev = callbench.require_gpu("stats_bench")
    import torch
    from pixpath import _native, formats, ops
    from pixpath.frames import FrameBatch
    w, h, n = callbench.W, callbench.H, a.frames
    b10, b8 = FrameBatch("yuv422p10le", w, h, n, device=dev), FrameBatch("yuv420p", w, h, n, device=dev)
    nb10, nb8 = n * formats.frame_bytes("yuv422p10le", w, h), n * formats.frame_bytes("yuv420p", w, h)
    res = callbench.header("stats_bench", a, callbench.HEAD + ("iters",),
                           timer="HIP events around one ops call (kernel + finalize), the calls taken in turn",
                           bytes="algorithmic: every sample once; the histograms (%d B for yuv422p10le) are not counted"
                                 % (n * 3 * 1024 * 4),
                           library=os.path.basename(_native.LIB_PATH))
    if "PIXPATH_LIB" in os.environ:  # a measurement build: record its knobs
        res["PIXPATH_STATS_ABL"] = os.environ.get("PIXPATH_STATS_ABL", "0")
    out = {}
    for ci, content in enumerate(a.contents.split(",")):
        fill(b10, content, 910 + ci)
        fill(b8, content, 920 + ci)
        torch.cuda.synchronize()
        verify(b10)
        verify(b8)
        luma = b10.planes[0]
        fns = {
            "stats_yuv422p10le": lambda: out.__setitem__("a", ops.frame_stats(b10)),
            "stats_nosad_yuv422p10le": lambda: out.__setitem__("b", ops.frame_stats(b10, want_sad=False)),
            "adler_yuv422p10le": lambda: out.__setitem__("c", ops.frame_adler32(b10)),
            "pp_siti_luma": lambda: out.__setitem__("d", ops.siti(luma, 10)),
            "stats_yuv420p": lambda: out.__setitem__("e", ops.frame_stats(b8)),
            "stats_nosad_yuv420p": lambda: out.__setitem__("f", ops.frame_stats(b8, want_sad=False)),
            "adler_yuv420p": lambda: out.__setitem__("g", ops.frame_adler32(b8)),
        }
        ms = callbench.timed_round_robin(fns, a.warmup, a.iters)
        r = {k: callbench.throughput(ms[k], n * w * h * 2 if k == "pp_siti_luma" else nb10 if "10le" in k else nb8,
                                     median=True, rate=("TBps", 1e9, 3)) for k in fns}
        r["vs_adler"] = {k: round(r["adler_" + k.split("_")[-1]]["avg_launch_ms"] / r[k]["avg_launch_ms"], 3)
                         for k in fns if k.startswith("stats")}
        res[content] = r
    if "constant" in res and "noise" in res:
        res["constant_vs_noise_time"] = {k: round(res["constant"][k]["avg_launch_ms"] / res["noise"][k]["avg_launch_ms"], 3)
                                         for k in res["noise"] if k.startswith("stats")}
    callbench.emit(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
