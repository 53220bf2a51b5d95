#!/usr/bin/env python3
"""Time pp_motion (PP-MOTION-1) on one MI355X with HIP events, next to pp_siti
and pp_frame_stats (with sad) on the same buffers in the same process.

Shape: --frames (600) frames of 1920x1080 luma, 8-bit (yuv420p) and 10-bit
(yuv420p10le), noise over the legal range.
  motion    one ops.motion call over the clip's luma (motion_kernel and
            motion_finalize of every launch of 256 frames)
  siti      one ops.siti call over the same luma: the neighbour with the same
            temporal structure (the previous frame kept on chip)
  stats     one ops.frame_stats call with sad over the same batch (all three
            planes, histograms included): the raw-sample SAD
The box-to-box spread cancels in the ratios.  Before timing, the GPU sums of
the first frames are compared with a CPU restatement (numpy int64 on
`reflect`-padded planes) for equality.  Next to the time the json records the
bytes the algorithm must move (every luma sample read once) and their rate
against the HBM peaks (8.0 TB/s spec, 6.29 TB/s measured copy).
Prints one JSON line; a measurement, not a gate; it fails without a GPU.

  python tools/motion_bench.py [--frames 600] [--out profiles/motion/NAME.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "processing-chain_amd"))

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
CHECKED = 6  # frames compared with the CPU: a segment seam among them


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


def cpu_sad(y, depth):
    """PP-MOTION-1 sums of the planes y [n, h, w] in numpy int64; entry 0 absent."""
    import numpy as np

    from pixpath import motion
    f = motion.TAPS

    def blur(p):
        x = np.minimum(p.astype(np.int64), (1 << depth) - 1)
        h, w = x.shape
        q = np.pad(x, ((2, 2), (0, 0)), mode="reflect")
        t = (sum(f[k] * q[k:k + h] for k in range(5)) + (1 << (depth - 1))) >> depth
        q = np.pad(t, ((0, 0), (2, 2)), mode="reflect")
        return (sum(f[k] * q[:, k:k + w] for k in range(5)) + 32768) >> 16
    b = [blur(p) for p in y]
    return [motion.SAD_ABSENT] + [int(np.abs(b[k] - b[k - 1]).sum()) for k in range(1, len(b))]


def one_depth(fmt, a, dev):
    import torch

    from pixpath import ops
    from pixpath.frames import FrameBatch
    w, h, n = 1920, 1080, a.frames
    ten = fmt.endswith("10le")
    depth = 10 if ten else 8
    lo, hi = (64, 941) if ten else (16, 236)
    src = FrameBatch(fmt, w, h, n, device=dev)
    for p in range(3):
        sp = src.planes[p].view(torch.int16) if ten else src.planes[p]
        for k in range(n):  # frame by frame: no batch-sized temporaries
            sp[k].copy_(torch.randint(lo, hi, sp[k].shape, dtype=torch.int16, device=dev))
    torch.cuda.synchronize()
    keep = {}

    def motion_pass():
        keep["motion"] = ops.motion(src)

    def siti_pass():
        keep["siti"] = ops.siti(src.view(0), depth)

    def stats_pass():
        keep["stats"] = ops.frame_stats(src)

    motion_pass()
    torch.cuda.synchronize()
    got = [int(v) for v in keep["motion"].cpu().numpy()]
    want = cpu_sad(src.view(0)[:CHECKED].cpu().numpy(), depth)
    if got[:CHECKED] != want:
        raise SystemExit("motion_bench: %s differs from the CPU restatement: %r against %r" % (fmt, got[:CHECKED], want))
    mo = timed(motion_pass, a.warmup, a.iters)
    si = timed(siti_pass, a.warmup, a.iters)
    st = timed(stats_pass, a.warmup, a.iters)
    traffic = n * w * h * (2 if ten else 1)  # every luma sample once
    rate = traffic / (mo["avg_ms"] * 1e-3)
    return {"fmt": fmt, "motion": mo, "siti": si, "stats_sad": st,
            "motion_over_siti": round(mo["avg_ms"] / si["avg_ms"], 3),
            "motion_over_stats_sad": round(mo["avg_ms"] / st["avg_ms"], 3),
            "algorithmic_bytes": traffic, "tb_per_s": round(rate / 1e12, 3),
            "share_of_hbm_spec": round(rate / HBM_SPEC, 3), "share_of_hbm_copy": round(rate / HBM_COPY, 3),
            "cpu_check_frames": CHECKED, "cpu_check": "equal"}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("motion_bench: no GPU visible (a timing needs the MI355X)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(910)
    res = {"tool": "motion_bench", "device": torch.cuda.get_device_name(0), "w": 1920, "h": 1080, "frames": a.frames,
           "warmup": a.warmup,
           "timer": "HIP events around one call over the clip: every launch of pp_motion (motion_kernel, "
                    "motion_finalize) / of pp_siti (luma) / of pp_frame_stats with sad (three planes, histograms)",
           "hbm_spec_bytes_per_s": HBM_SPEC, "hbm_copy_bytes_per_s": HBM_COPY,
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
