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
the first frames are compared with the tests' numpy int64 restatement
(tests/motion_ref.py: sad) for equality.  Next to the time the json records the
bytes the algorithm must move (every luma sample read once) and their rate
against the HBM peaks (8.0 TB/s spec, 6.29 TB/s measured copy).
Prints one JSON line; a measurement, not a gate; it fails without a GPU.

  python tools/motion_bench.py [--frames 600] [--out profiles/motion/NAME.json]
"""
import sys

import callbench

CHECKED = 6  # frames compared with the CPU: a segment seam among them


def one_depth(fmt, a, dev):
    import torch

    import motion_ref
    from pixpath import ops
    from pixpath.frames import FrameBatch
    w, h, n = callbench.W, callbench.H, a.frames
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
    want = motion_ref.sad(src.view(0)[:CHECKED].cpu().numpy(), depth)
    if got[:CHECKED] != want:
        raise SystemExit("motion_bench: %s differs from the CPU restatement: %r against %r" % (fmt, got[:CHECKED], want))
    mo = callbench.timed(motion_pass, a.warmup, a.iters)
    si = callbench.timed(siti_pass, a.warmup, a.iters)
    st = callbench.timed(stats_pass, a.warmup, a.iters)
    traffic = n * w * h * (2 if ten else 1)  # every luma sample once
    rate = traffic / (mo["avg_ms"] * 1e-3)
    return {"fmt": fmt, "motion": mo, "siti": si, "stats_sad": st,
            "motion_over_siti": round(mo["avg_ms"] / si["avg_ms"], 3),
            "motion_over_stats_sad": round(mo["avg_ms"] / st["avg_ms"], 3),
            "algorithmic_bytes": traffic, "tb_per_s": round(rate / 1e12, 3),
            "share_of_hbm_spec": round(rate / callbench.HBM_PEAK, 3), "share_of_hbm_copy": round(rate / callbench.HBM_COPY, 3),
            "cpu_check_frames": CHECKED, "cpu_check": "equal"}


def main(argv=None):
    ap = callbench.parser(600, 3, 20)
    a = ap.parse_args(argv)
    dev = callbench.require_gpu("motion_bench", seed=910)
    res = callbench.header(
        "motion_bench", a,
        timer="HIP events around one call over the clip: every launch of pp_motion (motion_kernel, "
              "motion_finalize) / of pp_siti (luma) / of pp_frame_stats with sad (three planes, histograms)",
        hbm_spec_bytes_per_s=callbench.HBM_PEAK, hbm_copy_bytes_per_s=callbench.HBM_COPY,
        depths=[one_depth(f, a, dev) for f in ("yuv420p", "yuv420p10le")])
    callbench.emit(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
