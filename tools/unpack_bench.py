#!/usr/bin/env python3
"""Time pp_unpack_execute on one MI355X with HIP events, each next to the
packer that moves the same bytes the other way (pp_cpvs_execute, no pad) in
the same process.

Shape: --frames (600) frames of 1920x1080.  Algorithmic bytes per frame =
packed frame read once + planar output written once (the packer: the reverse):
  v210 -> yuv422p10le      5,529,600 + 8,294,400 = 13,824,000
  uyvy422 -> yuv422p       4,147,200 + 4,147,200 =  8,294,400
  v210 -> luma only        5,529,600 + 4,147,200 =  9,676,800
Prints one JSON line: avg / min / max launch time over --iters (>= 20) timed
launches after --warmup, GB/s and `frac` = bytes / time / 8 TB/s (the HBM
peak) for both directions, and unpack's time per byte over the packer's.  A
measurement, not a gate; it fails without a GPU.

  python tools/unpack_bench.py [--frames 600] [--out profiles/unpack/NAME.json]
"""
import sys

import callbench


def main(argv=None):
    ap = callbench.parser(600, 3, 20)
    a = ap.parse_args(argv)
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    dev = callbench.require_gpu("unpack_bench", seed=210)
    import torch
    from pixpath import formats, ops
    from pixpath.frames import FrameBatch
    w, h, n = callbench.W, callbench.H, a.frames
    res = callbench.header("unpack_bench", a, callbench.HEAD + ("iters",),
                           timer="HIP events around one pp_unpack_execute / one pp_cpvs_execute call (one kernel each)")
    for planar, packed in (("yuv422p10le", "v210"), ("yuv422p", "uyvy422")):
        src = FrameBatch(planar, w, h, n, device=dev)
        lo, hi = (64, 941) if planar == "yuv422p10le" else (16, 236)
        for p in range(3):
            t = src.planes[p].view(torch.int16) if src.bps == 2 else src.planes[p]
            for k in range(n):  # frame by frame: no batch-sized temporaries
                t[k].random_(lo, hi)
        pk = FrameBatch(packed, w, h, n, device=dev)
        back = FrameBatch(planar, w, h, n, device=dev)
        pbytes, ubytes = formats.frame_bytes(planar, w, h), formats.frame_bytes(packed, w, h)
        pack_ms = callbench.times(lambda: ops.cpvs(src, w, h, dst=pk), a.warmup, a.iters)
        unpack_ms = callbench.times(lambda: ops.unpack(pk, dst=back), a.warmup, a.iters)
        torch.cuda.synchronize()
        same = all(bool(torch.equal(back.view(p), src.view(p))) for p in range(3))
        entry = {"algorithmic_bytes_per_frame": pbytes + ubytes,
                 "unpack": callbench.throughput(unpack_ms, n * (pbytes + ubytes)),
                 "pack_cpvs": callbench.throughput(pack_ms, n * (pbytes + ubytes)),
                 "round_trip_equal": same}
        entry["unpack_time_per_byte_vs_pack"] = round(entry["unpack"]["avg_launch_ms"] /
                                                      entry["pack_cpvs"]["avg_launch_ms"], 3)
        res["%s_to_%s" % (packed, planar)] = entry
        if packed == "v210":
            luma = torch.empty((n, h, w), dtype=torch.uint16, device=dev)
            lbytes = ubytes + w * h * 2
            luma_ms = callbench.times(lambda: ops.unpack(pk, luma_only=True, dst=luma), a.warmup, a.iters)
            torch.cuda.synchronize()
            res["v210_to_luma"] = {"algorithmic_bytes_per_frame": lbytes, "unpack": callbench.throughput(luma_ms, n * lbytes),
                                   "luma_equal": bool(torch.equal(luma, src.view(0)))}
        del src, pk, back
    callbench.emit(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
