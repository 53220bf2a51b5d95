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
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "processing-chain_amd"))

HBM_PEAK = 8.0e12  # B/s


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
    return ms


def stats(ms, nbytes):
    avg = sum(ms) / len(ms)
    return {"avg_launch_ms": round(avg, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "bytes": nbytes, "GBps": round(nbytes / avg / 1e6, 1), "frac": round(nbytes / (avg * 1e-3) / HBM_PEAK, 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("unpack_bench: no GPU visible (a timing needs the MI355X)")
    from pixpath import formats, ops
    from pixpath.frames import FrameBatch
    w, h, n = 1920, 1080, a.frames
    dev = torch.device("cuda", 0)
    torch.manual_seed(210)
    res = {"tool": "unpack_bench", "device": torch.cuda.get_device_name(0), "w": w, "h": h, "frames": n,
           "warmup": a.warmup, "iters": a.iters,
           "timer": "HIP events around one pp_unpack_execute / one pp_cpvs_execute call (one kernel each)"}
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
        pack_ms = timed(lambda: ops.cpvs(src, w, h, dst=pk), a.warmup, a.iters)
        unpack_ms = timed(lambda: ops.unpack(pk, dst=back), a.warmup, a.iters)
        torch.cuda.synchronize()
        same = all(bool(torch.equal(back.view(p), src.view(p))) for p in range(3))
        entry = {"algorithmic_bytes_per_frame": pbytes + ubytes,
                 "unpack": stats(unpack_ms, n * (pbytes + ubytes)),
                 "pack_cpvs": stats(pack_ms, n * (pbytes + ubytes)),
                 "round_trip_equal": same}
        entry["unpack_time_per_byte_vs_pack"] = round(entry["unpack"]["avg_launch_ms"] /
                                                      entry["pack_cpvs"]["avg_launch_ms"], 3)
        res["%s_to_%s" % (packed, planar)] = entry
        if packed == "v210":
            luma = torch.empty((n, h, w), dtype=torch.uint16, device=dev)
            lbytes = ubytes + w * h * 2
            luma_ms = timed(lambda: ops.unpack(pk, luma_only=True, dst=luma), a.warmup, a.iters)
            torch.cuda.synchronize()
            res["v210_to_luma"] = {"algorithmic_bytes_per_frame": lbytes, "unpack": stats(luma_ms, n * lbytes),
                                   "luma_equal": bool(torch.equal(luma, src.view(0)))}
        del src, pk, back
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
