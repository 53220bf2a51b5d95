#!/usr/bin/env python3
"""Time pp_frame_adler32 (PP-HASH-1) on one MI355X with HIP events.

Shape: --frames (600) frames of 1920x1080 yuv422p10le, the same frames as
yuv420p (ops.Scaler's format conversion) and as v210 (ops.v210_pack).  For each
layout: avg / min / max / median time of one pp_frame_adler32 call (crc_kernel +
crc_finalize) over --iters (>= 20) timed calls after --warmup; `bytes` = the bytes PP-HASH-1 hashes, read once; `frac` =
bytes / avg time / 8 TB/s (the HBM peak).  In the same process, on the same
buffers, the two read-only reducers the parent commit has: pp_siti on the
10-bit luma and pp_metrics on the 10-bit batch against a noisy copy (it reads
two batches and computes SSIM windows), and pp_metrics on the yuv420p pair:
the yardstick is pp_metrics' bytes per second, which a kernel that only adds
bytes should not fall below.  Also one thread of zlib.adler32 over one frame's
bytes, the CPU figure.  The calls are taken in turn (adler, siti, metrics,
adler, ...) so that drift hits all alike.
Checksums of frame 0 are compared with zlib before anything is timed.  A
measurement, not a gate; it fails without a GPU.

  python tools/framecrc_bench.py [--frames 600] [--out profiles/framecrc/NAME.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "processing-chain_amd"))

HBM_PEAK = 8.0e12  # B/s


def timed_round_robin(fns, warmup, iters):
    """Event-pair times (ms) of each callable, the callables taken in turn."""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


def stats(ms, nbytes):
    avg = sum(ms) / len(ms)
    return {"avg_launch_ms": round(avg, 4), "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "bytes": nbytes, "GBps": round(nbytes / avg / 1e6, 1),
            "frac": round(nbytes / (avg * 1e-3) / HBM_PEAK, 4)}


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
        raise SystemExit("framecrc_bench: no GPU visible (a timing needs the MI355X)")
    from pixpath import formats, ops
    from pixpath.frames import FrameBatch
    fmt, w, h, n = "yuv422p10le", 1920, 1080, a.frames
    dev = torch.device("cuda", 0)
    torch.manual_seed(910)
    ref, dist = FrameBatch(fmt, w, h, n, device=dev), FrameBatch(fmt, w, h, n, device=dev)
    for p in range(3):
        r16, d16 = ref.planes[p].view(torch.int16), dist.planes[p].view(torch.int16)
        for k in range(n):  # frame by frame: no batch-sized temporaries
            r16[k].random_(64, 941)
            d16[k].copy_((r16[k] + torch.randint(-8, 9, r16[k].shape, dtype=torch.int16, device=dev)).clamp_(0, 1023))
    to420 = ops.Scaler(fmt, w, h, "yuv420p", w, h, device=dev)
    b420, d420 = to420(ref), to420(dist)
    bv210 = ops.v210_pack(ref)
    torch.cuda.synchronize()

    # exactness first: frame 0 of each layout against zlib on the host
    check = {}
    for name, b in (("yuv422p10le", ref), ("yuv420p", b420), ("v210", bv210)):
        got = int(ops.frame_adler32(b, 0).cpu()[0])
        s = b"".join(b.view(p)[0].cpu().numpy().tobytes() for p in range(len(b.planes)))
        want = zlib.adler32(s, 0) & 0xffffffff
        if got != want:
            raise SystemExit("framecrc_bench: %s frame 0: 0x%08x, zlib 0x%08x" % (name, got, want))
        check[name] = "0x%08x" % got
    frame = b"".join(ref.view(p)[0].cpu().numpy().tobytes() for p in range(3))
    t0 = time.perf_counter()
    reps = 20
    for _ in range(reps):
        zlib.adler32(frame, 0)
    cpu_s = (time.perf_counter() - t0) / reps

    out = {}
    luma = ref.planes[0]
    fns = {
        "adler_yuv422p10le": lambda: out.__setitem__("a", ops.frame_adler32(ref)),
        "pp_siti_luma": lambda: out.__setitem__("s", ops.siti(luma, 10)),
        "pp_metrics": lambda: out.__setitem__("m", ops.metrics(ref, dist)),
        "adler_yuv420p": lambda: out.__setitem__("b", ops.frame_adler32(b420)),
        "pp_metrics_yuv420p": lambda: out.__setitem__("n", ops.metrics(b420, d420)),
        "adler_v210": lambda: out.__setitem__("c", ops.frame_adler32(bv210)),
    }
    ms = timed_round_robin(fns, a.warmup, a.iters)
    nbytes = {"adler_yuv422p10le": n * formats.frame_bytes(fmt, w, h), "pp_siti_luma": n * w * h * 2,
              "pp_metrics": 2 * n * formats.frame_bytes(fmt, w, h),
              "adler_yuv420p": n * formats.frame_bytes("yuv420p", w, h),
              "pp_metrics_yuv420p": 2 * n * formats.frame_bytes("yuv420p", w, h),
              "adler_v210": n * formats.frame_bytes("v210", w, h)}
    res = {"tool": "framecrc_bench", "device": torch.cuda.get_device_name(0), "w": w, "h": h, "frames": n,
           "warmup": a.warmup, "iters": a.iters,
           "timer": "HIP events around one ops call (kernel + finalize), the six calls taken in turn",
           "frame0_equals_zlib": check}
    for k in fns:
        res[k] = stats(ms[k], nbytes[k])
    res["adler_vs_metrics_per_byte"] = {k: round(res[k]["GBps"] / res["pp_metrics"]["GBps"], 3)
                                        for k in fns if k.startswith("adler")}
    res["adler_yuv420p_vs_metrics_yuv420p_per_byte"] = round(res["adler_yuv420p"]["GBps"] /
                                                             res["pp_metrics_yuv420p"]["GBps"], 3)
    res["zlib_adler32_one_thread"] = {"bytes": len(frame), "ms_per_frame": round(cpu_s * 1e3, 4),
                                      "GBps": round(len(frame) / cpu_s / 1e9, 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
