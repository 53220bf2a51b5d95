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
import sys
import time
import zlib

import callbench


def main(argv=None):
    ap = callbench.parser(600, 3, 20)
    a = ap.parse_args(argv)
    if a.iters < 20:
        ap.error("--iters must be at least 20")
    dev = callbench.require_gpu("framecrc_bench", seed=910)
    import torch
    from pixpath import formats, ops
    from pixpath.frames import FrameBatch
    fmt, w, h, n = "yuv422p10le", callbench.W, callbench.H, a.frames
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
    ms = callbench.timed_round_robin(fns, a.warmup, a.iters)
    nbytes = {"adler_yuv422p10le": n * formats.frame_bytes(fmt, w, h), "pp_siti_luma": n * w * h * 2,
              "pp_metrics": 2 * n * formats.frame_bytes(fmt, w, h),
              "adler_yuv420p": n * formats.frame_bytes("yuv420p", w, h),
              "pp_metrics_yuv420p": 2 * n * formats.frame_bytes("yuv420p", w, h),
              "adler_v210": n * formats.frame_bytes("v210", w, h)}
    res = callbench.header("framecrc_bench", a, callbench.HEAD + ("iters",),
                           timer="HIP events around one ops call (kernel + finalize), the six calls taken in turn",
                           frame0_equals_zlib=check)
    for k in fns:
        res[k] = callbench.throughput(ms[k], nbytes[k], median=True)
    res["adler_vs_metrics_per_byte"] = {k: round(res[k]["GBps"] / res["pp_metrics"]["GBps"], 3)
                                        for k in fns if k.startswith("adler")}
    res["adler_yuv420p_vs_metrics_yuv420p_per_byte"] = round(res["adler_yuv420p"]["GBps"] /
                                                             res["pp_metrics_yuv420p"]["GBps"], 3)
    res["zlib_adler32_one_thread"] = {"bytes": len(frame), "ms_per_frame": round(cpu_s * 1e3, 4),
                                      "GBps": round(len(frame) / cpu_s / 1e9, 3)}
    callbench.emit(res, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
