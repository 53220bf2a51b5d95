#!/usr/bin/env python3
"""Benchmark of the MI355X raw-frame pixel path (BASELINE.json metric).

Unit of work = one PVS of BASELINE config 2: a 10 s 1080p60 SRC ->
  * P.910 SI/TI over its 600 frames of 1920x1080 10-bit luma, and
  * its 600 frames of 1280x720 yuv422p10le upscaled (lanczos, swscale-exact)
    to a 1920x1080 yuv422p10le AVPVS.
A step = every rank runs its share of a batch of PVSes (pixpath.batch.my_pvs,
the reference's ParallelRunner unit, lib/cmd_utils.py:93-101), then the
per-frame SI/TI of every PVS is gathered to rank 0 on the host (gloo).  Inputs
are resident in HBM when the timed region starts.  Default: BASELINE config 5,
a fixed batch of 256 PVS (153,600 frames) split over the ranks (strong
scaling); --pvs-per-rank K instead gives every rank K PVS (weak scaling).
value = frames of that workload per second over all ranks (each frame gets
both its AVPVS upscale and its SI/TI).

Multi-GPU: one process per GPU.  Under `torch.distributed.run` the ranks come
from its environment; `bench.py --gpus N` without it spawns the N ranks
itself (pixpath.batch.spawn_local; the parent never touches the GPU).  The
timing barrier, the max-over-ranks of the elapsed time and the SI/TI gather
use a gloo group -- no RCCL, no device-side exchange.

Extra fields: the roofline of the dominant kernel (strip_kernel) from HIP
events around its launches on the launch stream, the PMC traffic of a
separate rocprofv3 --pmc pass (profiles/pmc_traffic.json, tools/pmc_traffic.py),
the PCIe-inclusive pipeline rate (pinned host buffers -> H2D -> kernels ->
D2H, pixpath.pipeline, never `value`), and the CPU baseline (the oracle's C
restatement, scale and SI/TI timed separately on host threads).

A plain run (`bench.py --gpus 1 --steps N --warmup W`) sets up, warms up,
times the N steps and prints the result line with the fields the timed steps
themselves give (value, ms_per_step, the HIP-event kernel times).  Everything
that takes runs of its own -- the PCIe pipeline, the SI/TI file hook, the
end-to-end AVPVS line, the CPU baseline, and in the other workloads the canvas
chain, the FFV1 decode / concurrent / writer-lane lines and the reference-shape
stream decode -- runs only with --full (the --no-* options then drop single
parts of it, as before).

--dump-outputs DIR writes, after the timed steps, what the timed path computed
in its last step as DIR/<name>.npy (float32 / float64, every value finite; a
fixed seeded sample of the frames: well under 64 MB).  The inputs are seeded,
so two runs with the same arguments dump the same arrays.

Other workloads (profiles only, same schema): --workload config3-10 /
config3-8 (2160p -> 1080p yuv422p10le bicubic) and config4 (stall frames).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "processing-chain_amd"))

FRAMES = 600
HBM_PEAK_GBS = 8000.0                              # MI355X_MICROARCH.md: 8.0 TB/s spec
METRIC = "1080p yuv422p10 AVPVS frames/sec + SI/TI frames/sec; achieved HBM GB/s"
PMC_FILE = os.path.join(ROOT, "profiles", "pmc_traffic.json")

# workload -> (src fmt, sw, sh, dst fmt, dw, dh, flags, siti luma (w, h) or None)
WORKLOADS = {
    "config2": ("yuv422p10le", 1280, 720, "yuv422p10le", 1920, 1080, "lanczos", (1920, 1080)),
    "config3-10": ("yuv422p10le", 3840, 2160, "yuv422p10le", 1920, 1080, "bicubic", None),
    "config3-8": ("yuv420p", 3840, 2160, "yuv422p10le", 1920, 1080, "bicubic", None),
}
DESCR = {
    "config2": "config2 PVS: 10 s 1080p60 SRC -> SI/TI (1920x1080 10-bit luma) + 1280x720->1920x1080 "
               "yuv422p10le lanczos AVPVS upscale",
    "config3-10": "config3: 2160p60 yuv422p10le SRC -> 1920x1080 yuv422p10le (scale=1920:-2:flags=bicubic)",
    "config3-8": "config3: 2160p60 yuv420p SRC -> 1920x1080 yuv422p10le (scale=1920:-2:flags=bicubic)",
    "config4": "config4: stall frames (frozen 1080p yuv422p10le frame + spinner-128-white alpha blend)",
}


def frame_bytes(fmt, w, h):
    from pixpath import formats
    return formats.frame_bytes(fmt, w, h)


# Settings a product run may carry (device choice, backend, codec); every
# other PIXPATH_* variable is a measurement override (tools/) and voids a
# bench line: bench.py refuses to run with one unless --allow-tuning, and then
# records them in the line.  The product library reads no environment at all
# (csrc/common.hpp PP_KNOB); these guard the Python side and PIXPATH_LIB.
PRODUCT_ENV = {"PIXPATH_DEVICE", "PIXPATH_SLOT_DIR", "PIXPATH_BACKEND", "PIXPATH_FFV1", "PIXPATH_FFV1_SLICES",
               "PIXPATH_FFV1_SPLIT", "PIXPATH_FFV1_DECODE", "PIXPATH_SPINNER", "PIXPATH_HOME"}


def tuning_overrides():
    """PIXPATH_* variables of this process that are not product settings."""
    from pixpath import _native
    bad = {k: v for k, v in os.environ.items() if k.startswith("PIXPATH_") and k not in PRODUCT_ENV}
    default_lib = os.path.join(ROOT, "processing-chain_amd", "pixpath", "libpixpath.so")
    if "PIXPATH_LIB" in bad and os.path.realpath(bad["PIXPATH_LIB"]) == os.path.realpath(default_lib):
        del bad["PIXPATH_LIB"]
    if os.path.realpath(_native.LIB_PATH) != os.path.realpath(default_lib):
        bad.setdefault("PIXPATH_LIB", _native.LIB_PATH)
    return bad


def library_id():
    """sha256[:16] of the loaded libpixpath.so (what the line measured)."""
    import hashlib
    from pixpath import _native
    with open(_native.LIB_PATH, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)  # ~11 s timed at 1 GPU (config 5: 256 PVS per step)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=FRAMES, help="frames per PVS")
    ap.add_argument("--pvs-per-rank", type=int, default=None, help="PVS per rank (weak scaling)")
    ap.add_argument("--pvs-total", type=int, default=256, help="fixed batch (strong scaling): config 5 = 256")
    ap.add_argument("--pool", type=int, default=8, help="distinct resident PVS inputs per rank")
    ap.add_argument("--workload", default="config2", choices=sorted(list(WORKLOADS) + ["config4", "ffv1"]))
    ap.add_argument("--ffv1-slices", default="8x8", help="FFV1 slice grid (workload ffv1)")
    ap.add_argument("--ffv1-concurrent", type=int, default=4, help="PVS batches in flight for the concurrent FFV1 line")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: PCIe pipeline, SI/TI file hook, "
                         "end-to-end AVPVS, CPU baseline (config2/3); canvas chain (config4); decode, concurrent, "
                         "writer lanes, CPU baseline, reference-shape streams (ffv1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (a fixed sample) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=6.0, help="per CPU-baseline stage at full width")
    ap.add_argument("--cpu-threads", type=int, default=0, help="0 = every thread of the affinity mask")
    ap.add_argument("--cpu-sweep", default="16,64", help="extra thread counts timed (shorter) beside the full width")
    ap.add_argument("--no-siti-file", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--overlap", action="store_true", help="SI/TI on a second stream, concurrent with the scaler")
    ap.add_argument("--allow-tuning", action="store_true",
                    help="run with PIXPATH_* measurement overrides set (tools/ only; recorded in the line)")
    ap.add_argument("--e2e-pvs", type=int, default=4, help="PVSes in a row for the e2e_avpvs line")
    ap.add_argument("--e2e-encode", default="shared", choices=["shared", "private"],
                    help="e2e_avpvs writers: one encode stream + lock per device (product), or own streams")
    ap.add_argument("--cpu-e2e-seconds", type=float, default=4.0, help="CPU counterpart of e2e_avpvs: sample length")
    return ap.parse_args()


def host_cpu():
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    try:
        aff = len(os.sched_getaffinity(0))
    except AttributeError:
        aff = os.cpu_count()
    return model, os.cpu_count(), aff


def cgroup_cpus():
    """CPU quota of this cgroup (cpu.max) in CPUs, or None when unlimited/unknown."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else round(int(q) / int(per), 2)
    except (OSError, ValueError):
        return None


ORACLE_SRCS = ("pixoracle.c", "spinner_oracle.c", "siti_oracle.c", "ffv1_oracle.c")
ORACLE_SCALAR_FLAGS = "gcc -O3 -ffp-contract=off (oracle/Makefile, the parity checker's build)"


def oracle_native_build():
    """The oracle sources built with gcc -O3 -march=native for THIS host (the
    GPU box's CPU, compiled there: a few seconds), into a temp dir -- the
    vectorised CPU baseline.  Returns (path, flags) or (None, reason)."""
    import subprocess
    import tempfile
    flags = ["-O3", "-march=native", "-ffp-contract=off", "-fPIC", "-std=c11", "-D_GNU_SOURCE"]
    out = os.path.join(tempfile.mkdtemp(prefix="pixoracle_native_"), "libpixoracle_native.so")
    try:
        subprocess.run(["gcc"] + flags + ["-shared", "-o", out] + [os.path.join(ROOT, "oracle", f) for f in ORACLE_SRCS]
                       + ["-lm"], check=True, capture_output=True, timeout=180)
    except (OSError, subprocess.SubprocessError) as e:
        return None, "native build failed: %s" % e
    return out, " ".join(["gcc"] + flags)


def oracle_modules(lib_path):
    """Fresh pyoracle / ffv1_ref module instances bound to the oracle build at
    lib_path (None: oracle/lib/libpixoracle.so)."""
    import importlib.util
    old = os.environ.get("PIXORACLE_LIB")
    if lib_path:
        os.environ["PIXORACLE_LIB"] = lib_path
    else:
        os.environ.pop("PIXORACLE_LIB", None)
    mods = []
    try:
        for name in ("pyoracle", "ffv1_ref"):
            spec = importlib.util.spec_from_file_location("%s_%s" % (name, "native" if lib_path else "scalar"),
                                                          os.path.join(ROOT, "oracle", name + ".py"))
            m = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(m)
            mods.append(m)
    finally:
        if old is None:
            os.environ.pop("PIXORACLE_LIB", None)
        else:
            os.environ["PIXORACLE_LIB"] = old
    return mods


def cpu_baseline(args, wl):
    """Oracle C restatement on host threads (ctypes releases the GIL); the
    scaler and SI/TI are timed separately, the combined rate is per frame that
    gets both (1 / (1/scale + 1/siti)).  Two builds of the same sources: the
    parity checker's -O3 build (a thread sweep up to every thread of the
    affinity mask) and gcc -O3 -march=native compiled on this host, timed at
    the sweep's best thread count; each stage is taken at its faster build."""
    import threading
    import numpy as np
    sfmt, sw, sh, dfmt, dw, dh, flags, siti_wh = wl
    model, nproc, aff = host_cpu()
    full = args.cpu_threads or aff
    native_path, native_flags = oracle_native_build()
    po, ffv1_mod = oracle_modules(native_path)
    po_s, ffv1_s = oracle_modules(None)

    def setup(po, nt):
        rng = np.random.default_rng(910)
        sf, df = po.FMT_BY_NAME[sfmt], po.FMT_BY_NAME[dfmt]
        depth = po.fmt_info(sf)[0]
        hi = 1024 if depth > 8 else 256
        # 16 distinct read-only inputs shared by the threads (each has its own Sws scratch)
        src = [[rng.integers(0, hi, s).astype(po.plane_dtype(sf)) for s in po.plane_shapes(sf, sw, sh)]
               for _ in range(16)]
        fl = {"lanczos": po.SWS_LANCZOS, "bicubic": po.SWS_BICUBIC}[flags]
        sws = [po.Sws(sf, sw, sh, df, dw, dh, fl) for _ in range(nt)]
        luma = None
        if siti_wh:
            w, h = siti_wh
            luma = [rng.integers(0, 1024, (4, h, w)).astype(np.uint16) for _ in range(16)]
        return src, sws, [x.out_planes() for x in sws], luma

    def timed(fn, nt, secs):
        done = [0] * nt

        def work(t):
            while time.perf_counter() - t0 < secs:
                done[t] += fn(t)
        t0 = time.perf_counter()
        th = [threading.Thread(target=work, args=(t,)) for t in range(nt)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        return sum(done), time.perf_counter() - t0

    def point(po, state, nt, secs):
        src, sws, outs, luma = state

        def do_scale(t):
            sws[t].scale_into(src[t % 16], outs[t], 4)  # 4 frames per C call
            return 4

        def do_siti(t):
            po.siti_c(luma[t % 16], 10)  # 4 frames: 4 SI + 3 TI
            return 4
        ns, ts = timed(do_scale, nt, secs)
        r = {"threads": nt, "scale_fps": round(ns / ts, 2), "scale_frames": ns, "scale_s": round(ts, 2)}
        if siti_wh:
            nq, tq = timed(do_siti, nt, secs)
            r.update(siti_fps=round(nq / tq, 2), siti_frames=nq, siti_s=round(tq, 2))
            r["value"] = round(1.0 / (1.0 / r["scale_fps"] + 1.0 / r["siti_fps"]), 2)
        else:
            r["value"] = r["scale_fps"]
        return r

    quota = cgroup_cpus()
    pts = {int(v) for v in args.cpu_sweep.split(",") if v.strip() and 0 < int(v) < full}
    if quota and int(quota) < full:
        pts.add(int(quota))
    state = setup(po_s, full)
    sweep = [point(po_s, state, k, max(2.0, args.cpu_seconds / 2)) for k in sorted(pts)]
    widest = point(po_s, state, full, args.cpu_seconds)
    sweep.append(widest)
    # the best rate this box's host gives the CPU path (the cgroup's CPU quota
    # caps it below the affinity width; more threads than the quota only add
    # contention), with the thread count that reached it; then the other
    # build at that count: `value` is the faster build's.  The box's EPYC
    # (Zen 5) runs the -march=native SCALER slower than the scalar build
    # (576-715 vs 760-1,040 frames/s) while its SI/TI is faster: the native
    # build vectorises each output's short tap loop of hscale_row (8 taps:
    # vpmovzxwd + vpmulld, then a horizontal reduction through vextracti128 /
    # vpsrldq / vpaddd per output -- checked in gcc's x86-64-v4 assembly of
    # oracle/pixoracle.c), which costs more per output than the scalar
    # multiply-adds; the Sobel / difference loops are contiguous streams that
    # vectorise well.  Each stage is timed
    # at both builds and taken at its faster one, so the baseline is the most
    # favourable CPU number either build gives.
    top = max(sweep, key=lambda r: r["value"])
    other = point(po, setup(po, top["threads"]), top["threads"], max(2.0, args.cpu_seconds / 2)) if native_path else None
    builds = {ORACLE_SCALAR_FLAGS: top}
    if other:
        builds[native_flags] = other
    # each stage at its faster build (the most favourable CPU baseline)
    build, best = max(builds.items(), key=lambda kv: kv[1]["scale_fps"])
    best = dict(best)
    if siti_wh:
        sb, sv = max(builds.items(), key=lambda kv: kv[1]["siti_fps"])
        best["siti_fps"] = sv["siti_fps"]
        best["value"] = round(1.0 / (1.0 / best["scale_fps"] + 1.0 / best["siti_fps"]), 2)
        if sb != build:
            build = "scale: %s; SI/TI: %s" % (build, sb)
    best_po, best_ffv1 = (po_s, ffv1_s) if build.startswith(ORACLE_SCALAR_FLAGS) else (po, ffv1_mod)
    out = {"value": best["value"], "unit": "frames/s", "cores": best["threads"], "kind": "port", "host_nproc": nproc,
           "host_affinity": aff, "cgroup_cpus": quota, "cpu_model": model, "build": build,
           "scale_fps": best["scale_fps"], "sweep": sweep,
           "per_thread_scale_fps": round(best["scale_fps"] / best["threads"], 2),
           "builds": {k: {"value": v["value"], "threads": v["threads"], "scale_fps": v["scale_fps"],
                          "siti_fps": v.get("siti_fps")} for k, v in builds.items()}}
    if not native_path:
        out["builds"]["-march=native"] = native_flags  # the reason it is missing
    if args.workload == "config2":
        bst = state if best_po is po_s else setup(po, best["threads"])
        out["e2e"] = cpu_e2e(best["threads"], wl, bst[1], bst[2], best_po, best_ffv1, seconds=args.cpu_e2e_seconds)
        out["e2e"]["build"] = build
    top = best
    if siti_wh:
        out["siti_fps"] = top["siti_fps"]
        out["sample"] = ("%d-thread oracle C restatement (oracle/pixoracle.c + siti_oracle.c, %s), the best point "
                         "of a sweep up to every thread of the affinity mask (%d; the cgroup allows %s CPUs): %d frames "
                         "%dx%d %s -> %dx%d %s %s in %.1f s, then %d frames of %dx%d 10-bit SI/TI in %.1f s; value = "
                         "per frame that gets both; `builds`: the scalar -O3 and the -march=native builds at that "
                         "thread count, each stage taken at its faster build; ffmpeg is absent on the box"
                         % (top["threads"], build, full, quota, top["scale_frames"], sw, sh, sfmt, dw, dh, dfmt, flags,
                            top["scale_s"], top["siti_frames"], siti_wh[0], siti_wh[1], top["siti_s"]))
    else:
        out["sample"] = ("%d-thread oracle C restatement (%s), best point of a sweep up to %d threads: %d frames "
                         "%dx%d %s -> %dx%d %s %s in %.1f s; ffmpeg is absent on the box"
                         % (top["threads"], build, full, top["scale_frames"], sw, sh, sfmt, dw, dh, dfmt, flags,
                            top["scale_s"]))
    return out


def cpu_e2e(nt, wl, sws, outs, po, ffv1_ref, seconds=4.0):
    """CPU counterpart of e2e_avpvs: per frame, the oracle's scaler then the
    oracle's FFV1 encoder (oracle/ffv1_oracle.c, the same bitstream as the GPU
    encoder, 8x8 slices) on the compressible content e2e_avpvs uses, on nt
    threads for `seconds` (every thread finishes the frame it started);
    decode and file writes excluded (a lower bound on the CPU time)."""
    import threading
    import numpy as np
    sfmt, sw, sh, dfmt, dw, dh, flags, _ = wl
    sf = po.FMT_BY_NAME[sfmt]
    rng = np.random.default_rng(77)
    planes = []
    for p, (r, c) in enumerate(po.plane_shapes(sf, sw, sh)):
        yy, xx = np.mgrid[0:r, 0:c]
        planes.append(np.clip((xx * (p + 1) + yy * 2) % 800 + 100 + rng.integers(-4, 5, (r, c)), 64, 940)
                      .astype(np.uint16))
    depth, hs, vs = po.fmt_info(po.FMT_BY_NAME[dfmt])
    done = [0] * nt

    def work(t):
        while time.perf_counter() - t0 < seconds:
            sws[t].scale_into(planes, outs[t], 1)
            ffv1_ref.encode_frame(outs[t], depth, hs, vs, 8, 8)
            done[t] += 1
    t0 = time.perf_counter()
    th = [threading.Thread(target=work, args=(t,)) for t in range(nt)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    dt = time.perf_counter() - t0
    return {"frames_per_s": round(sum(done) / dt, 2), "threads": nt, "frames": sum(done), "seconds": round(dt, 2),
            "sample": "%d frames in %.1f s: oracle scale 720p->1080p yuv422p10le %s + oracle FFV1 encode (8x8 "
                      "slices) per frame, %d threads" % (sum(done), dt, flags, nt)}


def siti_file(dev, n=600, w=1920, h=1080):
    """The SRC-analysis SI/TI hook on a file: a 600-frame 1080p yuv422p10le Y4M
    (written to the temp dir first, so it is in the page cache) through
    pixpath.siti.siti_of_file -- luma-only read, pinned double buffers, H2D
    overlapped with the kernel.  File -> per-frame SI/TI on the host."""
    import tempfile
    import numpy as np
    from pixpath import formats, io as pio, siti
    fb = formats.frame_bytes("yuv422p10le", w, h)
    rng = np.random.default_rng(600)
    pool = [rng.integers(64, 941, fb // 2).astype(np.uint16).view(np.uint8) for _ in range(4)]
    d = tempfile.mkdtemp(prefix="pixpath_bench_")
    path = os.path.join(d, "src.y4m")
    try:
        wr = pio.Y4MWriter(path, "yuv422p10le", w, h, 60)
        for i in range(n):
            wr.write(pool[i % 4])
        wr.close()
        siti.siti_of_file(path, batch=120)  # warm-up (pinned buffers, kernel load)
        t0 = time.perf_counter()
        si, ti = siti.siti_of_file(path, batch=120)
        dt = time.perf_counter() - t0
    finally:
        if os.path.exists(path):
            os.remove(path)
        os.rmdir(d)
    assert len(si) == n
    return {"frames_per_s": round(n / dt, 1), "frames": n, "seconds": round(dt, 3),
            "luma_gbs": round(n * w * h * 2 / dt / 1e9, 2),
            "note": "600-frame 1080p yuv422p10le Y4M (page cache) -> luma-only read -> pinned double buffers -> "
                    "H2D (copy stream) -> siti_kernel (compute stream) -> per-frame SI/TI on the host"}


def pcie_pipeline(wl, n_frames, dev, batch=60):
    """Pinned host frames -> H2D -> scaler -> D2H through pixpath.pipeline
    (two streams, double buffers); PCIe-inclusive, reported beside `value`."""
    import numpy as np
    from pixpath import ops
    from pixpath.pipeline import Pipeline, Stage
    sfmt, sw, sh, dfmt, dw, dh, flags, _ = wl
    in_fb, out_fb = frame_bytes(sfmt, sw, sh), frame_bytes(dfmt, dw, dh)
    pool = np.random.default_rng(7).integers(0, 256, (8, in_fb), dtype=np.uint8)

    class MemReader:
        def __init__(self):
            self.left = n_frames

        def read_into(self, buf, n):
            k = min(n, self.left)
            b = np.frombuffer(buf, np.uint8).reshape(-1, in_fb)
            for i in range(k):
                b[i] = pool[(n_frames - self.left + i) % len(pool)]
            self.left -= k
            return k

    class NullWriter:
        def write(self, frames):
            pass
    sc = ops.Scaler(sfmt, sw, sh, dfmt, dw, dh, flags=flags, device=dev.index)
    stage = Stage(sfmt, sw, sh, dfmt, dw, dh, lambda s, d, st: sc(s, d, stream=st))
    pl = Pipeline(stage, batch=batch, device=dev.index)
    pl.run(MemReader(), NullWriter())  # warm-up pass (pinned buffers, plan)
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = pl.run(MemReader(), NullWriter())
    dt = time.perf_counter() - t0
    return {"frames_per_s": round(n / dt, 1), "pcie_gbs": round(n * (in_fb + out_fb) / dt / 1e9, 2),
            "frames": n, "batch": batch,
            "note": "host pinned -> H2D (copy stream) -> strip_kernel (compute stream) -> D2H -> host; "
                    "host fill of the pinned input is included, decode/encode are not"}


def e2e_avpvs(wl, n_frames, dev, n_pvs=4, depth=None, shared=True):
    """The product path of `cli avpvs --gpu-ffv1` end to end (SURVEY.md 8d's
    third row): dense host frames -> pinned batches -> H2D -> strip_kernel ->
    FFV1 encode of the DEVICE output (no D2H of pixels) -> packets D2H -> AVI
    bytes written to a file.  Host decode is replaced by a memory reader of
    compressible synthetic frames (moving gradients + noise: FFV1 codes them
    at ~4:1, like upscaled video); the rate includes the reader's copies and
    the file writes.  Several PVSes in a row, as the reference's ParallelRunner
    feeds them (lib/cmd_utils.py:93-101): each writer encodes and writes its
    PVS on its own worker thread and stream while the next PVS is scaled, so
    the scale, encode and file-write stages of consecutive PVSes overlap.
    The encoder pool holds `depth` encoders (with their staging batch) before
    the timed region, as a long-running writer process keeps them; writer
    construction is timed as its own stage (`setup_s`).  `single_pvs` is the
    same path for one PVS with nothing to overlap.  Never `value`."""
    import tempfile
    import threading
    import numpy as np
    import torch
    from pixpath import ffv1, formats, ops
    from pixpath.ffv1 import Ffv1AviWriter
    from pixpath.pipeline import Pipeline, Stage
    sfmt, sw, sh, dfmt, dw, dh, flags, _ = wl
    in_fb = frame_bytes(sfmt, sw, sh)
    rng = np.random.default_rng(77)
    pool = []
    for k in range(8):
        planes = []
        for p, (r, c) in enumerate(formats.plane_shapes(sfmt, sw, sh)):
            yy, xx = np.mgrid[0:r, 0:c]
            v = (xx * (p + 1) + yy * 2 + 5 * k) % 800 + 100 + rng.integers(-4, 5, (r, c))
            planes.append(np.clip(v, 64, 940).astype(np.uint16).view(np.uint8).reshape(-1))
        pool.append(np.concatenate(planes))

    class MemReader:
        def __init__(self):
            self.i = 0

        def read_into(self, buf, n):
            k = min(n, n_frames - self.i)
            b = np.frombuffer(buf, np.uint8).reshape(-1, in_fb)
            for j in range(k):
                b[j] = pool[(self.i + j) % len(pool)]
            self.i += k
            return k

    sc = ops.Scaler(sfmt, sw, sh, dfmt, dw, dh, flags=flags, device=dev.index)
    stage = Stage(sfmt, sw, sh, dfmt, dw, dh, lambda s, d, st: sc(s, d, stream=st))
    pl = Pipeline(stage, batch=60, device=dev.index)
    d = tempfile.mkdtemp(prefix="pixpath_e2e_")
    # fresh output names per run: replacing a 1.2 GB AVI left by an earlier run
    # frees its pages inside close() (0.2 s), which is not this run's work
    runs = [0]

    def new_paths(count):
        runs[0] += 1
        return [os.path.join(d, "r%d_PVS%d.avi" % (runs[0], k)) for k in range(count)]
    depth = depth or n_pvs  # every PVS of the run can be in flight at once
    t_res = time.perf_counter()
    # encoder lanes per writer (writer_split): default_split() for a writer that
    # codes alone on the device, 1 for writers opened while another is open
    split = ffv1.default_split()
    forced = bool(os.environ.get("PIXPATH_FFV1_SPLIT"))
    made = ffv1.reserve_writers(dfmt, dw, dh, depth, slices=(8, 8), batch=n_frames, device=dev.index)
    torch.cuda.synchronize()
    reserve_s = time.perf_counter() - t_res

    def run(count):
        for f in os.listdir(d):  # the previous run's files, outside the timed region
            os.remove(os.path.join(d, f))
        paths = new_paths(count)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        closers, errs, stats, n = [], [], [], 0
        setup_s, pipe_s = [], []

        def close(wr):  # encode + write of PVS k overlap the scale of PVS k + 1
            try:
                wr.close()
                stats.append(dict(wr.stats))
            except Exception as e:  # re-raised below
                errs.append(e)
        for k in range(count):
            tw = time.perf_counter()
            wr = Ffv1AviWriter(paths[k], dfmt, dw, dh, 60, slices=(8, 8), batch=n_frames, device=dev.index,
                               shared=shared)
            tp = time.perf_counter()
            n += pl.run(MemReader(), wr)
            te = time.perf_counter()
            setup_s.append(round(tp - tw, 4))
            pipe_s.append(round(te - tp, 4))
            th = threading.Thread(target=close, args=(wr,))
            th.start()
            closers.append(th)
            del wr
        t_main = time.perf_counter()
        for th in closers:
            th.join()
        t_end = time.perf_counter()
        if errs:
            raise errs[0]
        dt = t_end - t0
        order = sorted(stats, key=lambda w: w["timeline"][0][0] if w["timeline"] else 0)
        st = {"setup_s": setup_s, "pipeline_s": pipe_s, "tail_s": round(t_end - t_main, 4),
              # per PVS, seconds from the run's start: first (sub-)batch queued, its
              # frames ready on the GPU (encode starts), the last encode done, the
              # last packets written (D2H chunks overlapped with the writes), AVI
              # closed; lanes: each sub-batch's (queued, encode start, encode done,
              # written)
              "timeline": [[round(x - t0, 4) for x in (w["timeline"][0][0], w["timeline"][0][2],
                                                       max(t[3] for t in w["timeline"]),
                                                       max(t[4] for t in w["timeline"]), w["closed_at"])]
                           for w in order if w["timeline"]],
              "lanes": [[[round(t[i] - t0, 4) for i in (0, 2, 3, 4)] for t in w["timeline"]] for w in order],
              "encode_s": [round(w["encode_s"], 4) for w in order],
              "d2h_and_avi_write_s": [round(w["write_s"], 4) for w in order],
              "encode_launches": [w["launches"] for w in order],
              "writer_lanes": [w["lanes"] for w in order]}
        # the main thread's stages plus the wait for the last writers: the wall time
        st["explained_s"] = round(sum(setup_s) + sum(pipe_s) + st["tail_s"], 4)
        st["explained_frac"] = round(st["explained_s"] / dt, 4)
        st["avi_bytes"] = os.path.getsize(paths[0])
        return n, dt, st

    try:
        run(1)  # warm-up (kernel loads, pinned buffers, the pipeline's device batches)
        # one PVS alone: the best of 3 runs (its host stage -- frames into the
        # pinned batches -- varies run to run; every run's seconds are reported)
        singles = [run(1) for _ in range(3)]
        n1, dt1, w1 = min(singles, key=lambda r: r[1])
        single_runs = [round(r[1], 3) for r in singles]
        size = w1["avi_bytes"]
        # the PVSes in flight: the best of 2 runs (their host stages -- frames
        # into pinned batches, packet D2H and AVI writes -- contend for host
        # memory and vary run to run; both runs' seconds are reported)
        multi = [run(n_pvs) for _ in range(2)]
        n, dt, ws = min(multi, key=lambda r: r[1])
        multi_runs = [round(r[1], 3) for r in multi]
    finally:
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)
    enc_mem = {}
    for k in sorted({split, 1}):
        try:
            e = ffv1.acquire_encoder(dfmt, dw, dh, slices=(8, 8), max_frames=-(-n_frames // k), device=dev.index)
            enc_mem["%d_lanes" % k] = k * (e.memory_bytes + sum(b.storage.numel() for b in (e.stages or [])))
            ffv1.release_encoder(e)
        except Exception:
            pass
    ffv1.clear_pool()
    return {"frames_per_s": round(n / dt, 1), "frames": n, "pvs": n_pvs, "seconds": round(dt, 3), "runs_s": multi_runs,
            "stages": ws,
            "single_pvs": {"frames_per_s": round(n1 / dt1, 1), "seconds": round(dt1, 3), "runs_s": single_runs,
                           "stages": w1},
            "writers": ("%d encoder lanes per writer (sub-batches of %d frames coded side by side, packets written "
                        "in frame order; PIXPATH_FFV1_SPLIT forced)" % (split, -(-n_frames // split)) if forced else
                        "writer_split: %d encoder lanes (sub-batches of %d frames coded side by side, packets written "
                        "in frame order) for a writer coding alone on the device, one encoder of the whole batch "
                        "for writers opened while another is open (stages.writer_lanes)"
                        % (split, -(-n_frames // split))),
            "encoder_pool": {"depth": depth, "created": made, "reserve_s": round(reserve_s, 3),
                             "bytes_per_writer": enc_mem},
            "avi_bytes_per_pvs": size, "compression": round(n1 * frame_bytes(dfmt, dw, dh) / size, 3),
            "note": "%d PVSes of %d frames: host frames -> pinned batches of 60 -> H2D -> strip_kernel "
                    "(720p->1080p yuv422p10le lanczos) -> FFV1 v3 encode on the device output (8x8 slices, the "
                    "writer's encoder lanes: worker threads and streams) -> packets D2H -> AVI file; consecutive "
                    "PVSes overlap; %d pooled encoders reserved before timing; decode of the SRC bitstream "
                    "excluded (ffmpeg is absent on the box); frames_per_s: the best of 2 runs of the %d PVSes "
                    "(runs_s), single_pvs: the best of 3" % (n_pvs, n_frames, depth, n_pvs)}


DUMP_SEED = 910
DUMP_FRAMES = 16   # frames sampled per dumped batch
DUMP_ROWS = 64     # rows sampled per plane of a sampled frame


def sample_frames(fb, seed=DUMP_SEED):
    """A fixed, seeded sample of a FrameBatch for --dump-outputs: DUMP_FRAMES
    frames (the first and the last among them), and of every plane of those
    DUMP_ROWS whole rows (the first and the last among them).  Returns
    {"plane<p>": float32 [frames, rows, cols], "frames": ..., "rows<p>": ...}:
    a 1080p yuv422p10le batch gives 15.7 MB."""
    import numpy as np
    rng = np.random.default_rng(seed)

    def pick(n, k):
        if n <= k:
            return np.arange(n)
        mid = rng.choice(np.arange(1, n - 1), size=k - 2, replace=False)
        return np.sort(np.concatenate([[0, n - 1], mid]))
    frames = pick(fb.n, DUMP_FRAMES)
    out = {"frames": frames.astype(np.float64)}
    for p in range(len(fb.planes)):
        v = fb.view(p)
        rows = pick(v.shape[1], DUMP_ROWS)
        out["rows%d" % p] = rows.astype(np.float64)
        out["plane%d" % p] = np.stack([v[int(f)].cpu().numpy()[rows] for f in frames]).astype(np.float32)
    return out


def dump_outputs(path, arrays):
    """arrays: {name: numpy array} -> path/<name>.npy, float32 or float64."""
    import numpy as np
    out = {}
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        if not np.isfinite(a).all():
            raise ValueError("--dump-outputs: %s holds a value that is not finite" % name)
        out[name] = a
    total = sum(a.nbytes for a in out.values())
    if total > 64 << 20:
        raise ValueError("--dump-outputs: %d bytes exceed 64 MB" % total)
    os.makedirs(path, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(path, name + ".npy"), a)


def make_inputs(wl, n, seed, dev):
    import torch
    from pixpath.frames import FrameBatch
    sfmt, sw, sh, _, _, _, _, siti_wh = wl
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    src = FrameBatch(sfmt, sw, sh, n, device=dev)
    depth = src.fmt.depth
    rng_y = (64, 941) if depth > 8 else (16, 236)
    rng_c = (64, 961) if depth > 8 else (16, 241)
    for p, (lo, hi) in enumerate([rng_y, rng_c, rng_c]):
        v = src.view(p)
        v.copy_(torch.randint(lo, hi, v.shape, generator=g, device=dev, dtype=torch.int32).to(v.dtype))
    luma = None
    if siti_wh:
        w, h = siti_wh
        luma = torch.randint(64, 941, (n, h, w), generator=g, device=dev, dtype=torch.int32).to(torch.uint16)
    return src, luma


def main():
    args = parse()
    from pixpath import batch
    over = tuning_overrides()
    if over and not args.allow_tuning:
        print("bench: refusing to run with measurement overrides set: %s (they change kernel plans or outputs; "
              "unset them, or pass --allow-tuning for a tools/ run)" % " ".join(sorted(over)), file=sys.stderr)
        return 2
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # parent: start one rank per GPU and relay their exit status (no HIP here)
        sys.exit(batch.spawn_local(args.gpus, [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]))
    rank, world, local = batch.rank_env()
    if "WORLD_SIZE" in os.environ and args.gpus not in (1, world) and rank == 0:
        print("bench: --gpus %d but WORLD_SIZE=%d; using the launcher's world" % (args.gpus, world), file=sys.stderr)
    import torch
    batch.init_group(world)
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if args.workload == "config4":
        return bench_stall(args, rank, world, dev)
    if args.workload == "ffv1":
        return bench_ffv1(args, rank, world, dev)

    from pixpath import ops
    from pixpath.frames import FrameBatch
    wl = WORKLOADS[args.workload]
    sfmt, sw, sh, dfmt, dw, dh, flags, siti_wh = wl
    n = args.frames
    total = world * args.pvs_per_rank if args.pvs_per_rank else args.pvs_total
    ids = ["PVS%03d" % i for i in range(total)]
    mine = batch.my_pvs(ids, rank, world)
    k_pool = max(1, min(args.pool, len(mine)))
    pool = [make_inputs(wl, n, 910 + int(pid[3:]), dev) for pid in mine[:k_pool]]
    outs = [FrameBatch(dfmt, dw, dh, n, device=dev) for _ in range(min(2, max(1, len(mine))))]
    scaler = ops.Scaler(sfmt, sw, sh, dfmt, dw, dh, flags=flags)
    torch.cuda.synchronize()

    ev = []
    side = torch.cuda.Stream(dev) if args.overlap else None

    def step(timed):
        res = []
        for i, pid in enumerate(mine):
            src, luma = pool[i % k_pool]
            if timed:
                a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                a.record()
            scaler(src, outs[i % len(outs)])
            if timed:
                b.record()
            if luma is not None and side is not None:
                # --overlap: SI/TI of the SRC on its own stream, concurrent with the
                # scaler (independent inputs): the VALU-bound Sobel under the
                # store-bound scaler.  Events then time each kernel under co-execution.
                with torch.cuda.stream(side):
                    if timed:
                        b2 = torch.cuda.Event(enable_timing=True)
                        b2.record(side)
                    res.append(ops.siti(luma, 10, stream=side))
                    if timed:
                        c.record(side)
                        ev.append((a, b, b2, c))
                continue
            if luma is not None:
                res.append(ops.siti(luma, 10))
            if timed:
                c.record()
                ev.append((a, b, b, c))
        gathered = None
        if siti_wh:
            si = torch.stack([r[0] for r in res]).cpu().numpy() if res else None
            ti = torch.stack([r[1] for r in res]).cpu().numpy() if res else None
            local_res = {pid: (si[i], ti[i]) for i, pid in enumerate(mine)}
            gathered = batch.gather_results(local_res, rank, world)
        else:
            torch.cuda.synchronize()
        return gathered

    for _ in range(args.warmup):
        step(False)
    torch.cuda.synchronize()
    batch.barrier(world)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        gathered = step(True)
    torch.cuda.synchronize()
    batch.barrier(world)
    elapsed = batch.max_over_ranks(time.perf_counter() - t0, world)

    scale_ms = sum(a.elapsed_time(b) for a, b, _, _ in ev) / max(1, len(ev))
    siti_ms = sum(b2.elapsed_time(c) for _, _, b2, c in ev) / max(1, len(ev)) if siti_wh else None
    frames_total = total * n * args.steps
    value = frames_total / elapsed
    per_rank = batch.gather_values(len(mine), rank, world)
    if rank != 0:
        return 0
    if args.dump_outputs:
        # the last step's outputs as its caller holds them: the AVPVS batches
        # still in the output buffers (the last PVSes of this rank) and the
        # gathered per-frame SI/TI of every PVS
        arrays = {}
        last = {(i % len(outs)): pid for i, pid in enumerate(mine)}
        for slot, pid in sorted(last.items()):
            for k, a in sample_frames(outs[slot], DUMP_SEED + slot).items():
                arrays["avpvs_%s_%s" % (pid, k)] = a
        if gathered:
            import numpy as np
            arrays["si"] = np.stack([gathered[pid]["si"] for pid in ids])
            # TI of a PVS's first frame is undefined (NaN, no frame before it): left out
            arrays["ti"] = np.stack([gathered[pid]["ti"][1:] for pid in ids])
        dump_outputs(args.dump_outputs, arrays)
    bytes_pf = frame_bytes(sfmt, sw, sh) + frame_bytes(dfmt, dw, dh)
    achieved = bytes_pf * n / (scale_ms / 1000.0) / 1e9
    traffic = None
    if os.path.exists(PMC_FILE) and args.workload == "config2":
        try:
            pm = json.load(open(PMC_FILE))
            k = pm.get("kernels", {}).get("strip_kernel")
            if k and pm.get("frames_per_launch") == n:
                traffic = k["hbm_bytes_per_launch"]
        except (OSError, ValueError, KeyError):
            traffic = None
    out = {
        "metric": METRIC,
        "value": round(value, 1),
        "unit": "frames/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed * 1000.0 / args.steps, 4),
        "higher_is_better": True,
        "scaling": "weak" if args.pvs_per_rank else "strong",
        "vs_baseline": None,
        "dtype": "u16",
        "data": "synthetic (seeded legal-range samples generated in HBM; %d distinct resident PVS inputs per rank)"
                % k_pool,
        "config": {
            "workload": DESCR[args.workload],
            "pvs_total": total, "pvs_per_rank": per_rank, "frames_per_pvs": n,
            "frames_per_rank_per_step": [k * n for k in per_rank],
            "parallelism": "pvs-sharded x%d (one process per GPU; gloo host gather of SI/TI, no RCCL)" % world,
        },
        "avpvs_fps_kernel": round(n / (scale_ms / 1000.0), 1),
        "roofline": {
            "bound": "hbm",
            "kernel": "strip_kernel (fused H+V polyphase over 256-column strips, one launch per 600-frame PVS)",
            "achieved": round(achieved, 1),
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 4),
            "traffic": traffic,
            "traffic_source": ("copied from profiles/pmc_traffic.json: HBM bytes per launch of separate rocprofv3 "
                               "--pmc FETCH_SIZE / WRITE_SIZE passes of this workload (tools/pmc_traffic.py, "
                               "read side doubled per MI355X_MICROARCH.md), not measured in this run"
                               if traffic is not None else None),
            "algorithmic_bytes_per_launch": bytes_pf * n,
            "avg_launch_ms": round(scale_ms, 4),
            "plan": dict(scaler.stats, kernel_path=scaler.kernel_path),
        },
        "cpu_baseline": None,
        "library": library_id(),
        "tuning_overrides": tuning_overrides() or None,
    }
    if siti_wh:
        luma_b = siti_wh[0] * siti_wh[1] * 2
        out["siti_fps_kernel"] = round(n / (siti_ms / 1000.0), 1)
        out["siti_kernel"] = {"avg_launch_ms": round(siti_ms, 4), "algorithmic_bytes_per_launch": luma_b * n,
                              "achieved": round(luma_b * n / (siti_ms / 1000.0) / 1e9, 1),
                              "frac": round(luma_b * n / (siti_ms / 1000.0) / 1e9 / HBM_PEAK_GBS, 4)}
        some = gathered[mine[0]] if gathered else None
        if some is not None:
            out["siti_gather"] = {"pvs": len(gathered), "example": {"pvs": mine[0], "SI": round(some["SI"], 4),
                                                                   "TI": round(some["TI"], 4)}}
    if args.full and world == 1 and not args.no_pipeline:
        out["pcie_pipeline"] = pcie_pipeline(wl, 600, dev)
    if args.full and world == 1 and siti_wh and not args.no_siti_file:
        out["siti_file"] = siti_file(dev)
    if args.full and world == 1 and args.workload == "config2" and not args.no_e2e:
        out["e2e_avpvs"] = e2e_avpvs(wl, 600, dev, n_pvs=args.e2e_pvs, shared=args.e2e_encode == "shared")
    if args.full and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args, wl)
        ce = out["cpu_baseline"].get("e2e") if out["cpu_baseline"] else None
        if ce and out.get("e2e_avpvs") and ce.get("frames_per_s"):
            e = out["e2e_avpvs"]
            e["vs_cpu_e2e"] = {"pvs_in_flight": round(e["frames_per_s"] / ce["frames_per_s"], 1),
                               "single_pvs": round(e["single_pvs"]["frames_per_s"] / ce["frames_per_s"], 1),
                               "cpu_threads": ce.get("threads")}
    print(json.dumps(out), flush=True)
    return 0


def bench_stall(args, rank, world, dev):
    """config 4: stall frames (frozen frame + spinner) composed on the GPU."""
    import numpy as np
    import torch
    from pixpath import ops, spinner
    from pixpath.frames import FrameBatch
    w, h, n = 1920, 1080, args.frames
    anim, delays = spinner.load_apng(os.path.join(ROOT, "tests", "golden", "spinner-128-white.png"))
    ops.spinner_upload(anim, "yuv422p10le", device=dev.index)
    src, _ = make_inputs(("yuv422p10le", w, h, None, 0, 0, None, None), 8, 404 + rank, dev)
    dst = FrameBatch("yuv422p10le", w, h, n, device=dev)
    # as the product composes a stall run (pixpath/stall.py, PP-STALL-1): ONE
    # frozen frame repeated, the spinner animating over it (round 5 cycled 8
    # source frames, which the L2 held: VERDICT r5 item 7)
    src_idx = np.zeros(n, dtype=np.int32)
    sp_idx = np.arange(n, dtype=np.int32) % len(anim)
    ev = []
    for i in range(args.warmup + args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.stall_compose(src, src_idx, sp_idx, dst=dst)
        b.record()
        if i >= args.warmup:
            ev.append((a, b))
    torch.cuda.synchronize()
    ms = sum(a.elapsed_time(b) for a, b in ev) / len(ev)
    fb = frame_bytes("yuv422p10le", w, h)
    achieved = 2 * fb * n / (ms / 1000.0) / 1e9
    # the honest HBM figure of a stall run: its write stream (the frozen frame
    # is read once per launch), against the measured store ceiling of the box
    # (contiguous dwordx4 stores, profiles/r2/strip_experiments.md: 6,774 GB/s)
    write_gbs = fb * n / (ms / 1000.0) / 1e9
    # PMC traffic of the stall launches, copied from the committed profile of
    # this workload (tools/gpu_final_r6.sh: separate --pmc FETCH_SIZE /
    # WRITE_SIZE passes, tools/pmc_traffic.py), scaled from its per-launch
    # mean (<= 256 frames a launch) to this line's frames
    stall_traffic = None
    try:
        pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic_config4.json")))
        k = pm["kernels"].get("stall_kernel")
        if k and pm.get("frames_per_launch") == n:
            nl = (n + 255) // 256
            stall_traffic = {"hbm_bytes": round(k["hbm_bytes_per_launch"] * nl),
                             "read_bytes": round(k["read_bytes_corrected"] * nl),
                             "write_bytes": round(k["write_bytes"] * nl),
                             "source": "copied from profiles/pmc_traffic_config4.json (separate rocprofv3 --pmc "
                                       "passes of this workload), not measured in this run"}
    except (OSError, ValueError, KeyError):
        stall_traffic = None
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"stall_" + k: a for k, a in sample_frames(dst).items()})
    canvas = stall_canvas(args, rank, dev, dst) if args.full else None
    if rank == 0:
        print(json.dumps({"metric": "stall frames/s (config 4)", "value": round(world * n / (ms / 1000.0), 1),
                          "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(ms, 4), "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": "u16", "data": "synthetic",
                          "config": {"workload": DESCR["config4"], "frames_per_launch": n},
                          "roofline": {"bound": "hbm", "kernel": "stall_kernel", "achieved": round(achieved, 1),
                                       "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                                       "traffic": stall_traffic["hbm_bytes"] if stall_traffic else None,
                                       "traffic_detail": stall_traffic, "algorithmic_bytes_per_launch": 2 * fb * n,
                                       "avg_launch_ms": round(ms, 4),
                                       "note": "SURVEY 8d bytes (read + write per frame); the frozen frame is "
                                               "read from HBM once per launch, so write_gbs is the HBM figure"},
                          "write_gbs": round(write_gbs, 1), "write_frac_of_store_ceiling": round(write_gbs / 6774.0, 4),
                          "write_frac_of_peak": round(write_gbs / HBM_PEAK_GBS, 4),
                          "canvas_chain": canvas, "cpu_baseline": None, "library": library_id(),
                          "tuning_overrides": tuning_overrides() or None}), flush=True)
    return 0


def stall_canvas(args, rank, dev, dst):
    """--full, config 4: the canvas chain of a stall run, timed on its own."""
    import torch
    from pixpath import ops
    from pixpath.frames import FrameBatch
    w, h, n = dst.w, dst.h, dst.n
    fb = frame_bytes("yuv422p10le", w, h)
    # the long test's canvases (create_avpvs_segment): 720p yuv420p10le segment
    # frames -> overlay yuv420p -> yuv422p10le 1080p, one chain-plan launch
    seg = FrameBatch("yuv420p10le", 1280, 720, n, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(405 + rank)
    for p in range(3):
        v = seg.view(p)
        v.copy_(torch.randint(64, 941, v.shape, generator=g, device=dev, dtype=torch.int32).to(v.dtype))
    chain = ops.Scaler("yuv420p10le", 1280, 720, "yuv422p10le", w, h, flags="bicubic", chain=True)
    cev = []
    for i in range(args.warmup + args.steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        chain(seg, dst)
        b.record()
        if i >= args.warmup:
            cev.append((a, b))
    torch.cuda.synchronize()
    cms = sum(a.elapsed_time(b) for a, b in cev) / len(cev)
    cbytes = (frame_bytes("yuv420p10le", 1280, 720) + fb) * n
    canvas = {"kernel": "strip_kernel chain (FUSE=10)" if chain.kernel_path else "two launches",
              "frames_per_s": round(n / (cms / 1000.0), 1), "avg_launch_ms": round(cms, 4),
              "algorithmic_bytes_per_launch": cbytes, "achieved": round(cbytes / (cms / 1000.0) / 1e9, 1),
              "frac": round(cbytes / (cms / 1000.0) / 1e9 / HBM_PEAK_GBS, 4),
              "note": "1280x720 yuv420p10le -> bicubic -> overlay yuv420p -> yuv422p10le 1920x1080"}
    return canvas


def bench_ffv1(args, rank, world, dev):
    """FFV1 encode of the config-2 AVPVS (600 frames of 1920x1080 yuv422p10le,
    SURVEY.md section 8f row 1): frames/s through the GPU encoder (one lane per
    slice, packets laid out in HBM), against the CPU restatement on a bounded
    sample.  Content: smooth gradients moving per frame plus +-4 noise (a
    compressible picture; pure noise is FFV1's worst case)."""
    import time
    import numpy as np
    import torch
    from pixpath import ffv1
    from pixpath.frames import FrameBatch
    w, h, n = 1920, 1080, args.frames
    nh, nv = (int(v) for v in args.ffv1_slices.split("x"))
    src = FrameBatch("yuv422p10le", w, h, n, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(910 + rank)
    fr = torch.arange(n, device=dev, dtype=torch.int32).view(n, 1, 1)
    for p in range(3):
        v = src.view(p)
        yy = torch.arange(v.shape[1], device=dev, dtype=torch.int32).view(1, -1, 1)
        xx = torch.arange(v.shape[2], device=dev, dtype=torch.int32).view(1, 1, -1)
        noise = torch.randint(-4, 5, v.shape, generator=g, device=dev, dtype=torch.int32)
        v.copy_(((xx * (p + 1) + yy * 2 + 3 * fr) % 800 + 100 + noise).clamp(64, 940).to(v.dtype))
    enc = ffv1.Ffv1Encoder("yuv422p10le", w, h, slices=(nh, nv), max_frames=n, device=dev)
    for _ in range(args.warmup):
        enc.encode(src)
    torch.cuda.synchronize()
    from pixpath import batch as batch_barrier
    batch_barrier.barrier(world)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        buf, sizes = enc.encode(src)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    dt = batch_barrier.max_over_ranks(dt, world)
    raw = frame_bytes("yuv422p10le", w, h)
    head = {"metric": "FFV1 AVPVS encode frames/s (1080p yuv422p10le)", "value": round(world * n / dt, 1),
            "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u16", "data": "synthetic (moving gradients + uniform noise in [-4, 4])",
            "config": {"workload": "ffv1: FFV1 v3 intra encode of a 600-frame config-2 AVPVS", "frames": n,
                       "slices": [nh, nv], "bytes_per_frame": round(float(sizes.mean()), 1),
                       "compression": round(raw / float(sizes.mean()), 3)}}
    if args.dump_outputs and rank == 0:
        # the encoder's outputs: every packet size, and the first 4 MiB of the packet bytes
        dump_outputs(args.dump_outputs, {"packet_sizes": np.asarray(sizes, np.float64),
                                         "packet_bytes": buf.reshape(-1)[:4 << 20].cpu().numpy().astype(np.float32)})
    if not args.full:
        if rank == 0:
            print(json.dumps(dict(head, roofline=None, library=library_id(),
                                  tuning_overrides=tuning_overrides() or None)), flush=True)
        return 0
    # decode of the same packets (pinned host packets -> H2D -> one lane per
    # slice), as Ffv1AviReader hands them over (read into a pinned buffer)
    pk = buf.cpu().pin_memory().numpy()
    dec = ffv1.Ffv1Decoder(enc.extradata, w, h, max_frames=n, device=dev)
    back = FrameBatch("yuv422p10le", w, h, n, device=dev)
    dec.decode(pk, sizes, dst=back)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        dec.decode(pk, sizes, dst=back)
    torch.cuda.synchronize()
    ddt = batch_barrier.max_over_ranks((time.perf_counter() - t0) / args.steps, world)
    lossless = all(bool(torch.equal(back.view(p), src.view(p))) for p in range(3))
    # several PVS batches in flight at once, each on its own encoder / decoder,
    # stream and host thread -- how the reference's ParallelRunner feeds the
    # AVPVS stage (lib/cmd_utils.py:93-101: one process per PVS, -p at a time).
    # One 600-frame batch has 38,400 slice chains = 600 full waves for 1,024
    # SIMDs, so concurrent batches fill the idle SIMDs and pair waves per SIMD.
    conc = None
    if args.ffv1_concurrent > 1:
        import threading
        K = args.ffv1_concurrent
        encs = [enc] + [ffv1.Ffv1Encoder("yuv422p10le", w, h, slices=(nh, nv), max_frames=n, device=dev)
                        for _ in range(K - 1)]
        decs = [dec] + [ffv1.Ffv1Decoder(enc.extradata, w, h, max_frames=n, device=dev) for _ in range(K - 1)]
        outs_d = [back] + [FrameBatch("yuv422p10le", w, h, n, device=dev) for _ in range(K - 1)]
        streams = [torch.cuda.Stream(dev) for _ in range(K)]

        def concurrent(fn):
            ths = [threading.Thread(target=fn, args=(k,)) for k in range(K)]
            t0 = time.perf_counter()
            for t in ths:
                t.start()
            for t in ths:
                t.join()
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        def enc_k(k):
            with torch.cuda.stream(streams[k]):
                encs[k].encode(src, stream=streams[k])

        def dec_k(k):
            with torch.cuda.stream(streams[k]):
                decs[k].decode(pk, sizes, dst=outs_d[k], stream=streams[k])
        concurrent(enc_k)  # warm-up
        edt = min(concurrent(enc_k) for _ in range(max(1, args.steps)))
        concurrent(dec_k)
        ddt_c = min(concurrent(dec_k) for _ in range(max(1, args.steps)))
        ok = all(bool(torch.equal(outs_d[k].view(p), src.view(p))) for k in range(K) for p in range(3))
        conc = {"pvs_in_flight": K, "encode_frames_per_s": round(world * K * n / edt, 1),
                "decode_frames_per_s": round(world * K * n / ddt_c, 1), "lossless": ok,
                "note": "%d 600-frame batches at once (own encoder/decoder, stream and host thread each); "
                        "best of %d" % (K, max(1, args.steps))}
    # the AVPVS writer's encoder lanes (PIXPATH_FFV1_SPLIT): the same batch as
    # K sub-batches on K encoders, streams and host threads at once
    lanes = None
    K = ffv1.default_split()
    if K > 1 and n % K == 0:
        import threading
        sub = n // K
        lencs = [ffv1.Ffv1Encoder("yuv422p10le", w, h, slices=(nh, nv), max_frames=sub, device=dev) for _ in range(K)]
        lstreams = [torch.cuda.Stream(dev) for _ in range(K)]
        parts = [FrameBatch.interleaved("yuv422p10le", w, h, sub, device=dev) for _ in range(K)]
        for k in range(K):
            for p in range(3):
                parts[k].view(p).copy_(src.view(p)[k * sub:(k + 1) * sub])
        torch.cuda.synchronize()

        def lanes_once():
            def one(k):
                with torch.cuda.stream(lstreams[k]):
                    lencs[k].encode(parts[k], stream=lstreams[k])
            ths = [threading.Thread(target=one, args=(k,)) for k in range(K)]
            t0 = time.perf_counter()
            for t in ths:
                t.start()
            for t in ths:
                t.join()
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        lanes_once()
        ldt = min(lanes_once() for _ in range(max(1, args.steps)))
        one_dt = []
        for _ in range(max(1, args.steps)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lencs[0].encode(parts[0])
            torch.cuda.synchronize()
            one_dt.append(time.perf_counter() - t0)
        lanes = {"lanes": K, "frames_per_lane": sub, "batch_s": round(ldt, 4),
                 "frames_per_s": round(world * n / ldt, 1), "one_sub_batch_alone_s": round(min(one_dt), 4),
                 "note": "the %d-frame batch as %d sub-batches encoded at once (own encoder, stream and host thread "
                         "each: the AVPVS writer's lanes), best of %d; one_sub_batch_alone_s: one sub-batch with "
                         "the GPU to itself" % (n, K, max(1, args.steps))}
        del lencs, parts
    out = dict(head, **{
           "decode": {"frames_per_s": round(world * n / ddt, 1), "ms_per_step": round(ddt * 1e3, 3),
                      "lossless": lossless, "note": "packets from host memory (H2D included)"},
           "concurrent": conc, "writer_lanes": lanes,
           "roofline": None, "library": library_id(), "tuning_overrides": tuning_overrides() or None})
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import ffv1_ref
        k = 3
        frames = [[src.view(p)[f].cpu().numpy() for p in range(3)] for f in range(k)]
        t0 = time.perf_counter()
        for f in frames:
            ffv1_ref.encode_frame(f, 10, 1, 0, nh, nv)
        cdt = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(k / cdt, 3), "unit": "frames/s", "cores": 1, "kind": "port",
                               "sample": "%d frames through oracle/ffv1_oracle.c (gcc -O3, one thread)" % k,
                               "cpu_model": host_cpu()[0]}
        out["reference_stream_decode"] = reference_stream_decode(args, src, dev, ffv1_ref)
    if rank == 0:
        print(json.dumps(out), flush=True)
    return 0


def reference_stream_decode(args, src, dev, ffv1_ref):
    """GPU decode of AVPVSes in the reference's own FFV1 shape
    (`-threads 4 -level 3 -coder 1 -context 1`, /root/reference/lib/ffmpeg.py:993:
    2x2 slices, -context 1's 5-input set, a transmitted state table, GOPs of 12
    with states carried).  The oracle's general encoder writes one GOP of the
    bench content (input generation, untimed; FFmpeg is absent); a stream is
    that GOP repeated 50 times (600 frames = 200 slice chains, one lane each).
    A chain is one slice over a whole GOP, so one stream has 200 serial chains
    where pixpath's 8x8 intra stream has 38,400: it decodes slower than the
    host's cores.  K streams decoded in ONE launch (pp_ffv1_decode_group, as
    the reference's ParallelRunner feeds the CPVS stage several PVSes at once)
    fill the SIMDs: frames/s at K = 1, 4, 16, each checked lossless, beside
    the oracle's general decoder on 1 and 16 host threads (one GOP per thread,
    threads in parallel: ctypes releases the GIL)."""
    import threading
    import time
    import numpy as np
    import torch
    from pixpath import ffv1
    from pixpath.frames import FrameBatch
    w, h, n, gop = src.w, src.h, src.n, 12
    reps = n // gop
    if reps < 1:
        return None
    sets = ffv1_ref.ffmpeg_context1_sets(10)
    pf = ffv1_ref.make_prof(10, 1, 0, 2, 2, sets, tidx=(1, 1), coder=2, gop=gop)
    frames = [[src.view(p)[f].cpu().numpy() for p in range(3)] for f in range(gop)]
    genc = ffv1_ref.GenEncoder(pf, w, h)
    pkts = [genc.encode(f) for f in frames]
    extra = ffv1_ref.gen_extradata(pf)

    def cpu_decode(nthreads):
        ok = [True] * nthreads

        def one(t):
            gdec = ffv1_ref.GenDecoder(extra, w, h)
            for f, p in zip(frames, pkts):
                rc, planes, _ = gdec.decode(p)
                ok[t] = ok[t] and rc == 0 and all(np.array_equal(planes[q], f[q]) for q in range(3))
        ths = [threading.Thread(target=one, args=(t,)) for t in range(nthreads)]
        t0 = time.perf_counter()
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        return {"frames_per_s": round(nthreads * gop / (time.perf_counter() - t0), 3), "threads": nthreads,
                "lossless": all(ok)}
    cpu = [cpu_decode(1), cpu_decode(16)]
    m = reps * gop
    one = np.frombuffer(b"".join(pkts), np.uint8)
    data = torch.from_numpy(np.tile(one, reps)).pin_memory().numpy()
    sizes = np.tile(np.array([len(p) for p in pkts], np.int64), reps)
    fb = frame_bytes("yuv422p10le", w, h)
    rows = []
    decs = []
    for K in (1, 4, 16):
        free = torch.cuda.mem_get_info(dev)[0]
        if K * m * (fb + len(one) / gop) * 1.1 > 0.85 * free:
            rows.append({"streams": K, "skipped": "needs %.1f GB of HBM" % (K * m * fb / 1e9)})
            continue
        while len(decs) < K:
            decs.append(ffv1.Ffv1Decoder(extra, w, h, max_frames=m, device=dev))
        back = FrameBatch("yuv422p10le", w, h, K * m, device=dev)
        ffv1.decode_group(decs[:K], [data] * K, [sizes] * K, dst=back)  # warm-up (workspace growth)
        torch.cuda.synchronize()
        steps = max(1, min(args.steps, 2))
        t0 = time.perf_counter()
        for _ in range(steps):
            for d in decs[:K]:
                d.reset()
            ffv1.decode_group(decs[:K], [data] * K, [sizes] * K, dst=back)
        torch.cuda.synchronize()
        ddt = (time.perf_counter() - t0) / steps
        ok = all(bool(torch.equal(back.view(p)[k * m + r * gop:k * m + (r + 1) * gop], src.view(p)[:gop]))
                 for p in range(3) for k in (0, K - 1) for r in (0, reps - 1))
        rows.append({"streams": K, "frames_per_s": round(K * m / ddt, 1), "ms_per_step": round(ddt * 1e3, 3),
                     "chains": K * reps * 4, "lossless": ok})
        del back
        torch.cuda.empty_cache()
    best = max((r["frames_per_s"] for r in rows if "frames_per_s" in r), default=None)
    return {"frames_per_s": rows[0].get("frames_per_s"), "streams": rows, "frames": m,
            "slices": [2, 2], "gop": gop, "chains_per_stream": reps * 4,
            "slices_per_workgroup": decs[0].slices_per_workgroup if decs else None,
            "bytes_per_frame": round(len(one) / gop, 1),
            "cpu_oracle": cpu[0], "cpu_oracle_16": cpu[1],
            "gpu_best_vs_cpu_16": round(best / cpu[1]["frames_per_s"], 3) if best else None,
            "note": "oracle-encoded GOP (FFmpeg's -coder 1 -context 1 shape) repeated %dx per stream; K streams in "
                    "one pp_ffv1_decode_group launch; packets from pinned host memory (H2D included); CPU: the "
                    "oracle's general decoder, one GOP per thread; FFmpeg's own files unpinned" % reps}


if __name__ == "__main__":
    sys.exit(main())
