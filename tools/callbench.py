"""What the single-call timing tools (tools/*_bench.py) share: the import
paths, the event timer, the throughput summary, the command line, the GPU
preamble, the head of the result, its output, and the noise clip that several
of them time.  Plain functions; nothing here knows a feature.  Importing it
makes `pixpath` and the tests' restatements (tests/*_ref.py) importable and does
not import torch.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "processing-chain_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

W, H = 1920, 1080
HBM_PEAK = 8.0e12  # B/s, the spec
HBM_COPY = 6.29e12  # B/s, a measured copy
FP64_ISSUE_RATE = 256 * 4 * 16 * 2.4e9  # vector fp64 instructions/s: CUs x SIMDs x lanes a clock x clock
HEAD = ("w", "h", "frames", "warmup")


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


def times(fn, warmup, iters):
    """Event-pair times (ms) of one callable: the round robin of one."""
    return timed_round_robin({0: fn}, warmup, iters)[0]


def timed(fn, warmup, iters, count="launches"):
    ms = times(fn, warmup, iters)
    return {"avg_ms": round(sum(ms) / len(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            count: len(ms)}


def throughput(ms, nbytes, median=False, rate=("GBps", 1e6, 1)):
    """Launch times and the rate of `nbytes` moved once per launch; `rate` is (key, bytes a ms per unit, digits)."""
    avg = sum(ms) / len(ms)
    key, unit, digits = rate
    res = {"avg_launch_ms": round(avg, 4)}
    if median:
        res["median_ms"] = round(statistics.median(ms), 4)
    res.update({"min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "bytes": nbytes,
                key: round(nbytes / avg / unit, digits), "frac": round(nbytes / (avg * 1e-3) / HBM_PEAK, 4)})
    return res


def parser(frames, warmup, iters):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=frames)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--iters", type=int, default=iters)
    ap.add_argument("--out", default=None)
    return ap


def require_gpu(tool, seed=None):
    """Device 0, after seeding torch's generators when the tool draws from them; exits without a GPU."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("%s: no GPU visible (a timing needs the MI355X)" % tool)
    if seed is not None:
        torch.manual_seed(seed)
    return torch.device("cuda", 0)


def header(tool, a, order=HEAD, **extra):
    """The head of a result: tool, device, then `order` (w and h, options of `a`
    and entries of `extra` by name), then the rest of `extra` as given."""
    import torch
    vals = {"w": W, "h": H, **vars(a), **extra}
    res = {"tool": tool, "device": torch.cuda.get_device_name(0)}
    res.update((k, vals[k]) for k in order)
    res.update((k, v) for k, v in extra.items() if k not in order)
    return res


def emit(res, out):
    line = json.dumps(res)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def noise_pair(fmt, n, dev):
    """(ref, dist) FrameBatches of n frames: noise over the legal range and the same plus noise of +-8."""
    import torch

    from pixpath.frames import FrameBatch
    ten = fmt.endswith("10le")
    lo, hi = (64, 941) if ten else (16, 236)
    ref, dist = FrameBatch(fmt, W, H, n, device=dev), FrameBatch(fmt, W, H, n, device=dev)
    for p in range(3):
        rp, dp = (t.planes[p].view(torch.int16) if ten else t.planes[p] for t in (ref, dist))
        for k in range(n):  # frame by frame: no batch-sized temporaries
            r = torch.randint(lo, hi, rp[k].shape, dtype=torch.int16, device=dev)
            rp[k].copy_(r)
            dp[k].copy_((r + torch.randint(-8, 9, r.shape, dtype=torch.int16, device=dev)).clamp_(0, 1023 if ten else 255))
    torch.cuda.synchronize()
    return ref, dist
