#!/usr/bin/env python3
"""SHA-256 of what the luma-only analysis ops and ops.metrics give on seeded
inputs: sse_band, ms_ssim, vif, adm, motion, banding, metrics.

Their kernels promise run-to-run identical bits, so a change that is meant to
leave results alone can be held to bit identity: run this on two builds
(PIXPATH_LIB names the library to load) and compare the lines.  The sizes sit
where the GPU tests put theirs: the smallest with every scale of vif and adm,
an odd one, one across a wave's 64 columns and a band's 64 rows, one across a
tile's 256 (254) columns, one across two bands, the smallest with every scale
of ms_ssim (176 each way), and rows wide enough to cross the piece tiles of
pp_motion, pp_frame_sse_band and pp_metrics; each at 8 and 10 bits; one layout
off the 16-byte grid (pointer one sample in, rows three samples longer); and
257 frames of the smallest size under a frame map that is no identity, so that
the split at 256 frames a launch is crossed.  The inputs are noise, except
banding's: noise is all unmasked there, so it gets staircases beside noise.
Prints one JSON line: {"digests": {op: sha256 of all its outputs}, "cases":
{op: {case: sha256}}}.  It fails without a GPU.

  python tools/luma_digest.py [--out profiles/refactor/NAME.json]
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "processing-chain_amd"))

SIZES = ((16, 16), (37, 23), (75, 70), (267, 41), (130, 139), (177, 176), (1030, 9), (2020, 9))  # (w, h)
OFF_GRID = (75, 70)
SMALL = (16, 16)
MAPPED_FRAMES = 257
POOL = 40  # frames a map picks from


def sample(rng, n, w, h, depth):
    import numpy as np
    return rng.integers(0, 1 << depth, (n, h, w)).astype(np.uint16 if depth > 8 else np.uint8)


def stepped(rng, n, w, h, depth):
    """Left of 55 % of the width a slanted staircase of steps 5 + f samples wide
    and 1 .. 4 ten-bit codes high, right of it noise: what banding answers to."""
    import numpy as np
    ii, jj = np.mgrid[0:h, 0:w]
    out = sample(rng, n, w, h, depth)
    for f in range(n):
        band = (jj + ii // 3 + f) // (5 + f % 7)
        val = 200 + band * (1 + (ii // 8) % 4) if depth > 8 else 40 + band
        out[f] = np.where(jj * 100 < w * 55, np.minimum(val, (1 << depth) - 1), out[f])
    return out


def noisy(rng, a, depth):
    import numpy as np
    return np.clip(a.astype(np.int32) + rng.integers(-6, 7, a.shape), 0, (1 << depth) - 1).astype(a.dtype)


def put(a, dev, off_grid=False):
    """[n, h, w] luma on the device; off_grid: a view one sample into rows three samples longer."""
    import torch
    t = torch.from_numpy(a).to(dev)
    if not off_grid:
        return t
    n, h, w = a.shape
    store = torch.zeros((n * h * (w + 3) + 1,), dtype=t.dtype, device=dev)
    v = store.as_strided((n, h, w), (h * (w + 3), w + 3, 1), 1)
    v.copy_(t)
    return v


def cases(dev):
    """(op, case name, thunk giving a device tensor or a tuple of them)"""
    import numpy as np

    from pixpath import formats, ops
    from pixpath.frames import FrameBatch
    rng = np.random.default_rng(20261020)
    out = []

    def pair_ops(tag, r, d, ref_index, first):
        out.append(("sse_band", tag, lambda: ops.sse_band(r, d, first, 3)))
        out.append(("ms_ssim", tag, lambda: ops.ms_ssim(r, d, ref_index)))
        out.append(("vif", tag, lambda: ops.vif(r, d, ref_index)))
        out.append(("adm", tag, lambda: ops.adm(r, d, ref_index)))

    def seq_ops(tag, s, b, index, prev):
        out.append(("motion", tag, lambda: ops.motion(s, index=index, prev=prev)))
        out.append(("banding", tag, lambda: ops.banding(b, index=index)))

    def metric_op(tag, fmt, w, h, n, ref_index, nref):
        shapes = formats.plane_shapes(formats.fmt(fmt), w, h)
        hi = 1 << formats.fmt(fmt).depth
        rp = [rng.integers(0, hi, (nref, r, c)) for r, c in shapes]
        dp = [np.clip(rp[p][np.arange(n) % nref] + rng.integers(-6, 7, (n,) + tuple(shapes[p])), 0, hi - 1)
              for p in range(3)]
        rb, db = FrameBatch.from_numpy(fmt, rp, device=dev), FrameBatch.from_numpy(fmt, dp, device=dev)
        out.append(("metrics", tag, lambda: ops.metrics(rb, db, ref_index)))

    for depth in (8, 10):
        fmt = "yuv420p10le" if depth > 8 else "yuv420p"
        for (w, h), off in [(wh, False) for wh in SIZES] + [(OFF_GRID, True)]:
            tag = "%dx%d_%dbit%s" % (w, h, depth, "_offgrid" if off else "")
            ra = sample(rng, 3, w, h, depth)
            r, d = put(ra, dev, off), put(noisy(rng, ra, depth), dev, off)
            pair_ops(tag, r, d, None, [0, -1, 1])
            seq_ops(tag, r, put(stepped(rng, 3, w, h, depth), dev, off), None, d[1])
            if not off:
                metric_op(tag, fmt, w, h, 3, None, 3)
        w, h = SMALL
        tag = "%dx%d_%dbit_%dmapped" % (w, h, depth, MAPPED_FRAMES)
        idx = ((np.arange(MAPPED_FRAMES) * 7 + 3) % POOL).astype(np.int32)
        ra = sample(rng, POOL, w, h, depth)
        r, d = put(ra, dev), put(noisy(rng, ra[idx], depth), dev)
        pair_ops(tag, r, d, idx, idx - 2)
        seq_ops(tag, r, put(stepped(rng, POOL, w, h, depth), dev), idx, None)
        metric_op(tag, fmt, w, h, MAPPED_FRAMES, idx, POOL)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("luma_digest: no GPU visible")
    dev = torch.device("cuda", 0)
    whole, per = {}, {}
    for op, tag, thunk in cases(dev):
        res = thunk()
        torch.cuda.synchronize()
        raw = b"".join(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()
                       for t in (res if isinstance(res, (tuple, list)) else (res,)) if t is not None)
        whole.setdefault(op, hashlib.sha256()).update(raw)
        per.setdefault(op, {})[tag] = hashlib.sha256(raw).hexdigest()
    line = json.dumps({"tool": "luma_digest", "device": torch.cuda.get_device_name(0),
                       "digests": {op: h.hexdigest() for op, h in whole.items()}, "cases": per})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
