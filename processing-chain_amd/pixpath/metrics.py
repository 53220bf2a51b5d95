"""Full-reference PSNR / SSIM of a PVS against its source (spec PP-METRIC-1).

The step a user of the chain takes right after p03: how far the AVPVS is from
the SRC, per frame.  The reference has no code for it (its image builds FFmpeg
with libvmaf for the purpose); the numbers are modelled on FFmpeg's vf_psnr
and vf_ssim and their parity with FFmpeg is unpinned.  The sums
run on the MI355X (pp_metrics) over the decoded frames both files' readers
already put into HBM; everything derived from them (MSE, PSNR, the frame and
clip values) is host arithmetic in this module.
"""
import math
import os

import numpy as np

from . import formats

PLANES = ("y", "u", "v")
# kernel geometry (csrc/metrics.hip), for tests that place sizes on its seams
LANE_BYTES = 16   # kMetLaneBytes: bytes a lane loads per row and input
OWN_LANES = 63    # kMetOwnLanes: lanes of a wave that own blocks
WAVES = 4         # kMetWaves: waves per workgroup
BAND_ROWS = 64    # 4 * kBandBlocks: sample rows of a band


def _psnr(mse, peak):
    """10 log10(peak^2 / MSE); NaN (absent) where MSE is 0 or undefined."""
    mse = np.asarray(mse, dtype=np.float64)
    out = np.full(mse.shape, np.nan)
    ok = mse > 0
    out[ok] = 10.0 * np.log10(peak * peak / mse[ok])
    return out


def summarize(sse, ssim, fmt, w, h):
    """Host side of PP-METRIC-1: per-frame arrays ``mse_y/u/v/all``,
    ``psnr_y/u/v/all``, ``ssim_y/u/v/all`` (float64 [N]) from pp_metrics' sums
    (sse [N, 3] integers, ssim [N, 3]), plus ``mean``: the clip values (mean
    MSE, PSNR of the mean MSE, mean SSIM over the frames that have one).
    Identical planes (MSE 0) have no PSNR: NaN.  ``all``: MSE over the samples
    of all planes; SSIM weighted by plane size over the planes whose SSIM is
    defined."""
    f = formats.fmt(fmt)
    sse = np.asarray(sse).reshape(-1, 3)
    ssim = np.asarray(ssim, dtype=np.float64).reshape(-1, 3)
    size = np.array([r * c for r, c in formats.plane_shapes(f, w, h)], dtype=np.float64)
    peak = float((1 << f.depth) - 1)
    # exact integers up to 2^53: a 2160p 4:4:4 frame of full-range error stays below
    sse = sse.astype(np.float64)
    res = {}
    for p, name in enumerate(PLANES):
        res["mse_" + name] = sse[:, p] / size[p]
        res["ssim_" + name] = ssim[:, p].copy()
    res["mse_all"] = sse.sum(axis=1) / size.sum()
    ok = ~np.isnan(ssim)
    wsum = (ok * size).sum(axis=1)
    num = (np.where(ok, ssim, 0.0) * size).sum(axis=1)
    res["ssim_all"] = np.where(wsum > 0, num / np.where(wsum > 0, wsum, 1.0), np.nan)
    for name in PLANES + ("all",):
        res["psnr_" + name] = _psnr(res["mse_" + name], peak)
    mean = {}
    for name in PLANES + ("all",):
        m = res["mse_" + name]
        mean["mse_" + name] = float(m.mean()) if m.size else float("nan")
        mean["psnr_" + name] = float(_psnr(mean["mse_" + name], peak))
        s = res["ssim_" + name]
        s = s[~np.isnan(s)]
        mean["ssim_" + name] = float(s.mean()) if s.size else float("nan")
    res["mean"] = mean
    res["frames"] = int(sse.shape[0])
    return res


def _open(path, batch):
    """The reader of a file: an AVI by its video fourcc (v210 / UYVY: the
    packed reader, unpacked on the GPU by _read_device; anything else, FFV1
    first of all, the FFV1 reader), other files through io.open_reader."""
    from . import avi, ffv1, io as pio
    if path.lower().endswith(".avi"):
        if pio.packed_fourcc(avi.scan(path, headers_only=True)[0].get("fourcc")):
            return pio.PackedAviReader(path)
        return ffv1.open_avpvs_reader(path, batch=batch)
    return pio.open_reader(path)


def planar_format(rd):
    """The planar format _read_device delivers a reader's frames in."""
    if rd.fmt.packed:
        return formats.fmt("yuv422p10le" if rd.fmt.id == formats.V210 else "yuv422p")
    return rd.fmt


def crop_window(W, H, w, h, crop_from="yuv422p"):
    """(x, y, w, h) of a w x h picture on the W x H canvas where the CPVS pad
    put it: pad_offset's rule (csrc/pack_plan.hpp, pp_pad_execute with
    x = y = -1) -- the centring expression (outer - inner) / 2 rounded down to
    the chroma grid of the padded format ``crop_from`` (the AVPVS's: x to even
    for 4:2:0 and 4:2:2, y to even for 4:2:0 only)."""
    f = formats.fmt(crop_from)
    w, h = int(w), int(h)
    if w < 1 or h < 1 or w > W or h > H:
        raise ValueError("crop %dx%d does not fit the %dx%d canvas" % (w, h, W, H))
    return (((W - w) // 2) >> f.hsub) << f.hsub, (((H - h) // 2) >> f.vsub) << f.vsub, w, h


def _read_device(rd, n, device, window=None):
    """Up to n frames of a reader as a planar device FrameBatch the caller
    owns, or None.  A packed reader's packets go to the GPU as they are and are
    unpacked there (ops.unpack), to ``window`` (x, y, w, h) if given."""
    import torch

    from .frames import FrameBatch
    if rd.fmt.packed:
        from . import ops
        host = np.empty((n, rd.frame_bytes), np.uint8)
        k = rd.read_into(host, n)
        if k == 0:
            return None
        return ops.unpack(rd.device_batch(torch.from_numpy(host[:k]).to(device)), crop=window)
    if hasattr(rd, "read_device"):
        b = rd.read_device(n)  # a view of the reader's own buffer
        if b is None:
            return None
        return FrameBatch.interleaved(rd.fmt, rd.w, rd.h, b.n, device=b.device, storage=b.storage.clone())
    host = np.empty((n, rd.frame_bytes), np.uint8)
    k = rd.read_into(host, n)
    if k == 0:
        return None
    return FrameBatch.interleaved(rd.fmt, rd.w, rd.h, k, device=device, storage=torch.from_numpy(host[:k]).to(device))


def _map_entries(k0, n, in_rate, out_rate, n_in=None):
    """vf_fps entries [k0, k0 + n) of the dist <- ref frame map.  Before the
    reference's length is known the map of a long enough clip is used: the two
    agree on every entry below the true clip's end, up to the clamp to its
    last frame."""
    from . import ops
    if n_in is None:
        n_in = int((k0 + n) * in_rate / out_rate) + 4
    return ops.fps_map(n_in, in_rate, out_rate)[k0:k0 + n]


def metrics_of_files(ref_path, dist_path, batch=32, flags="bicubic", crop=None, crop_from="yuv422p"):
    """PP-METRIC-1 of the file ``dist_path`` (the PVS) against ``ref_path``
    (the SRC); returns ``summarize``'s dict.  Both are read with the chain's
    own readers (FFV1 AVIs through ffv1.open_avpvs_reader, anything else
    through io.open_reader).  A reference of another size or pixel format is
    first brought to the distorted clip's with ops.Scaler (``flags``); at
    another rate, distorted frame k is compared with the reference frame
    vf_fps would show there (ops.fps_map).  Frames stream through the GPU
    ``batch`` at a time; the comparison ends with the shorter of the distorted
    clip and the rate-converted reference.

    A v210 or UYVY AVI (a CPVS, or an uncompressed SRC) is read by
    io.PackedAviReader and unpacked on the GPU (ops.unpack) to yuv422p10le /
    yuv422p.  ``crop`` = (w, h): the distorted clip is a CPVS canvas and only
    the w x h AVPVS picture inside it is compared, at the offsets the CPVS pad
    put it (crop_window; ``crop_from``: the AVPVS's pixel format, which decides
    the rounding of the offsets -- pass "yuv420p" / "yuv420p10le" for a 4:2:0
    AVPVS).  Without ``crop`` the whole canvas is compared."""
    import torch

    from . import ops
    from .frames import FrameBatch
    batch = int(batch)
    ref, dist = _open(ref_path, batch), _open(dist_path, batch)
    try:
        dev = torch.device("cuda", torch.cuda.current_device())
        window = None
        if crop is not None:
            if not dist.fmt.packed:
                raise ValueError("crop applies to a packed (v210 / UYVY) distorted clip")
            window = crop_window(dist.w, dist.h, crop[0], crop[1], crop_from)
        rfmt, dfmt = planar_format(ref), planar_format(dist)
        dw, dh = (dist.w, dist.h) if window is None else window[2:]
        same = (rfmt.id, ref.w, ref.h) == (dfmt.id, dw, dh)
        scaler = None if same else ops.Scaler(rfmt, ref.w, ref.h, dfmt, dw, dh, flags=flags, device=dev)
        in_rate, out_rate = ref.rate, dist.rate
        win, win0, n_ref, ref_end = None, 0, 0, False  # resident reference frames [win0, n_ref), dist geometry
        outs, k0 = [], 0
        while True:
            d = _read_device(dist, batch, dev, window)
            if d is None:
                break
            m = _map_entries(k0, d.n, in_rate, out_rate)
            while not ref_end and n_ref <= int(m[-1]):
                r = _read_device(ref, batch, dev)
                if r is None:
                    ref_end = True
                    break
                if scaler is not None:
                    r = scaler(r)
                keep = max(int(m[0]) - win0, 0) if win is not None else 0
                if win is None or keep >= win.n:
                    win, win0 = r, n_ref
                else:
                    k1 = win.n - keep
                    nw = FrameBatch(dfmt, dw, dh, k1 + r.n, device=dev)
                    for p in range(3):
                        nw.view(p)[:k1].copy_(win.view(p)[keep:])
                        nw.view(p)[k1:].copy_(r.view(p))
                    win, win0 = nw, win0 + keep
                n_ref += r.n
            if ref_end:  # the reference's length is known now: the map's true end and clamp
                m = _map_entries(k0, d.n, in_rate, out_rate, n_in=n_ref)
            if len(m) == 0 or win is None:
                break
            if len(m) < d.n:
                d = FrameBatch(dfmt, dw, dh, len(m), device=d.device, planes=[t[:len(m)] for t in d.planes])
            outs.append(ops.metrics(win, d, ref_index=m - win0))
            k0 += d.n
        torch.cuda.current_stream(dev).synchronize()
    finally:
        ref.close()
        dist.close()
    if outs:
        sse = torch.cat([o[0] for o in outs]).cpu().numpy()
        ssim = torch.cat([o[1] for o in outs]).cpu().numpy()
    else:
        sse, ssim = np.zeros((0, 3), np.int64), np.zeros((0, 3))
    return summarize(sse, ssim, dfmt, dw, dh)


def _json_value(v):
    v = float(v)
    return v if math.isfinite(v) else None


def report(res, ref_path, dist_path, per_frame=False):
    """The JSON object `cli metrics` prints: clip values, and with per_frame
    the per-frame lists; NaN and infinite values become null."""
    out = {"ref": os.path.basename(ref_path), "file": os.path.basename(dist_path), "frames": int(res["frames"]),
           "spec": "PP-METRIC-1"}
    for k, v in res["mean"].items():
        out[k] = _json_value(v)
    if per_frame:
        for kind in ("mse", "psnr", "ssim"):
            for name in PLANES + ("all",):
                key = "%s_%s" % (kind, name)
                out[key + "_frames"] = [_json_value(v) for v in res[key]]
    return out
