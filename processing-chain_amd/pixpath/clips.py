"""Reading a clip file into HBM for `cli metrics`, `cli stats` and `cli
framecrc`: the reader of a file, the planar format of its frames, the window of
an AVPVS picture in a CPVS canvas, the loop that streams ``batch`` frames."""
import contextlib
import math

import numpy as np

from . import formats


def open_clip(path, batch):
    """The reader of a file: an AVI by its video fourcc (v210 / UYVY: the
    packed reader, unpacked on the GPU by read_device; anything else, FFV1
    first of all, the FFV1 reader), other files through io.open_reader."""
    from . import avi, ffv1, io as pio
    if path.lower().endswith(".avi"):
        if pio.packed_fourcc(avi.scan(path, headers_only=True)[0].get("fourcc")):
            return pio.PackedAviReader(path)
        return ffv1.open_avpvs_reader(path, batch=batch)
    return pio.open_reader(path)


def planar_format(rd):
    """The planar format read_device delivers a reader's frames in."""
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


def read_packets(rd, n, device):
    """Up to n packets of a packed reader on the device as they are, or None."""
    import torch
    host = np.empty((n, rd.frame_bytes), np.uint8)
    k = rd.read_into(host, n)
    if k == 0:
        return None
    return rd.device_batch(torch.from_numpy(host[:k]).to(device))


def read_device(rd, n, device, window=None):
    """Up to n frames of a reader as a planar device FrameBatch the caller
    owns, or None.  A packed reader's packets go to the GPU as they are and are
    unpacked there (ops.unpack), to ``window`` (x, y, w, h) if given."""
    import torch

    from .frames import FrameBatch
    if rd.fmt.packed:
        from . import ops
        b = read_packets(rd, n, device)
        return None if b is None else ops.unpack(b, crop=window)
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


@contextlib.contextmanager
def clip_batches(path, batch, crop=None, crop_from="yuv422p", what="clip", read=read_device):
    """``with clip_batches(path, batch) as (rd, window, batches)``: the reader
    of a file (open_clip; closed on the way out), the crop_window of ``crop`` =
    (w, h) on its packed canvas (None without) and a generator of its batches
    on the current device, ``batch`` frames each, read by ``read``."""
    import torch
    rd = open_clip(path, batch)
    try:
        if crop is not None and not rd.fmt.packed:
            raise ValueError("crop applies to a packed (v210 / UYVY) %s" % what)
        window = None if crop is None else crop_window(rd.w, rd.h, crop[0], crop[1], crop_from)
        dev = torch.device("cuda", torch.cuda.current_device())

        def batches():
            while (b := read(rd, batch, dev, window)) is not None:
                yield b
        yield rd, window, batches()
    finally:
        rd.close()


def host_array(outs, tail, dtype):
    """The per-batch device tensors of a clip as one numpy array [N, *tail] of
    ``dtype``; of a clip without a frame, the empty array of that shape.
    uint64 sums, which torch does not concatenate, go through an int64 view
    (so do int64 tensors that hold the kernel's uint64)."""
    import torch
    if not outs:
        return np.zeros((0,) + tuple(tail), dtype)
    if np.dtype(dtype) == np.uint64:
        return torch.cat([o.view(torch.int64) for o in outs]).cpu().numpy().view(np.uint64)
    return torch.cat(outs).cpu().numpy()


def nan_mean(v):
    """The mean of the entries of an array that are not NaN; NaN if none."""
    v = v[~np.isnan(v)]
    return float(v.mean()) if v.size else float("nan")


def json_value(v):
    """A result for JSON: NaN and the infinities become null."""
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    v = float(v)
    return v if math.isfinite(v) else None
