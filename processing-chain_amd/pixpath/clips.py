"""Reading clip files into HBM for the file-level commands: the reader of a
file, the planar format of its frames, the window of an AVPVS picture in a CPVS
canvas, the loop that streams ``batch`` frames; a PVS and its SRC as a pair
with the resident reference frames; the luma reader of a file."""
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


def map_entries(k0, n, in_rate, out_rate, n_in=None):
    """vf_fps entries [k0, k0 + n) of the dist <- ref frame map.  Before the
    reference's length is known the map of a long enough clip is used: the two
    agree on every entry below the true clip's end, up to the clamp to its
    last frame."""
    from . import ops
    if n_in is None:
        n_in = int((k0 + n) * in_rate / out_rate) + 4
    return ops.fps_map(n_in, in_rate, out_rate)[k0:k0 + n]


class ReferenceWindow:
    """The resident reference frames of a pair: ``frames`` holds frames
    [first, count) (None before the first batch); ``ended``: the reference has
    been read to its end, ``count`` is its length.  ``batches``: an iterator of
    FrameBatches; ``scale``: None, or what brings each, once, to fmt, w, h."""

    def __init__(self, batches, scale, fmt, w, h):
        self._batches, self._scale, self._geometry = batches, scale, (fmt, w, h)
        self.frames, self.first, self.count, self.ended = None, 0, 0, False

    def extend(self, upto, behind):
        """Reads on until ``count`` reaches ``upto`` or the reference ends.
        Each batch that arrives drops the frames below ``behind``: the tail kept
        and the batch are copied into a fresh FrameBatch; without a tail the
        batch itself becomes the window."""
        from .frames import FrameBatch
        while not self.ended and self.count < upto:
            r = next(self._batches, None)
            if r is None:
                self.ended = True
                break
            if self._scale is not None:
                r = self._scale(r)
            tail = max(self.count - max(int(behind), self.first), 0)  # resident frames at or past ``behind``
            if tail:
                win, joined = self.frames, FrameBatch(*self._geometry, tail + r.n, device=r.device)
                for p in range(3):
                    joined.view(p)[:tail].copy_(win.view(p)[win.n - tail:])
                    joined.view(p)[tail:].copy_(r.view(p))
            self.frames = joined if tail else r
            self.first, self.count = self.count - tail, self.count + r.n


@contextlib.contextmanager
def clip_pair(ref_path, dist_path, batch, flags="bicubic", crop=None, crop_from="yuv422p"):
    """``as (ref, dist, dfmt, dw, dh, dists, window)``: the readers of a SRC
    and its PVS (clip_batches; ``crop`` is the PVS's), the planar format and
    size of the distorted frames, a generator of their batches, and the
    ReferenceWindow of the reference, through ops.Scaler (``flags``) if it differs."""
    from . import ops
    with clip_batches(ref_path, batch) as (ref, _, refs), \
            clip_batches(dist_path, batch, crop, crop_from, "distorted clip") as (dist, cropped, dists):
        rfmt, dfmt = planar_format(ref), planar_format(dist)
        dw, dh = (dist.w, dist.h) if cropped is None else cropped[2:]
        same = (rfmt.id, ref.w, ref.h) == (dfmt.id, dw, dh)
        scaler = None if same else ops.Scaler(rfmt, ref.w, ref.h, dfmt, dw, dh, flags=flags)  # on the current device
        yield ref, dist, dfmt, dw, dh, dists, ReferenceWindow(refs, scaler, dfmt, dw, dh)


class LumaOf:
    """A full-frame pixpath.io reader seen as a luma reader."""

    def __init__(self, rd):
        self.rd, self.w, self.h, self.depth = rd, rd.w, rd.h, rd.fmt.depth
        self.luma_bytes = self.w * self.h * (2 if self.depth > 8 else 1)
        self._buf = None

    def read_into(self, buf, n):
        fb = self.rd.frame_bytes
        if self._buf is None or len(self._buf) < n * fb:
            self._buf = np.empty(n * fb, np.uint8)
        k = self.rd.read_into(self._buf, n)
        out = np.frombuffer(memoryview(buf).cast("B"), np.uint8)
        lb = self.luma_bytes
        for i in range(k):
            out[i * lb:(i + 1) * lb] = self._buf[i * fb:i * fb + lb]
        return k

    def close(self):
        self.rd.close()


def open_luma(videofile, reader=None):
    """(rd, packed) for the luma of a file.  A v210 or UYVY AVI needs no
    decoder: rd is its io.PackedAviReader, whose packets go to the GPU as they
    are, the luma unpacked there.  Otherwise rd is a luma reader: io.LumaReader
    (y4m / raw seek past chroma, ffmpeg decodes to gray / gray10le) or, of
    ``reader``, a full-frame pixpath.io reader, its luma plane (LumaOf).  The
    caller closes rd."""
    from . import avi, io as pio
    if reader is not None:
        return LumaOf(reader), False
    if isinstance(videofile, str) and videofile.lower().endswith(".avi") \
            and pio.packed_fourcc(avi.scan(videofile, headers_only=True)[0].get("fourcc")):
        return pio.PackedAviReader(videofile), True
    return pio.LumaReader(videofile), False


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
