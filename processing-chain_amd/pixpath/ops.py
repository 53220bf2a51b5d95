"""Python face of the HIP pixel path (thin wrappers over include/pixpath.h).

Every function enqueues on the current torch stream of the frames' device
(or an explicit ``stream``) and returns without synchronising.  There is no
CPU fallback: a missing libpixpath.so raises ``NativeMissing``.
"""
import collections
import ctypes
from fractions import Fraction

import numpy as np
import torch

from . import formats
from . import _native
from ._native import check, lib
from .frames import FrameBatch

FLAGS = {"bilinear": 0x2, "bicubic": 0x4, "lanczos": 0x200}
PARAM_DEFAULT = 123456.0
PLAN_GENERIC = 0x10000000  # PP_PLAN_GENERIC (ABI v5)

# PP_SCALE_FAM_* (pp_scale_plan_instances), by value
FAMILIES = ("plain", "packed", "chain", "chain-luma", "chain-chroma", "general", "copy", "interleave", "two-launch")
InstanceKey = collections.namedtuple(
    "InstanceKey", "family sbytes outb win vtm direct tw256 vtp2 clamped clamp_path cho chunks")

_contexts = {}


class Context:
    """One pp_ctx per process and device (the one-process-per-GPU model)."""

    def __init__(self, device=0):
        h = ctypes.c_void_p()
        check(lib().pp_ctx_create(int(device), ctypes.byref(h)))
        self.handle = h
        self.device = int(device)

    def __del__(self):
        if getattr(self, "handle", None) and lib is not None:
            try:
                lib().pp_ctx_destroy(self.handle)
            except Exception:
                pass
            self.handle = None


def context(device=None):
    if device is None:
        device = torch.cuda.current_device()
    if isinstance(device, torch.device):
        device = device.index if device.index is not None else torch.cuda.current_device()
    device = int(device)
    if device not in _contexts:
        _contexts[device] = Context(device)
    return _contexts[device]


def _stream(t, stream):
    if stream is not None:
        return ctypes.c_void_p(stream if isinstance(stream, int) else stream.cuda_stream)
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class Scaler:
    """swscale-equivalent plan: `scale=W:H:flags=<f>` plus the -pix_fmt conversion.

    Mirrors the filter the reference requests at lib/ffmpeg.py:992 / :1038 /
    :1213 / :800.  flags: "bicubic" (the reference's), "lanczos", "bilinear".
    """

    def __init__(self, src_fmt, sw, sh, dst_fmt, dw, dh, flags="bicubic", param0=None, param1=None,
                 device=None, chain=False, generic=False, host_only=False):
        """chain=True: create_avpvs_segment's two stages (scale into the overlay's
        yuv420p, then yuv420p -> dst_fmt bicubic at the same size) as one plan
        (pp_scale_chain_plan_create): one launch when kernel_path > 0.
        generic=True: the general scale_kernel even where the strip kernel
        applies (PP_PLAN_GENERIC; both are bit-exact, tests run both).
        host_only=True: a plan without a context (no GPU needed): introspection
        only (kernel_path, stats, filter, instance_keys), it cannot execute."""
        self.src_fmt, self.dst_fmt = formats.fmt(src_fmt), formats.fmt(dst_fmt)
        self.sw, self.sh, self.dw, self.dh = int(sw), int(sh), int(dw), int(dh)
        self.ctx = None if host_only else context(device)
        fl = FLAGS[flags] if isinstance(flags, str) else int(flags)
        if generic:
            fl |= PLAN_GENERIC
        h = ctypes.c_void_p()
        create = lib().pp_scale_chain_plan_create if chain else lib().pp_scale_plan_create
        check(create(
            self.ctx.handle if self.ctx else None, self.src_fmt.id, self.sw, self.sh, self.dst_fmt.id, self.dw, self.dh, fl,
            PARAM_DEFAULT if param0 is None else float(param0),
            PARAM_DEFAULT if param1 is None else float(param1), ctypes.byref(h)))
        self.handle = h

    def __del__(self):
        if getattr(self, "handle", None):
            try:
                lib().pp_scale_plan_destroy(self.handle)
            except Exception:
                pass
            self.handle = None

    @property
    def kernel_path(self):
        """> 0: the strip kernel runs (its H window in dwords); 0: the general kernel."""
        return check(lib().pp_scale_plan_path(self.handle))

    @property
    def stats(self):
        """Launch geometry (pp_scale_plan_stats) as a dict."""
        keys = ("lds_bytes", "threads", "tiles_per_frame", "cho", "seg_rows", "vtp_luma", "vtp_chroma",
                "staged_cols", "window_rows", "max_new_rows")
        v = np.zeros(len(keys), dtype=np.int64)
        n = check(lib().pp_scale_plan_stats(self.handle, v.ctypes.data, len(keys)))
        return dict(zip(keys[:n], (int(x) for x in v[:n])))

    @property
    def instance_keys(self):
        """instance_keys_for() aligned sources and destinations."""
        return self.instance_keys_for()

    def instance_keys_for(self, vec_src=True, vec_dst=True):
        """The compiled kernel instance of every launch this plan makes
        (pp_scale_plan_instances), as InstanceKey tuples in launch order, for
        16-B aligned source planes (vec_src) and 8-B aligned destination rows
        (vec_dst)."""
        cap, nf = 8, len(InstanceKey._fields)
        v = np.zeros(cap * nf, dtype=np.int32)
        n = check(lib().pp_scale_plan_instances(self.handle, int(bool(vec_src)), int(bool(vec_dst)),
                                                v.ctypes.data, cap))
        rows = v[: n * nf].reshape(n, nf).tolist()
        return [InstanceKey(FAMILIES[r[0]], *r[1:]) for r in rows]

    def filter(self, which):
        """FFmpeg-layout filter (coef [n, size] int16, pos [n] int32) or None (unscaled path)."""
        n = [self.dw, -((-self.dw) >> (self.dst_fmt.hsub)), self.dh,
             -((-self.dh) >> (0 if self.dst_fmt.packed else self.dst_fmt.vsub))][which]
        cap = n * 64
        coef = np.zeros(cap, dtype=np.int16)
        pos = np.zeros(n, dtype=np.int32)
        size = check(lib().pp_scale_plan_filter(self.handle, which, coef.ctypes.data, pos.ctypes.data, cap))
        if size == 0:
            return None
        return coef[: n * size].reshape(n, size).copy(), pos

    def __call__(self, src, dst=None, stream=None):
        if self.ctx is None:
            raise ValueError("a host-only plan cannot execute")
        if (src.fmt.id, src.w, src.h) != (self.src_fmt.id, self.sw, self.sh):
            raise ValueError("source batch does not match the plan")
        if dst is None:
            dst = FrameBatch(self.dst_fmt, self.dw, self.dh, src.n, device=src.device)
        if (dst.fmt.id, dst.w, dst.h) != (self.dst_fmt.id, self.dw, self.dh) or dst.n < src.n:
            raise ValueError("destination batch does not match the plan")
        s, d = src.frames_struct(), dst.frames_struct()
        check(lib().pp_scale_execute(self.handle, ctypes.byref(s), ctypes.byref(d), src.n,
                                     _stream(src.planes[0], stream)))
        return dst


def pad(src, dw, dh, x=-1, y=-1, dst=None, stream=None):
    """vf_pad with the reference's centring (lib/ffmpeg.py:1183); x=y=-1 -> (ow-iw)/2."""
    ctx = context(src.device.index)
    if dst is None:
        dst = FrameBatch(src.fmt, dw, dh, src.n, device=src.device)
    s, d = src.frames_struct(), dst.frames_struct()
    check(lib().pp_pad_execute(ctx.handle, src.fmt.id, src.w, src.h, ctypes.byref(s), dw, dh, x, y,
                               ctypes.byref(d), src.n, _stream(src.planes[0], stream)))
    return dst


def v210_pack(src, dst=None, stream=None):
    """yuv422p10le -> v210 (libavcodec/v210enc.c), the PC CPVS codec for 10-bit AVPVS."""
    if src.fmt.id != formats.YUV422P10LE:
        raise ValueError("v210 packs yuv422p10le")
    ctx = context(src.device.index)
    if dst is None:
        dst = FrameBatch(formats.V210, src.w, src.h, src.n, device=src.device)
    s, d = src.frames_struct(), dst.frames_struct()
    check(lib().pp_v210_pack(ctx.handle, src.w, src.h, ctypes.byref(s), ctypes.byref(d), src.n,
                             _stream(src.planes[0], stream)))
    return dst


def cpvs(src, W=None, H=None, out_fmt=None, x=-1, y=-1, dst=None, stream=None):
    """Fused PC CPVS: pad to W x H (reference centring) + 4:2:0->4:2:2 + uyvy422
    (8-bit AVPVS) or v210 (10-bit) packing in one pass (lib/ffmpeg.py:1177-1201)."""
    W = src.w if W is None else int(W)
    H = src.h if H is None else int(H)
    if out_fmt is None:
        out_fmt = formats.UYVY422 if src.fmt.depth == 8 else formats.V210
    of = formats.fmt(out_fmt)
    ctx = context(src.device.index)
    if dst is None:
        dst = FrameBatch(of, W, H, src.n, device=src.device)
    s, d = src.frames_struct(), dst.frames_struct()
    check(lib().pp_cpvs_execute(ctx.handle, src.fmt.id, src.w, src.h, ctypes.byref(s), W, H, x, y, of.id,
                                ctypes.byref(d), src.n, _stream(src.planes[0], stream)))
    return dst


# unpack kernel geometry (csrc/unpack_plan.hpp), for tests that place sizes on its seams
UNPACK_LANES = 64                          # kUnpackLanes: lanes of the one wave that owns a row
UNPACK_UNROLL = 4                          # kUnpackUnroll: input chunks a lane decodes per trip of the row loop
UNPACK_CHUNK_PX = {"v210": 6, "uyvy422": 8}  # unpack_px: pixels per 16-B input chunk (one chunk a lane at a time)
UNPACK_PIECE_BYTES = 16                    # output granule: a lane stores one per trip of the store loop
UNPACK_ROWS_PER_WORKGROUP = 1


def unpack_trip_px(fmt):
    """Pixels of a row one trip of the decode loop covers: a window wider than
    this takes a second trip."""
    return UNPACK_LANES * UNPACK_UNROLL * UNPACK_CHUNK_PX[formats.fmt(fmt).name]


def unpack(src, crop=None, luma_only=False, dst=None, stream=None):
    """v210 -> yuv422p10le / uyvy422 -> yuv422p (pp_unpack_execute), the inverse
    of ``cpvs`` and ``v210_pack``.  ``src``: a FrameBatch of v210 or uyvy422
    (its plane may have any pitch the format allows); ``crop``: the window
    (x, y, w, h) to unpack, default the whole frame (x even).  Returns (or
    fills) a planar FrameBatch of the window's size; with ``luma_only`` a
    [N, h, w] luma tensor (uint16 / uint8, a pitched view) as ``siti`` takes,
    and no chroma is written anywhere."""
    if src.fmt.id not in (formats.V210, formats.UYVY422):
        raise ValueError("unpack takes v210 or uyvy422, not %s" % src.fmt.name)
    x, y, w, h = (0, 0, src.w, src.h) if crop is None else (int(v) for v in crop)
    of = formats.fmt(formats.YUV422P10LE if src.fmt.id == formats.V210 else formats.YUV422P)
    ctx = context(src.device.index)
    s = src.frames_struct()
    if luma_only:
        es = of.bytes_per_sample
        if dst is None:
            pitch = (max(w, 1) * es + 15) // 16 * 16 // es
            dst = torch.empty((src.n, max(h, 1), pitch), dtype=torch.uint16 if es == 2 else torch.uint8,
                              device=src.device)[:, :h, :w]
        if dst.dim() != 3 or tuple(dst.shape[1:]) != (h, w) or dst.shape[0] < src.n or dst.element_size() != es \
                or (w > 1 and dst.stride(2) != 1):
            raise ValueError("luma destination must be a [N, %d, %d] tensor of %d-byte samples" % (h, w, es))
        d = _native.pp_frames()
        d.data[0] = dst.data_ptr()
        d.linesize[0] = dst.stride(1) * es
        d.frame_stride[0] = dst.stride(0) * es
        t = dst
    else:
        if dst is None:
            dst = FrameBatch(of, w, h, src.n, device=src.device)
        if (dst.fmt.id, dst.w, dst.h) != (of.id, w, h) or dst.n < src.n:
            raise ValueError("destination batch does not match the window")
        d = dst.frames_struct()
        t = dst.planes[0]
    check(lib().pp_unpack_execute(ctx.handle, src.fmt.id, src.w, src.h, ctypes.byref(s), x, y, w, h, ctypes.byref(d),
                                  src.n, _stream(t, stream)))
    return dst


SitiPlan = collections.namedtuple("SitiPlan", "tiles_x bands ntiles ragged interior_bands fchunk chunks groups")


def siti_plan(bitdepth, w, h, nframes, slots):
    """The launch plan of the SI/TI kernel for ``nframes`` frames of w x h on
    ``slots`` resident workgroups (pp_siti_plan): host only, no GPU.  A depth
    or size pp_siti refuses raises its PixpathError."""
    out = (ctypes.c_int32 * len(SitiPlan._fields))()
    check(lib().pp_siti_plan(int(bitdepth), int(w), int(h), int(nframes), int(slots), out, len(out)))
    p = SitiPlan(*out)
    return p._replace(ragged=bool(p.ragged))


def siti(luma, bitdepth, prev=None, stream=None, normalize=False, *, slots=None):
    """Per-frame P.910 SI/TI of a [N, H, W] luma tensor (uint8 / uint16, may be a
    pitched view).  Returns two float64 device tensors [N]; ti[0] is NaN when
    ``prev`` (the frame before luma[0]) is not given.  ``normalize``: values
    divided by 2^(bitdepth-8) (the 8-bit scale, PP_SITI_NORMALIZE).  ``slots``:
    plan the launch for that many resident workgroups instead of the device's
    own count (pp_siti_slots; tests force small clips onto every arm of the
    kernel with it); the results do not depend on it."""
    if luma.dim() != 3:
        raise ValueError("luma must be [N, H, W]")
    n, h, w = luma.shape
    es = luma.element_size()
    if luma.stride(2) != 1:
        raise ValueError("luma rows must be contiguous")
    ctx = context(luma.device.index)
    si = torch.empty(n, dtype=torch.float64, device=luma.device)
    ti = torch.empty(n, dtype=torch.float64, device=luma.device)
    if n == 0:  # an empty tensor has no address to hand over
        return si, ti
    pp = None
    if prev is not None:
        if prev.stride(-1) != 1 or prev.stride(-2) != luma.stride(1):
            raise ValueError("prev must share the luma row pitch")
        pp = ctypes.c_void_p(prev.data_ptr())
    check(lib().pp_siti_slots(ctx.handle, int(bitdepth), w, h, ctypes.c_void_p(luma.data_ptr()), luma.stride(1) * es,
                              luma.stride(0) * es, n, pp, ctypes.c_void_p(si.data_ptr()),
                              ctypes.c_void_p(ti.data_ptr()), 1 if normalize else 0, 0 if slots is None else int(slots),
                              _stream(luma, stream)))
    return si, ti


def _same_frames(ref, dist, f):
    """Two FrameBatches of the format ``f``, of one size and on one device, or ValueError."""
    if (ref.fmt.id, ref.w, ref.h) != (f.id, dist.w, dist.h) or dist.fmt.id != f.id:
        raise ValueError("ref and dist differ in format or size")
    if ref.device != dist.device:
        raise ValueError("ref and dist are on different devices")


def _ref_index(ref_index, n):
    """``ref_index`` as a contiguous int32 array with one entry per distorted frame; None stays None."""
    if ref_index is None:
        return None
    idx = np.ascontiguousarray(ref_index, dtype=np.int32)
    if idx.shape != (n,):
        raise ValueError("ref_index needs one entry per dist frame")
    return idx


def _prev_plane(prev, s, sd, who):
    """(pointer, pitch in bytes) of ``prev``, the frame shown before the first
    of the luma ``s`` of bit depth ``sd``: a FrameBatch, [1, H, W] or [H, W];
    (None, 0) without one."""
    if prev is None:
        return None, 0
    p, pd = _luma(prev if hasattr(prev, "planes") or prev.dim() == 3 else prev[None], who)
    if pd != sd or tuple(p.shape[1:]) != tuple(s.shape[1:]) or p.shape[0] < 1:
        raise ValueError("prev must be one luma plane of the input's size and bit depth")
    if p.device != s.device:
        raise ValueError("prev is on another device")
    return ctypes.c_void_p(p.data_ptr()), p.stride(1) * s.element_size()


def metrics(ref, dist, ref_index=None, stream=None):
    """Per-frame, per-plane SSE and SSIM of ``dist`` against ``ref`` (spec
    PP-METRIC-1): two FrameBatches of one planar format and size, any pitches.
    dist frame k is compared with ref frame ``ref_index[k]`` (None: frame k).
    Returns device tensors (sse int64 [N, 3], ssim float64 [N, 3]); the SSIM of
    a plane under 8 samples wide or high is NaN."""
    _same_frames(ref, dist, dist.fmt)
    n = dist.n
    ri = _ref_index(ref_index, n)
    if ri is not None:
        if ri.size and ri.max() >= ref.n:
            raise ValueError("ref index out of range")
    elif ref.n < n:
        raise ValueError("ref has fewer frames than dist")
    ctx = context(dist.device.index)
    sse = torch.empty((n, 3), dtype=torch.int64, device=dist.device)
    ssim = torch.empty((n, 3), dtype=torch.float64, device=dist.device)
    r, d = ref.frames_struct(), dist.frames_struct()
    check(lib().pp_metrics(ctx.handle, dist.fmt.id, dist.w, dist.h, ctypes.byref(r), ctypes.byref(d),
                           None if ri is None else ri.ctypes.data, n, ctypes.c_void_p(sse.data_ptr()),
                           ctypes.c_void_p(ssim.data_ptr()), _stream(dist.planes[0], stream)))
    return sse, ssim


# frame_adler32 kernel geometry (csrc/framecrc.hip), for tests that place sizes on its seams
CRC_LANE_BYTES = 16   # kCrcLaneBytes: bytes a lane loads per piece
CRC_LANES = 64        # kCrcLanes: a wave covers CRC_LANES * CRC_LANE_BYTES bytes of a row per trip
CRC_WAVE_ROWS = 16    # kCrcWaveRows: rows of a band one wave sums
CRC_BAND_ROWS = 64    # kCrcBandRows: rows of a unit (4 waves)


def frame_adler32(batch, init=0, stream=None):
    """Per-frame Adler-32 of a FrameBatch of any of the eight formats (spec
    PP-HASH-1, pp_frame_adler32): zlib.adler32 of each frame's byte string
    (planes in order, row by row without the pitch padding; packed formats the
    rows of plane 0) continued from ``init`` -- 0 is what FFmpeg's framecrc
    starts from, 1 zlib's default.  Returns a device tensor [N] of dtype
    torch.uint32 (the kernel's own output, no conversion pass): ``.cpu()``,
    ``.tolist()``, ``.numpy()`` and indexing give the unsigned values; torch
    implements little arithmetic for this dtype, so compare and combine on the
    host."""
    n = batch.n
    dev = batch.device
    if n == 0:  # an empty batch has no plane pointers to pass
        return torch.empty(0, dtype=torch.uint32, device=dev)
    out = torch.empty(n, dtype=torch.uint32, device=dev)
    ctx = context(dev.index)
    s = batch.frames_struct()
    check(lib().pp_frame_adler32(ctx.handle, batch.fmt.id, batch.w, batch.h, ctypes.byref(s), n,
                                 ctypes.c_uint32(int(init) & 0xffffffff), ctypes.c_void_p(out.data_ptr()),
                                 _stream(batch.planes[0], stream)))
    return out


def frame_stats(batch, prev=None, want_sad=True, stream=None):
    """Per-frame, per-plane histogram, difference sum and out-of-container
    count of a planar FrameBatch (spec PP-STATS-1, pp_frame_stats).  Returns
    device tensors on the current stream: ``hist`` int32 [N, 3, bins]
    (bins = 1 << depth; a bin stays below 2^31), ``sad`` int64 [N, 3] (the sum
    of |frame k - frame k-1| per plane, below 2^47; frame 0 against ``prev``,
    a one-frame batch of the same format and size, or without it -1 = absent:
    the kernel's UINT64_MAX read as int64; None with ``want_sad`` False, which
    skips the differences) and ``over`` int32 [N, 3] (10-bit samples >= 1024,
    in no bin).  pixpath.stats.summarize turns the three into the reported
    values."""
    if batch.fmt.packed:
        raise ValueError("frame_stats takes a planar batch: unpack %s first (ops.unpack)" % batch.fmt.name)
    n, dev = batch.n, batch.device
    bins = 1 << batch.fmt.depth
    hist = torch.empty((n, 3, bins), dtype=torch.int32, device=dev)
    over = torch.empty((n, 3), dtype=torch.int32, device=dev)
    sad = torch.empty((n, 3), dtype=torch.int64, device=dev) if want_sad else None
    if n == 0:  # an empty batch has no plane pointers to pass
        return hist, sad, over
    pp = None
    if prev is not None and want_sad:
        if (prev.fmt.id, prev.w, prev.h) != (batch.fmt.id, batch.w, batch.h) or prev.n < 1:
            raise ValueError("prev must be one frame of the batch's format and size")
        if prev.device != dev:
            raise ValueError("prev is on another device")
        ps = prev.frames_struct()
        pp = ctypes.byref(ps)
    ctx = context(dev.index)
    s = batch.frames_struct()
    check(lib().pp_frame_stats(ctx.handle, batch.fmt.id, batch.w, batch.h, ctypes.byref(s), n, pp,
                               ctypes.c_void_p(hist.data_ptr()), None if sad is None else ctypes.c_void_p(sad.data_ptr()),
                               ctypes.c_void_p(over.data_ptr()), _stream(batch.planes[0], stream)))
    return hist, sad, over


def _luma(x, who):
    """([N, H, W] luma tensor, bit depth) of a FrameBatch or of such a tensor
    (uint8: 8 bits, uint16: the 10-bit container) for the operation ``who``."""
    if hasattr(x, "planes"):
        if x.fmt.packed:
            raise ValueError("%s takes planar frames: unpack %s first (ops.unpack)" % (who, x.fmt.name))
        return x.view(0), x.fmt.depth
    if x.dim() != 3 or (x.shape[2] > 1 and x.stride(2) != 1):
        raise ValueError("luma must be [N, H, W] with contiguous rows")
    if x.dtype not in (torch.uint8, torch.uint16):
        raise ValueError("luma must be uint8 or uint16")
    return x, 8 if x.dtype == torch.uint8 else 10


def _luma_pair(ref_batch, dist_batch, who):
    """(ref luma, dist luma, bit depth) of two batches of one size and depth."""
    r, rd = _luma(ref_batch, who)
    d, dd = _luma(dist_batch, who)
    if rd != dd or tuple(r.shape[1:]) != tuple(d.shape[1:]):
        raise ValueError("ref and dist differ in bit depth or size")
    if r.device != d.device:
        raise ValueError("ref and dist are on different devices")
    return r, d, dd


def _ref_dist(who, entry, ref_batch, dist_batch, ref_index, tail, stream):
    """The (ref, dist, ref_index) family: the operation ``who`` calls the
    library's ``entry`` and returns its float64 [ndist, *tail] on the device."""
    r, d, dd = _luma_pair(ref_batch, dist_batch, who)
    n, h, w = d.shape
    idx = _ref_index(ref_index, n)
    out = torch.empty((n,) + tail, dtype=torch.float64, device=d.device)
    if n == 0:  # an empty batch has no data pointer to pass
        return out
    es = d.element_size()
    ctx = context(d.device.index)
    rp = r.data_ptr() if r.shape[0] else d.data_ptr()  # an empty reference: the call rejects the map
    check(getattr(lib(), entry)(ctx.handle, dd, w, h, ctypes.c_void_p(rp), r.stride(1) * es, r.stride(0) * es,
                                r.shape[0], ctypes.c_void_p(d.data_ptr()), d.stride(1) * es, d.stride(0) * es, n,
                                None if idx is None else idx.ctypes.data, ctypes.c_void_p(out.data_ptr()),
                                _stream(d, stream)))
    return out


def _sequence(who, batch_or_luma, bitdepth, index, tail, dtype):
    """The (sequence, index) family, for the operation ``who``: (the luma, its
    own bit depth, the one to pass, index as int32 or None, the result
    [n, *tail] to fill, n the shown frames)."""
    s, sd = _luma(batch_or_luma, who)
    d = sd if bitdepth is None else int(bitdepth)
    idx = None
    n = s.shape[0]
    if index is not None:
        idx = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
        n = int(idx.shape[0])
    out = torch.empty((n,) + tail, dtype=dtype, device=s.device)
    if n and s.shape[0] == 0:
        raise ValueError("index names frames of an empty batch")
    return s, sd, d, idx, out


def _sequence_call(entry, s, d, idx, out, args, stream):
    """Fills ``out`` through the library's ``entry``; ``args`` stand between n and the stream."""
    nsrc, h, w = s.shape
    es = s.element_size()
    ctx = context(s.device.index)
    check(getattr(lib(), entry)(ctx.handle, d, w, h, ctypes.c_void_p(s.data_ptr()), s.stride(1) * es, s.stride(0) * es,
                                nsrc, None if idx is None else idx.ctypes.data, out.shape[0], *args, _stream(s, stream)))
    return out


def sse_band(ref_batch, dist_batch, first, ncand, stream=None):
    """Luma SSE of every frame of ``dist_batch`` against a band of ``ncand``
    frames of ``ref_batch`` (spec PP-ALIGN-1, pp_frame_sse_band): two
    FrameBatches of one size and bit depth, or their [N, H, W] luma tensors
    (any pitches).  ``first``: one int per distorted frame, the reference index
    of its candidate 0 (negative allowed).  Returns a device tensor int64
    [ndist, ncand] on the current stream: out[k, c] = sum (dist[k] -
    ref[first[k] + c])^2, exact, or -1 (the kernel's UINT64_MAX read as int64:
    absent) where first[k] + c is no frame of ``ref_batch``."""
    r, d, dd = _luma_pair(ref_batch, dist_batch, "sse_band")
    n, h, w = d.shape
    fi = np.ascontiguousarray(first, dtype=np.int32)
    if fi.shape != (n,):
        raise ValueError("first needs one entry per dist frame")
    ncand = int(ncand)
    if ncand < 1:
        raise ValueError("ncand must be at least 1")
    out = torch.empty((n, ncand), dtype=torch.int64, device=d.device)
    if n == 0:  # an empty batch has no data pointer to pass
        return out
    es = d.element_size()
    ctx = context(d.device.index)
    # an empty reference has no data pointer: dist's stands in (no candidate exists, nothing is read)
    rp = r.data_ptr() if r.shape[0] else d.data_ptr()
    check(lib().pp_frame_sse_band(ctx.handle, dd, w, h, ctypes.c_void_p(d.data_ptr()), d.stride(1) * es,
                                  d.stride(0) * es, n, ctypes.c_void_p(rp), r.stride(1) * es, r.stride(0) * es,
                                  r.shape[0], fi.ctypes.data, ncand, ctypes.c_void_p(out.data_ptr()),
                                  _stream(d, stream)))
    return out


def ms_ssim(ref_batch, dist_batch, ref_index=None, stream=None):
    """Per-scale MS-SSIM terms of every frame of ``dist_batch`` against
    ``ref_batch`` (spec PP-MSSSIM-1, pp_ms_ssim): two FrameBatches of one size
    and bit depth, or their [N, H, W] luma tensors (any pitches).  Distorted
    frame k is compared with reference frame ``ref_index[k]`` (default: k).
    Returns a device tensor float64 [ndist, 5, 2] on the current stream:
    out[k, s, 0] the mean cs and out[k, s, 1] the mean l * cs of scale s, NaN
    for a scale without a window.  pixpath.msssim.pool turns it into MS-SSIM."""
    return _ref_dist("ms_ssim", "pp_ms_ssim", ref_batch, dist_batch, ref_index, (5, 2), stream)


def vif(ref_batch, dist_batch, ref_index=None, stream=None):
    """Per-scale VIF sums of every frame of ``dist_batch`` against ``ref_batch``
    (spec PP-VIF-1, pp_vif): two FrameBatches of one size and bit depth, or
    their [N, H, W] luma tensors (any pitches).  Distorted frame k is compared
    with reference frame ``ref_index[k]`` (default: k).  Returns a device
    tensor float64 [ndist, 4, 2] on the current stream: out[k, s, 0] the sum of
    num and out[k, s, 1] the sum of den over the positions of scale s, NaN for
    a scale that does not exist.  pixpath.vif.pool turns it into the per-scale
    ratios and VIF."""
    return _ref_dist("vif", "pp_vif", ref_batch, dist_batch, ref_index, (4, 2), stream)


def adm(ref_batch, dist_batch, ref_index=None, stream=None):
    """Per-scale ADM sums of every frame of ``dist_batch`` against ``ref_batch``
    (spec PP-ADM-1, pp_adm): two FrameBatches of one size and bit depth, or
    their [N, H, W] luma tensors (any pitches).  Distorted frame k is compared
    with reference frame ``ref_index[k]`` (default: k).  Returns a device
    tensor float64 [ndist, 4, 6] on the current stream: out[k, s, 0:3] the sums
    of the cubed masked restored coefficients of H, V, D and out[k, s, 3:6] the
    sums of the cubed weighted reference coefficients over the region of scale
    s, NaN for a scale that does not exist.  pixpath.adm.pool turns it into
    adm_scale0..3 and adm2."""
    return _ref_dist("adm", "pp_adm", ref_batch, dist_batch, ref_index, (4, 6), stream)


def _planar_pair(who, entry, f, ref, dist, ref_index, options, tail, stream):
    """The planar (ref, dist, ref_index) family: the operation ``who`` on
    FrameBatches of the format ``f`` calls the library's ``entry`` and returns
    its float64 [ndist, *tail] on the device.  ``options()`` gives the
    arguments between ndist and the result; an empty batch does not ask."""
    if f.packed:
        raise ValueError("%s takes planar frames: unpack %s first (ops.unpack)" % (who, f.name))
    _same_frames(ref, dist, f)
    n = dist.n
    idx = _ref_index(ref_index, n)
    out = torch.empty((n,) + tail, dtype=torch.float64, device=dist.device)
    if n == 0:  # an empty batch has no plane pointers to pass
        return out
    ctx = context(dist.device.index)
    r, d = (ref if ref.n else dist).frames_struct(), dist.frames_struct()  # an empty reference: the call rejects the map
    check(getattr(lib(), entry)(ctx.handle, f.id, dist.w, dist.h, ctypes.byref(r), ctypes.byref(d),
                                None if idx is None else idx.ctypes.data, ref.n, n, *options(),
                                ctypes.c_void_p(out.data_ptr()), _stream(dist.planes[0], stream)))
    return out


def ciede(ref, dist, fmt=None, ref_index=None, weights=(1, 1, 1), stream=None):
    """Per-frame CIEDE2000 sums of ``dist`` against ``ref`` (spec PP-CIEDE-1,
    pp_ciede): two FrameBatches of one planar format and size, any pitches.
    ``fmt`` (a name, an id or a format; default: the batches' own) must be the
    format both carry.  Distorted frame k is compared with reference frame
    ``ref_index[k]`` (default: k).  ``weights``: kL, kC, kH (the CIE's 1, 1, 1).
    Returns a device tensor float64 [ndist, 2] on the current stream: out[k, 0]
    the sum of dE00 over the w h luma positions and out[k, 1] the largest.
    pixpath.ciede.pool turns it into delta_e, delta_e_max and ciede2000."""
    f = dist.fmt if fmt is None else formats.fmt(fmt)
    kL, kC, kH = (float(v) for v in weights)
    return _planar_pair("ciede", "pp_ciede", f, ref, dist, ref_index, lambda: (kL, kC, kH), (2,), stream)


def psnr_hvs(ref, dist, ref_index=None, step=8, stream=None):
    """Per-frame, per-plane PSNR-HVS / PSNR-HVS-M sums of ``dist`` against
    ``ref`` (spec PP-HVS-1, pp_psnr_hvs): two FrameBatches of one planar format
    and size, any pitches.  Distorted frame k is compared with reference frame
    ``ref_index[k]`` (default: k).  ``step``: 8 (the published definition) or
    7 (overlapping blocks).  Returns a device tensor float64 [ndist, 3, 2] on
    the current stream: out[k, p, 0] = S_hvs and out[k, p, 1] = S_hvsm of plane
    p over its 8 x 8 blocks, 0.0 for a plane with no block.
    pixpath.psnrhvs.pool turns it into the MSE and PSNR values."""
    return _planar_pair("psnr_hvs", "pp_psnr_hvs", dist.fmt, ref, dist, ref_index, lambda: [int(step)], (3, 2), stream)


def motion(batch_or_luma, bitdepth=None, index=None, prev=None, stream=None):
    """Blurred-luma difference sums of a shown sequence (spec PP-MOTION-1,
    pp_motion): a FrameBatch or its [N, H, W] luma tensor (any pitches;
    ``bitdepth`` overrides what the input implies).  The sequence shown is
    frame ``index[0]``, ``index[1]``, .. of the input (default: every frame in
    order; repeats and backward steps allowed).  ``prev``: the frame shown
    before the first, a FrameBatch or [1, H, W] / [H, W] luma of the same size
    and depth.  Returns a device tensor uint64 [n] on the current stream:
    sad[k] = sum |B(frame k) - B(frame k - 1)| over the plane, exact; sad[0]
    without ``prev``, and every entry of a plane under 3 x 3, is 2^64 - 1 =
    absent.  pixpath.motion.pool turns it into motion and motion2."""
    s, sd, d, idx, out = _sequence("motion", batch_or_luma, bitdepth, index, (), torch.uint64)
    if out.shape[0] == 0:  # an empty sequence has no data pointer to pass
        return out
    pp, pls = _prev_plane(prev, s, sd, "motion")
    return _sequence_call("pp_motion", s, d, idx, out, (pp, pls, ctypes.c_void_p(out.data_ptr())), stream)


def banding(batch_or_luma, bitdepth=None, index=None, window=None, tvi=None, stream=None):
    """Contrast-value histograms of a shown sequence (spec PP-BAND-1,
    pp_banding): a FrameBatch or its [N, H, W] luma tensor (any pitches;
    ``bitdepth`` overrides what the input implies).  The sequence shown is
    frame ``index[0]``, ``index[1]``, .. of the input (default: every frame in
    order; repeats and backward steps allowed).  ``window``: the odd window
    size 3 .. 63 (default pixpath.banding.default_window(w, h)).  ``tvi``: four
    values, the largest y at which a step of k = 1 .. 4 codes counts (default:
    1023 for all four, no display model).  Returns a device tensor uint32
    [n, 5, 1024] on the current stream: hist[k, s, q] = positions of scale s of
    frame k with contrast value q.  pixpath.banding.pool turns it into the
    banding index."""
    from . import banding as _banding
    s, _, d, idx, out = _sequence("banding", batch_or_luma, bitdepth, index, (_banding.SCALES, _banding.BINS), torch.uint32)
    if out.shape[0] == 0:  # an empty sequence has no data pointer to pass
        return out
    h, w = s.shape[1:]
    win = _banding.default_window(w, h) if window is None else int(window)
    tv = None
    if tvi is not None:
        tv = np.ascontiguousarray(tvi, dtype=np.uint16).reshape(-1)
        if tv.shape != (4,):
            raise ValueError("tvi needs four entries")
    return _sequence_call("pp_banding", s, d, idx, out,
                          (win, None if tv is None else tv.ctypes.data, ctypes.c_void_p(out.data_ptr())), stream)


def dct_energy(batch_or_luma, bitdepth=None, index=None, prev=None, blocks=False, stream=None):
    """DCT-energy sums of a shown sequence (spec PP-DCTE-1, pp_dct_energy): a
    FrameBatch or its [N, H, W] luma tensor (any pitches; ``bitdepth``
    overrides what the input implies).  ``index`` and ``prev``: as
    ops.motion's.  Returns a device tensor uint64 [n, 3] on the current stream:
    out[k] = (energy, dc, tdiff) over the whole 32 x 32 blocks of frame k,
    exact; tdiff[0] without ``prev``, and every entry of a plane under 32 x 32,
    is 2^64 - 1 = absent.  With ``blocks`` also a uint64 [n, by, bx]: the
    blocks' energies, the spatial complexity map.  pixpath.dctenergy.pool
    turns the sums into E, h and L."""
    from . import dctenergy as _dct
    s, sd, d, idx, out = _sequence("dct_energy", batch_or_luma, bitdepth, index, (3,), torch.uint64)
    n = out.shape[0]
    bx, by = _dct.geometry(s.shape[2], s.shape[1])
    bl = torch.empty((n, by, bx), dtype=torch.uint64, device=s.device) if blocks else None
    if n == 0:  # an empty sequence has no data pointer to pass
        return (out, bl) if blocks else out
    pp, pls = _prev_plane(prev, s, sd, "dct_energy")
    # a map without a block has no data pointer: NULL, nothing is written
    bp = ctypes.c_void_p(bl.data_ptr()) if blocks and bx * by else None
    _sequence_call("pp_dct_energy", s, d, idx, out, (pp, pls, ctypes.c_void_p(out.data_ptr()), bp), stream)
    return (out, bl) if blocks else out


def spinner_upload(rgba_frames, f, device=None):
    """Upload an RGBA8 animation [n, h, w, 4] (host) for stall compositing."""
    a = np.ascontiguousarray(rgba_frames, dtype=np.uint8)
    if a.ndim == 3:
        a = a[None]
    n, h, w, _ = a.shape
    ctx = context(device)
    check(lib().pp_spinner_upload(ctx.handle, formats.fmt(f).id, a.ctypes.data, n, w, h))


def stall_compose(src, src_index, spinner_index, dst=None, stream=None):
    """dst[k] = src[src_index[k]] (black if < 0) + spinner frame spinner_index[k] (none if < 0)."""
    si = np.ascontiguousarray(src_index, dtype=np.int32)
    sp = np.ascontiguousarray(spinner_index, dtype=np.int32)
    if si.shape != sp.shape:
        raise ValueError("index arrays differ in length")
    if si.size and (si.max() >= src.n):
        raise ValueError("source index out of range")
    ctx = context(src.device.index)
    if dst is None:
        dst = FrameBatch(src.fmt, src.w, src.h, si.size, device=src.device)
    s, d = src.frames_struct(), dst.frames_struct()
    check(lib().pp_stall_compose(ctx.handle, src.fmt.id, src.w, src.h, ctypes.byref(s), si.ctypes.data,
                                 sp.ctypes.data, ctypes.byref(d), si.size, _stream(src.planes[0], stream)))
    return dst


# enum pp_pack_arm (include/pixpath.h), by value, and the PP_PACK_OP_* / PP_PACK_INST_* values
PACK_ARMS = (
    "cpvs_row_live", "cpvs_row_pad", "cpvs_stage_vec_one", "cpvs_stage_vec_multi", "cpvs_stage_samples",
    "cpvs_group_vec", "cpvs_group_samples", "cpvs_group_clamped", "cpvs_group_vec_ragged", "cpvs_tap_above",
    "cpvs_tap_below", "cpvs_groups_gt64", "cpvs_c8_fast", "cpvs_c8_offgrid", "cpvs_c8_slow_full", "cpvs_c8_slow_tail",
    "cpvs_v210_full", "cpvs_v210_tail2", "cpvs_v210_tail4", "cpvs_v210_zero", "cpvs_chunks_gt64",
    "row_src_vec", "row_src_edge", "row_src_outside", "row_src_scalar", "row_src_null", "row_dst_vec",
    "row_dst_tail", "row_dst_scalar", "row_chunks_gt256", "row_420", "row_422", "row_444",
    "stall_tile_full", "stall_tile_short", "stall_src_change", "stall_black", "stall_no_spinner",
    "stall_spin_left", "stall_spin_right", "stall_spin_inside", "stall_spin_clipped", "stall_launch_split")
PACK_OPS = ("pad", "cpvs", "v210", "stall")
PACK_INSTANCES = ("cpvs8_420", "cpvs8_422", "cpvs10_420", "cpvs10_422", "pad8", "pad16", "stall8", "stall16")


def _layout_struct(layout):
    """pp_frames from a FrameBatch or from alignment facts (data[3], linesize[3], frame_stride[3])."""
    if hasattr(layout, "frames_struct"):
        return layout.frames_struct()
    s = _native.pp_frames()
    for p in range(3):
        s.data[p], s.linesize[p], s.frame_stride[p] = (int(v[p]) for v in layout)
    return s


def pack_arms(op, fmt, w, h, src, dst, W=None, H=None, x=-1, y=-1, nframes=1, src_index=None, spinner_index=None,
              spinner=(0, 0, 0)):
    """Which arms of the pad / stall row kernels or the fused CPVS kernel one
    launch executes (pp_pack_arms): host only, no GPU.  op: "pad", "cpvs",
    "v210" or "stall"; src / dst: the batches, or their alignment facts as
    (data[3], linesize[3], frame_stride[3]); spinner: (frames, width, height)
    uploaded for ``fmt``.  Returns (kernel instance, frozenset of arm names);
    a launch the execute call rejects raises its PixpathError."""
    q = _native.pp_pack_query()
    q.op, q.fmt = PACK_OPS.index(op), formats.fmt(fmt).id
    q.w, q.h = int(w), int(h)
    q.W, q.H = int(w if W is None else W), int(h if H is None else H)
    q.x, q.y, q.nframes = int(x), int(y), int(nframes)
    q.src, q.dst = _layout_struct(src), _layout_struct(dst)
    if op == "stall":
        si = np.ascontiguousarray(src_index, dtype=np.int32)
        sp = np.ascontiguousarray(spinner_index, dtype=np.int32)
        if si.shape != sp.shape:
            raise ValueError("index arrays differ in length")
        q.nframes = si.size
        q.src_index, q.spinner_index = si.ctypes.data, sp.ctypes.data
        q.spin_n, q.spin_w, q.spin_h = (int(v) for v in spinner)
    mask = ctypes.c_uint64()
    inst = check(lib().pp_pack_arms(ctypes.byref(q), ctypes.byref(mask)))
    return PACK_INSTANCES[inst], frozenset(a for i, a in enumerate(PACK_ARMS) if mask.value >> i & 1)


def fps_map(n_in, in_rate, out_rate):
    """vf_fps output->input frame indices (host, no GPU needed)."""
    a, b = Fraction(in_rate), Fraction(out_rate)
    cap = int(n_in * b / a) + 4
    m = np.zeros(max(cap, 1), dtype=np.int32)
    n = check(lib().pp_fps_map(int(n_in), a.numerator, a.denominator, b.numerator, b.denominator,
                               m.ctypes.data, cap))
    return m[:n].copy()
