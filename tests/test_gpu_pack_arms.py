"""Every case of the pad / stall / CPVS arm table (pack_arms.py) on the GPU,
bit-exact against the oracle, with guard bytes round every destination.

Each case runs in its recorded layout and, where that is dense or unaligned,
in the pitched one too; 4:2:0 and v210 cases also run on full-range noise (the
vertical filter's clip and v210's [4, 1019] clip).  The destination is wider
than the picture by 16 bytes a row and one row taller, pre-filled with a
sentinel: after the call everything outside each row's own extent (2 W bytes
of uyvy422, the v210 line size, W samples of a plane) still holds it, and
the v210 bytes between the last pixel group and the line size are zero.  The
launch's arms, asked of the library for the buffers actually passed, are the
ones the CPU test recorded for the case."""
import numpy as np
import pytest

import pyoracle as po
import synth

import pack_arms as pa
import pack_arms_table

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
LIVE = [c for c in pa.CASES if not c.error]


def _variants():
    out = []
    for c in LIVE:
        layouts = [(c.src, c.dst)]
        if layouts[0] != ("pitched", "guard"):
            layouts.append(("pitched", "guard"))
        depth, hs, vs = po.fmt_info(po.FMT_BY_NAME[c.fmt])
        contents = ["legal"] + (["full"] if c.op in ("cpvs", "v210") and (vs or depth > 8) else [])
        out += [pytest.param(c, s, d, k, id="%s-%s-%s-%s" % (c.id, s, d, k)) for s, d in layouts for k in contents]
    return out


def _frames(c, content):
    fmt = po.FMT_BY_NAME[c.fmt]
    rng = np.random.default_rng(len(c.id) * 1009 + c.w)
    if content == "legal":
        return [synth.noise_frame(rng, fmt, c.w, c.h) for _ in range(c.n)]
    return [synth.extreme_frame("noise", fmt, c.w, c.h, seed=i + 1) for i in range(c.n)]


def _source(c, frames, gpu, layout):
    import torch
    from pixpath.frames import FrameBatch
    if layout == "pitched":
        return FrameBatch.from_numpy(c.fmt, synth.batch(frames), device=gpu)
    b = FrameBatch.interleaved(c.fmt, c.w, c.h, len(frames), device=gpu)
    for p, a in enumerate(synth.batch(frames)):
        b.planes[p].copy_(torch.from_numpy(np.ascontiguousarray(a)).to(gpu))
    return b


def _destination(c, n, gpu, layout):
    """(batch, buffers, first sample): every plane [n, rows + 1, pitch + guard] full of the sentinel."""
    import torch
    from pixpath import formats
    from pixpath.frames import FrameBatch
    f = pa.out_fmt(c)
    bps = 1 if f.packed else f.bytes_per_sample
    off = 1 if layout == "offset" else 0
    bufs, planes = [], []
    for r, cols in formats.plane_shapes(f, c.W, c.H):
        pitch = ((cols * bps + 15) // 16 * 16 + pa.GUARD) // bps
        a = np.full((n, r + 1, pitch), SENTINEL * (0x0101 if bps == 2 else 1), np.uint16 if bps == 2 else np.uint8)
        t = torch.from_numpy(a).to(gpu)
        bufs.append(t)
        planes.append(t[:, :, off:])
    return FrameBatch(f, c.W, c.H, n, device=gpu, planes=planes), bufs, off


def _check_guards(c, batch, bufs, off):
    for p, t in enumerate(bufs):
        a = t.cpu().numpy()
        r, cols = batch.shapes[p]
        s = a.dtype.type(SENTINEL * (0x0101 if a.itemsize == 2 else 1))
        assert (a[:, :r, :off] == s).all(), "plane %d: store before a row" % p
        assert (a[:, :r, off + cols:] == s).all(), "plane %d: store past a row's extent" % p
        assert (a[:, r] == s).all(), "plane %d: store into the guard row" % p


def _black(fmt, w, h):
    depth = po.fmt_info(fmt)[0]
    return [np.full(s, (16 if p == 0 else 128) << (depth - 8), dtype=po.plane_dtype(fmt))
            for p, s in enumerate(po.plane_shapes(fmt, w, h))]


def _packed_reference(c, fmt, frame):
    depth = po.fmt_info(fmt)[0]
    if c.op == "v210":
        return po.v210_pack(frame)
    x = c.x if c.x >= 0 else (c.W - c.w) // 2
    y = c.y if c.y >= 0 else (c.H - c.h) // 2
    padded = po.pad(fmt, frame, c.W, c.H, x, y)
    if depth == 8:
        return po.scale(fmt, padded, po.UYVY422, c.W, c.H)[0]
    return po.v210_pack(padded if fmt == po.YUV422P10LE else po.scale(fmt, padded, po.YUV422P10LE, c.W, c.H))


@pytest.mark.parametrize("c,src_layout,dst_layout,content", _variants())
def test_case_matches_oracle_inside_its_guards(gpu, c, src_layout, dst_layout, content):
    from pixpath import ops
    fmt = po.FMT_BY_NAME[c.fmt]
    frames = _frames(c, content)
    src = _source(c, frames, gpu, src_layout)
    nout = len(c.src_index) if c.op == "stall" else c.n
    dst, bufs, off = _destination(c, nout, gpu, dst_layout)
    # the arms of the buffers actually passed are the ones computed from the layout's facts
    inst, arms = pa.query(c, src=src, dst=dst)
    assert arms == pa.query(c, src=pa.src_facts(c, src_layout), dst=pa.dst_facts(c, dst_layout))[1]
    if (src_layout, dst_layout) == (c.src, c.dst):
        rec_inst, rec = pack_arms_table.HELD[c.id]
        assert (pa.instance(c, inst), arms) == (rec_inst, frozenset(rec))
    if c.op == "pad":
        ops.pad(src, c.W, c.H, c.x, c.y, dst=dst)
        x = c.x if c.x >= 0 else (c.W - c.w) // 2
        y = c.y if c.y >= 0 else (c.H - c.h) // 2
        ref = [po.pad(fmt, f, c.W, c.H, x, y) for f in frames]
    elif c.op == "cpvs":
        ops.cpvs(src, c.W, c.H, x=c.x, y=c.y, dst=dst)
        ref = [[_packed_reference(c, fmt, f)] for f in frames]
    elif c.op == "v210":
        ops.v210_pack(src, dst=dst)
        ref = [[_packed_reference(c, fmt, f)] for f in frames]
    else:
        anim = pa.spinner_rgba(c) if c.spin else None
        if anim is not None:
            ops.spinner_upload(anim, c.fmt)
            yuva = [po.spinner_to_yuva(a, fmt) for a in anim]
        ops.stall_compose(src, c.src_index, c.spinner_index, dst=dst)
        black, ref = _black(fmt, c.w, c.h), []
        for si, sp in zip(c.src_index, c.spinner_index):
            base = frames[si] if si >= 0 else black
            ref.append(base if sp < 0 else po.overlay_spinner(fmt, base, yuva[sp]))
    out = dst.to_numpy()
    for k, planes in enumerate(ref):
        for p, want in enumerate(planes):
            np.testing.assert_array_equal(out[p][k], want, err_msg="frame %d plane %d" % (k, p))
    _check_guards(c, dst, bufs, off)
    if pa.out_fmt(c).name == "v210":
        used = (c.W + 5) // 6 * 16
        assert not out[0][:, :, used:].any(), "v210 bytes past the last pixel group are not zero"


def test_stall_source_frame_on_a_skewed_stride(gpu):
    """Aligned rows, frame stride off the 16-B grid, one output frame from
    source frame 1: its rows are misaligned, and since the vector decision
    follows the source extent the kernel reads them by samples.  (The bytes
    were the same before that fix: the hardware tolerates the misaligned
    16-B load.)"""
    import torch
    from pixpath import ops
    from pixpath.frames import FrameBatch
    fmt, w, h, n = po.YUV422P10LE, 24, 4, 2
    rng = np.random.default_rng(77)
    frames = [synth.noise_frame(rng, fmt, w, h) for _ in range(n)]
    planes = []
    for p, (r, cols) in enumerate(po.plane_shapes(fmt, w, h)):
        ls = (cols * 2 + 15) // 16 * 16 // 2
        fs = r * ls + 4  # samples: 8 bytes off the grid
        store = torch.zeros(n * fs, dtype=torch.uint16, device=gpu)
        t = store.as_strided((n, r, ls), (fs, ls, 1))
        t[:, :, :cols].copy_(torch.from_numpy(np.stack([f[p] for f in frames])).to(gpu))
        planes.append(t)
    src = FrameBatch(fmt, w, h, n, device=gpu, planes=planes)
    c = pa.case("skew", "stall", "yuv422p10le", w, h, n=n, spin=(1, 4, 2), src_index=[1], spinner_index=[0])
    assert {"row_src_scalar"} <= pa.query(c, src=src)[1] and "row_src_vec" not in pa.query(c, src=src)[1]
    anim = pa.spinner_rgba(c)
    ops.spinner_upload(anim, fmt)
    dst, bufs, off = _destination(c, 1, gpu, "guard")
    ops.stall_compose(src, c.src_index, c.spinner_index, dst=dst)
    ref = po.overlay_spinner(fmt, frames[1], po.spinner_to_yuva(anim[0], fmt))
    out = dst.to_numpy()
    for p in range(3):
        np.testing.assert_array_equal(out[p][0], ref[p])
    _check_guards(c, dst, bufs, off)
