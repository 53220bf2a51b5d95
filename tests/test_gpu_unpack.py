"""pp_unpack_execute on the GPU, bit-exact against the numpy restatement
(unpack_ref.py), with guard samples round every destination.

Inputs are random bytes -- full 32-bit words, bits 30-31 of every v210 word
set, the fields past the last pixel and the line padding random too -- so a
kernel that reads a field it must not shows up.  Destinations are 16 bytes a
row wider and one row taller than the picture and pre-filled with a sentinel:
after the call everything outside each row's own extent still holds it (the
pattern of test_gpu_pack_arms.py).  Sizes are the smallest that reach each
seam of the kernel: the v210 tails, a line of exactly one 128-byte unit and
just over, windows at pixel phase 0 / 2 / 4 of a v210 group and off uyvy422's
8-pixel grid, odd widths, the last pixel pair of the last row, a second trip
of the row loop (from the exported geometry), unaligned pointers and pitches,
batches with padded frame strides, luma-only launches."""
import numpy as np
import pytest

import pyoracle as po
import synth
import unpack_ref

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
GUARD = 16  # bytes


def _ref_fn(fmt):
    return unpack_ref.unpack_v210 if fmt == "v210" else unpack_ref.unpack_uyvy


def _min_linesize(fmt, W):
    from pixpath import formats
    return formats.v210_linesize(W) if fmt == "v210" else (2 * W + 15) // 16 * 16


def _packed(fmt, W, H, n=1, ls=None, seed=0):
    """[n, H, ls] random bytes; v210 words get bits 30-31 set."""
    ls = _min_linesize(fmt, W) if ls is None else ls
    rng = np.random.default_rng(seed * 7919 + W * 31 + H)
    a = rng.integers(0, 256, (n, H, ls), dtype=np.uint8)
    if fmt == "v210":
        a.view("<u4")[...] |= np.uint32(0xC0000000)
    return a


def _source(gpu, fmt, W, H, arr, ptr_off=0, extra_rows=0):
    """FrameBatch over the packed frames ``arr`` [n, H, ls]; ptr_off: bytes the
    plane starts off the allocation; extra_rows: rows of padding per frame."""
    import torch
    from pixpath.frames import FrameBatch
    n, _, ls = arr.shape
    fs = (H + extra_rows) * ls
    store = torch.full((ptr_off + n * fs + 16,), 0x5A, dtype=torch.uint8, device=gpu)
    t = store.as_strided((n, H, ls), (fs, ls, 1), ptr_off)
    t.copy_(torch.from_numpy(arr).to(gpu))
    return FrameBatch(fmt, W, H, n, device=gpu, planes=[t])


def _destination(gpu, fmt, w, h, n, unaligned=False):
    """(planar batch, buffers, first sample): every plane [n, rows + 1, pitch]
    full of the sentinel; unaligned: planes start 2 bytes into their rows and
    the pitches are off the 16-byte grid."""
    import torch
    from pixpath.frames import FrameBatch
    of = "yuv422p10le" if fmt == "v210" else "yuv422p"
    es = 2 if fmt == "v210" else 1
    off = 2 // es if unaligned else 0
    bufs, planes = [], []
    for cols in (w, (w + 1) // 2, (w + 1) // 2):
        pitch = ((cols * es + 15) // 16 * 16 + GUARD + (8 if unaligned else 0)) // es
        a = np.full((n, h + 1, pitch), SENTINEL * (0x0101 if es == 2 else 1), np.uint16 if es == 2 else np.uint8)
        t = torch.from_numpy(a).to(gpu)
        bufs.append(t)
        planes.append(t[:, :, off:])
    return FrameBatch(of, w, h, n, device=gpu, planes=planes), bufs, off


def _check_guards(bufs, off, w, h, planes=(0, 1, 2)):
    for p, t in enumerate(bufs):
        a = t.cpu().numpy()
        s = a.dtype.type(SENTINEL * (0x0101 if a.itemsize == 2 else 1))
        if p not in planes:
            assert (a == s).all(), "plane %d was not handed to the call and changed" % p
            continue
        cols = w if p == 0 else (w + 1) // 2
        assert (a[:, :h, :off] == s).all(), "plane %d: store before a row" % p
        assert (a[:, :h, off + cols:] == s).all(), "plane %d: store past a row's extent" % p
        assert (a[:, h] == s).all(), "plane %d: store into the guard row" % p


def _run(gpu, fmt, W, H, window=None, n=1, ls=None, ptr_off=0, extra_rows=0, unaligned_dst=False, seed=0):
    """Unpack ``window`` of random frames; returns the planes [n, rows, cols] after checking them."""
    from pixpath import ops
    arr = _packed(fmt, W, H, n, ls, seed)
    src = _source(gpu, fmt, W, H, arr, ptr_off, extra_rows)
    x, y, w, h = window or (0, 0, W, H)
    dst, bufs, off = _destination(gpu, fmt, w, h, n, unaligned_dst)
    assert ops.unpack(src, crop=window, dst=dst) is dst
    out = dst.to_numpy()
    for k in range(n):
        for p, want in enumerate(_ref_fn(fmt)(arr[k], W, window)):
            assert want.shape == out[p][k].shape
            assert np.array_equal(out[p][k], want), "frame %d plane %d" % (k, p)
    _check_guards(bufs, off, w, h)
    return out


def _second_trip(fmt):
    from pixpath import ops
    px = ops.UNPACK_CHUNK_PX[fmt]
    assert ops.unpack_trip_px(fmt) == ops.UNPACK_LANES * ops.UNPACK_UNROLL * px and ops.UNPACK_ROWS_PER_WORKGROUP == 1
    return ops.unpack_trip_px(fmt) + px + 2  # one whole chunk and a ragged one past the first trip


V210_WHOLE = [(2, 1), (4, 2), (6, 3), (8, 2), (10, 2), (46, 3), (48, 3), (50, 3)]
V210_WINDOWS = [(0, 0, 62, 7), (2, 1, 58, 5), (4, 2, 54, 3), (6, 0, 50, 7), (14, 3, 35, 2), (60, 6, 2, 1)]
UYVY_WHOLE = [(2, 1), (6, 2), (16, 2), (18, 3)]
UYVY_WINDOWS = [(x, 1, w, 3) for x in (0, 2, 6, 14) for w in (62 - x, 17)]


@pytest.mark.parametrize("W,H", V210_WHOLE)
def test_v210_whole_frame(gpu, W, H):
    _run(gpu, "v210", W, H)


def test_v210_second_trip_of_the_row_loop(gpu):
    _run(gpu, "v210", _second_trip("v210"), 2)


@pytest.mark.parametrize("window", V210_WINDOWS, ids=lambda v: "x%d-y%d-%dx%d" % v)
def test_v210_windows(gpu, window):
    _run(gpu, "v210", 62, 7, window)


@pytest.mark.parametrize("W,H", UYVY_WHOLE)
def test_uyvy_whole_frame(gpu, W, H):
    _run(gpu, "uyvy422", W, H)


@pytest.mark.parametrize("window", UYVY_WINDOWS, ids=lambda v: "x%d-y%d-%dx%d" % v)
def test_uyvy_windows(gpu, window):
    _run(gpu, "uyvy422", 62, 5, window)


def test_uyvy_second_trip_of_the_row_loop(gpu):
    _run(gpu, "uyvy422", _second_trip("uyvy422"), 2)


@pytest.mark.parametrize("fmt,W,H,ls", [("v210", 50, 3, 148), ("uyvy422", 18, 3, 40)])
def test_unaligned_arguments_give_the_aligned_output(gpu, fmt, W, H, ls):
    """Source 4 bytes off its allocation with a line size that is a multiple of
    4 but not of 16; destination planes 2 bytes into their rows with pitches
    off the 16-byte grid; each alone and both together."""
    assert ls % 4 == 0 and ls % 16
    # the same sample bytes in both layouts: the unaligned source's lines are the aligned ones cut / extended
    base = _packed(fmt, W, H, 1, max(ls, _min_linesize(fmt, W)), seed=3)
    want = _ref_fn(fmt)(base[0][:, :ls], W)
    from pixpath import ops
    for ptr_off, lsz, und in ((0, base.shape[2], False), (4, ls, False), (0, base.shape[2], True), (4, ls, True)):
        arr = np.ascontiguousarray(base[:, :, :lsz])
        src = _source(gpu, fmt, W, H, arr, ptr_off)
        assert src.frames_struct().data[0] % 16 == (ptr_off % 16)
        dst, bufs, off = _destination(gpu, fmt, W, H, 1, und)
        ops.unpack(src, dst=dst)
        out = dst.to_numpy()
        for p in range(3):
            assert np.array_equal(out[p][0], want[p]), "plane %d (src +%d, dst unaligned %s)" % (p, ptr_off, und)
        _check_guards(bufs, off, W, H)


@pytest.mark.parametrize("fmt,W,H,window", [("v210", 50, 3, None), ("v210", 62, 7, (14, 3, 35, 2)),
                                            ("uyvy422", 18, 3, None), ("uyvy422", 62, 5, (6, 1, 17, 3))])
def test_batches_with_padded_frame_strides(gpu, fmt, W, H, window):
    out = _run(gpu, fmt, W, H, window, n=3, extra_rows=2, seed=9)
    assert not np.array_equal(out[0][0], out[0][1]) and not np.array_equal(out[0][1], out[0][2])


@pytest.mark.parametrize("fmt", ["v210", "uyvy422"])
def test_no_frames_is_ok_and_writes_nothing(gpu, fmt):
    import ctypes
    from pixpath import _native, ops
    src = _source(gpu, fmt, 18, 3, _packed(fmt, 18, 3))
    dst, bufs, off = _destination(gpu, fmt, 18, 3, 1)
    s, d = src.frames_struct(), dst.frames_struct()
    rc = _native.lib().pp_unpack_execute(ops.context(0).handle, src.fmt.id, 18, 3, ctypes.byref(s), 0, 0, 18, 3,
                                         ctypes.byref(d), 0, None)
    assert rc == 0
    import torch
    torch.cuda.synchronize()
    _check_guards(bufs, off, 0, 0, planes=())


LUMA_CASES = ([("v210", 62, 7, w) for w in V210_WINDOWS] + [("v210", 50, 3, None), ("uyvy422", 18, 3, None)] +
              [("uyvy422", 62, 5, w) for w in UYVY_WINDOWS[:4]])


@pytest.mark.parametrize("fmt,W,H,window", LUMA_CASES)
def test_luma_only(gpu, fmt, W, H, window):
    from pixpath import ops
    arr = _packed(fmt, W, H, 2, seed=4)
    src = _source(gpu, fmt, W, H, arr)
    x, y, w, h = window or (0, 0, W, H)
    full = ops.unpack(src, crop=window).to_numpy()
    dst, bufs, off = _destination(gpu, fmt, w, h, 2)
    luma = dst.planes[0][:, :h, :w]
    assert ops.unpack(src, crop=window, luma_only=True, dst=luma) is luma
    got = luma.cpu().numpy()
    assert np.array_equal(got, full[0])
    for k in range(2):
        assert np.array_equal(got[k], _ref_fn(fmt)(arr[k], W, window)[0])
    _check_guards(bufs, off, w, h, planes=(0,))  # the chroma buffers were not handed over: all sentinel
    # the tensor ops.unpack allocates itself is what ops.siti takes
    own = ops.unpack(src, crop=window, luma_only=True)
    assert own.shape == (2, h, w) and own.stride(2) == 1 and np.array_equal(own.cpu().numpy(), got)


def _legal_batch(gpu, fmt, w, h, n, seed):
    from pixpath.frames import FrameBatch
    rng = np.random.default_rng(seed)
    frames = [synth.noise_frame(rng, po.FMT_BY_NAME[fmt], w, h) for _ in range(n)]
    return FrameBatch.from_numpy(fmt, synth.batch(frames), device=gpu), synth.batch(frames)


@pytest.mark.parametrize("fmt", ["yuv422p10le", "yuv422p"])
def test_round_trip_through_the_cpvs_packer(gpu, fmt):
    from pixpath import ops
    src, planes = _legal_batch(gpu, fmt, 64, 36, 2, 21)
    packed = ops.cpvs(src, 64, 48)
    assert packed.fmt.name == ("v210" if fmt == "yuv422p10le" else "uyvy422")
    back = ops.unpack(packed, crop=(0, 6, 64, 36))
    assert back.fmt.name == fmt
    for got, want in zip(back.to_numpy(), planes):
        assert np.array_equal(got, want)
    # the rows the pad added are black
    top = ops.unpack(packed, crop=(0, 0, 64, 6)).to_numpy()
    s = 4 if fmt == "yuv422p10le" else 1
    assert (top[0] == 16 * s).all() and (top[1] == 128 * s).all() and (top[2] == 128 * s).all()


def test_round_trip_through_v210_pack(gpu):
    from pixpath import ops
    src, planes = _legal_batch(gpu, "yuv422p10le", 50, 4, 2, 22)
    back = ops.unpack(ops.v210_pack(src))
    for got, want in zip(back.to_numpy(), planes):
        assert np.array_equal(got, want)
