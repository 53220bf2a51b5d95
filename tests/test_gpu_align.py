"""pp_frame_sse_band / ops.sse_band on the GPU (spec PP-ALIGN-1) against the
numpy reference (align_ref.sse_band_ref): every comparison is np.array_equal.
The shapes are the smallest at which the kernel can still be wrong: rows on the
piece loader's seams, heights around a tile, several tiles, every alignment
combination, candidate counts around the loop's group and chunk, `first`
entries outside the reference, and sums a 32-bit accumulator would wrap.
Invalid arguments are rejected on the host before any launch."""
import ctypes

import numpy as np
import pytest

import align_ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A


def _make(gpu, depth, n, w, h, layout="std", seed=0, data=None):
    """n luma planes on the device as an [n, h, w] view and their samples as
    numpy.  Layouts: std (pointer, pitch and frame stride on the 16-B grid, at
    least 16 B of pitch padding), odd (one element off the grid, an odd pitch).
    The padding holds random samples of the whole container: poison."""
    import torch
    rng = np.random.default_rng(seed)
    es = 2 if depth > 8 else 1
    dt = np.uint16 if es == 2 else np.uint8
    top = (1 << (8 * es)) - 1
    if layout == "std":
        R, C, x0, y0 = h + 2, ((w * es + 15) // 16 * 16 + 16) // es, 0, 0
        if (R * C * es) % 16:
            R += 1
    else:
        R, C, x0, y0 = h + 3, (w + 7) | 1, 1, 1
    big = rng.integers(0, top + 1, (max(n, 1), R, C)).astype(dt)
    if data is None:
        data = rng.integers(0, top + 1, (n, h, w))
    big[:n, y0:y0 + h, x0:x0 + w] = data
    t = torch.from_numpy(big).to(gpu)[:n, y0:y0 + h, x0:x0 + w]
    on_grid = (t.data_ptr() | t.stride(1) * es | t.stride(0) * es) % 16 == 0
    assert on_grid == (layout == "std")
    return t, big[:n, y0:y0 + h, x0:x0 + w]


def _call(gpu, depth, w, h, dist, ref, first, ncand, out=None, nd=None, nr=None, dls=None, rls=None, null=()):
    """pp_frame_sse_band itself on a sentinel-filled output; returns (rc, out as uint64 numpy)."""
    import torch
    from pixpath import _native, ops
    L = _native.lib()
    nd = dist.shape[0] if nd is None else nd
    nr = ref.shape[0] if nr is None else nr
    es = dist.element_size()
    if out is None:
        out = torch.full((max(nd, 1), max(ncand, 1)), SENTINEL, dtype=torch.int64, device=gpu)
    fi = np.ascontiguousarray(first, dtype=np.int32)
    ptr = lambda name, v: None if name in null else ctypes.c_void_p(v)
    rc = L.pp_frame_sse_band(None if "ctx" in null else ops.context(gpu.index).handle, depth, w, h,
                             ptr("dist", dist.data_ptr()), dist.stride(1) * es if dls is None else dls,
                             dist.stride(0) * es, nd, ptr("ref", ref.data_ptr()),
                             ref.stride(1) * es if rls is None else rls, ref.stride(0) * es, nr,
                             ptr("first", fi.ctypes.data), ncand, ptr("sse", out.data_ptr()),
                             ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    torch.cuda.synchronize(gpu)
    return rc, out.cpu().numpy().view(np.uint64)


def _check(gpu, depth, w, h, nd, nr, first, ncand, dl="std", rl="std", seed=0, ddata=None, rdata=None):
    dist, da = _make(gpu, depth, nd, w, h, dl, seed, ddata)
    ref, ra = _make(gpu, depth, nr, w, h, rl, seed + 1000, rdata)
    rc, got = _call(gpu, depth, w, h, dist, ref, first, ncand)
    assert rc == 0
    want = align_ref.sse_band_ref(da, ra, first, ncand)
    ok = np.array_equal(got, want)
    if not ok:
        bad = np.argwhere(got != want)
        print("%d bit %dx%d dist %s ref %s ncand %d: differs at" % (depth, w, h, dl, rl, ncand), bad[:5].tolist(),
              "of", len(bad), "got", got[tuple(bad[0])], "want", want[tuple(bad[0])])
    assert ok
    assert not (got == SENTINEL).any()  # every element written
    return got


def test_geometry_constants():
    from pixpath import align
    assert (align.LANE_BYTES, align.TILE_BYTES, align.WAVE_ROWS, align.TILE_ROWS) == (16, 1024, 16, 64)
    assert align.TILE_ROWS == 4 * align.WAVE_ROWS and align.TILE_BYTES == 64 * align.LANE_BYTES


@pytest.mark.parametrize("depth", [8, 10])
def test_sizes_on_the_loader_seams(gpu, depth):
    from pixpath import align
    es = 2 if depth > 8 else 1
    span, piece, rows = align.TILE_BYTES, align.LANE_BYTES, align.TILE_ROWS
    row_bytes = [1, 15, 16, 17, span - piece, span + piece]
    widths = sorted({max(1, (b + es - 1) // es) for b in row_bytes})
    for w in widths:
        for h in (1, rows - 1, rows, rows + 1):
            got = _check(gpu, depth, w, h, nd=2, nr=3, first=[0, -1], ncand=3, seed=w + h)
            assert got[1, 0] == align_ref.ABSENT and got[0, 2] != align_ref.ABSENT
    # at least three tiles a frame: two across, two down
    _check(gpu, depth, (span + piece) // es, rows + 1, nd=3, nr=4, first=[1, 0, 2], ncand=2, seed=7)
    _check(gpu, depth, (2 * span + 2 * es) // es, 2 * rows + 3, nd=1, nr=2, first=[0], ncand=2, seed=8)


@pytest.mark.parametrize("depth", [8, 10])
def test_the_four_alignments_agree(gpu, depth):
    w, h, nd, nr = 333, 67, 3, 5
    top = 65535 if depth > 8 else 255
    rng = np.random.default_rng(depth)
    dd, rd = rng.integers(0, top + 1, (nd, h, w)), rng.integers(0, top + 1, (nr, h, w))
    outs = [_check(gpu, depth, w, h, nd, nr, [0, 1, 2], 3, dl=dl, rl=rl, ddata=dd, rdata=rd, seed=i)
            for i, (dl, rl) in enumerate((("std", "std"), ("odd", "std"), ("std", "odd"), ("odd", "odd")))]
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    # a full-piece row (no ragged edge) on the grid, and off it
    _check(gpu, depth, 64, 5, 2, 3, [0, 1], 2, ddata=dd[:2, :5, :64], rdata=rd[:3, :5, :64])
    _check(gpu, depth, 64, 5, 2, 3, [0, 1], 2, dl="odd", ddata=dd[:2, :5, :64], rdata=rd[:3, :5, :64])


@pytest.mark.parametrize("depth", [8, 10])
def test_pitch_padding_never_counts(gpu, depth):
    """Equal pictures in poisoned pitches: every SSE against the own frame is 0."""
    w, h = 37, 9
    top = 65535 if depth > 8 else 255
    data = np.random.default_rng(3).integers(0, top + 1, (2, h, w))
    for dl, rl in (("std", "std"), ("odd", "std"), ("std", "odd")):
        got = _check(gpu, depth, w, h, 2, 2, [0, 1], 1, dl=dl, rl=rl, ddata=data, rdata=data, seed=11)
        assert got.tolist() == [[0], [0]]


def test_candidate_counts(gpu):
    from pixpath import align
    assert (align.GROUP, align.CHUNK) == (4, 32)
    for ncand in (1, 2, align.GROUP + 1, align.CHUNK, align.CHUNK + 1, 2 * align.CHUNK + 1):
        _check(gpu, 8, 50, 20, nd=2, nr=ncand + 2, first=[0, 2], ncand=ncand, seed=ncand)
    _check(gpu, 10, 50, 20, nd=2, nr=36, first=[0, 2], ncand=align.CHUNK + 1, seed=5)
    _check(gpu, 10, 50, 20, nd=2, nr=36, first=[0, 2], ncand=align.CHUNK + 1, dl="odd", seed=6)


@pytest.mark.parametrize("depth", [8, 10])
def test_first_entries(gpu, depth):
    A = align_ref.ABSENT
    nr, ncand = 6, 4
    first = [-2, 4, 0, -9, 6, 100, 3]  # negative, past nref - ncand, inside, wholly outside three ways
    got = _check(gpu, depth, 21, 7, nd=len(first), nr=nr, first=first, ncand=ncand, seed=2)
    assert (got[0, :2] == A).all() and (got[0, 2:] != A).all()
    assert (got[1, :2] != A).all() and (got[1, 2:] == A).all()
    assert (got[3] == A).all() and (got[4] == A).all() and (got[5] == A).all()
    assert (got[2] != A).all() and (got[6, :3] != A).all() and got[6, 3] == A
    # no reference frames at all
    dist, _ = _make(gpu, depth, 2, 21, 7)
    ref, _ = _make(gpu, depth, 1, 21, 7)
    rc, got = _call(gpu, depth, 21, 7, dist, ref, [0, -1], 3, nr=0)
    assert rc == 0 and (got == A).all()
    # extreme entries: first[k] + c is formed in 64 bits
    rc, got = _call(gpu, depth, 21, 7, dist, ref, [2 ** 31 - 1, -2 ** 31], 3)
    assert rc == 0 and (got == A).all()


def test_more_frames_than_one_launch_carries(gpu):
    from pixpath import align
    nd = align.FIRST_PER_LAUNCH + 3
    first = [(k * 7) % 11 - 2 for k in range(nd)]
    _check(gpu, 8, 19, 3, nd=nd, nr=9, first=first, ncand=3, seed=4)


def test_exact_where_32_bits_would_wrap(gpu):
    w, h = 128, 65  # 8,320 samples of 65535^2: 2^45, a lane's share alone passes 2^32
    full = np.full((1, h, w), 65535)
    zero = np.zeros((2, h, w), np.int64)
    for dl, rl in (("std", "std"), ("odd", "std")):
        got = _check(gpu, 10, w, h, 1, 2, [0], 2, dl=dl, rl=rl, ddata=full, rdata=zero)
        assert got.tolist() == [[w * h * 65535 ** 2] * 2] and w * h * 65535 ** 2 > 2 ** 45
        got = _check(gpu, 10, w, h, 2, 1, [0, 0], 1, dl=dl, rl=rl, ddata=zero, rdata=full)  # the other sign
        assert got.tolist() == [[w * h * 65535 ** 2]] * 2
        assert _check(gpu, 10, w, h, 1, 1, [0], 1, dl=dl, rl=rl, ddata=full, rdata=full).tolist() == [[0]]
    got = _check(gpu, 8, 1024, 64, 1, 1, [0], 1, ddata=np.full((1, 64, 1024), 255), rdata=np.zeros((1, 64, 1024)))
    assert got.tolist() == [[1024 * 64 * 255 ** 2]]  # 2^32 and a little: one full tile of an 8-bit plane
    assert _check(gpu, 8, 1024, 64, 1, 1, [0], 1, ddata=zero[:1, :64, :128].repeat(8, axis=2),
                  rdata=np.zeros((1, 64, 1024))).tolist() == [[0]]


def test_runs_are_identical(gpu):
    dist, _ = _make(gpu, 10, 4, 300, 70, seed=1)
    ref, _ = _make(gpu, 10, 8, 300, 70, seed=2)
    a = _call(gpu, 10, 300, 70, dist, ref, [0, 1, 2, 3], 5)[1]
    b = _call(gpu, 10, 300, 70, dist, ref, [0, 1, 2, 3], 5)[1]
    assert np.array_equal(a, b)


def test_no_distorted_frames_writes_nothing(gpu):
    import torch
    dist, _ = _make(gpu, 8, 1, 20, 5)
    ref, _ = _make(gpu, 8, 2, 20, 5)
    out = torch.full((4, 3), SENTINEL, dtype=torch.int64, device=gpu)
    rc, got = _call(gpu, 8, 20, 5, dist, ref, [0], 3, out=out, nd=0)
    assert rc == 0 and (got == SENTINEL).all()
    from pixpath import ops
    assert tuple(ops.sse_band(ref, dist[:0], [], 3).shape) == (0, 3)


def test_wrapper_and_agreement_with_pp_metrics(gpu):
    """ops.sse_band on FrameBatches; for a 4:2:0 case sse[:, c] equals
    pp_metrics' plane-0 SSE with ref_index = first + c."""
    import torch
    from pixpath import ops
    from pixpath.frames import FrameBatch
    for fmt, top in (("yuv420p", 255), ("yuv420p10le", 1023)):
        w, h = 70, 37
        rng = np.random.default_rng(9)
        mk = lambda n: [rng.integers(0, top + 1, (n, r, c)) for r, c in ((h, w), (19, 35), (19, 35))]
        rp, dp = mk(6), mk(3)
        ref, dist = FrameBatch.from_numpy(fmt, rp, device=gpu), FrameBatch.from_numpy(fmt, dp, device=gpu)
        first = np.array([0, 1, 3])
        got = ops.sse_band(ref, dist, first, 3)
        torch.cuda.synchronize(gpu)
        assert got.dtype == torch.int64 and tuple(got.shape) == (3, 3)
        got = got.cpu().numpy()
        assert np.array_equal(got.view(np.uint64), align_ref.sse_band_ref(dp[0], rp[0], first, 3))
        for c in range(3):
            sse, _ = ops.metrics(ref, dist, ref_index=first + c)
            torch.cuda.synchronize(gpu)
            assert np.array_equal(got[:, c], sse.cpu().numpy()[:, 0])
        assert (ops.sse_band(ref, dist, [5, 5, 5], 2).cpu().numpy()[:, 1] == -1).all()  # absent reads as -1
        # the luma tensors themselves
        assert np.array_equal(ops.sse_band(ref.view(0), dist.view(0), first, 3).cpu().numpy(), got)
    with pytest.raises(ValueError):
        ops.sse_band(ref, dist, [0, 1], 3)
    with pytest.raises(ValueError):
        ops.sse_band(ref, dist, [0, 1, 2], 0)


def test_return_codes(gpu):
    from pixpath import _native
    L = _native.lib()
    INVALID, UNSUPPORTED = -1, -4
    dist, _ = _make(gpu, 8, 2, 20, 5)
    ref, _ = _make(gpu, 8, 3, 20, 5)
    d16, _ = _make(gpu, 10, 2, 20, 5)
    r16, _ = _make(gpu, 10, 3, 20, 5)

    def bad(code, word, depth=8, w=20, h=5, d=dist, r=ref, ncand=2, **kw):
        L.pp_frame_sse_band(None, 8, 1, 1, None, 0, 0, 0, None, 0, 0, 0, None, 1, None, None)  # leaves "null argument"
        rc, got = _call(gpu, depth, w, h, d, r, [0, 0], ncand, **kw)
        msg = L.pp_last_error().decode()
        assert rc == code and word in msg, (rc, msg)
        assert (got == SENTINEL).all()  # nothing was launched

    for name in ("ctx", "dist", "ref", "first", "sse"):
        rc, _ = _call(gpu, 8, 20, 5, dist, ref, [0, 0], 2, null=(name,))
        assert rc == INVALID and b"null" in L.pp_last_error()
    bad(INVALID, "frame", w=0)
    bad(INVALID, "frame", h=0)
    bad(INVALID, "ndist", nd=-1)
    bad(INVALID, "nref", nr=-1)
    bad(INVALID, "ncand", ncand=0)
    bad(INVALID, "bitdepth", depth=9)
    bad(INVALID, "bitdepth", depth=16)
    bad(INVALID, "dist plane 0: linesize", dls=19)
    bad(INVALID, "ref plane 0: linesize", rls=19)
    bad(INVALID, "linesize", depth=10, d=d16, r=r16, dls=39)
    bad(INVALID, "2-byte grid", depth=10, d=d16, r=r16, rls=41)
    bad(UNSUPPORTED, "2 GiB buffer range", h=64, dls=1 << 25)
    bad(UNSUPPORTED, "2 GiB buffer range", h=64, rls=1 << 25)
    rc, got = _call(gpu, 8, 20, 5, dist, ref, [0, 0], 2)  # and the same buffers are fine
    assert rc == 0 and not (got == SENTINEL).any()
