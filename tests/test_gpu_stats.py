"""pp_frame_stats / ops.frame_stats on the GPU (spec PP-STATS-1) against the
numpy reference (stats_ref): every comparison is np.array_equal.  The shapes
are the smallest at which the kernel can still be wrong: planes smaller than a
lane's piece, odd sizes, the row trip, the band and the frames-per-workgroup
seams, unaligned layouts, and the sizes at which a narrow counter would
overflow.  Then the file reader and `summarize` end to end."""
import ctypes
import math

import numpy as np
import pytest

import pyoracle as po
import stats_ref

pytestmark = pytest.mark.gpu

PLANAR = ("yuv420p", "yuv422p", "yuv444p", "yuv420p10le", "yuv422p10le", "yuv444p10le")


def _noise(rng, shape, top):
    return rng.integers(0, top + 1, shape)


def _make(gpu, fmt, w, h, n=2, seed=0, layout="std", content=_noise, data=None):
    """A FrameBatch of n frames and its planes as numpy [n, rows, >= cols]
    views.  Layouts: std (pitch rounded up to 16 B), dense (pitch = row),
    view (a window of a wider, taller tensor on the 16-B grid), view_odd (the
    same, one sample off the grid, odd pitch).  The padding holds random
    samples; ``content(rng, shape, top)`` fills the pixels (top = the largest
    value the container holds), or ``data`` gives them."""
    import torch
    from pixpath import formats
    from pixpath.frames import FrameBatch
    f = formats.fmt(fmt)
    rng = np.random.default_rng(seed)
    es = f.bytes_per_sample
    dt = np.uint16 if es == 2 else np.uint8
    top = (1 << (8 * es)) - 1
    tens, arrs = [], []
    for p, (rows, cols) in enumerate(formats.plane_shapes(f, w, h)):
        p16 = (cols * es + 15) // 16 * 16 // es
        R, C, x0, y0 = {"std": (rows, p16, 0, 0), "dense": (rows, cols, 0, 0),
                        "view": (rows + 5, p16 + 32 // es, 16 // es, 2),
                        "view_odd": (rows + 3, (cols + 7) | 1, 1, 1)}[layout]
        big = rng.integers(0, top + 1, (n, R, C)).astype(dt)
        big[:, y0:y0 + rows, x0:x0 + cols] = content(rng, (n, rows, cols), top) if data is None else data[p]
        t = torch.from_numpy(big).to(gpu)
        tens.append(t[:, y0:y0 + rows, x0:])
        arrs.append(big[:, y0:y0 + rows, x0:])
    return FrameBatch(f, w, h, n, planes=tens), arrs


def _got(out):
    hist, sad, over = out
    return (hist.cpu().numpy(), None if sad is None else sad.cpu().numpy().view(np.uint64), over.cpu().numpy())


def _equal(got, want, what=""):
    for name, g, w in zip(("hist", "sad", "over"), got, want):
        if g is None:
            continue
        ok = np.array_equal(g, w)
        if not ok:
            bad = np.argwhere(np.asarray(g) != np.asarray(w))
            print(what, name, "differs at", bad[:5].tolist(), "of", len(bad))
        assert ok, "%s %s" % (what, name)


def _check(gpu, fmt, w, h, prev=False, **kw):
    from pixpath import ops
    from pixpath.frames import FrameBatch
    b, arrs = _make(gpu, fmt, w, h, **kw)
    pb = pa = None
    if prev:
        pbatch, parrs = _make(gpu, fmt, w, h, n=1, seed=kw.get("seed", 0) + 1000, layout="view")
        pb, pa = pbatch, [a[0] for a in parrs]
    got = _got(ops.frame_stats(b, prev=pb))
    want = stats_ref.batch_arrays(fmt, w, h, arrs, prev=pa)
    print(fmt, w, h, {k: v for k, v in kw.items() if k != "data"}, "over", got[2].sum(axis=0).tolist(),
          "sad[-1]", got[1][-1].tolist())
    _equal(got, want, "%s %dx%d" % (fmt, w, h))
    return b, arrs, got


@pytest.mark.parametrize("fmt", PLANAR)
def test_formats_and_sizes(gpu, fmt):
    for w, h in ((1, 1), (2, 2), (17, 3), (64, 64), (130, 67), (1026, 5)):
        _, _, got = _check(gpu, fmt, w, h, n=3, seed=w, prev=(w % 2 == 0))
        if fmt.endswith("10le") and w * h > 16:
            assert got[2].all()  # noise over the container: samples above bit 9 in every plane


def test_the_row_trip_seam(gpu):
    from pixpath import stats
    tb = stats.TILE_BYTES
    assert tb == 1024
    for rowbytes in (tb - 1, tb, tb + 1, 2 * tb + 16):
        _check(gpu, "yuv444p", rowbytes, 2, seed=rowbytes)
    for rowbytes in (tb - 2, tb, tb + 2):
        _check(gpu, "yuv444p10le", rowbytes // 2, 2, seed=rowbytes)
    _check(gpu, "yuv420p", 2 * tb + 2, 3, seed=1)  # chroma one sample past a trip


def test_the_band_and_wave_row_seams(gpu):
    from pixpath import stats
    band, rows = stats.TILE_ROWS, stats.WAVE_ROWS
    for h in (rows - 1, rows, rows + 1, band - 1, band, band + 1, 2 * band + 1):
        _check(gpu, "yuv444p", 20, h, seed=h)
    _check(gpu, "yuv420p10le", 20, 2 * band + 1, seed=1)  # chroma one row past a band


def test_the_frames_per_workgroup_seam(gpu):
    from pixpath import stats
    F = stats.FRAMES_PER_WORKGROUP
    for n in (F - 1, F, F + 1, 2 * F + 1):
        _check(gpu, "yuv420p", 33, 9, n=n, seed=n)
    _check(gpu, "yuv422p10le", 33, 9, n=F + 1, seed=2, prev=True)
    _check(gpu, "yuv422p10le", 33, 9, n=F + 1, seed=3, layout="view_odd")


@pytest.mark.parametrize("fmt", ["yuv420p", "yuv422p10le"])
def test_contents(gpu, fmt):
    ten = fmt.endswith("10le")
    w, h, n = 130, 67, 4
    fills = [0, 1023 if ten else 255] + ([65535] if ten else [])
    for v in fills:
        _, _, got = _check(gpu, fmt, w, h, n=n, content=lambda rng, shape, top, v=v: np.full(shape, v))
        assert (got[1][1:] == 0).all()
        if v == 65535:
            assert not got[0].any() and got[2][0].tolist() == [w * h, 65 * 67, 65 * 67]
        else:
            assert got[0][0, 0, v] == w * h and not got[2].any()

    def checker(rng, shape, top):
        yy, xx = np.indices(shape[1:])
        a = np.where((yy + xx) % 2 == 0, 16, top if not ten else 940)
        return np.broadcast_to(a, shape)

    def ramp(rng, shape, top):
        return np.broadcast_to((np.arange(shape[2]) * 7) % ((1023 if ten else 255) + 1), shape)

    _, _, got = _check(gpu, fmt, w, h, n=n, content=checker)
    assert np.count_nonzero(got[0][0, 0]) == 2
    _check(gpu, fmt, w, h, n=n, content=ramp)
    _check(gpu, fmt, 1300, 3, n=2, content=ramp)  # more than one tile across, runs across lanes


@pytest.mark.parametrize("fmt", ["yuv422p", "yuv420p10le"])
def test_duplicated_frames_have_no_difference(gpu, fmt):
    from pixpath import formats
    w, h = 70, 37
    rng = np.random.default_rng(5)
    top = 1023 if fmt.endswith("10le") else 255
    order = [0, 1, 1, 2, 3, 3, 3, 4]
    data = []
    for rows, cols in formats.plane_shapes(formats.fmt(fmt), w, h):
        base = rng.integers(0, top + 1, (5, rows, cols))
        data.append(base[order])
    _, _, got = _check(gpu, fmt, w, h, n=len(order), data=data)
    zero = (got[1] == 0).all(axis=1).tolist()
    assert zero == [False, False, True, False, False, True, True, False]


@pytest.mark.parametrize("fmt", ["yuv420p", "yuv422p10le", "yuv444p10le"])
def test_unaligned_sources_equal_the_aligned_path(gpu, fmt):
    from pixpath import formats, ops
    w, h, n = 333, 67, 3
    f = formats.fmt(fmt)
    rng = np.random.default_rng(6)
    top = (1 << (8 * f.bytes_per_sample)) - 1
    data = [rng.integers(0, top + 1, (n, r, c)) for r, c in formats.plane_shapes(f, w, h)]
    std, _, got = _check(gpu, fmt, w, h, n=n, data=data)
    es = f.bytes_per_sample
    assert all((t.data_ptr() | t.stride(1) * es | t.stride(0) * es) % 16 == 0 for t in std.planes)
    for layout in ("view_odd", "dense", "view"):
        b, _, other = _check(gpu, fmt, w, h, n=n, data=data, layout=layout, seed=9)
        if layout == "view_odd":  # one sample off the grid, an odd pitch
            t = b.planes[0]
            assert t.data_ptr() % 16 and t.stride(1) % 2 == 1
        _equal(other, got, layout)


def test_prev_chains_two_calls(gpu):
    from pixpath import ops
    from pixpath.frames import FrameBatch
    for fmt in ("yuv420p", "yuv422p10le"):
        w, h = 50, 21
        b, arrs = _make(gpu, fmt, w, h, n=7, seed=12)
        whole = _got(ops.frame_stats(b))
        want = stats_ref.batch_arrays(fmt, w, h, arrs)
        _equal(whole, want, "whole")
        assert (whole[1][0] == stats_ref.SAD_ABSENT).all() and (whole[1][1:] != stats_ref.SAD_ABSENT).all()
        cut = lambda lo, hi: FrameBatch(fmt, w, h, hi - lo, planes=[t[lo:hi] for t in b.planes])
        first = _got(ops.frame_stats(cut(0, 3)))
        second = _got(ops.frame_stats(cut(3, 7), prev=cut(2, 3)))
        for k in range(3):
            assert np.array_equal(np.concatenate([first[k], second[k]]), whole[k])
        # a prev with pitches of its own
        pb, parrs = _make(gpu, fmt, w, h, n=1, seed=13, layout="view_odd")
        got = _got(ops.frame_stats(cut(3, 7), prev=pb))
        _equal(got, stats_ref.batch_arrays(fmt, w, h, [a[3:7] for a in arrs], prev=[a[0] for a in parrs]), "own prev")


def test_without_sad(gpu):
    from pixpath import ops
    for fmt in ("yuv420p", "yuv444p10le"):
        b, arrs = _make(gpu, fmt, 130, 67, n=3, seed=14)
        full = _got(ops.frame_stats(b))
        hist, sad, over = ops.frame_stats(b, want_sad=False)
        assert sad is None
        assert np.array_equal(hist.cpu().numpy(), full[0]) and np.array_equal(over.cpu().numpy(), full[2])
        # prev is ignored without sad
        hist2, _, over2 = ops.frame_stats(b, prev=b, want_sad=False)
        assert np.array_equal(hist2.cpu().numpy(), full[0]) and np.array_equal(over2.cpu().numpy(), full[2])


@pytest.mark.parametrize("w,h", [(512, 300), (4096, 4100)])
def test_counter_width(gpu, w, h):
    """One constant frame: 153,600 samples in one bin (past 16 bits), and
    2^24 + 16,384 (past what a float accumulator holds)."""
    _, _, got = _check(gpu, "yuv420p", w, h, n=1, content=lambda rng, shape, top: np.full(shape, 77))
    assert int(got[0][0, 0, 77]) == w * h
    if w == 4096:
        assert w * h == (1 << 24) + 16384


def test_outputs_are_fully_overwritten_and_argument_checks(gpu):
    import torch
    from pixpath import _native, formats, ops
    L = _native.lib()
    ctx = ops.context(gpu).handle
    for fmt in ("yuv420p", "yuv422p10le"):
        w, h, n = 40, 9, 3
        bins = 1 << formats.fmt(fmt).depth
        b, arrs = _make(gpu, fmt, w, h, n=n, seed=15)
        hist = torch.full((n, 3, bins), -1, dtype=torch.int32, device=gpu)
        sad = torch.full((n, 3), -1, dtype=torch.int64, device=gpu)
        over = torch.full((n, 3), -1, dtype=torch.int32, device=gpu)
        s = b.frames_struct()
        call = lambda fmt_id, nf, src=s: L.pp_frame_stats(
            ctx, fmt_id, w, h, ctypes.byref(src), nf, None, ctypes.c_void_p(hist.data_ptr()),
            ctypes.c_void_p(sad.data_ptr()), ctypes.c_void_p(over.data_ptr()), None)
        # nothing to do, and refused calls: the buffers stay as they were
        assert call(b.fmt.id, 0) == 0
        assert call(formats.V210, n) == -1 and call(formats.UYVY422, n) == -1
        assert call(b.fmt.id, -1) == -1
        bad = b.frames_struct()
        bad.linesize[1] = 1
        assert call(b.fmt.id, n, bad) == -1
        bad = b.frames_struct()
        bad.data[2] = None
        assert call(b.fmt.id, n, bad) == -1
        torch.cuda.synchronize()
        assert (hist == -1).all() and (sad == -1).all() and (over == -1).all()
        assert call(b.fmt.id, n) == 0
        torch.cuda.synchronize()
        want = stats_ref.batch_arrays(fmt, w, h, arrs)
        _equal((hist.cpu().numpy(), sad.cpu().numpy().view(np.uint64), over.cpu().numpy()), want, "0xFF prefill")
    with pytest.raises(ValueError):
        ops.frame_stats(_make_packed(gpu))
    from pixpath.frames import FrameBatch
    hist, sad, over = ops.frame_stats(FrameBatch("yuv422p", 40, 9, 0, device=gpu))
    assert tuple(hist.shape) == (0, 3, 256) and tuple(sad.shape) == (0, 3) and tuple(over.shape) == (0, 3)


def _make_packed(gpu):
    from pixpath.frames import FrameBatch
    return FrameBatch("uyvy422", 16, 4, 1, device=gpu, zero=True)


def test_run_to_run_identical(gpu):
    from pixpath import ops
    b, _ = _make(gpu, "yuv422p10le", 1300, 131, n=5, seed=16)
    first = _got(ops.frame_stats(b))
    for _ in range(3):
        _equal(_got(ops.frame_stats(b)), first, "again")


# ------------------------------------------------------------------ through files
def _same(a, b, path=""):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], path + "/" + str(k))
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), path
    elif isinstance(a, float) and math.isnan(a):
        assert math.isnan(b), path
    else:
        assert a == b, path


W, H, CW, CH = 64, 48, 64, 60


@pytest.fixture(scope="module")
def clip():
    """Nine 64x48 yuv422p10le pictures with luma in 300 .. 900: frame 3 is
    black (Y 64 / C 512), frame 6 repeats frame 5; and the same on the 64x60
    CPVS canvas (bars of 6 rows above and below)."""
    rng = np.random.default_rng(33)
    frames = [[rng.integers(300, 901, (H, W)).astype(np.uint16), rng.integers(200, 800, (H, W // 2)).astype(np.uint16),
               rng.integers(200, 800, (H, W // 2)).astype(np.uint16)] for _ in range(9)]
    frames[3] = [np.full((H, W), 64, np.uint16), np.full((H, W // 2), 512, np.uint16), np.full((H, W // 2), 512, np.uint16)]
    frames[6] = [p.copy() for p in frames[5]]
    padded = [po.pad(po.YUV422P10LE, f, CW, CH, 0, 6) for f in frames]
    return frames, padded


def _stack(frames):
    return [np.stack([f[p] for f in frames]) for p in range(3)]


def test_ffv1_avi_end_to_end(gpu, clip, tmp_path):
    import torch
    from pixpath import ffv1, stats
    from pixpath.frames import FrameBatch
    frames, _ = clip
    path = str(tmp_path / "a.avi")
    wr = ffv1.Ffv1AviWriter(path, "yuv422p10le", W, H, 60, slices=(2, 2), batch=16, device=gpu)
    src = FrameBatch.interleaved("yuv422p10le", W, H, len(frames), device=gpu)
    for i, f in enumerate(frames):
        for p in range(3):
            src.view(p)[i].copy_(torch.from_numpy(f[p]))
    wr.write_device(src)
    wr.close()
    want = stats.summarize(*stats_ref.batch_arrays("yuv422p10le", W, H, _stack(frames)), "yuv422p10le", W, H)
    for batch in (4, 32):  # 4: prev carried over two batch seams
        got = stats.stats_of_file(path, batch=batch)
        assert (got.pop("fmt"), got.pop("w"), got.pop("h")) == ("yuv422p10le", W, H)
        _same(got, want)
    assert want["clip"]["black_frames"] == [[3, 3]] and want["clip"]["repeat_frames"] == [[6, 6]]
    assert math.isnan(want["dif_y"][0]) and want["clip"]["min_y"] == 64.0
    with pytest.raises(ValueError):
        stats.stats_of_file(path, crop=(32, 24))  # crop is for a packed canvas


def test_v210_cpvs_with_and_without_crop(gpu, clip, tmp_path, capsys):
    import json
    from pixpath import avi, cli, stats
    frames, padded = clip
    path = str(tmp_path / "cpvs.avi")
    wr = avi.AviWriter(path, CW, CH, 60, fourcc=b"v210")
    for f in padded:
        wr.write_packet(np.ascontiguousarray(po.v210_pack(f)).reshape(-1))
    wr.close()
    whole = stats.summarize(*stats_ref.batch_arrays("yuv422p10le", CW, CH, _stack(padded)), "yuv422p10le", CW, CH)
    inner = stats.summarize(*stats_ref.batch_arrays("yuv422p10le", W, H, _stack(frames)), "yuv422p10le", W, H)
    got = stats.stats_of_file(path, batch=4)
    assert (got.pop("fmt"), got.pop("w"), got.pop("h")) == ("yuv422p10le", CW, CH)
    _same(got, whole)
    got = stats.stats_of_file(path, batch=4, crop=(W, H))
    assert (got.pop("fmt"), got.pop("w"), got.pop("h")) == ("yuv422p10le", W, H)
    _same(got, inner)
    # the bars: 12 rows of Y 64 in every frame of the canvas, none inside the picture
    live = [k for k in range(9) if k != 3]
    assert (whole["min_y"][live] == 64).all() and (inner["min_y"][live] >= 300).all()
    assert (whole["out_of_range_y"][live] == 0).all() and (whole["low_y"][live] == 64).all()
    for r in (whole, inner):
        assert r["clip"]["black_frames"] == [[3, 3]] and r["clip"]["repeat_frames"] == [[6, 6]]
    capsys.readouterr()
    assert cli.main(["stats", path, "--crop", "%dx%d" % (W, H), "--per-frame", "--batch", "5"]) == 0
    d = json.loads(capsys.readouterr().out)
    assert d["spec"] == "PP-STATS-1" and d["frames"] == 9 and d["black_frames"] == [[3, 3]]
    assert d["repeat_frames"] == [[6, 6]] and d["dif_y_frames"][0] is None and d["dif_y_frames"][6] == 0.0
    assert d["min_y"] == 64.0 and min(d["min_y_frames"][:3]) >= 300
