"""pp_banding / ops.banding on the GPU (spec PP-BAND-1) against the numpy
restatement (banding_ref.hist).  The histograms are integers: the bar is
np.array_equal, no tolerance.

Every call of pp_banding itself writes into a sentinel-filled output two frames
longer than it needs and must change [n][5][1024] alone; planes carry poisoned
pitch padding (gpu_calls.make).  The content is banding_ref.content, half
banded and half noisy (test_banding_host checks that it exercises the mask, the
window and several bins).  The shapes are the smallest at which the kernels can
still be wrong: 1 x 1, a row, a column, the mask's 7 x 7, a window larger than
the plane, and widths and heights one below, at and one above the tiles of the
mask kernel (32 rows x 64 columns) and of the contrast kernel (32 x 32), and
two tiles and a sample, which is also more than one chunk of tiles."""

import numpy as np
import pytest

import banding_ref as R
from gpu_calls import call_sequence, make as _make, untouched

pytestmark = pytest.mark.gpu

_REF = {}


def _content(depth, n, w, h, seed=0):
    key = (depth, n, w, h, seed)
    if key not in _REF:
        _REF[key] = R.content(depth, n, w, h, seed)
    return _REF[key]


def _want(a, depth, window, idx=None, tvi=None):
    """hist [n, 5, 1024] of the shown sequence; a frame is restated once."""
    def one(f):
        key = ("h", depth, window, None if tvi is None else tuple(tvi), a.shape, a[f].tobytes())
        if key not in _REF:
            _REF[key] = R.frame_hist(a[f], depth, window, tvi)
        return _REF[key]
    return np.stack([one(f) for f in (range(a.shape[0]) if idx is None else idx)])


def _call(gpu, depth, w, h, src, window, idx=None, n=None, nsrc=None, tvi=None, sls=None, null=()):
    """pp_banding itself on a sentinel-filled output of two frames more than it
    needs; returns (rc, hist [n, 5, 1024] uint32, untouched: everything else kept the sentinel)."""
    tv = None if tvi is None else np.ascontiguousarray(tvi, dtype=np.uint16)
    rc, k, (raw,) = call_sequence(gpu, "pp_banding", depth, w, h, src, (window, None if tv is None else tv.ctypes.data),
                                  [("hist", (5, 1024), "int32")], idx, n, nsrc, sls, null)
    return rc, raw[:k].copy(), untouched(raw, k)


def _check(gpu, depth, a, window, idx=None, tvi=None, layout="std", label=""):
    """a [nsrc, h, w] planes: the call's histograms equal banding_ref's; returns them."""
    want = _want(a, depth, window, idx, tvi)  # CPU side first
    nsrc, h, w = a.shape
    src = _make(gpu, depth, a, layout, 1)
    rc, got, untouched = _call(gpu, depth, w, h, src, window, idx, tvi=tvi)
    assert rc == 0 and untouched, (label, rc)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        k, s, q = bad[0]
        raise AssertionError((label, depth, w, h, window, layout, len(bad), (int(k), int(s), int(q)),
                              int(got[k, s, q]), int(want[k, s, q])))
    sizes = [((w + (1 << s) - 1) >> s) * ((h + (1 << s) - 1) >> s) for s in range(5)]
    assert got.sum(axis=2).tolist() == [sizes] * got.shape[0]
    return got


def test_geometry_constants():
    from pixpath import banding
    assert (banding.MASK_TILE_ROWS, banding.MASK_TILE_COLS, banding.TILE, banding.CHUNK) == (32, 64, 32, 4)
    assert (banding.SCALES, banding.BINS, banding.FRAMES_PER_LAUNCH) == (5, 1024, 256)


@pytest.mark.parametrize("depth", [8, 10])
def test_smallest_planes(gpu, depth):
    for w, h in ((1, 1), (9, 1), (1, 9), (7, 7)):
        a = _content(depth, 2, w, h, seed=w * 10 + h)
        _check(gpu, depth, a, 3, label="small")
        _check(gpu, depth, a, 3, layout="odd", label="small odd")
        flat = np.full_like(a, 37)
        got = _check(gpu, depth, flat, 3, label="flat")
        assert (got[:, :, 1:] == 0).all()  # one value: no contrast anywhere
        two = flat.copy()
        two[:, :, w // 2:] += 1            # a step of one code (four on the ten-bit scale at 8 bits)
        got = _check(gpu, depth, two, 3, label="two values")
        assert got[:, 0, 1:].any() == ((w, h) == (7, 7))  # only the 7 x 7 plane has a masked position


@pytest.mark.parametrize("depth", [8, 10])
def test_windows(gpu, depth):
    a = _content(depth, 2, 40, 24, seed=1)
    _check(gpu, depth, a, 5, label="w5")
    got = _check(gpu, depth, a, 63, label="w63")  # the window is larger than the plane
    assert got[:, 0, 1:].any()
    b = _content(depth, 2, 131, 67, seed=2)
    _check(gpu, depth, b, 15, label="w15")
    _check(gpu, depth, b, 15, layout="odd", label="w15 odd")


@pytest.mark.parametrize("depth", [8, 10])
def test_default_window_of_a_small_plane(gpu, depth):
    a = _content(depth, 2, 200, 120, seed=3)
    got = _check(gpu, depth, a, 33, label="w33")
    assert (got[:, 0, 1:] != 0).sum() >= 3


@pytest.mark.parametrize("depth", [8, 10])
def test_width_seams(gpu, depth):
    for w in (31, 32, 33, 63, 64, 65, 129):
        a = _content(depth, 2, w, 9, seed=w)
        _check(gpu, depth, a, 5, label="width")
        _check(gpu, depth, a, 5, layout="odd", label="width odd")


@pytest.mark.parametrize("depth", [8, 10])
def test_height_seams(gpu, depth):
    for h in (31, 32, 33, 65):
        a = _content(depth, 2, 23, h, seed=h)
        _check(gpu, depth, a, 5, label="height")
        _check(gpu, depth, a, 5, layout="odd", label="height odd")


def test_two_tiles_and_a_sample_both_ways(gpu):
    """15 contrast tiles at scale 0: four chunks of tiles, the last a short one."""
    for depth in (8, 10):
        a = _content(depth, 2, 129, 65, seed=6)
        _check(gpu, depth, a, 9, label="tiles")


def test_layouts_give_equal_results(gpu):
    for depth in (8, 10):
        a = _content(depth, 3, 77, 41, seed=5)
        got = [_check(gpu, depth, a, 7, layout=lay, label="layout") for lay in ("std", "odd")]
        assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("depth", [8, 10])
def test_index(gpu, depth):
    a = _content(depth, 4, 45, 37, seed=7)
    idx = [2, 2, 0, 3, 1, 0]  # repeats and backward steps
    got = _check(gpu, depth, a, 7, idx=idx, label="index")
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[2], got[5])
    _check(gpu, depth, a, 7, idx=[3], layout="odd", label="index one")


def test_tvi_disables_small_steps(gpu):
    a = _content(10, 2, 64, 40, seed=8)
    full = _check(gpu, 10, a, 9, label="tvi none")
    assert np.array_equal(_check(gpu, 10, a, 9, tvi=[1023] * 4, label="tvi 1023"), full)
    cut = _check(gpu, 10, a, 9, tvi=[0, 0, 1023, 1023], label="tvi k 3 4")  # no sample is 0: k = 1, 2 are off
    assert not np.array_equal(cut, full)
    part = _check(gpu, 10, a, 9, tvi=[210, 205, 1023, 0], label="tvi mid")  # thresholds inside the staircase
    assert not np.array_equal(part, full) and not np.array_equal(part, cut)
    none = _check(gpu, 10, a, 9, tvi=[0, 0, 0, 0], label="tvi off")
    assert (none[:, :, 1:] == 0).all()


def test_clamp_of_the_16_bit_container(gpu):
    """A stored 10-bit sample above 1023 counts as 1023."""
    a = _content(10, 2, 70, 33, seed=9).copy()
    a[0, 5:20, 40:66] = 40000
    a[1, :, 50:] = np.random.default_rng(5).integers(0, 65536, (33, 20))
    got = _check(gpu, 10, a, 7, label="clamp")
    _check(gpu, 10, a, 7, layout="odd", label="clamp odd")
    assert np.array_equal(_check(gpu, 10, np.minimum(a, 1023), 7), got)


def test_two_runs_give_equal_bits(gpu):
    a = _content(10, 3, 150, 67, seed=12)
    src = _make(gpu, 10, a, "std", 1)
    runs = [_call(gpu, 10, 150, 67, src, 11)[1] for _ in range(2)]
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], _want(a, 10, 11))


def test_more_frames_than_a_launch(gpu):
    from pixpath import banding
    a = _content(8, 3, 20, 6, seed=13)
    idx = [(k * 7) % 3 for k in range(banding.FRAMES_PER_LAUNCH + 3)]
    _check(gpu, 8, a, 3, idx=idx, label="launch")


def test_no_frames_writes_nothing(gpu):
    import torch
    from pixpath import ops
    a = _content(8, 2, 20, 15)
    src = _make(gpu, 8, a)
    rc, got, untouched = _call(gpu, 8, 20, 15, src, 3, n=0)
    assert rc == 0 and got.shape[0] == 0 and untouched
    out = ops.banding(src[:0])
    assert out.dtype == torch.uint32 and tuple(out.shape) == (0, 5, 1024)
    assert tuple(ops.banding(src, index=[]).shape) == (0, 5, 1024)


def test_wrapper(gpu):
    import torch
    from pixpath import _native, banding, ops
    from pixpath.frames import FrameBatch
    for fmt, depth in (("yuv420p", 8), ("yuv422p10le", 10)):
        w, h, n = 44, 36, 3
        a = _content(depth, n, w, h, seed=21)
        cw, ch = w // 2, (h // 2 if fmt == "yuv420p" else h)
        b = FrameBatch.from_numpy(fmt, [a, np.zeros((n, ch, cw), np.int64), np.zeros((n, ch, cw), np.int64)], device=gpu)
        assert banding.default_window(w, h) == 3
        got = ops.banding(b)
        torch.cuda.synchronize(gpu)
        assert got.dtype == torch.uint32 and tuple(got.shape) == (n, 5, 1024)
        assert np.array_equal(got.cpu().numpy(), _want(a, depth, 3))
        got = ops.banding(b.view(0), index=[2, 0], window=9, tvi=[1023, 1023, 0, 0]).cpu().numpy()
        assert np.array_equal(got, _want(a, depth, 9, [2, 0], [1023, 1023, 0, 0]))
        val, top = banding.pool(got)
        assert val.shape == (2,) and top.shape == (2, 5) and (val >= 0).all() and (val < 1).all()
        with pytest.raises(ValueError):
            ops.banding(b, tvi=[1, 2, 3])
        with pytest.raises(_native.PixpathError):
            ops.banding(b, index=[0, n])
        with pytest.raises(_native.PixpathError):
            ops.banding(b, window=4)


def test_return_codes(gpu):
    from pixpath import _native
    L = _native.lib()
    INVALID, UNSUPPORTED = -1, -4
    a = _content(8, 3, 20, 15)
    src = _make(gpu, 8, a)
    a16 = _content(10, 3, 20, 15)
    s16 = _make(gpu, 10, a16)

    def bad(code, word, depth=8, w=20, h=15, s=src, window=3, **kw):
        L.pp_banding(None, 8, 1, 1, None, 0, 0, 0, None, 0, 3, None, None, None)  # leaves "null argument"
        rc, _, untouched = _call(gpu, depth, w, h, s, window, **kw)
        msg = L.pp_last_error().decode()
        assert rc == code and word in msg, (rc, msg)
        assert untouched  # nothing was launched

    for name in ("ctx", "src", "hist"):
        rc, _, _ = _call(gpu, 8, 20, 15, src, 3, null=(name,))
        assert rc == INVALID and b"null" in L.pp_last_error()
    bad(INVALID, "frame", w=0)
    bad(INVALID, "frame", h=0)
    bad(INVALID, "n -1", n=-1)
    bad(INVALID, "nsrc", nsrc=-1, n=0)
    bad(INVALID, "bitdepth", depth=9)
    bad(INVALID, "bitdepth", depth=16)
    for window in (-3, 0, 1, 2, 4, 32, 64, 65):
        bad(INVALID, "window", window=window)
    bad(INVALID, "src plane 0: linesize", sls=19)
    bad(INVALID, "linesize", depth=10, s=s16, sls=39)
    bad(INVALID, "2-byte grid", depth=10, s=s16, sls=41)
    bad(INVALID, "index[1] = 3", idx=[0, 3])
    bad(INVALID, "index[0] = -1", idx=[-1, 0])
    bad(INVALID, "without index", nsrc=1, n=2)
    bad(UNSUPPORTED, "2 GiB buffer range", h=64, sls=1 << 25)
    rc, got, untouched = _call(gpu, 8, 20, 15, src, 63, idx=[2, 0])  # and the same buffers are fine
    assert rc == 0 and untouched and np.array_equal(got, _want(a, 8, 63, [2, 0]))
