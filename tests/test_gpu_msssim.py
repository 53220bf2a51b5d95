"""pp_ms_ssim / ops.ms_ssim on the GPU (spec PP-MSSSIM-1) against the numpy
restatement (msssim_ref.terms, the direct 2-D form): every cs_s and ssim_s
within 1e-9 absolute, NaN exactly where a scale has no window.  The shapes are
the smallest at which the kernel can still be wrong: the sizes around the first
scale-4 window, one window and none, and the seams of the kernel's tiling (a
wave's 64 and a tile's 256 window columns, a band's 64 window rows, the row
loop's unroll by 11), all with poisoned pitch padding.  Every call writes into
a larger, sentinel-filled output and must change [ndist][5][2] alone."""

import numpy as np
import pytest

import msssim_ref as R
from gpu_calls import SENTINEL, call_pair, make as _make

pytestmark = pytest.mark.gpu

BAR = 1e-9
_REF = {}


def _planes(name, depth, w, h, seed=0):
    """Content planes (a, b) of msssim_ref.content, made once."""
    key = (name, depth, w, h, seed)
    if key not in _REF:
        _REF[key] = R.content(name, depth, w, h, seed)
    return _REF[key]


def _terms(a, b, depth):
    key = ("terms", depth, a.shape, a.tobytes(), b.tobytes())
    if key not in _REF:
        _REF[key] = R.terms(a, b, depth)
    return _REF[key]


def _call(gpu, depth, w, h, ref, dist, *args, **kw):
    """pp_ms_ssim itself on a sentinel-filled output of two frames more than it
    needs; returns (rc, out [nd, 5, 2] float64, untouched: everything else kept the sentinel)."""
    return call_pair(gpu, "pp_ms_ssim", (5, 2), depth, w, h, ref, dist, *args, **kw)


def _check(gpu, depth, a, b, idx=None, rl="std", dl="std", label=""):
    """a [nr, h, w] reference planes, b [nd, h, w] distorted ones: the call's
    values against msssim_ref within BAR; returns them."""
    nd, h, w = b.shape
    ref, dist = _make(gpu, depth, a, rl, 1), _make(gpu, depth, b, dl, 2)
    rc, got, untouched = _call(gpu, depth, w, h, ref, dist, idx)
    assert rc == 0 and untouched
    assert not (got.view(np.uint64) == SENTINEL).any()  # every element written
    worst = 0.0
    for k in range(nd):
        want = _terms(a[k if idx is None else idx[k]], b[k], depth)
        assert np.array_equal(np.isnan(got[k]), np.isnan(want)), (label, w, h, k, got[k], want)
        if not np.isnan(want).all():
            worst = max(worst, np.nanmax(np.abs(got[k] - want)))
    print("%s %d bit %dx%d ref %s dist %s: worst |gpu - numpy| = %.3e" % (label, depth, w, h, rl, dl, worst))
    assert worst <= BAR
    return got


def _pair(depth, w, h, seed=0):
    """Two frame pairs of one size: noise against noise, and a small error."""
    a0, b0 = _planes("noise", depth, w, h, seed)
    a1, b1 = _planes("small_error", depth, w, h, seed + 1)
    return np.stack([a0, a1]), np.stack([b0, b1])


def test_geometry_constants():
    from pixpath import msssim
    assert (msssim.TILE_COLS, msssim.WAVE_COLS, msssim.BAND_ROWS, msssim.WINDOW) == (256, 64, 64, 11)
    assert msssim.FRAMES_PER_LAUNCH == 256 and msssim.MIN_SIZE == 176


SPEC_SHAPES = [(176, 176), (177, 179), (191, 176), (11, 11), (10, 10), (175, 176)]


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", SPEC_SHAPES)
def test_sizes_of_the_spec(gpu, depth, w, h):
    a, b = _pair(depth, w, h, seed=w + h)
    got = _check(gpu, depth, a, b, label="spec")
    valid = [s for s in range(5) if (w >> s) >= 11 and (h >> s) >= 11]
    assert [s for s in range(5) if not np.isnan(got[0, s]).any()] == valid
    assert len(valid) == {(176, 176): 5, (177, 179): 5, (191, 176): 5, (11, 11): 1, (10, 10): 0, (175, 176): 4}[(w, h)]


def _seam_shapes():
    from pixpath import msssim
    halo = msssim.WINDOW - 1
    wave, tile, band = msssim.WAVE_COLS + halo, msssim.TILE_COLS + halo, msssim.BAND_ROWS + halo
    return [(wave, 12),          # a wave's last window column; 12 input rows: one past the row loop's unroll
            (wave + 1, 21),      # the first column of the second wave; one row short of two unrolled rounds
            (tile, band),        # exactly one tile: its last column and its last row
            (tile + 1, band + 1),  # a second tile across and a second band, one window each
            (330, 2 * band - halo + 1),  # a partial tile right of a full one; two full bands and one row
            (399, 33)]           # windows in two waves of the second tile


@pytest.mark.parametrize("depth", [8, 10])
def test_sizes_on_the_tiling_seams(gpu, depth):
    for w, h in _seam_shapes():
        assert w <= 400 and h <= 300
        a, b = _pair(depth, w, h, seed=w * h)
        _check(gpu, depth, a, b, label="seam")


@pytest.mark.parametrize("depth", [8, 10])
def test_contents(gpu, depth):
    w, h = 183, 178
    pairs = [_planes(name, depth, w, h, seed=1) for name in R.CONTENTS]
    a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    got = _check(gpu, depth, a, b, label="contents")
    names = list(R.CONTENTS)
    assert got[names.index("checker1"), 0, 0] < -0.9 and (got[names.index("checker16"), :, 0] < -0.5).all()
    assert np.abs(got[names.index("full_vs_zero"), :, 0] - 1).max() < 1e-9  # constants: cs = 1
    c1, _ = R.constants(depth)
    assert np.abs(got[names.index("full_vs_zero"), :, 1] - c1 / (((1 << depth) - 1) ** 2 + c1)).max() < 1e-9


def test_stored_16_bit_samples_are_taken_as_they_are(gpu):
    """bitdepth 10 with samples over the whole uint16 range, 0xFFFF among them: nothing is masked."""
    w, h = 177, 179
    a0, b0 = (x.copy() for x in _planes("noise", 16, w, h, 4))
    a1, b1 = (x.copy() for x in _planes("small_error", 16, w, h, 5))
    a0[0, :40] = 0xFFFF
    b1[-1, -40:] = 0xFFFF
    got = _check(gpu, 10, np.stack([a0, a1]), np.stack([b0, b1]), label="0xFFFF")
    masked = _terms(a0 & 1023, b0 & 1023, 10)
    assert np.abs(got[0] - masked).max() > 1e-3


@pytest.mark.parametrize("depth", [8, 10])
def test_identical_planes_give_exactly_one(gpu, depth):
    for w, h in ((183, 178), (267, 75)):
        a = np.stack([_planes("noise", depth, w, h, 9)[0], _planes("smooth_noise", depth, w, h, 9)[0],
                      _planes("checker16", depth, w, h)[0]])
        for rl, dl in (("std", "std"), ("odd", "std")):
            ref, dist = _make(gpu, depth, a, rl, 1), _make(gpu, depth, a, dl, 2)
            rc, got, untouched = _call(gpu, depth, w, h, ref, dist)
            assert rc == 0 and untouched
            ok = ~np.isnan(got)
            assert ok[:, :3].all() and (got[ok] == 1.0).all()


@pytest.mark.parametrize("depth", [8, 10])
def test_off_the_16_byte_grid_is_bit_equal(gpu, depth):
    w, h = 201, 77
    a, b = _pair(depth, w, h, seed=6)
    outs = [_check(gpu, depth, a, b, rl=rl, dl=dl, label="grid")
            for rl, dl in (("std", "std"), ("odd", "std"), ("std", "odd"), ("odd", "odd"))]
    for o in outs[1:]:
        assert np.array_equal(o.view(np.uint64), outs[0].view(np.uint64))


def test_ref_index(gpu):
    w, h = 60, 40
    rng = np.random.default_rng(12)
    a = rng.integers(0, 1024, (3, h, w))
    b = np.clip(a[[2, 2, 1, 0, 0]] + rng.integers(-30, 31, (5, h, w)), 0, 1023)
    idx = [2, 2, 1, 0, 0]  # repeats, going back, nref != ndist
    got = _check(gpu, 10, a, b, idx=idx, label="map")
    assert (got[:, 0, 1] > 0.9).all()
    wrong = _check(gpu, 10, a, b[:3], label="identity")  # frame 0 against reference 0: another picture
    assert wrong[0, 0, 1] < 0.5
    assert np.array_equal(_check(gpu, 10, a, b[:3], idx=[0, 1, 2], label="identity map").view(np.uint64),
                          wrong.view(np.uint64))


def test_more_frames_than_one_launch_carries(gpu):
    from pixpath import msssim
    nd, w, h = msssim.FRAMES_PER_LAUNCH + 3, 13, 12
    rng = np.random.default_rng(13)
    a = rng.integers(0, 256, (7, h, w))
    idx = [(k * 5) % 7 for k in range(nd)]
    b = np.clip(a[idx] + rng.integers(-9, 10, (nd, h, w)), 0, 255)
    _check(gpu, 8, a, b, idx=idx, label="launches")


def test_runs_are_identical(gpu):
    a, b = _pair(10, 300, 150, seed=3)
    ref, dist = _make(gpu, 10, a), _make(gpu, 10, b)
    x = _call(gpu, 10, 300, 150, ref, dist)[1]
    y = _call(gpu, 10, 300, 150, ref, dist)[1]
    assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


def test_no_distorted_frames_writes_nothing(gpu):
    from pixpath import ops
    a, b = _pair(8, 20, 15)
    ref, dist = _make(gpu, 8, a), _make(gpu, 8, b)
    rc, got, untouched = _call(gpu, 8, 20, 15, ref, dist, nd=0)
    assert rc == 0 and got.shape[0] == 0 and untouched
    assert tuple(ops.ms_ssim(ref, dist[:0]).shape) == (0, 5, 2)


def test_wrapper(gpu):
    import torch
    from pixpath import msssim, ops
    from pixpath.frames import FrameBatch
    for fmt, depth in (("yuv420p", 8), ("yuv422p10le", 10)):
        w, h = 180, 176
        a, b = _pair(depth, w, h, seed=21)
        cw = w // 2
        ch = h // 2 if fmt == "yuv420p" else h
        mk = lambda y: FrameBatch.from_numpy(fmt, [y, np.zeros((2, ch, cw), np.int64), np.zeros((2, ch, cw), np.int64)],
                                             device=gpu)
        ref, dist = mk(a), mk(b)
        got = ops.ms_ssim(ref, dist)
        torch.cuda.synchronize(gpu)
        assert got.dtype == torch.float64 and tuple(got.shape) == (2, 5, 2)
        got = got.cpu().numpy()
        want = np.stack([_terms(a[k], b[k], depth) for k in range(2)])
        assert np.abs(got - want).max() <= BAR
        assert np.abs(msssim.pool(got) - [R.pool(t) for t in want]).max() < 1e-7
        swapped = ops.ms_ssim(ref.view(0), dist.view(0), ref_index=[1, 0]).cpu().numpy()
        assert np.abs(swapped[0] - _terms(a[1], b[0], depth)).max() <= BAR
    with pytest.raises(ValueError):
        ops.ms_ssim(ref, dist, ref_index=[0])
    with pytest.raises(ValueError):
        ops.ms_ssim(ref.view(0), dist.view(0)[:, :-1])


def test_return_codes(gpu):
    from pixpath import _native
    L = _native.lib()
    INVALID, UNSUPPORTED = -1, -4
    a, b = _pair(8, 20, 15)
    ref, dist = _make(gpu, 8, np.concatenate([a, a[:1]])), _make(gpu, 8, b)
    a16, b16 = _pair(10, 20, 15)
    r16, d16 = _make(gpu, 10, a16), _make(gpu, 10, b16)

    def bad(code, word, depth=8, w=20, h=15, r=ref, d=dist, **kw):
        L.pp_ms_ssim(None, 8, 1, 1, None, 0, 0, 0, None, 0, 0, 0, None, None, None)  # leaves "null argument"
        rc, _, untouched = _call(gpu, depth, w, h, r, d, **kw)
        msg = L.pp_last_error().decode()
        assert rc == code and word in msg, (rc, msg)
        assert untouched  # nothing was launched

    for name in ("ctx", "ref", "dist", "out"):
        rc, _, _ = _call(gpu, 8, 20, 15, ref, dist, null=(name,))
        assert rc == INVALID and b"null" in L.pp_last_error()
    bad(INVALID, "frame", w=0)
    bad(INVALID, "frame", h=0)
    bad(INVALID, "ndist", nd=-1)
    bad(INVALID, "nref", nr=-1)
    bad(INVALID, "bitdepth", depth=9)
    bad(INVALID, "bitdepth", depth=16)
    bad(INVALID, "ref plane 0: linesize", rls=19)
    bad(INVALID, "dist plane 0: linesize", dls=19)
    bad(INVALID, "linesize", depth=10, r=r16, d=d16, dls=39)
    bad(INVALID, "2-byte grid", depth=10, r=r16, d=d16, rls=41)
    bad(INVALID, "ref_index[1] = 3", idx=[0, 3])
    bad(INVALID, "ref_index[0] = -1", idx=[-1, 0])
    bad(INVALID, "without ref_index", nr=1)
    bad(UNSUPPORTED, "2 GiB buffer range", h=64, dls=1 << 25)
    bad(UNSUPPORTED, "2 GiB buffer range", h=64, rls=1 << 25)
    rc, got, untouched = _call(gpu, 8, 20, 15, ref, dist, idx=[2, 0])  # and the same buffers are fine
    assert rc == 0 and untouched and not np.isnan(got[:, 0]).any()
