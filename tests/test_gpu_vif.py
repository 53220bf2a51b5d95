"""pp_vif / ops.vif on the GPU (spec PP-VIF-1) against the numpy restatement
(vif_ref.terms, the direct 2-D form): every num_s and den_s within BAR
relative, NaN exactly where a scale does not exist.

The bar.  Measured on the MI355X over every comparison of this file and of
test_gpu_vif_files.py (printed per case with `pytest -s`): the largest relative
difference of a GPU sum from the restatement is MEASURED = 2.02e-11, on the
stored 16-bit samples past 1023 (moments of 6e7 on the 8-bit scale); every
other case stays below 1.8e-12.  BAR = 100 * MEASURED = 2.02e-9 for headroom
across content, far below the 1e-7 cap: one fp32 rounding is 6e-8, so a float
step on the path cannot pass.

num jumps where a position sits on one of the spec's branches, so every seeded
input of a tolerance comparison is first checked to have no such position
(vif_ref.near_branch) on any scale.  Constant and identical planes are compared
on their own terms.  The shapes are the smallest at which the kernels can still
be wrong: the minimum sizes, odd sizes, and per scale the seams of the tiling (a
wave's 64 and a tile's 256 columns, a band's 64 rows; the decimation's 256
output columns and 32 output rows) one position before the mirrored border
region, inside it and one past it, all with poisoned pitch padding.  Every call
writes into a larger, sentinel-filled output and must change [ndist][4][2]
alone."""

import numpy as np
import pytest

import vif_ref as R
from gpu_calls import SENTINEL, call_pair, make as _make

pytestmark = pytest.mark.gpu

MEASURED = 2.02e-11
BAR = 100 * MEASURED
assert BAR <= 1e-7
_REF = {}


def _planes(name, depth, w, h, seed=0):
    key = (name, depth, w, h, seed)
    if key not in _REF:
        _REF[key] = R.content(name, depth, w, h, seed)
    return _REF[key]


def _terms(a, b, depth):
    """vif_ref.terms of one pair, made once, after checking that no position sits on a branch."""
    key = ("terms", depth, a.shape, a.tobytes(), b.tobytes())
    if key not in _REF:
        assert not any(R.near_branch(a, b, depth)), "a position on a branch: choose another seed"
        _REF[key] = R.terms(a, b, depth)
    return _REF[key]


def _call(gpu, depth, w, h, ref, dist, *args, **kw):
    """pp_vif itself on a sentinel-filled output of two frames more than it
    needs; returns (rc, out [nd, 4, 2] float64, untouched: everything else kept the sentinel)."""
    return call_pair(gpu, "pp_vif", (4, 2), depth, w, h, ref, dist, *args, **kw)


def _check(gpu, depth, a, b, idx=None, rl="std", dl="std", label=""):
    """a [nr, h, w] reference planes, b [nd, h, w] distorted ones: the call's
    sums against vif_ref within BAR relative; returns them."""
    nd, h, w = b.shape
    want = [_terms(a[k if idx is None else idx[k]], b[k], depth) for k in range(nd)]  # CPU side first
    ref, dist = _make(gpu, depth, a, rl, 1), _make(gpu, depth, b, dl, 2)
    rc, got, untouched = _call(gpu, depth, w, h, ref, dist, idx)
    assert rc == 0 and untouched
    assert not (got.view(np.uint64) == SENTINEL).any()  # every element written
    worst = 0.0
    for k in range(nd):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (label, w, h, k, got[k], want[k])
        zero = want[k] == 0  # every position of the scale on the num = 0 side: the same on the GPU
        assert np.array_equal(got[k][zero], want[k][zero])
        ok = ~np.isnan(want[k]) & ~zero
        if ok.any():
            worst = max(worst, np.abs(got[k][ok] / want[k][ok] - 1).max())
    print("%s %d bit %dx%d ref %s dist %s: worst relative |gpu / numpy - 1| = %.3e" % (label, depth, w, h, rl, dl, worst))
    assert worst <= BAR
    return got


def _pair(depth, w, h, seed=0):
    """Two frame pairs of one size: noise against noise, and a small error."""
    a0, b0 = _planes("noise", depth, w, h, seed)
    a1, b1 = _planes("small_error", depth, w, h, seed + 1)
    return np.stack([a0, a1]), np.stack([b0, b1])


def test_geometry_constants():
    from pixpath import vif
    assert (vif.TILE_COLS, vif.WAVE_COLS, vif.BAND_ROWS, vif.DEC_BAND_ROWS) == (256, 64, 64, 32)
    assert vif.FRAMES_PER_LAUNCH == 256 and vif.MIN_SIZE == 16 and vif.TAPS == (17, 9, 5, 3)


SPEC_SHAPES = [(16, 16), (15, 16), (16, 15), (37, 29), (9, 9), (8, 9), (9, 8), (12, 40), (73, 21)]


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", SPEC_SHAPES)
def test_sizes_of_the_spec(gpu, depth, w, h):
    """The minimum and the sizes around it, odd sizes (floor decimation drops
    the last row and column at several levels), planes narrower than a tile so
    that both mirrored borders fall into one."""
    from pixpath import vif
    a, b = _pair(depth, w, h, seed=w + 3 * h)
    got = _check(gpu, depth, a, b, label="spec")
    nsc = len(vif.scale_sizes(w, h))
    assert [s for s in range(4) if not np.isnan(got[0, s]).any()] == list(range(nsc))
    assert nsc == {(16, 16): 4, (15, 16): 3, (16, 15): 3, (37, 29): 4, (9, 9): 1, (8, 9): 0, (9, 8): 0, (12, 40): 3,
                   (73, 21): 4}[(w, h)]


def _seam_shapes(s):
    """(w, h) of planes whose scale s has a seam of the tiling one position
    before the mirrored border region (the last N_s // 2 columns / rows), on its
    first position, and on the plane's last position (one more and the seam is
    past the plane)."""
    from pixpath import vif
    r = vif.TAPS[s] // 2
    small = vif.MIN_SIZE
    ws = [vif.WAVE_COLS + r + 1, vif.WAVE_COLS + r, vif.WAVE_COLS + 1, vif.WAVE_COLS,
          vif.TILE_COLS + r + 1, vif.TILE_COLS + r, vif.TILE_COLS + 1]
    hs = [vif.BAND_ROWS + r + 1, vif.BAND_ROWS + r, vif.BAND_ROWS + 1, vif.DEC_BAND_ROWS + 1]
    return [((v << s) + (1 if s else 0), small) for v in ws] + [(small, (v << s) + (1 if s else 0)) for v in hs]


@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_sizes_on_the_tiling_seams(gpu, s):
    for n, (w, h) in enumerate(_seam_shapes(s)):
        assert w <= 2100 and h <= 600
        depth = (8, 10)[n & 1]
        a, b = _pair(depth, w, h, seed=w * h + s)
        _check(gpu, depth, a[:1], b[:1], label="seam %d" % s)


def test_two_tiles_two_bands_two_waves(gpu):
    """Scale 0 and scale 1 with more than one tile, band and wave at once; every decimation tile seam inside."""
    a, b = _pair(8, 531, 135, seed=8)
    _check(gpu, 8, a, b, label="tiles")


def test_stored_16_bit_samples_are_taken_as_they_are(gpu):
    """bitdepth 10 with samples over the whole uint16 range, 0xFFFF among them: nothing is masked."""
    w, h = 45, 38
    a0, b0 = (x.copy() for x in _planes("noise", 16, w, h, 4))
    a1, b1 = (x.copy() for x in _planes("small_error", 16, w, h, 5))
    a0[0, :20] = 0xFFFF
    b1[-1, -20:] = 0xFFFF
    got = _check(gpu, 10, np.stack([a0, a1]), np.stack([b0, b1]), label="0xFFFF")
    masked = R.terms(a0 & 1023, b0 & 1023, 10)
    assert np.abs(got[0] / masked - 1).max() > 1e-3


@pytest.mark.parametrize("depth", [8, 10])
def test_off_the_16_byte_grid_is_bit_equal(gpu, depth):
    w, h = 71, 37
    a, b = _pair(depth, w, h, seed=6)
    outs = [_check(gpu, depth, a, b, rl=rl, dl=dl, label="grid")
            for rl, dl in (("std", "std"), ("odd", "std"), ("std", "odd"), ("odd", "odd"))]
    for o in outs[1:]:
        assert np.array_equal(o.view(np.uint64), outs[0].view(np.uint64))


def test_ref_index(gpu):
    from pixpath import vif
    w, h = 36, 24
    rng = np.random.default_rng(12)
    a = rng.integers(0, 1024, (3, h, w))
    b = np.clip(a[[2, 2, 1, 0, 0]] + rng.integers(-30, 31, (5, h, w)), 0, 1023)
    idx = [2, 2, 1, 0, 0]  # repeats, going back, nref != ndist
    got = _check(gpu, 10, a, b, idx=idx, label="map")
    assert (vif.pool(got)[1] > 0.6).all()
    wrong = _check(gpu, 10, a, b[:3], label="identity")  # frame 0 against reference 0: another picture
    assert vif.pool(wrong)[1][0] < 0.1
    assert np.array_equal(_check(gpu, 10, a, b[:3], idx=[0, 1, 2], label="identity map").view(np.uint64),
                          wrong.view(np.uint64))


def test_more_frames_than_one_launch_carries(gpu):
    from pixpath import vif
    nd, w, h = vif.FRAMES_PER_LAUNCH + 3, 16, 16
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
    assert not np.isnan(x).any() and np.array_equal(x.view(np.uint64), y.view(np.uint64))


@pytest.mark.parametrize("depth,p,q", [(8, 200, 0), (8, 0, 0), (10, 1023, 0), (10, 65535, 0), (8, 200, 77), (10, 300, 301)])
def test_constant_planes(gpu, depth, p, q):
    """sigma1^2 < 2 everywhere: den is the position count exactly, and so is
    num against a zero plane (sigma2^2 = 0 exactly); a non-zero constant leaves
    the rounding of E[y^2] - mu2^2 in num, within 4e-14 relative (test_vif_host)."""
    from pixpath import vif
    w, h = 300, 70  # two tiles, two bands
    a, b = np.full((1, h, w), p), np.full((1, h, w), q)
    rc, got, untouched = _call(gpu, depth, w, h, _make(gpu, depth, a), _make(gpu, depth, b))
    assert rc == 0 and untouched
    count = np.array([ws * hs for ws, hs in vif.scale_sizes(w, h)], dtype=np.float64)
    assert np.array_equal(got[0, :, 1], count)
    if q == 0:
        assert np.array_equal(got[0, :, 0], count)
    assert np.abs(got[0, :, 0] / count - 1).max() <= 4e-14


def _blocky(depth, w, h, seed):
    """Noise held over 8 x 8 blocks: sigma1^2 stays far above 2 on every scale (test_vif_host)."""
    rng = np.random.default_rng(seed)
    top = (1 << depth) - 1
    return np.kron(rng.integers(0, top + 1, (h // 8 + 1, w // 8 + 1)), np.ones((8, 8), np.int64))[:h, :w]


@pytest.mark.parametrize("depth", [8, 10])
def test_identical_planes_are_within_1e_9_of_one(gpu, depth):
    from pixpath import vif
    w, h = 72, 56
    a = np.stack([_blocky(depth, w, h, 3), _blocky(depth, w, h, 4)])
    for s, p in enumerate(R.levels(a[0], depth)):
        assert R.moments(p, p, s)[0].min() > 2.0
    for rl, dl in (("std", "std"), ("odd", "std")):
        rc, got, untouched = _call(gpu, depth, w, h, _make(gpu, depth, a, rl, 1), _make(gpu, depth, a, dl, 2))
        assert rc == 0 and untouched and not np.isnan(got).any()
        scales, v = vif.pool(got)
        assert np.abs(scales - 1).max() < 1e-9 and np.abs(v - 1).max() < 1e-9
        assert np.abs(got[0] / R.terms(a[0], a[0], depth) - 1).max() <= BAR


def test_no_distorted_frames_writes_nothing(gpu):
    from pixpath import ops
    a, b = _pair(8, 20, 15)
    ref, dist = _make(gpu, 8, a), _make(gpu, 8, b)
    rc, got, untouched = _call(gpu, 8, 20, 15, ref, dist, nd=0)
    assert rc == 0 and got.shape[0] == 0 and untouched
    assert tuple(ops.vif(ref, dist[:0]).shape) == (0, 4, 2)


def test_wrapper(gpu):
    import torch
    from pixpath import ops, vif
    from pixpath.frames import FrameBatch
    for fmt, depth in (("yuv420p", 8), ("yuv422p10le", 10)):
        w, h = 44, 36
        a, b = _pair(depth, w, h, seed=21)
        cw = w // 2
        ch = h // 2 if fmt == "yuv420p" else h
        mk = lambda y: FrameBatch.from_numpy(fmt, [y, np.zeros((2, ch, cw), np.int64), np.zeros((2, ch, cw), np.int64)],
                                             device=gpu)
        ref, dist = mk(a), mk(b)
        got = ops.vif(ref, dist)
        torch.cuda.synchronize(gpu)
        assert got.dtype == torch.float64 and tuple(got.shape) == (2, 4, 2)
        got = got.cpu().numpy()
        want = np.stack([_terms(a[k], b[k], depth) for k in range(2)])
        assert np.abs(got / want - 1).max() <= BAR
        assert np.abs(vif.pool(got)[1] - [R.pool(t)[1] for t in want]).max() < 1e-7
        swapped = ops.vif(ref.view(0), dist.view(0), ref_index=[1, 0]).cpu().numpy()
        assert np.abs(swapped[0] / _terms(a[1], b[0], depth) - 1).max() <= BAR
    with pytest.raises(ValueError):
        ops.vif(ref, dist, ref_index=[0])
    with pytest.raises(ValueError):
        ops.vif(ref.view(0), dist.view(0)[:, :-1])


def test_return_codes(gpu):
    from pixpath import _native
    L = _native.lib()
    INVALID, UNSUPPORTED = -1, -4
    a, b = _pair(8, 20, 15)
    ref, dist = _make(gpu, 8, np.concatenate([a, a[:1]])), _make(gpu, 8, b)
    a16, b16 = _pair(10, 20, 15)
    r16, d16 = _make(gpu, 10, a16), _make(gpu, 10, b16)

    def bad(code, word, depth=8, w=20, h=15, r=ref, d=dist, **kw):
        L.pp_vif(None, 8, 1, 1, None, 0, 0, 0, None, 0, 0, 0, None, None, None)  # leaves "null argument"
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
    assert rc == 0 and untouched and not np.isnan(got[:, :2]).any()
