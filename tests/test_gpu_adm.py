"""pp_adm / ops.adm on the GPU (spec PP-ADM-1) against the numpy restatement
(adm_ref.terms, the direct 2-D form): each of the 24 sums of a frame within
|gpu - ref| <= REL |ref| + floor, NaN exactly where a scale does not exist.

The bar.  On the CPU (test_adm_host.py::test_three_evaluations_agree) the
direct fp64 evaluation, a separable fp64 one and the direct one in long double
differ by at most CPU_SPREAD = 2.08e-13 relative over noise, small error,
smooth plus noise, a blurred copy and checkerboards at 8 and 10 bits, and an
fp32 evaluation is off by at least 2.9e-6.  Measured on the MI355X over every
comparison of this file and of test_gpu_adm_files.py (printed per case with
`pytest -s`): the largest relative difference of a GPU sum from the
restatement is MEASURED = 5.41e-12, on the single position of scale 3 of a
35 x 37 plane, whose restored coefficient lies just above its threshold (the
cube of a small excess amplifies the threshold's rounding); every other case
stays below 3.2e-13.  REL = 100 * MEASURED = 5.41e-10 for headroom across
content, 100 times below the 6e-8 of one fp32 rounding, so a float step on the
path cannot pass.
floor_s = area_s (max rf_s * u_s)^3 with u_s = adm_ref.coef_rounding, the bound
on the rounding error of a coefficient: what a sum that is zero in exact
arithmetic may hold.

r and a jump where the angle test flips, so every seeded input of a tolerance
comparison is first checked to have no position within reach of that
(adm_ref.near_branch) on any scale.  Constant and identical planes are compared
on their own terms.  The shapes are the smallest at which the kernel can still
be wrong: the minimum sizes, odd sizes, and per scale one coefficient below,
at and above the seams of the tiling (a wave's first 63 columns, a tile's 254
columns, a band's 32 rows), all with poisoned pitch padding.  Every call writes
into a larger, sentinel-filled output and must change [ndist][4][6] alone."""

import numpy as np
import pytest

import adm_ref as R
from gpu_calls import SENTINEL, call_pair, make as _make

pytestmark = pytest.mark.gpu

CPU_SPREAD = 2.08e-13
MEASURED = 5.41e-12
REL = 100 * MEASURED
assert REL <= 1e-8
_REF = {}
WORST = [0.0]


def _planes(name, depth, w, h, seed=0):
    key = (name, depth, w, h, seed)
    if key not in _REF:
        _REF[key] = R.content(name, depth, w, h, seed)
    return _REF[key]


def _terms(a, b, depth):
    """adm_ref.terms of one pair, made once, after checking that no position can flip the angle test."""
    key = ("terms", depth, a.shape, a.tobytes(), b.tobytes())
    if key not in _REF:
        assert not any(R.near_branch(a, b, depth)), "a position within reach of the angle branch: choose another seed"
        _REF[key] = R.terms(a, b, depth)
    return _REF[key]


def floors(w, h, peak):
    """[4] floor_s for w x h planes of samples <= peak on the 8-bit scale."""
    rf = R.rf()
    return np.array([0.0 if np.isnan(area) else area * (rf[s].max() * R.coef_rounding(s, peak)) ** 3
                     for s, area in enumerate(R.areas(w, h))])


def compare(got, want, w, h, peak, label=""):
    """One frame's [4][6] against the restatement's; returns the worst relative difference of the sums above the floor."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), (label, w, h, got, want)
    fl = floors(w, h, peak)[:, None]
    ok = ~np.isnan(want)
    diff = np.abs(got - want)
    big = ok & (np.abs(want) > 1e6 * fl)
    worst = float((diff[big] / np.abs(want[big])).max()) if big.any() else 0.0
    WORST[0] = max(WORST[0], worst)
    bad = ok & ~(diff <= REL * np.abs(want) + fl)
    assert not bad.any(), (label, w, h, worst, got[bad], want[bad])
    return worst


def _call(gpu, depth, w, h, ref, dist, *args, **kw):
    """pp_adm itself on a sentinel-filled output of two frames more than it
    needs; returns (rc, out [nd, 4, 6] float64, untouched: everything else kept the sentinel)."""
    return call_pair(gpu, "pp_adm", (4, 6), depth, w, h, ref, dist, *args, **kw)


def _check(gpu, depth, a, b, idx=None, rl="std", dl="std", label=""):
    """a [nr, h, w] reference planes, b [nd, h, w] distorted ones: the call's
    sums against adm_ref within the bar; returns them."""
    nd, h, w = b.shape
    want = [_terms(a[k if idx is None else idx[k]], b[k], depth) for k in range(nd)]  # CPU side first
    ref, dist = _make(gpu, depth, a, rl, 1), _make(gpu, depth, b, dl, 2)
    rc, got, untouched = _call(gpu, depth, w, h, ref, dist, idx)
    assert rc == 0 and untouched
    assert not (got.view(np.uint64) == SENTINEL).any()  # every element written
    peak = float(max(a.max(), b.max())) / (1 << (depth - 8))
    worst = max(compare(got[k], want[k], w, h, peak, label) for k in range(nd))
    print("%s %d bit %dx%d ref %s dist %s: worst relative |gpu - numpy| / |numpy| = %.3e (so far %.3e)"
          % (label, depth, w, h, rl, dl, worst, WORST[0]))
    return got


def _pair(depth, w, h, seed=0):
    """Two frame pairs of one size: noise against noise, and a small error."""
    a0, b0 = _planes("noise", depth, w, h, seed)
    a1, b1 = _planes("small_error", depth, w, h, seed + 1)
    return np.stack([a0, a1]), np.stack([b0, b1])


def test_geometry_constants():
    from pixpath import adm
    assert (adm.TILE_COLS, adm.WAVE_COLS, adm.BAND_ROWS) == (254, 64, 32)
    assert adm.FRAMES_PER_LAUNCH == 256 and adm.MIN_SIZE == 33 and adm.SUMS == 6


SPEC_SHAPES = {(33, 33): 4, (32, 32): 3, (35, 37): 4, (64, 48): 4, (3, 3): 0, (2, 2): 0, (5, 5): 1, (33, 17): 3,
               (9, 40): 2}


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("w,h", sorted(SPEC_SHAPES))
def test_sizes_of_the_spec(gpu, depth, w, h):
    """The minimum and the sizes around it, odd sizes (a level halves rounding
    up, and its last coefficient reads two mirrored samples), planes far
    narrower than a tile so that both mirrored borders fall into one."""
    from pixpath import adm
    a, b = _pair(depth, w, h, seed=w + 3 * h)
    got = _check(gpu, depth, a, b, label="spec")
    nsc = len(adm.scale_sizes(w, h))
    assert [s for s in range(4) if not np.isnan(got[0, s]).any()] == list(range(nsc))
    assert nsc == SPEC_SHAPES[(w, h)]


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("content", ["smooth_noise", "blur", "checker"])
def test_other_content(gpu, depth, content):
    """The contents the bar was measured on, besides _pair's two."""
    w, h = 183, 78
    a, b = _planes(content, depth, w, h, 3)
    _check(gpu, depth, a[None], b[None], label=content)


def _seam_shapes(s):
    """(w, h) of planes whose scale s has one coefficient less than, exactly
    and one more than a wave's columns (its first lane is the halo: 63), a
    tile's columns and a band's rows; even and odd inputs of that level."""
    from pixpath import adm
    small = adm.MIN_SIZE
    cols = [adm.WAVE_COLS - 2, adm.WAVE_COLS - 1, adm.WAVE_COLS, adm.TILE_COLS - 1, adm.TILE_COLS, adm.TILE_COLS + 1]
    rows = [adm.BAND_ROWS - 1, adm.BAND_ROWS, adm.BAND_ROWS + 1]

    def up(n, v):  # a size that halves (rounding up) to v in s + 1 steps: even at every level, odd at the first, odd at every one
        return (v << (s + 1)) - (0, 1, 0, (1 << (s + 1)) - 1)[n & 3]
    return [(up(n, v), small) for n, v in enumerate(cols)] + [(small, up(n, v)) for n, v in enumerate(rows)]


@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_sizes_on_the_tiling_seams(gpu, s):
    from pixpath import adm
    for n, (w, h) in enumerate(_seam_shapes(s)):
        assert w <= 4100 and h <= 600
        sizes = adm.scale_sizes(w, h)
        assert len(sizes) == 4
        depth = (8, 10)[n & 1]
        a, b = _pair(depth, w, h, seed=w * h + s)
        _check(gpu, depth, a[:1], b[:1], label="seam %d (%dx%d coefficients)" % ((s,) + sizes[s]))


def test_two_tiles_two_bands_idle_waves(gpu):
    """Scale 0 with two tiles and two bands at once, the second tile's last two
    waves without a column; scale 1 with a partly filled wave."""
    a, b = _pair(8, 2 * (254 + 70), 2 * 37, seed=8)
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
    assert np.abs(got[0, :, 3:] / masked[:, 3:] - 1).min() > 1e-3  # the reference sums: none is zero


@pytest.mark.parametrize("depth", [8, 10])
def test_off_the_16_byte_grid_is_bit_equal(gpu, depth):
    w, h = 71, 37
    a, b = _pair(depth, w, h, seed=6)
    outs = [_check(gpu, depth, a, b, rl=rl, dl=dl, label="grid")
            for rl, dl in (("std", "std"), ("odd", "std"), ("std", "odd"), ("odd", "odd"))]
    for o in outs[1:]:
        assert np.array_equal(o.view(np.uint64), outs[0].view(np.uint64))


def test_ref_index(gpu):
    from pixpath import adm
    w, h = 36, 40
    rng = np.random.default_rng(12)
    a = rng.integers(0, 1024, (3, h, w))
    b = np.clip(a[[2, 2, 1, 0, 0]] + rng.integers(-30, 31, (5, h, w)), 0, 1023)
    idx = [2, 2, 1, 0, 0]  # repeats, going back, nref != ndist
    got = _check(gpu, 10, a, b, idx=idx, label="map")
    assert (adm.pool(got, w, h)[1] > 0.9).all()
    wrong = _check(gpu, 10, a, b[:3], label="identity")  # frame 0 against reference 0: another picture
    assert adm.pool(wrong, w, h)[1][0] < 0.6
    assert np.array_equal(_check(gpu, 10, a, b[:3], idx=[0, 1, 2], label="identity map").view(np.uint64),
                          wrong.view(np.uint64))


def test_more_frames_than_one_launch_carries(gpu):
    from pixpath import adm
    nd, w, h = adm.FRAMES_PER_LAUNCH + 3, 17, 9
    rng = np.random.default_rng(13)
    a = rng.integers(0, 256, (7, h, w))
    idx = [(k * 5) % 7 for k in range(nd)]
    b = np.clip(a[idx] + rng.integers(-9, 10, (nd, h, w)), 0, 255)
    _check(gpu, 8, a, b, idx=idx, label="launches")


def test_runs_are_identical(gpu):
    a, b = _pair(10, 600, 150, seed=3)
    ref, dist = _make(gpu, 10, a), _make(gpu, 10, b)
    x = _call(gpu, 10, 600, 150, ref, dist)[1]
    y = _call(gpu, 10, 600, 150, ref, dist)[1]
    assert not np.isnan(x).any() and np.array_equal(x.view(np.uint64), y.view(np.uint64))


@pytest.mark.parametrize("depth,p,q", [(8, 200, 0), (8, 0, 0), (10, 1023, 0), (10, 65535, 0), (8, 200, 77), (10, 300, 301)])
def test_constant_planes(gpu, depth, p, q):
    """Every H, V, D coefficient is zero in exact arithmetic: each of the 24
    sums is at most the floor, and both pooled sides are 3 c_s to within it."""
    from pixpath import adm
    w, h = 600, 70  # two tiles, two bands at scale 0
    a, b = np.full((1, h, w), p), np.full((1, h, w), q)
    rc, got, untouched = _call(gpu, depth, w, h, _make(gpu, depth, a), _make(gpu, depth, b))
    assert rc == 0 and untouched and not np.isnan(got).any()
    fl = floors(w, h, max(p, q, 1) / (1 << (depth - 8)))
    assert (got >= 0).all() and (got[0] <= fl[:, None]).all(), (got[0], fl)
    scales, adm2 = adm.pool(got, w, h)
    assert np.abs(scales - 1).max() <= 1e-9 and abs(adm2[0] - 1) <= 1e-9


@pytest.mark.parametrize("depth", [8, 10])
def test_identical_planes_are_exactly_one(gpu, depth):
    from pixpath import adm
    w, h = 300, 70
    a = np.stack([_planes("noise", depth, w, h, 3)[0], _planes("smooth_noise", depth, w, h, 4)[0]])
    for rl, dl in (("std", "std"), ("odd", "std")):
        rc, got, untouched = _call(gpu, depth, w, h, _make(gpu, depth, a, rl, 1), _make(gpu, depth, a, dl, 2))
        assert rc == 0 and untouched and not np.isnan(got).any()
        assert np.array_equal(got[:, :, 0:3].view(np.uint64), got[:, :, 3:6].view(np.uint64)) and (got > 0).all()
        scales, adm2 = adm.pool(got, w, h)
        assert (scales == 1.0).all() and (adm2 == 1.0).all()
        for k in range(2):  # the denominators are ordinary sums: against the restatement as any other
            compare(got[k], _terms(a[k], a[k], depth), w, h, float(a.max()) / (1 << (depth - 8)), "identical")


def test_no_distorted_frames_writes_nothing(gpu):
    from pixpath import ops
    a, b = _pair(8, 20, 15)
    ref, dist = _make(gpu, 8, a), _make(gpu, 8, b)
    rc, got, untouched = _call(gpu, 8, 20, 15, ref, dist, nd=0)
    assert rc == 0 and got.shape[0] == 0 and untouched
    assert tuple(ops.adm(ref, dist[:0]).shape) == (0, 4, 6)


def test_wrapper(gpu):
    import torch
    from pixpath import adm, ops
    from pixpath.frames import FrameBatch
    for fmt, depth in (("yuv420p", 8), ("yuv422p10le", 10)):
        w, h = 44, 36
        a, b = _pair(depth, w, h, seed=21)
        cw = w // 2
        ch = h // 2 if fmt == "yuv420p" else h
        mk = lambda y: FrameBatch.from_numpy(fmt, [y, np.zeros((2, ch, cw), np.int64), np.zeros((2, ch, cw), np.int64)],
                                             device=gpu)
        ref, dist = mk(a), mk(b)
        got = ops.adm(ref, dist)
        torch.cuda.synchronize(gpu)
        assert got.dtype == torch.float64 and tuple(got.shape) == (2, 4, 6)
        got = got.cpu().numpy()
        peak = float(max(a.max(), b.max())) / (1 << (depth - 8))
        for k in range(2):
            compare(got[k], _terms(a[k], b[k], depth), w, h, peak, "wrapper")
        assert np.abs(adm.pool(got, w, h)[1] - [R.pool(_terms(a[k], b[k], depth), w, h)[1] for k in range(2)]).max() < 1e-9
        swapped = ops.adm(ref.view(0), dist.view(0), ref_index=[1, 0]).cpu().numpy()
        compare(swapped[0], _terms(a[1], b[0], depth), w, h, peak, "swapped")
    with pytest.raises(ValueError):
        ops.adm(ref, dist, ref_index=[0])
    with pytest.raises(ValueError):
        ops.adm(ref.view(0), dist.view(0)[:, :-1])


def test_return_codes(gpu):
    from pixpath import _native
    L = _native.lib()
    INVALID, UNSUPPORTED = -1, -4
    a, b = _pair(8, 20, 15)
    ref, dist = _make(gpu, 8, np.concatenate([a, a[:1]])), _make(gpu, 8, b)
    a16, b16 = _pair(10, 20, 15)
    r16, d16 = _make(gpu, 10, a16), _make(gpu, 10, b16)

    def bad(code, word, depth=8, w=20, h=15, r=ref, d=dist, **kw):
        L.pp_adm(None, 8, 1, 1, None, 0, 0, 0, None, 0, 0, 0, None, None, None)  # leaves "null argument"
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
