"""HIP CIEDE2000 sums (pp_ciede, spec PP-CIEDE-1) vs the numpy restatement
(tests/ciede_ref.py).

Tolerance: every frame's sum and every frame's maximum within RTOL = 1e-9
relative of the restatement, the bound test_gpu_metrics.py (ATOL) and the fp64
metrics use.  The restatement in float64 and in 80-bit long double differ by at
most 2e-15 relative in a frame sum and 1e-10 absolute in one sample, so the
bound leaves six orders of magnitude for the device's maths library; a sum of
N <= 10^5 non-negative terms in another order adds at most N 2^-53 ~ 1e-11
relative.  Where the restatement gives exactly 0 the kernel must too.

The dE00 formula has branch boundaries at |h'_1 - h'_2| = 180 degrees and at a
hue sum of 360 degrees, where two correct implementations may take different
arms.  Every seeded input here keeps all of its samples more than MARGIN =
1e-6 degrees away from them (asserted by _check: a condition on the inputs,
checked on the CPU when the seeds were picked, not a tolerance on the kernel)."""
import numpy as np
import pytest

import ciede_ref
from pixpath import ciede as pc, formats

pytestmark = pytest.mark.gpu
RTOL = 1e-9
MARGIN = 1e-6
FORMATS = ["yuv420p", "yuv422p", "yuv444p", "yuv420p10le", "yuv422p10le", "yuv444p10le"]


def _dtype(fmt):
    return np.uint16 if formats.fmt(fmt).depth > 8 else np.uint8


def _noise(fmt, w, h, n, seed):
    """n frames of uniform noise over the whole sample range: a list of [n, rows, cols]."""
    rng = np.random.default_rng(seed)
    f = formats.fmt(fmt)
    return [rng.integers(0, 1 << f.depth, (n, r, c)).astype(_dtype(fmt)) for r, c in formats.plane_shapes(f, w, h)]


def _nudge(fmt, planes, seed, amp=2):
    """The planes +- amp code values, clipped to the sample range."""
    rng = np.random.default_rng(seed)
    mx = (1 << formats.fmt(fmt).depth) - 1
    return [np.clip(p.astype(np.int64) + rng.integers(-amp, amp + 1, p.shape), 0, mx).astype(p.dtype) for p in planes]


def _const(fmt, w, h, y, u, v, n=1):
    return [np.full((n, r, c), val, _dtype(fmt)) for (r, c), val in zip(formats.plane_shapes(fmt, w, h), (y, u, v))]


def _padded(fmt, planes, gpu, extra_bytes, shift):
    """A FrameBatch whose planes are views into wider tensors filled with junk.
    shift = 0: a pitch of the 16-B-rounded row plus `extra_bytes` (a multiple
    of 16: still on the 16-B grid); shift = 1: rows starting one sample in,
    pitch one sample more than the row (off the grid)."""
    import torch
    from pixpath.frames import FrameBatch
    views = []
    for i, p in enumerate(planes):
        n, r, c = p.shape
        es = p.dtype.itemsize
        pitch = c + 1 if shift else ((c * es + 15) // 16 * 16 + extra_bytes) // es
        junk = np.random.default_rng(77 + i).integers(0, 256, (n, r + 1, pitch)).astype(p.dtype)  # differs per plane and clip
        big = torch.from_numpy(junk).to(gpu)
        big[:, :r, shift:shift + c].copy_(torch.from_numpy(np.ascontiguousarray(p)).to(gpu))
        views.append(big[:, :r, shift:])
    h, w = planes[0].shape[1:]
    return FrameBatch(fmt, w, h, planes[0].shape[0], planes=views)


def _interleaved(fmt, planes, gpu):
    import torch
    from pixpath.frames import FrameBatch
    n, h, w = planes[0].shape
    ib = FrameBatch.interleaved(fmt, w, h, n, device=gpu)
    for p in range(3):
        ib.planes[p].copy_(torch.from_numpy(np.ascontiguousarray(planes[p])).to(gpu))
    return ib


def _batch(fmt, planes, gpu, layout):
    from pixpath.frames import FrameBatch
    if layout is None:
        return FrameBatch.from_numpy(fmt, planes, device=gpu)
    if layout == "interleaved":
        return _interleaved(fmt, planes, gpu)
    return _padded(fmt, planes, gpu, *layout)


def _gpu(fmt, ref, dist, gpu, ref_index=None, weights=(1, 1, 1), layouts=(None, None)):
    import torch
    from pixpath import ops
    rb, db = _batch(fmt, ref, gpu, layouts[0]), _batch(fmt, dist, gpu, layouts[1])
    out = ops.ciede(rb, db, fmt, ref_index=ref_index, weights=weights)
    torch.cuda.synchronize()
    assert out.dtype == torch.float64 and tuple(out.shape) == (db.n, 2)
    return out.cpu().numpy()


def _check(fmt, ref, dist, gpu, ref_index=None, weights=(1, 1, 1), layouts=(None, None)):
    f = formats.fmt(fmt)
    want, far = ciede_ref.ciede(ref, dist, f.depth, f.hsub, f.vsub, ref_index, weights)
    assert far > MARGIN, "a sample sits %.3g degrees from a branch boundary: pick another seed" % far
    got = _gpu(fmt, ref, dist, gpu, ref_index, weights, layouts)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(want > 0, np.abs(got - want) / np.where(want > 0, want, 1.0), np.where(got == want, 0.0, np.inf))
    print("%s %dx%d x%d: margin %.3g deg, rel err sum %.3g max %.3g (frame 0: sum %.17g max %.17g)" % (
        fmt, dist[0].shape[2], dist[0].shape[1], dist[0].shape[0], far, rel[:, 0].max(), rel[:, 1].max(), got[0, 0], got[0, 1]))
    assert np.isfinite(got).all() and (got >= 0).all()
    np.testing.assert_array_equal(got[want == 0], 0.0)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)
    return got


# ---------------------------------------------------------------- identical, formats
@pytest.mark.parametrize("fmt", ["yuv420p", "yuv422p10le"])
def test_identical_clips_are_exactly_zero(gpu, fmt):
    ref = _noise(fmt, 333, 97, 2, 1)
    got = _gpu(fmt, ref, [p.copy() for p in ref], gpu)
    assert (got == 0.0).all() and not np.signbit(got).any()
    d, mx, score = pc.pool(got, 333, 97)
    assert (d == 0).all() and (mx == 0).all() and (score == 100.0).all()


@pytest.mark.parametrize("w,h", [(70, 37), (333, 97)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_off_every_grid(gpu, fmt, w, h):
    ref = _noise(fmt, w, h, 3, 10 + w)
    _check(fmt, ref, _noise(fmt, w, h, 3, 20 + w), gpu)   # noise against noise
    got = _check(fmt, ref, _nudge(fmt, ref, 30 + w), gpu)  # a clip against itself +- 2 code values
    assert (got[:, 0] > 0).all() and (got[:, 1] < 25).all()


# ---------------------------------------------------------------- seams
@pytest.mark.parametrize("fmt", ["yuv420p", "yuv444p10le"])
@pytest.mark.parametrize("unit", ["lane", "wave"])
def test_width_seams(gpu, fmt, unit):
    """Widths one below, at and one above the lane span (a 16-B chroma piece's
    luma columns) and the wave span, which is the workgroup's too: the waves of
    a workgroup lie below one another.  Two units across at span + 1."""
    lane, wave, _, _ = pc.spans(fmt)
    span = {"lane": lane, "wave": wave}[unit]
    for w in (span - 1, span, span + 1):
        ref = _noise(fmt, w, 5, 1, w)
        _check(fmt, ref, _noise(fmt, w, 5, 1, w + 1), gpu)


@pytest.mark.parametrize("fmt", ["yuv420p", "yuv422p10le"])
@pytest.mark.parametrize("unit", ["wave", "workgroup"])
def test_height_seams(gpu, fmt, unit):
    """Heights around the rows a wave walks and the band of a workgroup's four waves."""
    _, _, wave_rows, band_rows = pc.spans(fmt)
    rows = {"wave": wave_rows, "workgroup": band_rows}[unit]
    for h in (rows - 1, rows, rows + 1, 2 * rows + 1):
        ref = _noise(fmt, 40, h, 1, h)
        _check(fmt, ref, _noise(fmt, 40, h, 1, h + 100), gpu)


@pytest.mark.parametrize("fmt,w,h", [("yuv420p", 33, 17), ("yuv420p10le", 17, 9), ("yuv420p", 1, 1), ("yuv422p", 35, 3)])
def test_odd_sizes_have_their_own_last_chroma(gpu, fmt, w, h):
    ref, dist = _noise(fmt, w, h, 2, 5 + w), _noise(fmt, w, h, 2, 6 + w)
    got = _check(fmt, ref, dist, gpu)
    # the last chroma sample serves the last column and row alone: changing it changes the sum
    other = [p.copy() for p in dist]
    other[2][:, -1, -1] ^= 0x55
    assert (_check(fmt, ref, other, gpu)[:, 0] != got[:, 0]).all()


# ---------------------------------------------------------------- layouts
@pytest.mark.parametrize("fmt,w,h", [("yuv420p10le", 70, 37), ("yuv422p", 333, 97), ("yuv444p", 45, 20)])
def test_layouts_change_no_bit(gpu, fmt, w, h):
    ref, dist = _noise(fmt, w, h, 2, 40), _noise(fmt, w, h, 2, 41)
    want = _check(fmt, ref, dist, gpu)
    for layouts in [((0, 1), (0, 1)),          # rows starting one sample in: off the 16-B grid, sample by sample
                    ((64, 0), (64, 0)),        # padded pitch on the 16-B grid: the junk in the padding never counts
                    ((32, 0), None),           # ref and dist with different pitches
                    (None, (0, 1)),            # one clip on the grid, the other off it
                    ("interleaved", None)]:    # ref frame-interleaved (dense Y|U|V frames), dist planar
        got = _gpu(fmt, ref, dist, gpu, layouts=layouts)
        assert got.tobytes() == want.tobytes(), layouts


def test_reference_interleaved_with_the_distorted_clip(gpu):
    """Both clips in one tensor, frame by frame: ref frame k at 2k, dist frame k at 2k + 1."""
    import torch
    from pixpath import ops
    from pixpath.frames import FrameBatch
    fmt, w, h = "yuv422p10le", 64, 24
    ref, dist = _noise(fmt, w, h, 3, 50), _noise(fmt, w, h, 3, 51)
    want = _check(fmt, ref, dist, gpu)
    both = [torch.from_numpy(np.stack([r, d], axis=1).reshape((6,) + r.shape[1:])).to(gpu) for r, d in zip(ref, dist)]
    rb = FrameBatch(fmt, w, h, 3, planes=[t[0::2] for t in both])
    db = FrameBatch(fmt, w, h, 3, planes=[t[1::2] for t in both])
    got = ops.ciede(rb, db, fmt)
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == want.tobytes()


# ---------------------------------------------------------------- range
def test_ten_bit_range(gpu):
    fmt, w, h = "yuv444p10le", 37, 11
    got = _check(fmt, _const(fmt, w, h, 0, 0, 0), _const(fmt, w, h, 1023, 1023, 1023), gpu)  # all-zero against all-max
    assert got[0, 0] == pytest.approx(got[0, 1] * w * h, rel=1e-12) and got[0, 1] > 10
    # out-of-range samples (below 64, above 940 / 960) against legal ones, and the 16-bit container's upper bits
    rng = np.random.default_rng(60)
    wild = [np.where(rng.integers(0, 2, p.shape) == 1, rng.integers(0, 64, p.shape), rng.integers(961, 1024, p.shape))
            .astype(np.uint16) for p in _noise(fmt, w, h, 2, 61)]
    _check(fmt, wild, _noise(fmt, w, h, 2, 62), gpu)
    high = [(p.astype(np.uint32) * 64).astype(np.uint16) for p in _noise(fmt, w, h, 1, 63)]  # used as stored, nothing masked
    _check(fmt, high, _noise(fmt, w, h, 1, 64), gpu)


@pytest.mark.parametrize("fmt", ["yuv420p", "yuv422p10le"])
def test_grey_saturated_and_black(gpu, fmt):
    w, h = 50, 14
    s = 1 << (formats.fmt(fmt).depth - 8)
    grey = [_noise(fmt, w, h, 1, 70)[0]] + _const(fmt, w, h, 0, 128 * s, 128 * s)[1:]
    for u, v in ((240, 16), (16, 240), (240, 240), (16, 16)):  # saturated colour of every quadrant
        _check(fmt, grey, [grey[0]] + _const(fmt, w, h, 0, u * s, v * s)[1:], gpu)
    _check(fmt, grey, [_noise(fmt, w, h, 1, 71)[0]] + grey[1:], gpu)   # grey against grey
    # black against black: different code values at and below black, every one clips to R = G = B = 0
    rng = np.random.default_rng(72)
    b1 = [rng.integers(0, 16 * s + 1, p.shape).astype(p.dtype) if i == 0 else p for i, p in enumerate(grey)]
    b2 = [rng.integers(0, 16 * s + 1, p.shape).astype(p.dtype) if i == 0 else p for i, p in enumerate(grey)]
    got = _check(fmt, b1, b2, gpu)
    assert (got == 0.0).all()  # through the maths, not the shortcut: the samples differ


# ---------------------------------------------------------------- ref_index, weights, determinism
def test_ref_index(gpu):
    from pixpath import _native
    fmt, w, h = "yuv420p", 72, 44
    ref = _noise(fmt, w, h, 3, 80)
    for idx in ([0, 0, 1, 1, 2, 2], [2, 1, 0], [2, 0, 0, 1, 2, 1]):  # repeats, reversal, both
        idx = np.array(idx, np.int32)
        dist = _nudge(fmt, [p[idx] for p in ref], 81 + len(idx), amp=9)
        got = _check(fmt, ref, dist, gpu, ref_index=idx)
        assert got.tobytes() == _gpu(fmt, [p[idx] for p in ref], dist, gpu).tobytes()  # equal to the gathered frames
    dist = _nudge(fmt, ref, 85)
    assert _gpu(fmt, ref, dist, gpu).tobytes() == _gpu(fmt, ref, dist, gpu, ref_index=np.arange(3)).tobytes()
    for bad in ([0, 1, 3], [0, -1, 2]):
        with pytest.raises(_native.PixpathError) as e:
            _gpu(fmt, ref, dist, gpu, ref_index=bad)
        assert e.value.code == -1 and "ref_index" in str(e.value)
    with pytest.raises(_native.PixpathError) as e:  # more distorted frames than reference frames without a map
        _gpu(fmt, [p[:2] for p in ref], dist, gpu)
    assert e.value.code == -1


def test_map_of_257_frames_spans_two_launches(gpu):
    fmt, w, h = "yuv420p", 6, 4
    ref = _noise(fmt, w, h, 3, 90)
    idx = (np.arange(257) * 7 % 3).astype(np.int32)
    idx[254:257] = [2, 0, 1]
    dist = _nudge(fmt, [p[idx] for p in ref], 91, amp=20)
    got = _check(fmt, ref, dist, gpu, ref_index=idx)
    assert got.shape == (257, 2) and (got[:, 0] > 0).all()


def test_weights(gpu):
    fmt, w, h = "yuv422p", 70, 37
    ref, dist = _noise(fmt, w, h, 2, 95), _noise(fmt, w, h, 2, 96)
    one = _check(fmt, ref, dist, gpu)
    got = _check(fmt, ref, dist, gpu, weights=(2.0, 1.0, 0.5))
    assert (got != one).all()
    np.testing.assert_allclose(_check(fmt, ref, dist, gpu, weights=(2, 2, 2)), one / 2.0, rtol=1e-12)


def test_two_runs_give_the_same_bits(gpu):
    from pixpath.frames import FrameBatch
    fmt, w, h = "yuv420p10le", 517, 131
    ref, dist = _noise(fmt, w, h, 2, 97), _noise(fmt, w, h, 2, 98)
    a = _check(fmt, ref, dist, gpu)
    assert a.tobytes() == _gpu(fmt, ref, dist, gpu).tobytes()
    assert isinstance(_batch(fmt, ref, gpu, None), FrameBatch)
