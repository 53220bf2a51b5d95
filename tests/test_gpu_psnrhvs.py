"""HIP PSNR-HVS / PSNR-HVS-M sums (pp_psnr_hvs, spec PP-HVS-1) vs the numpy
restatement (tests/psnrhvs_ref.py).

Tolerance: every S_hvs within RTOL = 1e-9 relative of the restatement, and
every S_hvsm within 1e-9 of the same plane's S_hvs (absolute: RTOL S_hvs): the
masked sum can be exactly 0 on one side and about 1e-26 on the other when a
coefficient sits on its threshold, so it has no relative bound of its own.
1e-9 is the bound the PP-VIF-1, PP-ADM-1 and PP-CIEDE-1 tests use for fp64
kernels against numpy.  The kernel folds each 8-point sum by the matrix's
symmetry and fuses its multiply-adds where the restatement takes two matrix
products: a coefficient differs by a few 2^-53 of the block's largest, and a
sum of at most 10^4 non-negative terms in another order by 10^4 2^-53 ~ 1e-12
relative.  Where the restatement gives exactly 0 for S_hvs the kernel must
too; every output lies in a sentinel-filled buffer two frames longer than
ndist whose other elements must stay as they were."""
import ctypes

import numpy as np
import pytest

import psnrhvs_ref
from pixpath import formats, psnrhvs

pytestmark = pytest.mark.gpu
RTOL = 1e-9
SENTINEL = -12345.678
FORMATS = ["yuv420p", "yuv422p10le", "yuv444p"]
SEEN = {"hvs": 0.0, "hvsm": 0.0}  # the largest differences of the session, printed by every comparison


def _dtype(fmt):
    return np.uint16 if formats.fmt(fmt).depth > 8 else np.uint8


def _noise(fmt, w, h, n, seed):
    """n frames of uniform noise over the whole sample range: a list of [n, rows, cols]."""
    rng = np.random.default_rng(seed)
    f = formats.fmt(fmt)
    return [rng.integers(0, 1 << f.depth, (n, r, c)).astype(_dtype(fmt)) for r, c in formats.plane_shapes(f, w, h)]


def _nudge(fmt, planes, seed, amp=6):
    """The planes +- amp code values, clipped to the sample range."""
    rng = np.random.default_rng(seed)
    mx = (1 << formats.fmt(fmt).depth) - 1
    return [np.clip(p.astype(np.int64) + rng.integers(-amp, amp + 1, p.shape), 0, mx).astype(p.dtype) for p in planes]


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
        junk = np.random.default_rng(77 + i).integers(0, 256, (n, r + 1, pitch)).astype(p.dtype)
        big = torch.from_numpy(junk).to(gpu)
        big[:, :r, shift:shift + c].copy_(torch.from_numpy(np.ascontiguousarray(p)).to(gpu))
        views.append(big[:, :r, shift:])
    h, w = planes[0].shape[1:]
    return FrameBatch(fmt, w, h, planes[0].shape[0], planes=views)


def _batch(fmt, planes, gpu, layout):
    from pixpath.frames import FrameBatch
    if layout is None:
        return FrameBatch.from_numpy(fmt, planes, device=gpu)
    return _padded(fmt, planes, gpu, *layout)


def _raw(fmt, rb, db, step, ref_index=None):
    """pp_psnr_hvs itself into a sentinel-filled [ndist + 2, 3, 2]: the first
    and the last frame of it are not the call's and must stay."""
    import torch
    from pixpath import _native, ops
    n = db.n
    buf = torch.full((n + 2, 3, 2), SENTINEL, dtype=torch.float64, device=db.device)
    idx = None if ref_index is None else np.ascontiguousarray(ref_index, dtype=np.int32)
    r, d = rb.frames_struct(), db.frames_struct()
    _native.check(_native.lib().pp_psnr_hvs(
        ops.context(db.device.index).handle, formats.fmt(fmt).id, db.w, db.h, ctypes.byref(r), ctypes.byref(d),
        None if idx is None else idx.ctypes.data, rb.n, n, step, ctypes.c_void_p(buf[1:].data_ptr()),
        ctypes.c_void_p(torch.cuda.current_stream(db.device).cuda_stream)))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert (out[0] == SENTINEL).all() and (out[-1] == SENTINEL).all(), "wrote outside its ndist x 3 x 2"
    return out[1:-1]


def _gpu(fmt, ref, dist, gpu, step=8, ref_index=None, layouts=(None, None)):
    import torch
    from pixpath import ops
    rb, db = _batch(fmt, ref, gpu, layouts[0]), _batch(fmt, dist, gpu, layouts[1])
    raw = _raw(fmt, rb, db, step, ref_index)
    out = ops.psnr_hvs(rb, db, ref_index=ref_index, step=step)
    torch.cuda.synchronize()
    assert out.dtype == torch.float64 and tuple(out.shape) == (db.n, 3, 2)
    assert out.cpu().numpy().tobytes() == raw.tobytes()  # ops.psnr_hvs is the same call
    return raw


def _check(fmt, ref, dist, gpu, step=8, ref_index=None, layouts=(None, None)):
    want = psnrhvs_ref.psnr_hvs(ref, dist, step, ref_index)
    got = _gpu(fmt, ref, dist, gpu, step, ref_index, layouts)
    assert np.isfinite(got).all() and (got >= 0).all() and not np.signbit(got).any()
    hvs, whvs = got[..., 0], want[..., 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(whvs > 0, np.abs(hvs - whvs) / np.where(whvs > 0, whvs, 1.0), np.where(hvs == whvs, 0.0, np.inf))
        relm = np.where(whvs > 0, np.abs(got[..., 1] - want[..., 1]) / np.where(whvs > 0, whvs, 1.0),
                        np.where(got[..., 1] == want[..., 1], 0.0, np.inf))
    SEEN["hvs"], SEEN["hvsm"] = max(SEEN["hvs"], rel.max(initial=0.0)), max(SEEN["hvsm"], relm.max(initial=0.0))
    print("%s %dx%d x%d step %d: S_hvs rel %.3g, S_hvsm over S_hvs %.3g (largest so far %.3g, %.3g); frame 0: %s" % (
        fmt, dist[0].shape[2], dist[0].shape[1], dist[0].shape[0], step, rel.max(initial=0.0), relm.max(initial=0.0),
        SEEN["hvs"], SEEN["hvsm"], got[0].tolist() if len(got) else None))
    np.testing.assert_array_equal(hvs[whvs == 0], 0.0)
    np.testing.assert_array_equal(got[..., 1][whvs == 0], 0.0)
    assert (got[..., 1] <= hvs).all()
    assert (rel <= RTOL).all(), rel.max()
    assert (relm <= RTOL).all(), relm.max()
    nb = np.array(psnrhvs.blocks(fmt, dist[0].shape[2], dist[0].shape[1], step))
    assert (got[:, nb == 0] == 0.0).all()  # a plane with no block: 0.0, 0.0
    return got


# ---------------------------------------------------------------- seams of the block grid
@pytest.mark.parametrize("step", psnrhvs.STEPS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_block_seams(gpu, fmt, step):
    """Widths and heights 8, 9, 15, 16, 22 and 23: at each step the sizes at
    which a block appears and the sample before; the chroma planes of the
    subsampled formats cross 8 at luma sizes of their own (15, 16)."""
    sizes = (8, 9, 15, 16, 22, 23)
    for i, w in enumerate(sizes):
        h = sizes[(i + 2) % len(sizes)]
        ref = _noise(fmt, w, h, 2, 100 + w)
        got = _check(fmt, ref, _nudge(fmt, ref, 200 + w), gpu, step)
        assert (got[:, 0, 0] > 0).all()
    ref = _noise(fmt, 23, 23, 1, 1)
    _check(fmt, ref, _noise(fmt, 23, 23, 1, 2), gpu, step)  # noise against noise


@pytest.mark.parametrize("step", psnrhvs.STEPS)
@pytest.mark.parametrize("fmt", ["yuv444p", "yuv422p10le"])
def test_workgroup_tile_seams(gpu, fmt, step):
    """A workgroup owns 32 consecutive blocks of a block row: widths a sample
    either side of the 32 blocks' span (the 32nd block appears), and either
    side of the width at which the 33rd, the next workgroup's first, appears;
    heights either side of a second and a third block row (a workgroup is one
    block row high)."""
    span = psnrhvs.tile_width(step)
    for w in (span - 1, span, span + 1, span + step - 1, span + step, span + step + 1):
        ref = _noise(fmt, w, 9, 1, w)
        _check(fmt, ref, _nudge(fmt, ref, w + 1), gpu, step)
    for h in (8 + step - 1, 8 + step, 8 + step + 1, 8 + 2 * step - 1, 8 + 2 * step):
        ref = _noise(fmt, 40, h, 1, h)
        _check(fmt, ref, _nudge(fmt, ref, h + 100), gpu, step)
    if fmt == "yuv422p10le":  # three workgroups across in luma, two in chroma; noise against noise
        ref = _noise(fmt, 2 * span + 3 * step + 8, 17, 1, 5)
        _check(fmt, ref, _noise(fmt, 2 * span + 3 * step + 8, 17, 1, 6), gpu, step)


@pytest.mark.parametrize("step", psnrhvs.STEPS)
@pytest.mark.parametrize("fmt,w,h", [("yuv420p", 33, 17), ("yuv422p10le", 35, 9), ("yuv420p", 15, 15)])
def test_odd_sizes_have_ceil_sized_chroma(gpu, fmt, w, h, step):
    ref, dist = _noise(fmt, w, h, 2, 5 + w), _noise(fmt, w, h, 2, 6 + w)
    got = _check(fmt, ref, dist, gpu, step)
    assert (got[:, 1:, 0] > 0).all()  # 33 -> 17, 17 -> 9, 15 -> 8: the chroma planes have blocks
    # the last chroma sample of a 15 x 15 frame's 8 x 8 chroma lies in its one block
    if (w, h) == (15, 15):
        other = [p.copy() for p in dist]
        other[2][:, -1, -1] ^= 0x55
        assert (_check(fmt, ref, other, gpu, step)[:, 2, 0] != got[:, 2, 0]).all()


@pytest.mark.parametrize("fmt,w,h", [("yuv420p", 64, 7), ("yuv422p10le", 7, 40), ("yuv420p", 14, 14), ("yuv444p", 1, 1)])
def test_planes_without_a_block_give_zero(gpu, fmt, w, h):
    """A frame under 8 rows or columns has no block at all (no unit is launched);
    14 x 14 as 4:2:0 has a luma block and 7 x 7 chroma planes."""
    for step in psnrhvs.STEPS:
        ref = _noise(fmt, w, h, 3, 9)
        got = _check(fmt, ref, _noise(fmt, w, h, 3, 10), gpu, step)
        if (w, h) == (14, 14):
            assert (got[:, 0] > 0).all() and (got[:, 1:] == 0).all()
        else:
            assert (got == 0.0).all()


# ---------------------------------------------------------------- layouts
@pytest.mark.parametrize("step", psnrhvs.STEPS)
@pytest.mark.parametrize("fmt,w,h", [("yuv420p", 70, 37), ("yuv422p10le", 333, 25)])
def test_layouts_change_no_bit(gpu, fmt, w, h, step):
    ref, dist = _noise(fmt, w, h, 2, 40), _noise(fmt, w, h, 2, 41)
    want = _check(fmt, ref, dist, gpu, step)
    for layouts in [((0, 1), (0, 1)),     # rows starting one sample in: pitch and base off the 16-B grid
                    ((64, 0), (64, 0)),   # padded pitch on the 16-B grid: the junk in the padding never counts
                    ((32, 0), None),      # ref and dist with different pitches
                    (None, (0, 1))]:      # one clip on the grid, the other off it
        got = _gpu(fmt, ref, dist, gpu, step, layouts=layouts)
        assert got.tobytes() == want.tobytes(), layouts


# ---------------------------------------------------------------- ref_index
def test_ref_index(gpu):
    from pixpath import _native
    fmt, w, h = "yuv420p", 72, 44
    ref = _noise(fmt, w, h, 3, 80)
    for idx in ([0, 0, 1, 1, 2, 2], [2, 1, 0], [2, 0, 0, 1, 2, 1]):  # repeats, a backward step, both
        idx = np.array(idx, np.int32)
        dist = _nudge(fmt, [p[idx] for p in ref], 81 + len(idx), amp=9)
        got = _check(fmt, ref, dist, gpu, 7, ref_index=idx)
        assert got.tobytes() == _gpu(fmt, [p[idx] for p in ref], dist, gpu, 7).tobytes()  # equal to the gathered frames
    dist = _nudge(fmt, ref, 85)
    assert _gpu(fmt, ref, dist, gpu).tobytes() == _gpu(fmt, ref, dist, gpu, ref_index=np.arange(3)).tobytes()
    for bad in ([0, 1, 3], [0, -1, 2]):
        with pytest.raises(_native.PixpathError) as e:
            _gpu(fmt, ref, dist, gpu, ref_index=bad)
        assert e.value.code == -1 and "ref_index" in str(e.value)
    with pytest.raises(_native.PixpathError) as e:  # more distorted frames than reference frames without a map
        _gpu(fmt, [p[:2] for p in ref], dist, gpu)
    assert e.value.code == -1
    with pytest.raises(_native.PixpathError) as e:
        _gpu(fmt, ref, dist, gpu, step=9)
    assert e.value.code == -1 and "step" in str(e.value)


def test_map_of_257_frames_spans_two_launches(gpu):
    fmt, w, h = "yuv420p", 16, 16
    ref = _noise(fmt, w, h, 3, 90)
    idx = (np.arange(257) * 7 % 3).astype(np.int32)
    idx[254:257] = [2, 0, 1]
    dist = _nudge(fmt, [p[idx] for p in ref], 91, amp=20)
    for step in psnrhvs.STEPS:
        got = _check(fmt, ref, dist, gpu, step, ref_index=idx)
        assert got.shape == (257, 3, 2) and (got[..., 0] > 0).all()


# ---------------------------------------------------------------- range, zero, determinism
def test_ten_bit_samples_stored_above_1023(gpu):
    """Used as stored, nothing masked: the variance integers need 64 bits."""
    fmt, w, h = "yuv422p10le", 37, 19
    rng = np.random.default_rng(60)
    high = [rng.integers(0, 65536, p.shape).astype(np.uint16) for p in _noise(fmt, w, h, 2, 61)]
    for step in psnrhvs.STEPS:
        _check(fmt, high, _nudge(fmt, _noise(fmt, w, h, 2, 62), 63), gpu, step)
        top = [np.where(p > 32767, p, 65535 - p).astype(np.uint16) for p in high]  # every sample above 32767
        _check(fmt, top, [(65535 - (65535 - p) // 2).astype(np.uint16) for p in top], gpu, step)


@pytest.mark.parametrize("fmt", ["yuv420p", "yuv422p10le"])
def test_identical_clips_are_exactly_zero(gpu, fmt):
    ref = _noise(fmt, 333, 41, 2, 1)
    for step in psnrhvs.STEPS:
        got = _gpu(fmt, ref, [p.copy() for p in ref], gpu, step)
        assert (got == 0.0).all() and not np.signbit(got).any()
        res = psnrhvs.summarize(got, 333, 41, None, fmt, step)
        assert (res["mse_hvs_all"] == 0).all() and np.isnan(res["psnr_hvsm_all"]).all()


def test_flat_and_constant_offset(gpu):
    """B = A + c: only DC differs and DC is never masked: both sums are 64 c^2 CSF[0][0]^2 a block."""
    fmt, w, h, c = "yuv444p", 47, 26, 5
    ref = [(p // 2).astype(p.dtype) for p in _noise(fmt, w, h, 1, 70)]
    got = _check(fmt, ref, [(p + c).astype(p.dtype) for p in ref], gpu, 8)
    nb = psnrhvs.blocks(fmt, w, h, 8)[0]
    np.testing.assert_allclose(got, 64.0 * nb * c * c * (25.735088 / 16.0) ** 2, rtol=1e-9)
    flat = [np.full_like(p, 100) for p in ref]
    got = _check(fmt, flat, [np.full_like(p, 117) for p in ref], gpu, 7)  # no variance: pop = 0, no mask
    assert (got[..., 0] == got[..., 1]).all()


def test_two_runs_give_the_same_bits(gpu):
    fmt, w, h = "yuv420p10le", 517, 67
    ref, dist = _noise(fmt, w, h, 2, 97), _noise(fmt, w, h, 2, 98)
    for step in psnrhvs.STEPS:
        a = _check(fmt, ref, dist, gpu, step)
        assert a.tobytes() == _gpu(fmt, ref, dist, gpu, step).tobytes()
