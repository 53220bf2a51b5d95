"""HIP PSNR/SSIM sums (pp_metrics, spec PP-METRIC-1) vs the numpy restatement
(tests/metrics_ref.py).

Tolerances: SSE is an exact integer and must be EQUAL.  SSIM within
atol = 1e-9: window values are O(1) with an fp64 error of a few 2^-53, and a
fixed-order sum of N <= 518,400 windows (the 2160p luma plane) adds at most
about N * 2^-53 ~ 6e-11 to the mean."""
import json

import numpy as np
import pytest

import metrics_ref
import synth
import pyoracle as po
from pixpath import formats, metrics as pm

pytestmark = pytest.mark.gpu
ATOL = 1e-9

# kernel geometry (csrc/metrics.hip), mirrored by pixpath.metrics
LANE_BYTES, OWN_LANES, WAVES, BAND_ROWS = pm.LANE_BYTES, pm.OWN_LANES, pm.WAVES, pm.BAND_ROWS


def _distort(rng, planes, depth, amp):
    """reference + bounded noise, clipped to the sample range."""
    mx = (1 << depth) - 1
    return [np.clip(p.astype(np.int64) + rng.integers(-amp, amp + 1, p.shape), 0, mx).astype(p.dtype) for p in planes]


def _clip(fmt, w, h, n, seed=7, amp=12):
    """n frames alternating smooth and noise content, and their distorted copies: lists of [n, rows, cols]."""
    f = po.FMT_BY_NAME[fmt]
    rng = np.random.default_rng(seed)
    frames = [synth.smooth_frame(t, f, w, h) if t % 2 == 0 else synth.noise_frame(rng, f, w, h) for t in range(n)]
    ref = synth.batch(frames)
    return ref, _distort(rng, ref, formats.fmt(fmt).depth, amp)


def _gpu(fmt, ref, dist, gpu, ref_index=None):
    import torch
    from pixpath import ops
    from pixpath.frames import FrameBatch
    rb = ref if isinstance(ref, FrameBatch) else FrameBatch.from_numpy(fmt, ref, device=gpu)
    db = dist if isinstance(dist, FrameBatch) else FrameBatch.from_numpy(fmt, dist, device=gpu)
    sse, ssim = ops.metrics(rb, db, ref_index=ref_index)
    torch.cuda.synchronize()
    assert sse.dtype == torch.int64 and ssim.dtype == torch.float64 and sse.shape == ssim.shape == (db.n, 3)
    return sse.cpu().numpy(), ssim.cpu().numpy()


def _check(fmt, ref, dist, gpu, ref_index=None, got=None):
    sse, ssim = got if got is not None else _gpu(fmt, ref, dist, gpu, ref_index)
    rsse, rssim = metrics_ref.metrics(ref, dist, formats.fmt(fmt).depth, ref_index)
    d = np.abs(ssim - rssim)
    d = d[~np.isnan(d)]
    print("%s %dx%d: sse unequal %d of %d, ssim max |d| %.3g (first frame: sse %s ssim %s)" % (
        fmt, dist[0].shape[2], dist[0].shape[1], int((sse != rsse).sum()), sse.size, d.max() if d.size else 0.0,
        sse[0].tolist(), ssim[0].tolist()))
    np.testing.assert_array_equal(sse, rsse)
    np.testing.assert_array_equal(np.isnan(ssim), np.isnan(rssim))
    np.testing.assert_allclose(ssim, rssim, rtol=0, atol=ATOL)
    return sse, ssim


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("fmt,w,h,n", [
    ("yuv420p", 8, 8, 2),            # one luma window, chroma NaN
    ("yuv444p", 3, 3, 2),            # every SSIM NaN, every SSE valid
    ("yuv420p10le", 70, 37, 2),      # w & 3 and h & 3 tails: in the SSE, not in SSIM
    ("yuv422p", 333, 97, 2),         # odd-size chroma tails
    ("yuv444p10le", 64, 48, 2),      # 4:4:4 planes
    ("yuv422p10le", 1920, 1080, 2),  # the real AVPVS geometry
])
def test_metrics_match_numpy(gpu, fmt, w, h, n):
    ref, dist = _clip(fmt, w, h, n)
    sse, ssim = _check(fmt, ref, dist, gpu)
    if (w, h) == (8, 8):
        assert not np.isnan(ssim[:, 0]).any() and np.isnan(ssim[:, 1:]).all()
    if (w, h) == (3, 3):
        assert np.isnan(ssim).all() and (sse > 0).any()


def _seam_sizes(span_px):
    return [span_px - 4, span_px, span_px + 4]


@pytest.mark.parametrize("fmt", ["yuv444p", "yuv444p10le"])
@pytest.mark.parametrize("unit", ["lane", "wave", "workgroup"])
def test_width_seams(gpu, fmt, unit):
    """Widths one block below, at and one block above the lane span (16 B),
    the wave span (kMetOwnLanes lanes) and the workgroup span (kMetWaves waves)."""
    lane_px = LANE_BYTES // formats.fmt(fmt).bytes_per_sample
    span = {"lane": lane_px, "wave": OWN_LANES * lane_px, "workgroup": WAVES * OWN_LANES * lane_px}[unit]
    for w in _seam_sizes(span):
        ref, dist = _clip(fmt, w, 12, 1, seed=w)
        _check(fmt, ref, dist, gpu)


@pytest.mark.parametrize("fmt", ["yuv420p", "yuv422p10le"])
@pytest.mark.parametrize("h", [BAND_ROWS - 4, BAND_ROWS, BAND_ROWS + 4, 2 * BAND_ROWS + 5])
def test_height_seams(gpu, fmt, h):
    """Heights around the band height (4 * kBandBlocks rows): the window that
    straddles two bands is counted once, by the upper band."""
    ref, dist = _clip(fmt, 40, h, 1, seed=h)
    _check(fmt, ref, dist, gpu)


# ---------------------------------------------------------------- integer range, 10 bits
def _const(fmt, w, h, v):
    dt = np.uint16 if formats.fmt(fmt).depth > 8 else np.uint8
    return [np.full((1, r, c), v, dt) for r, c in formats.plane_shapes(fmt, w, h)]


@pytest.mark.parametrize("pattern", ["max-max", "zero-max", "checker-inverse", "extreme-checker4", "extreme-noise",
                                     "extreme-steps"])
def test_ten_bit_integer_range(gpu, pattern):
    """s1^2, 64 ss and 2 s1 s2 pass 2^31 at 10 bits: exact SSE and SSIM on full-range patterns."""
    fmt, w, h = "yuv444p10le", 72, 40
    f = po.FMT_BY_NAME[fmt]
    if pattern == "max-max":
        ref, dist = _const(fmt, w, h, 1023), _const(fmt, w, h, 1023)
    elif pattern == "zero-max":
        ref, dist = _const(fmt, w, h, 0), _const(fmt, w, h, 1023)
    elif pattern == "checker-inverse":
        ref = synth.batch([synth.extreme_frame("checker", f, w, h)])
        dist = [(1023 - p).astype(np.uint16) for p in ref]
    else:
        kind = pattern.split("-")[1]
        ref = synth.batch([synth.extreme_frame(kind, f, w, h, seed=3, seams_x=(8, 37), seams_y=(5, 20))])
        other = "noise" if kind != "noise" else "checker"
        dist = synth.batch([synth.extreme_frame(other, f, w, h, seed=4)])
    sse, ssim = _check(fmt, ref, dist, gpu)
    if pattern == "max-max":
        assert (sse == 0).all() and (ssim == 1.0).all()
    if pattern in ("zero-max", "checker-inverse"):
        assert (sse == w * h * 1023 * 1023).all()


# ---------------------------------------------------------------- layout
def _padded(fmt, planes, gpu, extra_bytes, shift):
    """A FrameBatch whose planes are views into wider tensors filled with junk.
    shift = 0: a pitch of the 16-B-rounded row plus `extra_bytes` (a multiple
    of 16: still on the 16-B grid); shift = 1: rows starting one sample in,
    pitch one sample more than the row (off the grid)."""
    import torch
    from pixpath.frames import FrameBatch
    views = []
    for p in planes:
        n, r, c = p.shape
        es = p.dtype.itemsize
        pitch = c + 1 if shift else ((c * es + 15) // 16 * 16 + extra_bytes) // es
        big = torch.from_numpy(np.full((n, r + 1, pitch), 0x55, p.dtype)).to(gpu)
        big[:, :r, shift:shift + c].copy_(torch.from_numpy(np.ascontiguousarray(p)).to(gpu))
        views.append(big[:, :r, shift:])
    h, w = planes[0].shape[1:]
    return FrameBatch(fmt, w, h, planes[0].shape[0], planes=views)


@pytest.mark.parametrize("fmt,w,h", [("yuv420p10le", 70, 37), ("yuv422p", 333, 97)])
def test_layouts(gpu, fmt, w, h):
    import torch
    from pixpath.frames import FrameBatch
    ref, dist = _clip(fmt, w, h, 2)
    want = _check(fmt, ref, dist, gpu)

    def same(got):
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])  # same sums in the same order: bit-equal

    # rows starting one sample in: off the 16-B grid, the sample-by-sample path
    same(_gpu(fmt, _padded(fmt, ref, gpu, 0, 1), _padded(fmt, dist, gpu, 0, 1), gpu))
    # padded pitch, still on the 16-B grid
    same(_gpu(fmt, _padded(fmt, ref, gpu, 64, 0), _padded(fmt, dist, gpu, 64, 0), gpu))
    # ref and dist with different pitches
    same(_gpu(fmt, _padded(fmt, ref, gpu, 32, 0), dist, gpu))
    # ref frame-interleaved (dense Y|U|V frames), dist planar
    ib = FrameBatch.interleaved(fmt, w, h, 2, device=gpu)
    for p in range(3):
        ib.planes[p].copy_(torch.from_numpy(np.ascontiguousarray(ref[p])).to(gpu))
    same(_gpu(fmt, ib, dist, gpu))


def test_interleaved_aligned_reference(gpu):
    """An interleaved batch whose planes all sit on the 16-B grid takes the vector path."""
    import torch
    from pixpath.frames import FrameBatch
    fmt, w, h = "yuv422p10le", 64, 24
    ref, dist = _clip(fmt, w, h, 3)
    ib = FrameBatch.interleaved(fmt, w, h, 3, device=gpu)
    for p in range(3):
        ib.planes[p].copy_(torch.from_numpy(np.ascontiguousarray(ref[p])).to(gpu))
    _check(fmt, ref, dist, gpu, got=_gpu(fmt, ib, dist, gpu))


# ---------------------------------------------------------------- ref_index, determinism
def test_ref_index(gpu):
    from pixpath import ops
    fmt, w, h = "yuv420p", 72, 44
    ref, _ = _clip(fmt, w, h, 3)
    m = ops.fps_map(3, 30, 60)
    assert m.tolist() == [0, 0, 1, 1, 2, 2]
    order = np.array([2, 0, 0, 1, 2, 1], np.int32)
    rng = np.random.default_rng(5)
    for idx in (m, order):
        dist = _distort(rng, [p[idx] for p in ref], 8, 9)
        got = _check(fmt, ref, dist, gpu, ref_index=idx)
        # equal to comparing the gathered frames
        gathered = _gpu(fmt, [p[idx] for p in ref], dist, gpu)
        np.testing.assert_array_equal(got[0], gathered[0])
        np.testing.assert_array_equal(got[1], gathered[1])
    # NULL is the identity
    dist = _distort(rng, ref, 8, 9)
    a, b = _gpu(fmt, ref, dist, gpu), _gpu(fmt, ref, dist, gpu, ref_index=np.arange(3))
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        _gpu(fmt, ref, dist, gpu, ref_index=[0, 1, 3])


def test_long_ref_index_spans_launches(gpu):
    """More dist frames than one launch's index table (256) against few ref frames."""
    fmt, w, h = "yuv420p", 16, 12
    ref, _ = _clip(fmt, w, h, 2)
    idx = (np.arange(300) * 7 % 2).astype(np.int32)
    idx[255:258] = [1, 1, 0]
    rng = np.random.default_rng(6)
    dist = _distort(rng, [p[idx] for p in ref], 8, 5)
    _check(fmt, ref, dist, gpu, ref_index=idx)


def test_deterministic(gpu):
    fmt, w, h = "yuv422p10le", 1920, 1080
    ref, dist = _clip(fmt, w, h, 1)
    from pixpath.frames import FrameBatch
    rb, db = FrameBatch.from_numpy(fmt, ref, device=gpu), FrameBatch.from_numpy(fmt, dist, device=gpu)
    a, b = _gpu(fmt, rb, db, gpu), _gpu(fmt, rb, db, gpu)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---------------------------------------------------------------- files
def test_files_of_different_size_and_rate(gpu, tmp_path, capsys):
    """A 320x180 30 fps reference against a 640x360 60 fps clip: the reference
    goes through ops.Scaler and ops.fps_map; metrics_of_files and `cli metrics
    --per-frame` equal the numpy restatement applied to the same by hand."""
    from pixpath import cli, io as pio, ops
    from pixpath.frames import FrameBatch
    fmt = "yuv420p"
    src, _ = _clip(fmt, 320, 180, 5, seed=11)
    up = ops.Scaler(fmt, 320, 180, fmt, 640, 360, flags="bicubic")(FrameBatch.from_numpy(fmt, src, device=gpu)).to_numpy()
    m = ops.fps_map(5, 30, 60)
    assert len(m) == 10
    rng = np.random.default_rng(12)
    dist = _distort(rng, [p[m] for p in up], 8, 6)
    rp, dp = str(tmp_path / "src.y4m"), str(tmp_path / "pvs.y4m")
    for path, planes, size, rate in ((rp, src, (320, 180), 30), (dp, dist, (640, 360), 60)):
        wr = pio.Y4MWriter(path, fmt, size[0], size[1], rate)
        wr.write(np.ascontiguousarray(pio.join_planes(planes)))
        wr.close()
    rsse, rssim = metrics_ref.metrics(up, dist, 8, m)
    want = pm.summarize(rsse, rssim, fmt, 640, 360)
    for batch in (32, 3):  # one batch, and batches that cut the frame map
        got = pm.metrics_of_files(rp, dp, batch=batch)
        assert got["frames"] == 10
        for k in ("mse", "psnr", "ssim"):
            for pl in ("y", "u", "v", "all"):
                key = "%s_%s" % (k, pl)
                if k == "ssim":
                    np.testing.assert_allclose(got[key], want[key], rtol=0, atol=ATOL)
                else:  # from equal integers by the same host arithmetic
                    np.testing.assert_array_equal(got[key], want[key])
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", rp, "--input", dp, "--per-frame"]) == 0
    d = json.loads(capsys.readouterr().out)
    assert d["frames"] == 10 and d["ref"] == "src.y4m" and d["file"] == "pvs.y4m"
    np.testing.assert_array_equal(d["psnr_y_frames"], want["psnr_y"])
    np.testing.assert_array_equal(d["mse_all_frames"], want["mse_all"])
    np.testing.assert_allclose(d["ssim_all_frames"], want["ssim_all"], rtol=0, atol=ATOL)
    assert d["psnr_all"] == want["mean"]["psnr_all"]
