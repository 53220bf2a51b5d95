"""PP-METRIC-1 on the CPU: known answers of the numpy restatement
(tests/metrics_ref.py), the host arithmetic of pixpath.metrics.summarize,
pp_metrics' argument checks (they run before any HIP call) and `cli metrics`
with a stubbed metrics_of_files."""
import ctypes
import json
import math

import numpy as np
import pytest

import metrics_ref
from pixpath import _native, cli, formats, metrics


# ---------------------------------------------------------------- numpy reference
def test_ref_identical_planes():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 1024, (24, 40)).astype(np.uint16)
    assert metrics_ref.plane_sse(a, a) == 0
    assert metrics_ref.plane_ssim(a, a, 10) == 1.0


def test_ref_one_window_zero_against_max():
    """a = 0, b = 1023 on one 8x8 window: s1 = 0, so 2 s1 s2 = covar = 0 and
    vars = 64 ss - s2^2 = 64 * 64 * 1023^2 - (64 * 1023)^2 = 0:
    v = c1 c2 / ((s2^2 + c1) c2) = c1 / (s2^2 + c1)."""
    a = np.zeros((8, 8), np.uint16)
    b = np.full((8, 8), 1023, np.uint16)
    assert metrics_ref.plane_sse(a, b) == 64 * 1023 * 1023
    c1 = .01 * .01 * 1023.0 * 1023.0 * 64
    s2 = 64 * 1023
    want = c1 / (float(s2 * s2) + c1)
    assert metrics_ref.plane_ssim(a, b, 10) == pytest.approx(want, rel=1e-14)
    assert 0 < want < 1e-3


def test_ref_small_plane_has_sse_but_no_ssim():
    a = np.zeros((6, 6), np.uint8)
    b = np.full((6, 6), 3, np.uint8)
    assert metrics_ref.plane_sse(a, b) == 36 * 9
    assert math.isnan(metrics_ref.plane_ssim(a, b, 8))


def test_ref_tails_count_in_sse_only():
    """The trailing w & 3 columns and h & 3 rows count in the SSE and take no part in SSIM."""
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (19, 22)).astype(np.uint8)
    b = a.copy()
    b[16:, :] ^= 0x55
    b[:, 20:] ^= 0x2a
    assert metrics_ref.plane_sse(a, b) > 0
    assert metrics_ref.plane_ssim(a, b, 8) == 1.0


# ---------------------------------------------------------------- summarize
@pytest.mark.parametrize("fmt,sizes", [("yuv420p", (64 * 48, 32 * 24, 32 * 24)), ("yuv422p10le", (64 * 48, 32 * 48, 32 * 48)),
                                       ("yuv444p", (64 * 48,) * 3)])
def test_summarize_plane_weighting(fmt, sizes):
    sse = np.array([[6144, 1536, 768], [0, 0, 3072]], np.int64)
    ssim = np.array([[0.9, 0.5, 0.25], [1.0, 1.0, 0.5]])
    r = metrics.summarize(sse, ssim, fmt, 64, 48)
    assert r["frames"] == 2
    for p, name in enumerate("yuv"):
        np.testing.assert_array_equal(r["mse_" + name], sse[:, p] / sizes[p])
        np.testing.assert_array_equal(r["ssim_" + name], ssim[:, p])
    np.testing.assert_allclose(r["mse_all"], sse.sum(axis=1) / sum(sizes), rtol=1e-15)
    np.testing.assert_allclose(r["ssim_all"], (ssim * np.array(sizes)).sum(axis=1) / sum(sizes), rtol=1e-15)
    peak = float((1 << formats.fmt(fmt).depth) - 1)
    assert r["psnr_y"][0] == pytest.approx(10 * math.log10(peak * peak / (6144 / sizes[0])), rel=1e-14)
    # clip values: PSNR of the mean MSE, not the mean of the PSNRs
    m = r["mean"]
    assert m["mse_v"] == pytest.approx((768 + 3072) / 2 / sizes[2])
    assert m["psnr_v"] == pytest.approx(10 * math.log10(peak * peak / m["mse_v"]), rel=1e-14)
    assert m["ssim_u"] == pytest.approx(0.75)


def test_summarize_identical_frames_have_no_psnr():
    r = metrics.summarize(np.zeros((2, 3), np.int64), np.ones((2, 3)), "yuv420p", 16, 16)
    for name in ("y", "u", "v", "all"):
        assert np.all(r["mse_" + name] == 0) and np.all(np.isnan(r["psnr_" + name]))
        assert math.isnan(r["mean"]["psnr_" + name])
    assert np.all(r["ssim_all"] == 1.0)


def test_summarize_nan_planes_leave_ssim_all():
    # yuv420p 8x8: chroma 4x4 has no window; only luma weighs in
    r = metrics.summarize(np.array([[64, 16, 16]]), np.array([[0.5, np.nan, np.nan]]), "yuv420p", 8, 8)
    assert r["ssim_all"][0] == 0.5 and np.isnan(r["ssim_u"][0])
    assert r["mse_all"][0] == 96 / (64 + 16 + 16)
    # no plane has one: absent
    r = metrics.summarize(np.array([[9, 9, 9]]), np.full((1, 3), np.nan), "yuv444p", 3, 3)
    assert np.isnan(r["ssim_all"][0]) and math.isnan(r["mean"]["ssim_all"])
    assert r["mse_all"][0] == 1.0


# ---------------------------------------------------------------- C ABI argument checks
def _call(ctx, fmt, w, h, nframes, ref_index=None):
    L = _native.lib()
    fr = _native.pp_frames()
    buf = (ctypes.c_uint8 * 64)()
    for p in range(3):
        fr.data[p] = ctypes.addressof(buf)
        fr.linesize[p] = 64
        fr.frame_stride[p] = 64
    out = (ctypes.c_uint8 * 256)()
    idx = None if ref_index is None else np.asarray(ref_index, np.int32).ctypes.data
    return L.pp_metrics(ctx, fmt, w, h, ctypes.byref(fr), ctypes.byref(fr), idx, nframes, out, out, None)


def test_pp_metrics_argument_checks_need_no_gpu():
    L = _native.lib()
    ctx = (ctypes.c_uint8 * 256)()  # never dereferenced: every call below is refused first
    assert _call(None, formats.YUV420P, 8, 8, 1) == -1
    assert b"null" in L.pp_last_error()
    for packed in (formats.UYVY422, formats.V210, 99):
        assert _call(ctx, packed, 8, 8, 1) == -1
        assert b"planar" in L.pp_last_error()
    for n in (0, -3):
        assert _call(ctx, formats.YUV420P, 8, 8, n) == -1
        assert b"nframes" in L.pp_last_error()
    assert _call(ctx, formats.YUV420P, 8, 8, 3, ref_index=[0, -1, 1]) == -1
    assert b"ref_index[1]" in L.pp_last_error()
    assert _call(ctx, formats.YUV420P, 0, 8, 1) == -1


# ---------------------------------------------------------------- cli metrics
def _fake_result():
    sse = np.array([[640, 0, 16], [0, 0, 0]], np.int64)
    ssim = np.array([[0.75, np.nan, 0.5], [1.0, np.nan, 1.0]])
    return metrics.summarize(sse, ssim, "yuv420p", 16, 16)


def test_cli_metrics_json(monkeypatch, capsys):
    seen = {}

    def stub(ref, dist, batch=32, flags="bicubic"):
        seen.update(ref=ref, dist=dist, batch=batch, flags=flags)
        return _fake_result()

    monkeypatch.setattr(metrics, "metrics_of_files", stub)
    assert cli.main(["metrics", "--ref", "/a/src.y4m", "--input", "/b/pvs.avi", "--batch", "7", "--flags", "lanczos"]) == 0
    assert seen == {"ref": "/a/src.y4m", "dist": "/b/pvs.avi", "batch": 7, "flags": "lanczos"}
    line = capsys.readouterr().out.strip()
    assert "\n" not in line and "NaN" not in line and "Infinity" not in line
    d = json.loads(line)
    assert d["ref"] == "src.y4m" and d["file"] == "pvs.avi" and d["frames"] == 2 and d["spec"] == "PP-METRIC-1"
    assert d["mse_y"] == 640 / 256 / 2 and d["ssim_y"] == 0.875
    assert d["psnr_u"] is None and d["ssim_u"] is None  # identical plane / no window: absent
    assert d["psnr_y"] == pytest.approx(10 * math.log10(255 * 255 / 1.25))
    assert not any(k.endswith("_frames") for k in d)

    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--per-frame"]) == 0
    assert seen["batch"] == 32 and seen["flags"] == "bicubic"
    d = json.loads(capsys.readouterr().out)
    assert d["psnr_y_frames"][1] is None and d["psnr_y_frames"][0] == pytest.approx(10 * math.log10(255 * 255 / 2.5))
    assert d["ssim_u_frames"] == [None, None] and d["ssim_v_frames"] == [0.5, 1.0]
    assert d["ssim_all_frames"] == [pytest.approx((0.75 * 256 + 0.5 * 64) / 320), 1.0]
    assert len(d["mse_all_frames"]) == 2


def test_cli_metrics_requires_both_files():
    with pytest.raises(SystemExit):
        cli.main(["metrics", "--input", "d.y4m"])
    with pytest.raises(SystemExit):
        cli.main(["metrics", "--ref", "r.y4m"])
