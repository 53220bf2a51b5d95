"""The two product uses of the unpackers, through files: scoring a CPVS (a
v210 / UYVY AVI) against its AVPVS with metrics_of_files / `cli metrics
--crop`, and SI/TI of an uncompressed (v210 / UYVY) SRC with siti_of_file."""
import json

import numpy as np
import pytest

import pyoracle as po
import synth
from file_clips import write_cpvs, write_packed_avi, write_y4m
import unpack_ref

pytestmark = pytest.mark.gpu
SSIM_BAR = 1e-9  # DESIGN section 3, PP-METRIC-1


def _clip(fmt, w, h, n, t0=0):
    return synth.batch([synth.smooth_frame(t0 + t, po.FMT_BY_NAME[fmt], w, h) for t in range(n)])


def _write_y4m(path, fmt, planes):
    return write_y4m(path, fmt, 60, planes)


def _write_avi(path, fourcc, w, h, packets):
    return write_packed_avi(path, fourcc, w, h, 60, packets)


def _perturb(planes, depth, seed=5):
    rng = np.random.default_rng(seed)
    mx = (1 << depth) - 1
    return [np.clip(p.astype(np.int64) + rng.integers(-9, 10, p.shape), 0, mx).astype(p.dtype) for p in planes]


def _make_cpvs(gpu, tmp_path, fmt, planes, W, H):
    """ops.cpvs of the AVPVS onto the W x H canvas, written as an AVI; returns (path, packed frames)."""
    path = str(tmp_path / ("cpvs_%s_%d.avi" % (fmt, H)))
    return path, write_cpvs(path, gpu, fmt, planes, W, H, 60)


def _same(got, want):
    """SSE-derived values equal, SSIM within the project's bar."""
    assert got["frames"] == want["frames"]
    for name in ("y", "u", "v", "all"):
        print(name, "mse", got["mse_" + name], want["mse_" + name], "ssim", got["ssim_" + name], want["ssim_" + name])
        np.testing.assert_array_equal(got["mse_" + name], want["mse_" + name])
        np.testing.assert_allclose(got["ssim_" + name], want["ssim_" + name], rtol=0, atol=SSIM_BAR)


def test_scoring_a_v210_cpvs_against_its_avpvs(gpu, tmp_path, capsys):
    from pixpath import cli, metrics
    fmt, w, h, n = "yuv422p10le", 64, 36, 5
    planes = _clip(fmt, w, h, n)
    avpvs = _write_y4m(tmp_path / "avpvs.y4m", fmt, planes)
    cpvs, _ = _make_cpvs(gpu, tmp_path, fmt, planes, 64, 48)
    res = metrics.metrics_of_files(avpvs, cpvs, crop=(64, 36))
    assert res["frames"] == n
    for name in ("y", "u", "v", "all"):
        assert not res["mse_" + name].any(), "SSE of plane %s is not 0" % name
        np.testing.assert_allclose(res["ssim_" + name], 1.0, rtol=0, atol=SSIM_BAR)
    # a perturbed reference: the CPVS scores as the AVPVS it was made from does
    bad = _write_y4m(tmp_path / "perturbed.y4m", fmt, _perturb(planes, 10))
    got = metrics.metrics_of_files(bad, cpvs, crop=(64, 36))
    want = metrics.metrics_of_files(bad, avpvs)
    assert want["mse_y"].all() and want["mse_u"].all()
    _same(got, want)
    _same(metrics.metrics_of_files(bad, cpvs, crop=(64, 36), batch=2), want)  # several batches
    # without a crop the whole canvas is compared (the reference is scaled to it): another result
    whole = metrics.metrics_of_files(avpvs, cpvs)
    assert whole["frames"] == n and whole["mse_y"].all()
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", bad, "--input", cpvs, "--crop", "64x36"]) == 0
    d = json.loads(capsys.readouterr().out)
    assert d == json.loads(json.dumps(metrics.report(got, bad, cpvs)))
    assert d["frames"] == n and d["file"].startswith("cpvs_") and d["mse_y"] > 0


@pytest.mark.parametrize("H", [48, 50])  # 50: (50 - 36) / 2 = 7, rounded down to 6 for a 4:2:0 AVPVS
def test_scoring_a_uyvy_cpvs_of_a_420_avpvs(gpu, tmp_path, capsys, H):
    from pixpath import cli, metrics, ops
    from pixpath.frames import FrameBatch
    fmt, w, h, n = "yuv420p", 64, 36, 5
    planes = _clip(fmt, w, h, n)
    cpvs, packed = _make_cpvs(gpu, tmp_path, fmt, planes, 64, H)
    ref_planes = _perturb(planes, 8)
    ref = _write_y4m(tmp_path / "ref420.y4m", fmt, ref_planes)
    got = metrics.metrics_of_files(ref, cpvs, crop=(64, 36), crop_from="yuv420p")
    # by hand: the window of the canvas (numpy), the reference through the same 4:2:0 -> 4:2:2 scaler
    win = (0, 6, 64, 36)
    dist = [np.stack(pl) for pl in zip(*[unpack_ref.unpack_uyvy(f, 64, win) for f in packed])]
    dist_b = FrameBatch.from_numpy("yuv422p", dist, device=gpu)
    ref_b = ops.Scaler("yuv420p", w, h, "yuv422p", w, h, flags="bicubic", device=gpu)(
        FrameBatch.from_numpy(fmt, ref_planes, device=gpu))
    sse, ssim = ops.metrics(ref_b, dist_b)
    want = metrics.summarize(sse.cpu().numpy(), ssim.cpu().numpy(), "yuv422p", w, h)
    _same(got, want)
    # the luma of the window is the AVPVS's own: its SSE against the unperturbed AVPVS is 0
    clean = metrics.metrics_of_files(_write_y4m(tmp_path / "avpvs420.y4m", fmt, planes), cpvs, crop=(64, 36),
                                     crop_from="yuv420p")
    assert not clean["mse_y"].any()
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", ref, "--input", cpvs, "--crop", "64x36", "--avpvs-pix-fmt", "yuv420p"]) == 0
    assert json.loads(capsys.readouterr().out) == json.loads(json.dumps(metrics.report(got, ref, cpvs)))


@pytest.mark.parametrize("fmt,depth", [("yuv422p10le", 10), ("yuv422p", 8)])
def test_siti_of_a_packed_src(gpu, tmp_path, fmt, depth):
    from pixpath import siti
    w, h, n = 96, 64, 6
    planes = _clip(fmt, w, h, n)
    y4m = _write_y4m(tmp_path / "src.y4m", fmt, planes)
    if depth == 10:
        packets = [po.v210_pack([p[k] for p in planes]) for k in range(n)]
        path = _write_avi(tmp_path / "src.avi", b"v210", w, h, packets)
    else:
        Y, U, V = planes
        packets = np.zeros((n, h, 2 * w), np.uint8)
        packets[..., 0::4], packets[..., 2::4], packets[..., 1::2] = U, V, Y
        path = _write_avi(tmp_path / "src.avi", b"UYVY", w, h, packets)
    si, ti, d = siti.siti_of_file(path, batch=4, with_depth=True)  # two batches: the TI halo crosses them
    rsi, rti = siti.siti_of_file(y4m, batch=4)
    assert d == depth and len(si) == n
    print("si", si, rsi, "ti", ti, rti)
    np.testing.assert_allclose(si, rsi, rtol=1e-4)
    assert np.isnan(ti[0]) and np.isnan(rti[0])
    np.testing.assert_allclose(ti[1:], rti[1:], rtol=0, atol=1e-12)
    if not (np.array_equal(si, rsi) and np.array_equal(ti[1:], rti[1:])):  # same kernel, same luma: equality expected
        print("SI/TI of the packed file differ from the Y4M's inside the bars: max |dSI| %g, max |dTI| %g"
              % (np.abs(si - rsi).max(), np.abs(ti[1:] - rti[1:]).max()))
