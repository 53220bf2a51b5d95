"""Host side of PP-BAND-1 without a GPU: `banding.pool` against a sort-based
evaluation, `default_window`, `summarize` / `report`, `cli banding` and
`cli metrics --banding` on stubbed measurements, pp_banding's argument checks,
and the numpy restatement (banding_ref) on content: what it ranks above what,
and that the content of the GPU tests exercises the mask, the window and
several bins."""
import ctypes
import json
import math

import numpy as np
import pytest

import banding_ref as R
from pixpath import _native, banding, cli, metrics


def _sorted_pool(hist):
    """The spec's step 7 on the values themselves."""
    tops = []
    for s in range(5):
        q = np.repeat(np.arange(1024), np.asarray(hist[s], dtype=np.int64))
        need = -((-3 * q.size) // 5)  # ceil(0.6 n)
        top = np.sort(q)[::-1][:need]
        tops.append(float(top.sum()) / (need * 1024.0) if need else 0.0)
    return sum(wt * t for wt, t in zip((16, 8, 4, 2, 1), tops)) / 31.0, tops


def test_pool_against_sorting():
    rng = np.random.default_rng(3)
    hist = np.zeros((6, 5, 1024), dtype=np.uint32)
    for k in range(6):
        for s in range(5):
            bins = rng.choice(1024, size=rng.integers(1, 40), replace=False)
            hist[k, s, bins] = rng.integers(1, 2000 >> s, len(bins))
    hist[5, 2] = 0          # an empty scale pools to 0
    hist[4, 0] = 0
    hist[4, 0, 1023] = 7    # everything in the last bin
    val, top = banding.pool(hist)
    assert val.shape == (6,) and top.shape == (6, 5)
    for k in range(6):
        want, tops = _sorted_pool(hist[k])
        assert val[k] == pytest.approx(want, rel=1e-14, abs=0) and top[k].tolist() == pytest.approx(tops, rel=1e-14, abs=0)
    assert top[4, 0] == 1023 / 1024 and top[5, 2] == 0.0 and (val < 1).all()
    assert banding.pool(hist[0])[0].shape == (1,)
    with pytest.raises(ValueError):
        banding.pool(np.zeros((2, 4, 1024)))


def test_constant_plane_pools_to_zero():
    for depth in (8, 10):
        a = np.full((1, 40, 56), 77, dtype=np.uint16 if depth > 8 else np.uint8)
        hist = R.hist(a, depth, 9)
        assert hist[0, :, 0].tolist() == [40 * 56, 20 * 28, 10 * 14, 5 * 7, 3 * 4] and not hist[:, :, 1:].any()
        val, top = banding.pool(hist)
        assert val.tolist() == [0.0] and not top.any()


def test_default_window_and_scales():
    assert banding.default_window(3840, 2160) == 63 and banding.default_window(1920, 1080) == 33
    assert banding.default_window(1280, 720) == 21 and banding.default_window(1, 1) == 3
    assert banding.default_window(200, 120) == 5 and banding.default_window(20000, 20000) == 63
    for w, h in ((1, 1), (640, 360), (4096, 2304), (7680, 4320)):
        win = banding.default_window(w, h)
        assert win % 2 == 1 and banding.MIN_WINDOW <= win <= banding.MAX_WINDOW
    assert banding.scale_sizes(1920, 1080) == [(1920, 1080), (960, 540), (480, 270), (240, 135), (120, 68)]
    assert banding.scale_sizes(1, 9) == [(1, 9), (1, 5), (1, 3), (1, 2), (1, 1)]


def _ramp(w=192, h=48):
    """A horizontal 10-bit ramp of one code per three samples."""
    return np.tile(300 + np.arange(w) // 3, (h, 1)).astype(np.uint16)


def test_restatement_ranks_content():
    """Coarser quantisation bands a ramp; noise of +-8 is removed by the mask.

    The quantised ramp is the 10-bit ramp with its two low bits dropped, what
    the 8-bit CPVS conversion does: steps of 4 codes, which k = 4 counts, in
    bands four times as wide.  A ramp quantised to 6 bits has steps of 16 codes
    on the ten-bit scale; PP-BAND-1 (as CAMBI) counts steps of at most 4, so
    that staircase scores exactly 0 and cannot rank above the full-depth ramp
    (measured: full 0.195, 8-bit 0.570, 6-bit 0.0 at window 9)."""
    full = _ramp()
    eight = (full >> 2) << 2
    six = (full >> 4) << 4
    noisy = (full.astype(np.int64) + np.random.default_rng(1).integers(-8, 9, full.shape)).astype(np.uint16)
    b = {name: float(banding.pool(R.hist(a[None], 10, 9))[0][0])
         for name, a in (("full", full), ("eight", eight), ("six", six), ("noisy", noisy))}
    assert b["eight"] > b["full"] > b["noisy"] >= 0.0, b
    assert b["six"] == 0.0  # steps above 4 codes are no banding by this spec


def test_restatement_levels_and_mode():
    y = np.array([[5, 5, 7], [7, 9, 9], [1, 1, 2]])
    # the centre sees 5 5 7 7 9 9 1 1 2: four values twice, the smallest wins
    assert R.mode3(y)[1, 1] == 1
    # the corner (0, 0) sees 5 four times (replicated edge), 5, 7 ..: 5
    assert R.mode3(y)[0, 0] == 5
    lv = R.levels(np.zeros((9, 17), np.uint8), 8)
    assert [t[0].shape for t in lv] == [(9, 17), (5, 9), (3, 5), (2, 3), (1, 2)]
    u = R.ten_bit(np.array([[255]], np.uint8), 8)
    assert u[0, 0] == 1020 and R.ten_bit(np.array([[40000, 7]], np.uint16), 10).tolist() == [[1023, 7]]
    assert R.anti_dither(np.array([[0, 4], [8, 16]])).tolist() == [[7, 10], [12, 16]]


@pytest.mark.parametrize("depth", [8, 10])
def test_gpu_test_content_is_fit(depth):
    """The content of test_gpu_banding: a kernel that ignores the mask or the
    window cannot pass on it."""
    for w, h, window, seed in ((40, 24, 5, 1), (131, 67, 15, 2), (200, 120, 33, 3)):
        a = R.content(depth, 2, w, h, seed)
        for f in range(2):
            y, m = R.levels(a[f], depth)[0]
            assert 0.10 <= m.mean() <= 0.90, (w, h, m.mean())
            hist = R.frame_hist(a[f], depth, window)
            assert (hist[0, 1:] != 0).sum() >= 3
            assert not np.array_equal(hist, R.frame_hist(a[f], depth, window + 2))  # the window counts


def _fake_hist(n=3):
    hist = np.zeros((n, 5, 1024), dtype=np.uint32)
    hist[:, :, 0] = 100
    for k in range(n):
        hist[k, 0, 0] = 40
        hist[k, 0, 512] = 60 * (k + 1) // (k + 1)  # top_0 = 0.5: banding 16 / 31 / 2
        hist[k, 1, 0] = 100 - 60
        hist[k, 1, 256 * k] += 60                  # top_1 = k / 4
    return hist


def test_summarize_and_report():
    hist = _fake_hist()
    res = banding.summarize(hist)
    want = [(16 * 0.5 + 8 * k / 4) / 31 for k in range(3)]
    assert res["banding_y"].tolist() == pytest.approx(want, rel=1e-15)
    assert res["mean"]["banding_y"] == pytest.approx(sum(want) / 3) and res["mean"]["banding_max_y"] == pytest.approx(want[2])
    assert res["mean"]["banding_scales_y"] == pytest.approx([0.5, 0.25, 0, 0, 0])
    res.update({"frames": 3, "w": 64, "h": 48, "window": 7})
    out = banding.report(res, "/tmp/x/clip.avi")
    assert out["spec"] == "PP-BAND-1" and out["file"] == "clip.avi" and out["window"] == 7 and out["frames"] == 3
    assert len(out["banding_scales_y"]) == 5 and not [k for k in out if k.endswith("_frames")]
    per = banding.report(res, "clip.avi", per_frame=True)
    assert per["banding_y_frames"] == pytest.approx(want) and len(per["banding_scales_y_frames"]) == 3
    json.dumps(per)
    empty = banding.summarize(np.zeros((0, 5, 1024), np.uint32))
    assert math.isnan(empty["mean"]["banding_y"]) and empty["banding_y"].shape == (0,)
    empty.update({"frames": 0, "w": 1, "h": 1, "window": 3})
    assert banding.report(empty, "e.avi")["banding_y"] is None


def test_cli_banding(monkeypatch, capsys):
    seen = []

    def measured(path, **kw):
        seen.append((path, kw))
        res = banding.summarize(_fake_hist())
        res.update({"frames": 3, "w": 64, "h": 48, "window": kw.get("window") or 5})
        return res

    monkeypatch.setattr(banding, "banding_of_file", measured)
    assert cli.main(["banding", "a/clip.avi"]) == 0
    assert seen[-1] == ("a/clip.avi", {"batch": 32, "window": None})
    d = json.loads(capsys.readouterr().out)
    assert set(d) == {"file", "frames", "w", "h", "spec", "window", "banding_y", "banding_max_y", "banding_scales_y"}
    assert d["spec"] == "PP-BAND-1" and d["window"] == 5
    assert cli.main(["banding", "c.avi", "--per-frame", "--window", "9", "--crop", "64x48", "--avpvs-pix-fmt", "yuv420p",
                     "--batch", "4"]) == 0
    assert seen[-1] == ("c.avi", {"batch": 4, "window": 9, "crop": (64, 48), "crop_from": "yuv420p"})
    d = json.loads(capsys.readouterr().out)
    assert d["window"] == 9 and len(d["banding_y_frames"]) == 3 and len(d["banding_scales_y_frames"][0]) == 5
    with pytest.raises(SystemExit):
        cli.main(["banding", "c.avi", "--avpvs-pix-fmt", "yuv420p"])
    with pytest.raises(SystemExit):
        cli.main(["banding"])


def test_cli_metrics_banding(monkeypatch, capsys):
    sse = np.array([[10, 4, 2], [0, 0, 0], [30, 1, 1]], dtype=np.int64)
    ssim = np.array([[0.9, 0.8, 0.7], [1.0, 1.0, 1.0], [0.5, 0.6, 0.7]])
    hd, hr = _fake_hist(), _fake_hist()
    hr[:, 0, 512] = 0
    hr[:, 0, 0] = 100  # the reference has no contrast at scale 0
    seen = []

    def before(ref, dist, batch=32, flags="bicubic"):  # what `cli metrics` called before PP-BAND-1
        return metrics.summarize(sse, ssim, "yuv420p", 33, 33)

    def scored(ref, dist, **kw):
        seen.append(kw)
        return metrics.summarize(sse, ssim, "yuv420p", 33, 33, banding_terms=(hd, hr) if kw.get("banding") else None)

    monkeypatch.setattr(metrics, "metrics_of_files", before)
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--per-frame"]) == 0
    old = capsys.readouterr().out
    monkeypatch.setattr(metrics, "metrics_of_files", scored)
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--per-frame"]) == 0
    assert capsys.readouterr().out == old and "banding" not in seen[-1]  # unchanged byte for byte without the flag
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--banding"]) == 0
    assert seen[-1] == {"batch": 32, "flags": "bicubic", "banding": True}
    d = json.loads(capsys.readouterr().out)
    assert d["banding_added_y"] == pytest.approx(16 * 0.5 / 31) and d["banding_added_y"] == pytest.approx(d["banding_y"] - d["banding_ref_y"])
    assert not [k for k in d if k.endswith("_frames")]
    for k, v in json.loads(old).items():
        if not k.endswith("_frames"):
            assert d[k] == v
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--banding", "--per-frame"]) == 0
    d = json.loads(capsys.readouterr().out)
    assert len(d["banding_y_frames"]) == 3 and d["banding_added_y_frames"] == pytest.approx([16 * 0.5 / 31] * 3)
    res = metrics.summarize(sse, ssim, "yuv420p", 33, 33, matched=[True, False, True], banding_terms=(hd, hr))
    assert math.isnan(res["banding_y"][1]) and res["mean"]["banding_ref_y"] == pytest.approx((0 + 8 * 2 / 4 / 31) / 2)


def _call(ctx, depth=8, w=20, h=15, src=True, hist=True, sls=32, nsrc=2, n=2, idx=None, window=3):
    L = _native.lib()
    buf = (ctypes.c_uint8 * 64)()  # never read: every call below is refused, or has nothing to do, first
    p = lambda on: ctypes.c_void_p(ctypes.addressof(buf)) if on else None
    ix = None if idx is None else (ctypes.c_int32 * len(idx))(*idx)
    return L.pp_banding(ctx, depth, w, h, p(src), sls, 1024, nsrc, None if ix is None else ctypes.addressof(ix), n,
                        window, None, p(hist), None)


def test_pp_banding_argument_checks_need_no_gpu():
    L = _native.lib()
    assert "pp_banding" in _native.EXPORTS and L.pp_abi_version() == 7
    ctx = (ctypes.c_uint8 * 256)()  # never dereferenced
    for kw in ({"src": False}, {"hist": False}):
        assert _call(ctx, **kw) == -1 and b"null" in L.pp_last_error()
    assert _call(None) == -1 and b"null" in L.pp_last_error()
    for depth in (9, 12, 16, 0):
        assert _call(ctx, depth=depth) == -1 and b"bitdepth" in L.pp_last_error()
    assert _call(ctx, w=0) == -1 and b"frame" in L.pp_last_error()
    assert _call(ctx, h=-1) == -1 and b"frame" in L.pp_last_error()
    assert _call(ctx, n=-1) == -1 and b"n -1" in L.pp_last_error()
    assert _call(ctx, nsrc=-1, n=0) == -1 and b"nsrc" in L.pp_last_error()
    for window in (-1, 0, 1, 2, 4, 62, 64, 65, 1 << 20):
        assert _call(ctx, window=window) == -1 and b"window" in L.pp_last_error()
    assert _call(ctx, sls=19) == -1 and b"src plane 0: linesize" in L.pp_last_error()
    assert _call(ctx, depth=10, sls=39) == -1 and b"linesize" in L.pp_last_error()
    assert _call(ctx, depth=10, sls=41) == -1 and b"2-byte grid" in L.pp_last_error()
    assert _call(ctx, idx=[0, 2]) == -1 and b"index[1] = 2" in L.pp_last_error()
    assert _call(ctx, idx=[-1, 0]) == -1 and b"index[0] = -1" in L.pp_last_error()
    assert _call(ctx, nsrc=1) == -1 and b"without index" in L.pp_last_error()
    assert _call(ctx, h=64, sls=1 << 25) == -4 and b"2 GiB buffer range" in L.pp_last_error()
    for window in (3, 33, 63):
        assert _call(ctx, n=0, window=window) == 0 and _call(ctx, n=0, nsrc=0, window=window) == 0  # no HIP call
