"""PP-MOTION-1 on the CPU: closed forms of the numpy restatement (motion_ref),
the host pooling (pixpath.motion.pool / summarize), the plumbing of
`metrics.summarize`, `report`, `cli metrics --motion` and `--vmaf-features` on
canned terms, and the argument checks of pp_motion that need no GPU."""
import ctypes
import json
import math

import numpy as np
import pytest

import motion_ref as R
from pixpath import _native, cli, metrics, motion

ABSENT = (1 << 64) - 1


def test_taps_and_geometry():
    assert motion.TAPS == R.TAPS == (3571, 16004, 26386, 16004, 3571) and sum(R.TAPS) == 65536
    assert motion.SAD_ABSENT == R.ABSENT == ABSENT and motion.MIN_SIZE == 3
    assert motion.SEGMENT == 4 and motion.TILE_ROWS == 4 * motion.WAVE_ROWS == 64
    assert motion.tile_cols(8) == 992 and motion.tile_cols(10) == 496


@pytest.mark.parametrize("depth", [8, 10])
def test_constant_planes(depth):
    top = (1 << depth) - 1
    for c in (0, 1, 17, top // 2, top):
        b = R.blur(np.full((7, 9), c), depth)
        assert (b == c << (16 - depth)).all()
    c1, c2 = 40 << (depth - 8), 201 << (depth - 8)
    src = np.stack([np.full((6, 5), c1), np.full((6, 5), c2), np.full((6, 5), c2), np.full((6, 5), c2 + 1)])
    sad = R.sad(src, depth, prev=src[0])
    m, m2 = motion.pool(sad, 5, 6, first=False)
    # two constants: |c1 - c2| at 8 bits, |c1 - c2| / 4 at 10 bits; identical frames: 0
    assert m.tolist() == [0.0, abs(c1 - c2) / (1 << (depth - 8)), 0.0, 1.0 / (1 << (depth - 8))]
    assert m2.tolist() == [0.0, 0.0, 0.0, m[3]]
    assert R.motion(sad, 5, 6)[0] == m.tolist()


def test_ramp_keeps_its_interior():
    """The filter is symmetric and sums to 65536: a horizontal ramp is reproduced two samples from the border."""
    x = np.tile(np.arange(0, 200, 5), (6, 1))
    b = R.blur(x, 8)
    assert (b[:, 2:-2] == x[:, 2:-2] * 256).all() and not (b[:, :2] == x[:, :2] * 256).all()
    y = np.tile(np.arange(0, 1000, 25)[:, None], (1, 7))
    b = R.blur(y, 10)
    assert (b[2:-2] == y[2:-2] * 64).all()


def test_stored_samples_above_the_depth_are_clamped():
    rng = np.random.default_rng(3)
    x = rng.integers(0, 1024, (9, 11))
    x[4, 5], x[0, 0], x[8, 10] = 1023, 1023, 1023
    y = x.copy()
    y[4, 5], y[0, 0], y[8, 10] = 1024, 40000, 65535
    assert np.array_equal(R.blur(x, 10), R.blur(y, 10))
    assert R.sad(np.stack([x, y]), 10)[1] == 0


def test_three_by_three_uses_every_mirror():
    x = np.arange(9).reshape(3, 3) * 20
    f = R.TAPS
    # rows and columns -2, -1, 0, 1, 2 around index i of an axis of 3
    mir = lambda i: [[2, 1, 0, 1, 2], [1, 0, 1, 2, 1], [0, 1, 2, 1, 0]][i]
    t = np.array([[(sum(f[k] * x[mir(i)[k], j] for k in range(5)) + 128) >> 8 for j in range(3)] for i in range(3)])
    b = np.array([[(sum(f[k] * t[i, mir(j)[k]] for k in range(5)) + 32768) >> 16 for j in range(3)] for i in range(3)])
    assert np.array_equal(R.blur(x, 8), b)


def test_planes_under_three_are_absent():
    assert R.sad(np.zeros((2, 5, 2)), 8, prev=np.zeros((5, 2))) == [ABSENT, ABSENT]
    assert R.sad(np.zeros((2, 2, 5)), 10) == [ABSENT, ABSENT]
    with pytest.raises(ValueError):
        R.blur(np.zeros((5, 2)), 8)
    m, m2 = motion.pool([ABSENT, ABSENT], 2, 5)
    assert m[0] == 0.0 and math.isnan(m[1]) and math.isnan(m2[0]) and math.isnan(m2[1])


def test_accumulator_bounds():
    for depth, top, tmax in ((8, 255, 65280), (10, 1023, 65472)):
        bounds = {}
        R.blur(np.full((5, 5), top), depth, bounds)
        R.blur(np.full((5, 5), 65535), depth, bounds)  # clamped first
        assert bounds["vacc"] == 65536 * top + (1 << (depth - 1)) <= 65536 * 1023 + 512
        assert bounds["t"] == tmax and bounds["hacc"] == 65536 * tmax + 32768 < 1 << 32 and bounds["b"] == tmax
    # sad of all-0 against all-max of a plane just inside pp_motion's range stays below 2^47
    assert ((1 << 31) - 1) * 65472 < 1 << 47


def test_pool():
    w, h = 4, 3
    s = lambda v: int(v * 256 * w * h)
    m, m2 = motion.pool([ABSENT, s(3), s(1), s(2), s(5)], w, h)
    assert m.tolist() == [0.0, 3.0, 1.0, 2.0, 5.0] and m2.tolist() == [0.0, 1.0, 1.0, 2.0, 5.0]
    m, m2 = motion.pool([s(7), s(3)], w, h, first=False)
    assert m.tolist() == [7.0, 3.0] and m2.tolist() == [3.0, 3.0]
    m, m2 = motion.pool([ABSENT, s(3)], w, h, first=False)
    assert math.isnan(m[0]) and math.isnan(m2[0]) and m2[1] == 3.0
    # the kernel's uint64 read as int64 (-1), and a uint64 array
    m, _ = motion.pool(np.array([-1, s(2)], dtype=np.int64), w, h, first=False)
    assert math.isnan(m[0]) and m[1] == 2.0
    m, _ = motion.pool(np.array([ABSENT, s(2)], dtype=np.uint64), w, h)
    assert m.tolist() == [0.0, 2.0]
    m, m2 = motion.pool([], w, h)
    assert m.shape == (0,) and m2.shape == (0,)
    m, m2 = motion.pool([ABSENT], w, h)
    assert m.tolist() == [0.0] and m2.tolist() == [0.0]
    rm, rm2 = R.motion([ABSENT, s(3), s(1), s(2), s(5)], w, h)
    assert rm == [0.0, 3.0, 1.0, 2.0, 5.0] and rm2 == [0.0, 1.0, 1.0, 2.0, 5.0]


def test_summarize_and_matched():
    w, h = 4, 3
    s = lambda v: int(v * 256 * w * h)
    sad = [ABSENT, s(4), s(2), 0, s(6), s(8)]
    res = motion.summarize(sad, w, h)
    assert res["motion_y"].tolist() == [0.0, 4.0, 2.0, 0.0, 6.0, 8.0]
    assert res["motion2_y"].tolist() == [0.0, 2.0, 0.0, 0.0, 6.0, 8.0]
    assert res["mean"] == {"motion_y": 20.0 / 6, "motion2_y": 16.0 / 6}
    # frame 3 is unmatched: read against the held frame (sad 0), pooled as shown, then left out
    res = motion.summarize(sad, w, h, matched=[True, True, True, False, True, True])
    assert res["motion_y"][:3].tolist() == [0.0, 4.0, 2.0] and math.isnan(res["motion_y"][3])
    assert res["motion2_y"][:3].tolist() == [0.0, 2.0, 0.0] and math.isnan(res["motion2_y"][3])
    assert res["motion2_y"][4:].tolist() == [6.0, 8.0]
    assert res["mean"] == {"motion_y": 20.0 / 5, "motion2_y": 16.0 / 5}
    none = motion.summarize([], w, h)
    assert math.isnan(none["mean"]["motion_y"]) and none["motion_y"].shape == (0,)


def _fake(n=3):
    sse = np.arange(3 * n).reshape(n, 3) + 1
    ssim = np.full((n, 3), 0.5)
    w, h = 33, 33
    sad = [ABSENT] + [int((k + 1) * 256 * w * h) for k in range(1, n)]
    return sse, ssim, sad


def test_metrics_summarize_and_report():
    sse, ssim, sad = _fake()
    plain = metrics.summarize(sse, ssim, "yuv420p", 33, 33)
    res = metrics.summarize(sse, ssim, "yuv420p", 33, 33, motion_terms=sad)
    assert res["motion_y"].tolist() == [0.0, 2.0, 3.0] and res["motion2_y"].tolist() == [0.0, 2.0, 3.0]
    assert res["mean"]["motion_y"] == pytest.approx(5.0 / 3) and res["mean"]["motion2_y"] == pytest.approx(5.0 / 3)
    for k in plain:
        if k != "mean":
            assert np.array_equal(res[k], plain[k], equal_nan=True)
    assert {k: v for k, v in res["mean"].items() if k in plain["mean"]} == plain["mean"]
    assert not [k for k in list(plain) + list(plain["mean"]) if "motion" in k]
    res = metrics.summarize(sse, ssim, "yuv420p", 33, 33, matched=[True, False, True], motion_terms=sad)
    assert math.isnan(res["motion_y"][1]) and res["mean"]["motion_y"] == pytest.approx(1.5)
    out = metrics.report(res, "r.y4m", "d.y4m", per_frame=True)
    assert out["motion_y_frames"] == [0.0, None, 3.0] and out["motion2_y_frames"] == [0.0, None, 3.0]
    assert out["motion_y"] == pytest.approx(1.5)
    old = metrics.report(plain, "r.y4m", "d.y4m", per_frame=True)
    assert not [k for k in old if "motion" in k or "vmaf" in k]
    short = metrics.report(res, "r.y4m", "d.y4m")
    assert "motion_y" in short and "motion2_y" in short and not [k for k in short if k.endswith("_frames")]


def test_cli_flags(monkeypatch, capsys):
    sse, ssim, sad = _fake()
    seen = []
    vt = np.ones((3, 4, 2))
    vt[:, :, 0] = np.array([0.1, 0.2, 0.3, 0.4])[None, :] * np.array([1.0, 2.0, 0.5])[:, None]  # vif_scale_s = num / den
    at = np.ones((3, 4, 6))

    def before(ref, dist, batch=32, flags="bicubic"):  # what `cli metrics` called before PP-MOTION-1
        return metrics.summarize(sse, ssim, "yuv420p", 33, 33)

    def scored(ref, dist, **kw):
        seen.append(kw)
        return metrics.summarize(sse, ssim, "yuv420p", 33, 33, adm_terms=at if kw.get("adm") else None,
                                 vif_terms=vt if kw.get("vif") else None, motion_terms=sad if kw.get("motion") else None)

    monkeypatch.setattr(metrics, "metrics_of_files", before)
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--per-frame"]) == 0
    old = capsys.readouterr().out
    monkeypatch.setattr(metrics, "metrics_of_files", scored)
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--per-frame"]) == 0
    assert capsys.readouterr().out == old and "motion" not in seen[-1]  # the line is unchanged without the flags
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--motion", "--batch", "5"]) == 0
    assert seen[-1] == {"batch": 5, "flags": "bicubic", "motion": True}
    d = json.loads(capsys.readouterr().out)
    assert d["motion_y"] == pytest.approx(5.0 / 3) and d["motion2_y"] == pytest.approx(5.0 / 3)
    assert not [k for k in d if k.endswith("_frames") or "vmaf" in k or "vif" in k or "adm" in k]
    for k, v in json.loads(old).items():
        if not k.endswith("_frames"):
            assert d[k] == v
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--vmaf-features"]) == 0
    assert seen[-1] == {"batch": 32, "flags": "bicubic", "vif": True, "adm": True, "motion": True}
    d = json.loads(capsys.readouterr().out)
    assert d["vmaf_feature_names"] == ["adm2", "motion2", "vif_scale0", "vif_scale1", "vif_scale2", "vif_scale3"]
    assert d["vmaf_feature_names"] == list(metrics.VMAF_FEATURE_NAMES)
    assert d["vmaf_features"] == [d["adm2_y"], d["motion2_y"]] + d["vif_scales_y"] and len(d["vmaf_features"]) == 6
    assert "vmaf_features_frames" not in d and "motion_y" in d and "vif_y" in d
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--vmaf-features", "--per-frame", "--adm"]) == 0
    assert seen[-1] == {"batch": 32, "flags": "bicubic", "vif": True, "adm": True, "motion": True}
    d = json.loads(capsys.readouterr().out)
    rows = d["vmaf_features_frames"]
    assert len(rows) == 3 and all(len(r) == 6 for r in rows)
    for k, r in enumerate(rows):
        assert r == [d["adm2_y_frames"][k], d["motion2_y_frames"][k]] + d["vif_scales_y_frames"][k]
    assert [r[1] for r in rows] == [0.0, 2.0, 3.0]
    assert list(d)[-3:] == ["vmaf_features", "vmaf_feature_names", "vmaf_features_frames"]


def _call(ctx, depth=8, w=20, h=15, src=True, sad=True, sls=32, nsrc=2, n=2, idx=None, prev=False, pls=32):
    L = _native.lib()
    buf = (ctypes.c_uint8 * 64)()  # never read: every call below is refused, or has nothing to do, first
    p = lambda on: ctypes.c_void_p(ctypes.addressof(buf)) if on else None
    ix = None if idx is None else (ctypes.c_int32 * len(idx))(*idx)
    return L.pp_motion(ctx, depth, w, h, p(src), sls, 1024, nsrc, None if ix is None else ctypes.addressof(ix), n,
                       p(prev), pls, p(sad), None)


def test_pp_motion_argument_checks_need_no_gpu():
    L = _native.lib()
    assert "pp_motion" in _native.EXPORTS and L.pp_abi_version() == 7
    ctx = (ctypes.c_uint8 * 256)()  # never dereferenced
    for kw in ({"src": False}, {"sad": False}):
        L.pp_motion(ctx, 9, 1, 1, None, 0, 0, 0, None, 0, None, 0, None, None)
        assert _call(ctx, **kw) == -1 and b"null" in L.pp_last_error()
    assert _call(None) == -1 and b"null" in L.pp_last_error()
    for depth in (9, 12, 16, 0):
        assert _call(ctx, depth=depth) == -1 and b"bitdepth" in L.pp_last_error()
    assert _call(ctx, w=0) == -1 and b"frame" in L.pp_last_error()
    assert _call(ctx, h=-1) == -1 and b"frame" in L.pp_last_error()
    assert _call(ctx, n=-1) == -1 and b"n -1" in L.pp_last_error()
    assert _call(ctx, nsrc=-1, n=0) == -1 and b"nsrc" in L.pp_last_error()
    assert _call(ctx, sls=19) == -1 and b"src plane 0: linesize" in L.pp_last_error()
    assert _call(ctx, prev=True, pls=19) == -1 and b"prev plane 0: linesize" in L.pp_last_error()
    assert _call(ctx, depth=10, sls=39) == -1 and b"linesize" in L.pp_last_error()
    assert _call(ctx, depth=10, sls=41) == -1 and b"2-byte grid" in L.pp_last_error()
    assert _call(ctx, depth=10, sls=40, prev=True, pls=41) == -1 and b"2-byte grid" in L.pp_last_error()
    assert _call(ctx, idx=[0, 2]) == -1 and b"index[1] = 2" in L.pp_last_error()
    assert _call(ctx, idx=[-1, 0]) == -1 and b"index[0] = -1" in L.pp_last_error()
    assert _call(ctx, nsrc=1) == -1 and b"without index" in L.pp_last_error()
    assert _call(ctx, h=64, sls=1 << 25) == -4 and b"2 GiB buffer range" in L.pp_last_error()
    assert _call(ctx, h=64, prev=True, pls=1 << 25) == -4 and b"2 GiB buffer range" in L.pp_last_error()
    assert _call(ctx, n=0) == 0 and _call(ctx, n=0, nsrc=0) == 0  # nothing to do: no HIP call
