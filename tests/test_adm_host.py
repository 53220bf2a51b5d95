"""PP-ADM-1 on the CPU: the filters, contrast sensitivity, sizes and margins of
the spec, the host pooling (pixpath.adm.pool), closed forms of the numpy
restatement (adm_ref), the spread between its evaluations that sets the GPU
bar, the plumbing of `summarize`, `report` and `cli metrics --adm`, and the
argument checks of pp_adm that need no GPU."""
import ctypes
import json
import math

import numpy as np
import pytest

import adm_ref as R
from pixpath import _native, adm, cli, metrics

CONTENTS = ("noise", "small_error", "smooth_noise", "blur", "checker")


def test_filters_and_contrast_sensitivity():
    lo, hi = adm.filters()
    assert np.array_equal(lo, R.filters()[0]) and np.array_equal(hi, R.filters()[1])
    assert abs(lo.sum() - math.sqrt(2)) < 1e-15 and abs(hi.sum()) < 1e-15 and abs((lo * lo).sum() - 1) < 1e-15
    assert abs((lo * hi).sum()) < 1e-16 and abs(lo[0] * lo[2] + lo[1] * lo[3]) < 1e-16  # orthogonal to its shifts
    rf = adm.rf()
    assert rf.shape == (4, 3) and rf[0, 0] == pytest.approx(0.017381, rel=1e-4) and np.array_equal(rf[:, 0], rf[:, 1])
    want = R.rf(np.longdouble)
    assert np.abs(rf / want.astype(np.float64) - 1).max() < 1e-14
    assert np.array_equal(rf, R.rf())


@pytest.mark.parametrize("n,m", [(3, 1), (14, 1), (15, 1), (24, 1), (25, 2), (135, 13), (240, 23), (960, 95)])
def test_margins(n, m):
    assert adm.margin(n) == R.margin(n) == m == max(1, math.floor(0.1 * n - 0.5))


def test_scale_sizes_and_areas():
    assert adm.MIN_SIZE == 33 and adm.scale_sizes(33, 33) == [(17, 17), (9, 9), (5, 5), (3, 3)]
    assert adm.scale_sizes(32, 32) == [(16, 16), (8, 8), (4, 4)] and adm.scale_sizes(35, 37)[3] == (3, 3)
    assert adm.scale_sizes(3, 3) == [] and adm.scale_sizes(2, 2) == [] and adm.scale_sizes(5, 5) == [(3, 3)]
    assert adm.scale_sizes(1920, 1080) == [(960, 540), (480, 270), (240, 135), (120, 68)]
    assert adm.areas(33, 33).tolist() == [225.0, 49.0, 9.0, 1.0]
    a = adm.areas(32, 32)
    assert a[:3].tolist() == [196.0, 36.0, 4.0] and math.isnan(a[3]) and R.areas(32, 32)[:3] == [196, 36, 4]
    assert adm.areas(1920, 1080)[0] == (960 - 190) * (540 - 106)


def test_pool():
    t = np.zeros((4, 6))
    t[:, 0:3] = 1.0
    t[:, 3:6] = 8.0
    w = h = 33
    c = np.cbrt(np.array([225.0, 49.0, 9.0, 1.0]) / 32.0)
    scales, v = adm.pool(t, w, h)
    assert np.allclose(scales, (3 + 3 * c) / (6 + 3 * c), rtol=1e-15) and v == pytest.approx((12 + 3 * c.sum()) / (24 + 3 * c.sum()), rel=1e-15)
    rs, rv = R.pool(t, w, h)
    assert rs == pytest.approx(scales.tolist(), rel=1e-15) and rv == pytest.approx(v, rel=1e-15)
    scales, v = adm.pool(np.zeros((4, 6)), w, h)
    assert scales.tolist() == [1.0] * 4 and v == 1.0
    nan = t.copy()
    nan[3] = np.nan
    scales, v = adm.pool(np.stack([t, nan]), 32, 32)
    assert scales.shape == (2, 4) and np.isnan(scales[:, 3]).all() and np.isnan(v).all() and not np.isnan(scales[:, :3]).any()
    for bad in (np.ones((5, 6)), np.ones((4, 2)), np.ones(24)):
        with pytest.raises(ValueError):
            adm.pool(bad, w, h)


@pytest.mark.parametrize("depth", [8, 10])
def test_identical_planes_are_exactly_one(depth):
    for name in ("noise", "smooth_noise"):
        a = R.content(name, depth, 72, 56, seed=3)[0]
        t = R.terms(a, a, depth)
        assert not np.isnan(t).any() and np.array_equal(t[:, 0:3], t[:, 3:6])
        for o, d in R.levels(a, a, depth):
            assert R.decouple(o, d, R.cos2())[2].all()  # the angle branch everywhere
        scales, v = adm.pool(t, 72, 56)
        assert (scales == 1.0).all() and v == 1.0
        assert R.pool(t, 72, 56) == ([1.0] * 4, 1.0)


def test_half_the_reference():
    """dist = ref / 2 on an even-valued plane: t = o / 2 exactly, the same
    direction, so r = t, a = 0, M = 0 and every numerator sum is 1/8 of the
    denominator's: (D / 2 + 3c) / (D + 3c) per scale, D = sum of the cube roots."""
    a = 2 * R.content("noise", 7, 70, 54, seed=5)[0]
    t = R.terms(a, a // 2, 8)
    assert np.array_equal(t[:, 0:3] * 8, t[:, 3:6])
    d = np.cbrt(t[:, 3:6]).sum(axis=1)
    c = 3 * np.cbrt(adm.areas(70, 54) / 32.0)
    scales, v = adm.pool(t, 70, 54)
    assert np.abs(scales / ((d / 2 + c) / (d + c)) - 1).max() < 1e-15
    assert v == pytest.approx((d / 2 + c).sum() / (d + c).sum(), rel=1e-15)


def test_a_constant_distorted_plane_has_no_detail():
    """t_theta is zero in exact arithmetic: the numerators hold rounding only."""
    a = R.content("noise", 8, 64, 48, seed=2)[0]
    t = R.terms(a, np.full_like(a, 100), 8)
    rf = R.rf()
    for s, area in enumerate(R.areas(64, 48)):
        assert (t[s, 0:3] <= area * (rf[s].max() * R.coef_rounding(s, 255.0)) ** 3).all() and (t[s, 3:6] > 1e-3).all()
    scales, v = adm.pool(t, 64, 48)
    assert (scales < 0.5).all() and v < 0.5


def test_distortions_are_ranked():
    """No value is bounded by 1: in the angle branch r = t, which may exceed o (an enhanced contrast)."""
    vals = {}
    for name in CONTENTS:
        a, b = R.content(name, 8, 64, 48, seed=2)
        scales, v = adm.pool(R.terms(a, b, 8), 64, 48)
        assert (scales > 0).all() and (scales < 1.1).all() and 0 < v < 1.1
        vals[name] = v
    assert vals["small_error"] > 0.9 > vals["blur"] > vals["noise"]


def test_missing_scales_are_nan_from_there_on():
    a, b = R.content("noise", 8, 32, 32)
    t = R.terms(a, b, 8)
    assert not np.isnan(t[:3]).any() and np.isnan(t[3]).all()
    a, b = R.content("noise", 8, 33, 33)
    assert not np.isnan(R.terms(a, b, 8)).any()
    for w, h in ((3, 3), (2, 2), (100, 4)):
        a, b = R.content("noise", 8, w, h)
        assert np.isnan(R.terms(a, b, 8)).all()
    for w, h in ((33, 33), (32, 32), (35, 37), (9, 40), (5, 5)):
        lv = R.levels(np.zeros((h, w), np.int64), np.zeros((h, w), np.int64), 8)
        assert [(o.shape[2], o.shape[1]) for o, _ in lv] == adm.scale_sizes(w, h)


def test_borders_are_mirrored_without_the_edge_sample():
    lo, hi = R.filters()
    for w in (6, 7):  # even: the last coefficient reads n -> n - 2; odd: n -> n - 2 and n + 1 -> n - 3
        p = np.arange(3.0 * w).reshape(3, w) ** 2
        A = R.bands(p)[0]
        assert A.shape == (2, (w + 1) // 2)
        first = lo @ p[[1, 0, 1, 2]][:, [1, 0, 1, 2]] @ lo
        n = w
        cols = [n - 3, n - 2, n - 1, n - 2] if w % 2 == 0 else [n - 2, n - 1, n - 2, n - 3]
        last = lo @ p[[1, 0, 1, 2]][:, cols] @ lo
        assert A[0, 0] == pytest.approx(first, rel=1e-14) and A[0, -1] == pytest.approx(last, rel=1e-14)


def test_10_bit_is_the_8_bit_scale():
    a, b = R.content("small_error", 8, 40, 35, seed=4)
    assert np.array_equal(R.terms(a, b, 8), R.terms(a * 4, b * 4, 10))  # x = sample / 4, exact


def test_near_branch_counter():
    a, b = R.content("small_error", 8, 40, 35, seed=4)
    assert R.near_branch(a, b, 8) == [0, 0, 0, 0]
    c = np.full((35, 40), 100)
    assert R.near_branch(a, c, 8) == [20 * 18, 10 * 9, 5 * 5, 3 * 3]  # a flat side has no direction
    yy, xx = np.mgrid[0:35, 0:40]
    pure = np.where((xx + yy) & 1, 255, 0)
    assert R.near_branch(pure, 255 - pure, 8)[0] == 20 * 18  # H = V = 0: a pure checkerboard neither


@pytest.mark.parametrize("depth", [8, 10])
def test_three_evaluations_agree(depth):
    """The direct fp64 evaluation, a separable fp64 one and the direct one in
    long double lie within 2.08e-13 relative of each other on every sum above
    the floor; an fp32 evaluation does not come within 1e-6."""
    worst, least32 = 0.0, math.inf
    for name in CONTENTS:
        a, b = R.content(name, depth, 183, 178, seed=3)
        assert not any(R.near_branch(a, b, depth))
        d, s = R.terms(a, b, depth), R.terms(a, b, depth, separable=True)
        l = R.terms(a, b, depth, np.longdouble).astype(np.float64)
        f = R.terms(a, b, depth, np.float32).astype(np.float64)
        ok = np.abs(l) > 1e-30  # a numerator may be exactly zero: every position under its threshold
        assert np.array_equal(d[~ok], l[~ok]) and np.array_equal(s[~ok], l[~ok])
        worst = max(worst, np.abs(d[ok] / l[ok] - 1).max(), np.abs(s[ok] / l[ok] - 1).max(), np.abs(s[ok] / d[ok] - 1).max())
        least32 = min(least32, np.abs(f[ok] / l[ok] - 1).max())
    print("%d bit: spread %.3e, fp32 off by at least %.3e" % (depth, worst, least32))
    assert worst <= 2.08e-13 and least32 > 1e-6


def _fake(n=3):
    sse = np.array([[640, 64, 16]] * n, np.int64)
    ssim = np.array([[0.75, 0.5, 0.5]] * n)
    t = np.zeros((n, 4, 6))  # no coefficients at all: every pooled value is 3c / 3c
    t[1:, :, 3:6] = 1.0
    return sse, ssim, t


def _half():
    """What _fake's frames 1 and 2 pool to at 33 x 33, per scale and together."""
    c = 3 * np.cbrt(np.array([225.0, 49.0, 9.0, 1.0]) / 32.0)
    return (c / (3 + c)).tolist(), float(c.sum() / (12 + c.sum()))


def test_summarize_only_when_asked():
    sse, ssim, t = _fake()
    hs, hv = _half()
    plain = metrics.summarize(sse, ssim, "yuv420p", 33, 33)
    assert not [k for k in list(plain) + list(plain["mean"]) if "adm" in k]
    res = metrics.summarize(sse, ssim, "yuv420p", 33, 33, adm_terms=t)
    assert res["adm2_y"].tolist() == pytest.approx([1.0, hv, hv]) and res["adm_scales_y"].shape == (3, 4)
    assert res["mean"]["adm2_y"] == pytest.approx((1 + 2 * hv) / 3)
    assert res["mean"]["adm_scales_y"] == pytest.approx([(1 + 2 * x) / 3 for x in hs])
    for k in plain:
        if k != "mean":
            assert np.array_equal(res[k], plain[k], equal_nan=True)
    assert {k: v for k, v in res["mean"].items() if k in plain["mean"]} == plain["mean"]
    res = metrics.summarize(sse, ssim, "yuv420p", 33, 33, matched=[False, True, True], adm_terms=t)
    assert np.isnan(res["adm2_y"][0]) and res["mean"]["adm2_y"] == pytest.approx(hv) and np.isnan(res["adm_scales_y"][0]).all()
    small = metrics.summarize(sse, ssim, "yuv420p", 32, 32, adm_terms=np.where(np.arange(4)[None, :, None] == 3, np.nan, t))
    assert np.isnan(small["adm2_y"]).all() and math.isnan(small["mean"]["adm2_y"]) and not np.isnan(small["adm_scales_y"][:, :3]).any()
    none = metrics.summarize(sse[:0], ssim[:0], "yuv420p", 33, 33, adm_terms=np.zeros((0, 4, 6)))
    assert math.isnan(none["mean"]["adm2_y"]) and none["adm2_y"].shape == (0,)
    all3 = metrics.summarize(sse, ssim, "yuv420p", 33, 33, ms_terms=np.ones((3, 5, 2)), vif_terms=np.ones((3, 4, 2)), adm_terms=t)
    assert "ms_ssim_y" in all3 and "vif_y" in all3 and "adm2_y" in all3


def test_cli_flag(monkeypatch, capsys):
    sse, ssim, t = _fake()
    hs, hv = _half()
    seen = []

    def before(ref, dist, batch=32, flags="bicubic"):  # what `cli metrics` called before PP-ADM-1
        return metrics.summarize(sse, ssim, "yuv420p", 33, 33)

    def scored(ref, dist, **kw):
        seen.append(kw)
        return metrics.summarize(sse, ssim, "yuv420p", 33, 33, adm_terms=t if kw.get("adm") else None,
                                 vif_terms=np.ones((3, 4, 2)) if kw.get("vif") else None,
                                 ms_terms=np.ones((3, 5, 2)) if kw.get("ms_ssim") else None)

    monkeypatch.setattr(metrics, "metrics_of_files", before)
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--per-frame"]) == 0
    old = capsys.readouterr().out
    monkeypatch.setattr(metrics, "metrics_of_files", scored)
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--per-frame"]) == 0
    assert capsys.readouterr().out == old and "adm" not in seen[-1]  # the line is unchanged without the flag
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--adm", "--crop", "8x8", "--batch", "5"]) == 0
    assert seen[-1] == {"batch": 5, "flags": "bicubic", "crop": (8, 8), "adm": True}
    d = json.loads(capsys.readouterr().out)
    assert d["adm2_y"] == pytest.approx((1 + 2 * hv) / 3) and d["adm_scales_y"] == pytest.approx([(1 + 2 * x) / 3 for x in hs])
    assert "adm2_y_frames" not in d and "vif_y" not in d
    for k, v in json.loads(old).items():
        if not k.endswith("_frames"):
            assert d[k] == v
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--adm", "--vif", "--ms-ssim", "--per-frame"]) == 0
    assert seen[-1] == {"batch": 32, "flags": "bicubic", "adm": True, "vif": True, "ms_ssim": True}
    d = json.loads(capsys.readouterr().out)
    assert d["adm2_y_frames"] == pytest.approx([1.0, hv, hv]) and d["adm_scales_y_frames"][1] == pytest.approx(hs)
    assert d["ms_ssim_y"] == 1.0 and d["vif_y"] == 1.0
    t[1, 3] = np.nan
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--adm", "--per-frame"]) == 0
    d = json.loads(capsys.readouterr().out)
    assert d["adm2_y_frames"][1] is None and d["adm_scales_y_frames"][1][3] is None and d["adm_scales_y_frames"][1][0] is not None


def _call(ctx, depth=8, w=20, h=15, ref=True, dist=True, out=True, rls=32, dls=32, nref=2, ndist=2, idx=None):
    L = _native.lib()
    buf = (ctypes.c_uint8 * 64)()  # never read: every call below is refused, or has nothing to do, first
    p = lambda on: ctypes.c_void_p(ctypes.addressof(buf)) if on else None
    ix = None if idx is None else (ctypes.c_int32 * len(idx))(*idx)
    return L.pp_adm(ctx, depth, w, h, p(ref), rls, 1024, nref, p(dist), dls, 1024, ndist,
                    None if ix is None else ctypes.addressof(ix), p(out), None)


def test_pp_adm_argument_checks_need_no_gpu():
    L = _native.lib()
    assert "pp_adm" in _native.EXPORTS and L.pp_abi_version() == 7
    ctx = (ctypes.c_uint8 * 256)()  # never dereferenced
    for kw in ({"ref": False}, {"dist": False}, {"out": False}):
        L.pp_adm(ctx, 9, 1, 1, None, 0, 0, 0, None, 0, 0, 0, None, None, None)
        assert _call(ctx, **kw) == -1 and b"null" in L.pp_last_error()
    assert _call(None) == -1 and b"null" in L.pp_last_error()
    for depth in (9, 12, 16, 0):
        assert _call(ctx, depth=depth) == -1 and b"bitdepth" in L.pp_last_error()
    assert _call(ctx, w=0) == -1 and b"frame" in L.pp_last_error()
    assert _call(ctx, h=-1) == -1 and b"frame" in L.pp_last_error()
    assert _call(ctx, ndist=-1) == -1 and b"ndist" in L.pp_last_error()
    assert _call(ctx, nref=-1) == -1 and b"nref" in L.pp_last_error()
    assert _call(ctx, rls=19) == -1 and b"ref plane 0: linesize" in L.pp_last_error()
    assert _call(ctx, dls=19) == -1 and b"dist plane 0: linesize" in L.pp_last_error()
    assert _call(ctx, depth=10, rls=40, dls=39) == -1 and b"linesize" in L.pp_last_error()
    assert _call(ctx, depth=10, rls=41, dls=40) == -1 and b"2-byte grid" in L.pp_last_error()
    assert _call(ctx, idx=[0, 2]) == -1 and b"ref_index[1] = 2" in L.pp_last_error()
    assert _call(ctx, idx=[-1, 0]) == -1 and b"ref_index[0] = -1" in L.pp_last_error()
    assert _call(ctx, nref=1) == -1 and b"without ref_index" in L.pp_last_error()
    assert _call(ctx, h=64, dls=1 << 25) == -4 and b"2 GiB buffer range" in L.pp_last_error()
    assert _call(ctx, ndist=0) == 0 and _call(ctx, ndist=0, nref=0) == 0  # nothing to do: no HIP call
