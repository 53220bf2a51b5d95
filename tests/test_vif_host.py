"""PP-VIF-1 on the CPU: the windows and sizes of the spec, the host pooling
(pixpath.vif.pool), closed forms of the numpy restatement (vif_ref), the
plumbing of `summarize`, `report` and `cli metrics --vif`, and the argument
checks of pp_vif that need no GPU."""
import ctypes
import json
import math

import numpy as np
import pytest

import vif_ref as R
from pixpath import _native, cli, metrics, vif


def test_windows():
    assert vif.SCALES == R.SCALES == 4 and vif.TAPS == R.TAPS == (17, 9, 5, 3) and vif.MIN_SIZE == 16
    for s, n in enumerate(vif.TAPS):
        g = vif.window(s)
        assert g.shape == (n,) and np.array_equal(g, R.window(s))
        assert abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1])
        sigma = n / 5.0
        assert g[n // 2] / g[n // 2 - 1] == pytest.approx(math.exp(1 / (2 * sigma * sigma)), rel=1e-14)


def test_scale_sizes():
    assert vif.scale_sizes(16, 16) == [(16, 16), (8, 8), (4, 4), (2, 2)]
    assert vif.scale_sizes(15, 16) == [(15, 16), (7, 8), (3, 4)] and vif.scale_sizes(16, 15) == [(16, 15), (8, 7), (4, 3)]
    assert vif.scale_sizes(37, 29) == [(37, 29), (18, 14), (9, 7), (4, 3)]  # floor at every level
    assert vif.scale_sizes(8, 100) == [] and vif.scale_sizes(9, 9) == [(9, 9)]
    assert vif.scale_sizes(10, 10) == [(10, 10), (5, 5)] and vif.scale_sizes(1920, 1080)[3] == (240, 135)
    for w, h in ((16, 16), (15, 16), (37, 29), (9, 9), (8, 100)):
        lv = R.levels(np.zeros((h, w), np.int64), 8)
        assert [(p.shape[1], p.shape[0]) for p in lv] == vif.scale_sizes(w, h)


def test_pool():
    t = np.array([[1.0, 2.0], [3.0, 4.0], [0.5, 0.0], [0.0, 8.0]])
    scales, v = vif.pool(t)
    assert scales.tolist() == [0.5, 0.75, 1.0, 0.0] and v == 4.5 / 14.0
    rs, rv = R.pool(t)
    assert rs == scales.tolist() and rv == v
    zero = np.zeros((4, 2))
    scales, v = vif.pool(zero)
    assert scales.tolist() == [1.0] * 4 and v == 1.0 and R.pool(zero) == ([1.0] * 4, 1.0)
    nan = t.copy()
    nan[3] = np.nan
    scales, v = vif.pool(np.stack([t, nan]))
    assert scales.shape == (2, 4) and v.shape == (2,)
    assert scales[1, :3].tolist() == [0.5, 0.75, 1.0] and np.isnan(scales[1, 3]) and np.isnan(v[1]) and v[0] == 4.5 / 14.0
    assert math.isnan(R.pool(nan)[1]) and math.isnan(R.pool(nan)[0][3])
    for bad in (np.ones((5, 2)), np.ones((4, 3)), np.ones(8)):
        with pytest.raises(ValueError):
            vif.pool(bad)


def _blocky(depth, w, h, seed):
    """Noise held over 8 x 8 blocks: its variance survives the three low-pass
    stages, so sigma1^2 stays far above 2 on every scale."""
    rng = np.random.default_rng(seed)
    top = (1 << depth) - 1
    return np.kron(rng.integers(0, top + 1, (h // 8 + 1, w // 8 + 1)), np.ones((8, 8), np.int64))[:h, :w]


@pytest.mark.parametrize("depth", [8, 10])
def test_identical_planes_are_within_1e_9_of_one(depth):
    a = _blocky(depth, 72, 56, seed=3)
    for s, (pa, pb) in enumerate(zip(R.levels(a, depth), R.levels(a, depth))):
        assert R.moments(pa, pb, s)[0].min() > 2.0  # no position takes the flat-area branch
    t = R.terms(a, a, depth)
    scales, v = vif.pool(t)
    assert not np.isnan(t).any() and np.abs(scales - 1).max() < 1e-9 and abs(v - 1) < 1e-9
    assert (t[:, 0] < t[:, 1]).all()  # eps keeps g just under 1: below 1, not equal


def test_a_distorted_plane_lies_between_0_and_1():
    for name in ("small_error", "smooth_noise", "noise"):
        a, b = R.content(name, 8, 64, 48, seed=2)
        scales, v = vif.pool(R.terms(a, b, 8))
        assert (scales > 0).all() and (scales < 1).all() and 0 < v < 1
    weak = vif.pool(R.terms(*R.content("small_error", 8, 64, 48, seed=2), 8))[1]
    strong = vif.pool(R.terms(*R.content("noise", 8, 64, 48, seed=2), 8))[1]
    assert weak > 0.5 > strong


@pytest.mark.parametrize("depth,p,q", [(8, 200, 0), (8, 0, 0), (10, 1023, 0), (8, 200, 77), (10, 300, 301)])
def test_constant_planes(depth, p, q):
    """sigma1^2 < 2 everywhere: den = 1 and num = 1 - sigma2^2 * 4 / 65025 at
    every position.  A zero distorted plane has sigma2^2 = 0 exactly, so both
    sums are the position count exactly; a non-zero constant leaves the
    rounding of E[y^2] - mu2^2, at most 2 * 65025 * (2 * 17 + 2) * 2^-53 =
    5.2e-10, in num: within 4e-14 relative."""
    w, h = 21, 18
    t = R.terms(np.full((h, w), p), np.full((h, w), q), depth)
    count = np.array([ws * hs for ws, hs in vif.scale_sizes(w, h)], dtype=np.float64)
    assert count.tolist() == [378, 90, 20, 4]
    assert np.array_equal(t[:, 1], count)
    if q == 0:
        assert np.array_equal(t[:, 0], count)
    assert np.abs(t[:, 0] / count - 1).max() <= 4e-14
    assert vif.pool(t)[1] == pytest.approx(1.0, abs=4e-14)


def test_missing_scales_are_nan_from_there_on():
    a, b = R.content("noise", 8, 15, 16)
    t = R.terms(a, b, 8)
    assert not np.isnan(t[:3]).any() and np.isnan(t[3]).all()
    a, b = R.content("noise", 8, 100, 8)  # scale 0 needs 9 rows
    assert np.isnan(R.terms(a, b, 8)).all()
    a, b = R.content("noise", 8, 16, 16)
    assert not np.isnan(R.terms(a, b, 8)).any()


def test_borders_are_mirrored_without_the_edge_sample():
    p = np.arange(30.0).reshape(5, 6)
    q = np.pad(p, 2, mode="reflect")
    assert q[0, 2] == p[2, 0] and q[1, 2] == p[1, 0] and q[2, 0] == p[0, 2] and q[-1, -1] == p[2, 3]
    one = np.zeros((9, 9))
    one[0, 0] = 1.0  # the corner sample is counted once: weight g[r]^2 at (0, 0), and (1, 1) sees it once
    g = R.window(1)
    f = R.filt(one, 1)
    assert f[0, 0] == g[4] * g[4] and f[1, 1] == pytest.approx(g[3] * g[3])


def test_10_bit_is_the_8_bit_scale():
    a, b = R.content("small_error", 8, 40, 33, seed=4)
    assert np.array_equal(R.terms(a, b, 8), R.terms(a * 4, b * 4, 10))  # x = sample / 4, exact


def test_near_branch_counter():
    a, b = R.content("small_error", 8, 40, 33, seed=4)
    assert R.near_branch(a, b, 8) == [0, 0, 0, 0]
    c = np.full((33, 40), 100)
    assert R.near_branch(c, c, 8) == [40 * 33, 20 * 16, 10 * 8, 5 * 4]  # sigma12 = 0 everywhere


@pytest.mark.parametrize("depth", [8, 10])
def test_separable_and_direct_agree(depth):
    """terms_separable (what tools/vif_bench.py checks the GPU against) and the
    direct form sum the same fp64 products in another order.  The largest
    relative difference of a sum on these inputs is 3.3e-13 (3.0e-13 at 8 bits,
    3.3e-13 at 10: the variances are differences of nearly equal numbers, which
    magnifies the rounding of either order); the bar is 8 times that, for numpy
    builds whose einsum or vector width sums in yet another order.  A wrong tap
    or a window off by one moves a sum by 1e-3 or more."""
    cases = (("small_error", 40, 33, 4), ("small_error", 37, 29, 1),  # odd height; odd width and height
             ("noise", 15, 16, 0), ("small_error", 9, 9, 3),  # scale 3 / scales 1 to 3 do not exist
             ("smooth_noise", 72, 56, 2), ("noise", 64, 48, 2))
    for name, w, h, seed in cases:
        a, b = R.content(name, depth, w, h, seed=seed)
        assert not any(R.near_branch(a, b, depth)), (name, w, h)  # no position where num jumps
        d, s = R.terms(a, b, depth), R.terms_separable(a, b, depth)
        there = ~np.isnan(d)
        assert np.array_equal(there, ~np.isnan(s)) and there[:len(vif.scale_sizes(w, h))].all()
        assert there.all(axis=1).sum() == there.any(axis=1).sum() == len(vif.scale_sizes(w, h))
        assert np.abs(s[there] / d[there] - 1).max() <= 8 * 3.3e-13, (name, w, h)


def _fake(n=3):
    sse = np.array([[640, 64, 16]] * n, np.int64)
    ssim = np.array([[0.75, 0.5, 0.5]] * n)
    t = np.ones((n, 4, 2))
    t[:, :, 0] = 0.5
    t[0, :, 0] = 1.0
    return sse, ssim, t


def test_summarize_only_when_asked():
    sse, ssim, t = _fake()
    plain = metrics.summarize(sse, ssim, "yuv420p", 16, 16)
    assert not [k for k in list(plain) + list(plain["mean"]) if "vif" in k]
    res = metrics.summarize(sse, ssim, "yuv420p", 16, 16, vif_terms=t)
    assert res["vif_y"].tolist() == [1.0, .5, .5] and res["vif_scales_y"].shape == (3, 4)
    assert res["mean"]["vif_y"] == pytest.approx(2 / 3) and res["mean"]["vif_scales_y"] == [pytest.approx(2 / 3)] * 4
    for k in plain:
        if k != "mean":
            assert np.array_equal(res[k], plain[k], equal_nan=True)
    assert {k: v for k, v in res["mean"].items() if k in plain["mean"]} == plain["mean"]
    t[2, 3] = np.nan  # a frame without scale 3, and an unmatched one, are left out of the clip value
    res = metrics.summarize(sse, ssim, "yuv420p", 16, 16, matched=[False, True, True], vif_terms=t)
    assert np.isnan(res["vif_y"][[0, 2]]).all() and res["mean"]["vif_y"] == .5
    assert res["vif_scales_y"][2, :3].tolist() == [.5] * 3 and np.isnan(res["vif_scales_y"][0]).all()
    none = metrics.summarize(sse[:0], ssim[:0], "yuv420p", 16, 16, vif_terms=np.zeros((0, 4, 2)))
    assert math.isnan(none["mean"]["vif_y"]) and none["vif_y"].shape == (0,)
    both = metrics.summarize(sse, ssim, "yuv420p", 16, 16, ms_terms=np.ones((3, 5, 2)), vif_terms=t)
    assert "ms_ssim_y" in both and "vif_y" in both


def test_cli_flag(monkeypatch, capsys):
    sse, ssim, t = _fake()
    seen = []

    def before(ref, dist, batch=32, flags="bicubic"):  # what `cli metrics` called before PP-VIF-1
        return metrics.summarize(sse, ssim, "yuv420p", 16, 16)

    def scored(ref, dist, **kw):
        seen.append(kw)
        return metrics.summarize(sse, ssim, "yuv420p", 16, 16, vif_terms=t if kw.get("vif") else None,
                                 ms_terms=np.ones((3, 5, 2)) if kw.get("ms_ssim") else None)

    monkeypatch.setattr(metrics, "metrics_of_files", before)
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--per-frame"]) == 0
    old = capsys.readouterr().out
    monkeypatch.setattr(metrics, "metrics_of_files", scored)
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--per-frame"]) == 0
    assert capsys.readouterr().out == old and "vif" not in seen[-1]  # the line is unchanged without the flag
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--vif", "--crop", "8x8", "--batch", "5"]) == 0
    assert seen[-1] == {"batch": 5, "flags": "bicubic", "crop": (8, 8), "vif": True}
    d = json.loads(capsys.readouterr().out)
    assert d["vif_y"] == pytest.approx(2 / 3) and d["vif_scales_y"] == [pytest.approx(2 / 3)] * 4
    assert "vif_y_frames" not in d and "ms_ssim_y" not in d
    for k, v in json.loads(old).items():
        if not k.endswith("_frames"):
            assert d[k] == v
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--vif", "--ms-ssim", "--per-frame"]) == 0
    assert seen[-1] == {"batch": 32, "flags": "bicubic", "vif": True, "ms_ssim": True}
    d = json.loads(capsys.readouterr().out)
    assert d["vif_y_frames"] == [1.0, .5, .5] and d["vif_scales_y_frames"][1] == [.5] * 4 and d["ms_ssim_y"] == 1.0
    t[1, 3] = np.nan
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--vif", "--per-frame"]) == 0
    d = json.loads(capsys.readouterr().out)
    assert d["vif_y_frames"][1] is None and d["vif_scales_y_frames"][1] == [.5, .5, .5, None]


def _call(ctx, depth=8, w=20, h=15, ref=True, dist=True, out=True, rls=32, dls=32, nref=2, ndist=2, idx=None):
    L = _native.lib()
    buf = (ctypes.c_uint8 * 64)()  # never read: every call below is refused, or has nothing to do, first
    p = lambda on: ctypes.c_void_p(ctypes.addressof(buf)) if on else None
    ix = None if idx is None else (ctypes.c_int32 * len(idx))(*idx)
    return L.pp_vif(ctx, depth, w, h, p(ref), rls, 1024, nref, p(dist), dls, 1024, ndist,
                    None if ix is None else ctypes.addressof(ix), p(out), None)


def test_pp_vif_argument_checks_need_no_gpu():
    L = _native.lib()
    assert "pp_vif" in _native.EXPORTS and L.pp_abi_version() == 7
    ctx = (ctypes.c_uint8 * 256)()  # never dereferenced
    for kw in ({"ref": False}, {"dist": False}, {"out": False}):
        L.pp_vif(ctx, 9, 1, 1, None, 0, 0, 0, None, 0, 0, 0, None, None, None)
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
