"""PP-MSSSIM-1 on the CPU: the closed forms of the spec against its numpy
restatement (msssim_ref), the host pooling (pixpath.msssim.pool), and the
plumbing of `summarize`, `report` and `cli metrics --ms-ssim`.  No GPU."""
import json
import math

import numpy as np
import pytest

import msssim_ref as R
from pixpath import cli, metrics, msssim


def test_constants():
    assert msssim.EXPONENTS == R.EXPONENTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
    assert msssim.SCALES == 5 and msssim.WINDOW == 11 and msssim.MIN_SIZE == 176
    g = msssim.window()
    assert np.array_equal(g, R.window()) and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1])
    assert g[5] / g[4] == pytest.approx(math.exp(1 / 4.5))


@pytest.mark.parametrize("depth", [8, 10])
def test_identical_planes_give_one(depth):
    a, _ = R.content("noise", depth, 183, 178, seed=3)
    t = R.terms(a, a, depth)
    assert np.array_equal(t, np.ones((5, 2)))
    assert R.pool(t) == 1.0 and msssim.pool(t) == 1.0


@pytest.mark.parametrize("depth,p,q", [(8, 200, 40), (10, 1023, 0), (10, 300, 301)])
def test_constant_against_constant(depth, p, q):
    a, b = np.full((176, 176), p), np.full((176, 176), q)
    c1, _ = R.constants(depth)
    want = (2 * p * q + c1) / (p * p + q * q + c1)
    t = R.terms(a, b, depth)
    assert np.allclose(t[:, 0], 1.0, rtol=0, atol=1e-9) and np.allclose(t[:, 1], want, rtol=0, atol=1e-9)
    assert msssim.pool(t) == pytest.approx(want ** 0.1333, abs=1e-9)


def test_trailing_rows_and_columns_take_no_part():
    a, b = R.content("smooth_noise", 8, 191, 183, seed=5)
    t = R.terms(a, b, 8)
    a2, b2 = a.copy(), b.copy()
    # scale 4 uses 176 x 176; columns 176 .. 190 and rows 176 .. 182 are outside every scale-4 block
    a2[:, 176:] = 0
    b2[176:, :] = 255
    t2 = R.terms(a2, b2, 8)
    assert np.array_equal(t2[4], t[4]) and not np.array_equal(t2[0], t[0])
    # scale 1 drops only the last column and row
    a3 = a.copy()
    a3[:, 190] = 255 - a3[:, 190]
    a3[182, :] = 255 - a3[182, :]
    t3 = R.terms(a3, b, 8)
    assert np.array_equal(t3[1:], t[1:]) and not np.array_equal(t3[0], t[0])


def test_smallest_sizes():
    for w, h in ((175, 176), (176, 175)):
        a, b = R.content("small_error", 8, w, h, seed=1)
        t = R.terms(a, b, 8)
        assert np.isnan(t[4]).all() and not np.isnan(t[:4]).any()
        assert math.isnan(R.pool(t)) and np.isnan(msssim.pool(t))
    a, b = R.content("small_error", 8, 176, 176, seed=1)
    assert R.level(a, 4).shape == (11, 11)  # exactly one scale-4 window
    t = R.terms(a, b, 8)
    assert not np.isnan(t).any() and 0 < msssim.pool(t) < 1
    a, b = R.content("noise", 8, 10, 10)
    assert np.isnan(R.terms(a, b, 8)).all()
    a, b = R.content("noise", 8, 11, 11)
    t = R.terms(a, b, 8)
    assert not np.isnan(t[0]).any() and np.isnan(t[1:]).all()


def test_pool():
    t = np.ones((5, 2))
    t[:, 0] = [.9, .8, .7, .6, .123]   # cs of scale 4 takes no part
    t[:, 1] = [.1, .2, .3, .4, .5]     # of the ssim column only scale 4 does
    want = .9 ** .0448 * .8 ** .2856 * .7 ** .3001 * .6 ** .2363 * .5 ** .1333
    assert msssim.pool(t) == pytest.approx(want, rel=1e-15) and R.pool(t) == pytest.approx(want, rel=1e-15)
    neg = t.copy()
    neg[1, 0] = -0.5  # a negative mean is clamped to 0: the product is 0, not NaN
    assert msssim.pool(neg) == 0.0 and R.pool(neg) == 0.0
    neg = t.copy()
    neg[4, 1] = -1e-3
    assert msssim.pool(neg) == 0.0
    nan = t.copy()
    nan[4] = np.nan
    both = msssim.pool(np.stack([t, nan, neg]))
    assert both.shape == (3,) and both[0] == pytest.approx(want) and np.isnan(both[1]) and both[2] == 0.0
    a, b = R.content("checker16", 8, 183, 178)
    assert (R.terms(a, b, 8)[:, 0] < 0).all() and msssim.pool(R.terms(a, b, 8)) == 0.0
    with pytest.raises(ValueError):
        msssim.pool(np.ones((4, 2)))


@pytest.mark.parametrize("depth", [8, 10])
def test_separable_and_direct_agree(depth):
    """Any fp64 order of summation passes the 1e-9 bar by a wide margin, an
    fp32 evaluation does not (DESIGN.md's accuracy argument)."""
    worst = worst32 = 0.0
    for name in R.CONTENTS:
        a, b = R.content(name, depth, 183, 178, seed=1)
        d, s = R.terms(a, b, depth), R.terms_separable(a, b, depth)
        worst = max(worst, np.abs(d - s).max(), np.abs(d - R.terms_longdouble(a, b, depth)).max())
        worst32 = max(worst32, np.abs(d - R.terms(a, b, depth, np.float32)).max())
    print("%d bit: fp64 evaluations differ by %.2e, fp32 by %.2e" % (depth, worst, worst32))
    assert worst < 1e-12 and worst32 > 1e-6


HALF = .5 ** sum(R.EXPONENTS)  # every term .5; the paper's exponents add up to 1.0001


def _fake(n=3):
    sse = np.array([[640, 64, 16]] * n, np.int64)
    ssim = np.array([[0.75, 0.5, 0.5]] * n)
    t = np.ones((n, 5, 2)) * 0.5
    t[0] = 1.0
    return sse, ssim, t


def test_summarize_only_when_asked():
    sse, ssim, t = _fake()
    plain = metrics.summarize(sse, ssim, "yuv420p", 16, 16)
    assert not [k for k in plain if "ms_ssim" in k or "gauss" in k or "scales" in k]
    assert not [k for k in plain["mean"] if "ms_ssim" in k or "gauss" in k]
    res = metrics.summarize(sse, ssim, "yuv420p", 16, 16, ms_terms=t)
    assert res["ms_ssim_y"].tolist() == [1.0, pytest.approx(HALF, rel=1e-14), pytest.approx(HALF, rel=1e-14)]
    assert res["ssim_gauss_y"].tolist() == [1.0, .5, .5] and res["cs_scales_y"].shape == (3, 5)
    assert res["mean"]["ms_ssim_y"] == pytest.approx((1 + 2 * HALF) / 3) and res["mean"]["ssim_gauss_y"] == pytest.approx(2 / 3)
    for k in plain:
        if k != "mean":
            assert np.array_equal(res[k], plain[k], equal_nan=True)
    assert {k: v for k, v in res["mean"].items() if k in plain["mean"]} == plain["mean"]
    # an unmatched frame, and a frame too small for scale 4, are left out of the clip value
    t[2, 4] = np.nan
    res = metrics.summarize(sse, ssim, "yuv420p", 16, 16, matched=[False, True, True], ms_terms=t)
    assert np.isnan(res["ms_ssim_y"][[0, 2]]).all() and res["mean"]["ms_ssim_y"] == pytest.approx(HALF)
    assert np.isnan(res["ssim_gauss_y"][0]) and res["mean"]["ssim_gauss_y"] == .5
    none = metrics.summarize(sse[:0], ssim[:0], "yuv420p", 16, 16, ms_terms=np.zeros((0, 5, 2)))
    assert math.isnan(none["mean"]["ms_ssim_y"]) and none["ms_ssim_y"].shape == (0,)


def test_cli_flag(monkeypatch, capsys):
    sse, ssim, t = _fake()
    seen = []

    def before(ref, dist, batch=32, flags="bicubic"):  # what `cli metrics` called before PP-MSSSIM-1
        return metrics.summarize(sse, ssim, "yuv420p", 16, 16)

    def scored(ref, dist, **kw):
        seen.append(kw)
        return metrics.summarize(sse, ssim, "yuv420p", 16, 16, ms_terms=t if kw.get("ms_ssim") else None)

    monkeypatch.setattr(metrics, "metrics_of_files", before)
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--per-frame"]) == 0
    old = capsys.readouterr().out
    monkeypatch.setattr(metrics, "metrics_of_files", scored)
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--per-frame"]) == 0
    assert capsys.readouterr().out == old and "ms_ssim" not in seen[-1]  # the line is unchanged without the flag
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--ms-ssim", "--crop", "8x8", "--batch", "5"]) == 0
    assert seen[-1] == {"batch": 5, "flags": "bicubic", "crop": (8, 8), "ms_ssim": True}
    d = json.loads(capsys.readouterr().out)
    assert d["ms_ssim_y"] == pytest.approx((1 + 2 * HALF) / 3) and d["ssim_gauss_y"] == pytest.approx(2 / 3)
    assert "ms_ssim_y_frames" not in d
    for k, v in json.loads(old).items():
        if not k.endswith("_frames"):
            assert d[k] == v
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--ms-ssim", "--per-frame"]) == 0
    d = json.loads(capsys.readouterr().out)
    assert d["ms_ssim_y_frames"] == [1.0, pytest.approx(HALF), pytest.approx(HALF)] and d["ssim_gauss_y_frames"] == [1, .5, .5]
    assert d["cs_scales_y_frames"][1] == [.5] * 5 and len(d["ssim_scales_y_frames"]) == 3
    t[1, 4] = np.nan
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--ms-ssim", "--per-frame"]) == 0
    d = json.loads(capsys.readouterr().out)
    assert d["ms_ssim_y_frames"][1] is None and d["ssim_scales_y_frames"][1][4] is None
