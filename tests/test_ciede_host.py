"""Spec PP-CIEDE-1 on the CPU: the numpy restatement (tests/ciede_ref.py)
against the data pairs Sharma, Wu and Dalal published, the properties the spec
states, the host side (pixpath.ciede.pool, the JSON keys of `cli metrics
--ciede`) and the argument checks of pp_ciede that need no GPU."""
import ctypes
import json
import math

import numpy as np
import pytest

import ciede_ref
from pixpath import _native, ciede, cli, formats, metrics

# (L1, a1, b1 | L2, a2, b2 -> dE00) from the table of Sharma, Wu, Dalal 2005
SHARMA = [
    ((50, 2.6772, -79.7751), (50, 0, -82.7485), 2.0425),
    ((50, 3.1571, -77.2803), (50, 0, -82.7485), 2.8615),
    ((50, 2.8361, -74.0200), (50, 0, -82.7485), 3.4412),
    ((50, -1.3802, -84.2814), (50, 0, -82.7485), 1.0000),
    ((50, 2.5, 0), (50, 0, -2.5), 4.3065),
    ((50, 2.5, 0), (73, 25, -18), 27.1492),
    ((2.0776, 0.0795, -1.1350), (0.9033, -0.0636, -0.5514), 0.9082),
]


@pytest.mark.parametrize("p,q,want", SHARMA)
def test_published_pairs(p, q, want):
    got = float(ciede_ref.de00(*p, *q))
    print(p, q, got, want)
    assert abs(got - want) <= 5e-5
    assert float(ciede_ref.de00(*q, *p)) == got  # symmetric to the bit on these


def _samples(depth, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << depth, n) for _ in range(6)]


@pytest.mark.parametrize("depth", [8, 10])
def test_symmetry_and_zero(depth):
    s = _samples(depth, 20000, 3 + depth)
    a, b = ciede_ref.lab(*s[:3], depth), ciede_ref.lab(*s[3:], depth)
    ab, ba = ciede_ref.de00(*a, *b), ciede_ref.de00(*b, *a)
    # the two orders differ only in the rounding of sums that are written asymmetrically (h2 - h1 ...)
    np.testing.assert_allclose(ab, ba, rtol=1e-12, atol=1e-12)
    assert (ab >= 0).all() and np.isfinite(ab).all()
    same = ciede_ref.de00(*a, *a)
    assert (same == 0.0).all() and not np.signbit(same).any()  # exactly +0 for equal samples


@pytest.mark.parametrize("depth", [8, 10])
def test_black_takes_the_zero_hue_arm(depth):
    """Every sample at or below black clips R, G and B to 0: a = b = 0 exactly, h' = 0, C' = 0."""
    s = 1 << (depth - 8)
    for Y, U, V in ((0, 128 * s, 128 * s), (16 * s, 128 * s, 128 * s), (10 * s, 128 * s, 128 * s), (3 * s, 120 * s, 130 * s)):
        L, a, b = ciede_ref.lab(np.array([Y]), np.array([U]), np.array([V]), depth)
        assert L[0] == 0.0 and a[0] == 0.0 and b[0] == 0.0 and not np.signbit(a[0]) and not np.signbit(b[0])
    black = ciede_ref.lab(np.array([0]), np.array([128 * s]), np.array([128 * s]), depth)
    grey = ciede_ref.lab(np.array([126 * s]), np.array([128 * s]), np.array([128 * s]), depth)
    de, far = ciede_ref.de00(*black, *grey, with_margin=True)
    assert far[0] == np.inf  # C'_1 C'_2 = 0: no hue branch is looked at
    # with C' = 0 on one side and a near-neutral grey the difference is the lightness term alone
    L = grey[0][0]
    Lb = L / 2.0
    SL = 1.0 + 0.015 * (Lb - 50.0) ** 2 / math.sqrt(20.0 + (Lb - 50.0) ** 2)
    assert de[0] == pytest.approx(L / SL, rel=1e-9)
    assert float(ciede_ref.de00(*black, *black)[0]) == 0.0


def test_white_and_grey_are_neutral():
    L, a, b = ciede_ref.lab(np.array([235, 126]), np.array([128, 128]), np.array([128, 128]), 8)
    assert L[0] == pytest.approx(100.0, abs=1e-5) and np.abs(a).max() < 1e-4 and np.abs(b).max() < 1e-4
    # limited range: code values past white clip to it
    L2, _, _ = ciede_ref.lab(np.array([255]), np.array([128]), np.array([128]), 8)
    assert L2[0] == L[0]
    # 10 bits is the same scale
    for v8, v10 in zip(ciede_ref.lab(np.array([100]), np.array([90]), np.array([160]), 8),
                       ciede_ref.lab(np.array([400]), np.array([360]), np.array([640]), 10)):
        assert v8[0] == v10[0]


@pytest.mark.parametrize("fmt,w,h", [("yuv420p", 5, 3), ("yuv422p", 5, 3), ("yuv420p10le", 7, 5), ("yuv444p", 3, 3)])
def test_nearest_chroma_for_odd_sizes(fmt, w, h):
    """Position (x, y) reads chroma [y >> vsub][x >> hsub] of the ceil-sized
    planes: the last column and row have a chroma sample of their own."""
    f = formats.fmt(fmt)
    rng = np.random.default_rng(w * h)
    shapes = formats.plane_shapes(f, w, h)
    assert shapes[1] == (-(-h >> f.vsub), -(-w >> f.hsub))
    ref = [rng.integers(0, 1 << f.depth, (1,) + s) for s in shapes]
    dist = [rng.integers(0, 1 << f.depth, (1,) + s) for s in shapes]
    out, _ = ciede_ref.ciede(ref, dist, f.depth, f.hsub, f.vsub)
    tot, top = 0.0, 0.0
    for y in range(h):
        for x in range(w):
            pix = [(p[0][0, y, x], p[1][0, y >> f.vsub, x >> f.hsub], p[2][0, y >> f.vsub, x >> f.hsub]) for p in (ref, dist)]
            labs = [ciede_ref.lab(*(np.array([v]) for v in px), f.depth) for px in pix]
            de = float(ciede_ref.de00(*labs[0], *labs[1])[0])
            tot, top = tot + de, max(top, de)
    assert out[0, 0] == pytest.approx(tot, rel=1e-13) and out[0, 1] == top
    # changing the last chroma sample alone changes the result: it is read
    dist2 = [p.copy() for p in dist]
    dist2[1][0, -1, -1] ^= 0x40
    assert ciede_ref.ciede(ref, dist2, f.depth, f.hsub, f.vsub)[0][0, 0] != out[0, 0]


def test_weights():
    s = _samples(8, 5000, 11)
    a, b = ciede_ref.lab(*s[:3], 8), ciede_ref.lab(*s[3:], 8)
    one = ciede_ref.de00(*a, *b)
    # all three doubled: every term halves, so does dE00
    np.testing.assert_allclose(ciede_ref.de00(*a, *b, weights=(2, 2, 2)), one / 2.0, rtol=1e-14)
    # a heavier lightness weight can only lower the difference, and does for some
    kl = ciede_ref.de00(*a, *b, weights=(2, 1, 1))
    assert (kl <= one * (1 + 1e-15)).all() and (kl < one).any()
    # grey against grey differs in lightness alone, up to the tiny a, b of a neutral: kL = 2 halves it
    g = np.full(200, 128)
    ga, gb = ciede_ref.lab(s[0][:200], g, g, 8), ciede_ref.lab(s[3][:200], g, g, 8)
    np.testing.assert_allclose(ciede_ref.de00(*ga, *gb, weights=(2, 1, 1)), ciede_ref.de00(*ga, *gb) / 2.0, rtol=1e-6)
    assert ciede.WEIGHTS == (1.0, 1.0, 1.0)
    assert ciede.parse_weights("1,1,1") == (1.0, 1.0, 1.0) and ciede.parse_weights("2,1.5,0.5") == (2.0, 1.5, 0.5)
    for bad in ("1,1", "1,1,0", "1,-1,1", "a,b,c", "1,1,inf", "1,1,nan", ""):
        with pytest.raises(ValueError):
            ciede.parse_weights(bad)


def test_margin_reports_the_branch_boundaries():
    # hues 10 and 190 + 1e-9 degrees at equal chroma: |dh| sits 1e-9 from 180
    def at(deg, C=30.0):
        return 50.0, C * math.cos(math.radians(deg)), C * math.sin(math.radians(deg))
    _, far = ciede_ref.de00(*at(10.0), *at(190.0 + 1e-7), with_margin=True)
    assert float(far) < 1e-6
    _, far = ciede_ref.de00(*at(10.0), *at(100.0), with_margin=True)
    assert float(far) > 80.0
    _, far = ciede_ref.de00(*at(350.0), *at(10.0 + 1e-8), with_margin=True)  # sum 360 under |dh| > 180
    assert float(far) < 1e-6
    _, far = ciede_ref.de00(50.0, 0.0, 0.0, *at(77.0), with_margin=True)
    assert float(far) == np.inf


def test_pool_and_the_cap():
    out = np.array([[0.0, 0.0], [1000.0 * 2.0, 7.5], [1000.0 * 1e-4, 0.2], [1000.0 * 10 ** -2.75, 0.1], [np.nan, np.nan]])
    de, mx, sc = ciede.pool(out, 50, 20)
    assert de[:3].tolist() == [0.0, 2.0, 1e-4] and mx[:4].tolist() == [0.0, 7.5, 0.2, 0.1]
    assert sc[0] == 100.0                                        # delta_e = 0
    assert sc[1] == pytest.approx(45.0 - 20.0 * math.log10(2.0))
    assert sc[2] == 100.0                                        # 45 + 80 capped
    assert sc[3] == pytest.approx(100.0, abs=1e-9) and sc[3] <= 100.0
    assert np.isnan(de[4]) and np.isnan(sc[4])
    assert ciede.score(1.0) == 45.0
    res = ciede.summarize(out[:3], 50, 20)
    assert res["mean"]["delta_e"] == pytest.approx((2.0 + 1e-4) / 3) and res["mean"]["delta_e_max"] == 7.5
    assert res["mean"]["ciede2000"] == pytest.approx((200.0 + 45.0 - 20.0 * math.log10(2.0)) / 3)
    res = ciede.summarize(out[:3], 50, 20, matched=[True, False, True])
    assert np.isnan(res["delta_e"][1]) and res["mean"]["delta_e_max"] == 0.2 and res["mean"]["ciede2000"] == 100.0
    none = ciede.summarize(np.zeros((0, 2)), 50, 20)
    assert all(math.isnan(v) for v in none["mean"].values()) and none["delta_e"].shape == (0,)


def test_geometry_constants():
    assert (ciede.PIECE_BYTES, ciede.LANES, ciede.WAVES, ciede.WAVE_ROWS, ciede.FRAMES_PER_LAUNCH) == (16, 64, 4, 4, 256)
    assert ciede.spans("yuv420p") == (32, 2048, 8, 32)
    assert ciede.spans("yuv422p10le") == (16, 1024, 4, 16)
    assert ciede.spans("yuv444p") == (16, 1024, 4, 16)
    assert ciede.spans("yuv444p10le") == (8, 512, 4, 16)
    assert "PP-CIEDE-1" in ciede.SPEC and "unpinned" in ciede.SPEC


def _fake():
    sse = np.array([[0, 0, 0], [10, 5, 5], [20, 2, 2]])
    ssim = np.array([[1.0, 1.0, 1.0], [0.9, 0.95, 0.95], [0.8, 0.9, 0.9]])
    return sse, ssim, np.array([[0.0, 0.0], [33 * 33 * 2.0, 9.0], [33 * 33 * 4.0, 12.5]])


def test_json_keys_only_when_asked(monkeypatch, capsys):
    sse, ssim, t = _fake()
    seen = []

    def before(ref, dist, batch=32, flags="bicubic"):  # what `cli metrics` called before PP-CIEDE-1
        return metrics.summarize(sse, ssim, "yuv420p", 33, 33)

    def scored(ref, dist, **kw):
        seen.append(kw)
        return metrics.summarize(sse, ssim, "yuv420p", 33, 33, ciede_terms=t if kw.get("ciede") else None,
                                 vif_terms=np.ones((3, 4, 2)) if kw.get("vif") else None,
                                 adm_terms=np.ones((3, 4, 6)) if kw.get("adm") else None,
                                 motion_terms=np.zeros(3, np.uint64) if kw.get("motion") else None)

    base = ["metrics", "--ref", "r.y4m", "--input", "d.y4m"]
    monkeypatch.setattr(metrics, "metrics_of_files", before)
    assert cli.main(base + ["--per-frame"]) == 0
    old = capsys.readouterr().out
    monkeypatch.setattr(metrics, "metrics_of_files", scored)
    assert cli.main(base + ["--per-frame"]) == 0
    assert capsys.readouterr().out == old and "ciede" not in seen[-1]  # unchanged to the byte without the flag
    assert not [k for k in json.loads(old) if "delta_e" in k or "ciede" in k]

    assert cli.main(base + ["--ciede", "--crop", "8x8", "--batch", "5"]) == 0
    assert seen[-1] == {"batch": 5, "flags": "bicubic", "crop": (8, 8), "ciede": True}
    d = json.loads(capsys.readouterr().out)
    assert d["delta_e"] == pytest.approx(2.0) and d["delta_e_max"] == 12.5
    assert d["ciede2000"] == pytest.approx((100.0 + 90.0 - 20.0 * math.log10(2.0) - 20.0 * math.log10(4.0)) / 3)
    assert not [k for k in d if k.endswith("_frames")]
    for k, v in json.loads(old).items():
        if not k.endswith("_frames"):
            assert d[k] == v

    assert cli.main(base + ["--ciede", "--ciede-weights", "2,1,0.5", "--per-frame"]) == 0
    assert seen[-1] == {"batch": 32, "flags": "bicubic", "ciede": True, "ciede_weights": (2.0, 1.0, 0.5)}
    d = json.loads(capsys.readouterr().out)
    assert d["delta_e_frames"] == [0.0, 2.0, 4.0] and d["delta_e_max_frames"] == [0.0, 9.0, 12.5]
    assert d["ciede2000_frames"][0] == 100.0 and len(d["ciede2000_frames"]) == 3

    # --vmaf-features does not imply it
    assert cli.main(base + ["--vmaf-features"]) == 0
    assert "ciede" not in seen[-1] and "delta_e" not in json.loads(capsys.readouterr().out)
    assert cli.main(base + ["--vmaf-features", "--ciede"]) == 0
    d = json.loads(capsys.readouterr().out)
    assert "vmaf_features" in d and d["delta_e_max"] == 12.5

    for bad in (["--ciede-weights", "1,1,1"], ["--ciede", "--ciede-weights", "1,0,1"], ["--ciede", "--ciede-weights", "1,1"]):
        with pytest.raises(SystemExit):
            cli.main(base + bad)

    # an unmatched frame of an explicit map is null in the lists and left out of the clip values
    res = metrics.summarize(sse, ssim, "yuv420p", 33, 33, matched=[True, False, True], ciede_terms=t)
    r = metrics.report(res, "r", "d", per_frame=True)
    assert r["delta_e_frames"] == [0.0, None, 4.0] and r["delta_e"] == 2.0 and r["delta_e_max"] == 12.5


def _frames(planes=(True, True, True), ls=(32, 16, 16), fs=1024):
    buf = (ctypes.c_uint8 * 64)()  # never read: every call below is refused, or has nothing to do, first
    fr = _native.pp_frames()
    for p in range(3):
        fr.data[p] = ctypes.addressof(buf) if planes[p] else None
        fr.linesize[p] = ls[p]
        fr.frame_stride[p] = fs
    fr._keep = buf
    return fr


def _call(ctx, fmt="yuv420p", w=20, h=15, ref=None, dist=None, idx=None, nref=2, ndist=2, weights=(1.0, 1.0, 1.0), out=True):
    L = _native.lib()
    ref, dist = ref or _frames(), dist or _frames()
    ix = None if idx is None else (ctypes.c_int32 * len(idx))(*idx)
    o = (ctypes.c_double * 8)()
    return L.pp_ciede(ctx, formats.fmt(fmt).id, w, h, ctypes.byref(ref), ctypes.byref(dist),
                      None if ix is None else ctypes.addressof(ix), nref, ndist, *weights,
                      ctypes.addressof(o) if out else None, None)


def test_pp_ciede_argument_checks_need_no_gpu():
    L = _native.lib()
    assert "pp_ciede" in _native.EXPORTS and L.pp_abi_version() == 7
    ctx = (ctypes.c_uint8 * 256)()  # never dereferenced
    assert _call(None) == -1 and b"null" in L.pp_last_error()
    assert _call(ctx, out=False) == -1 and b"null" in L.pp_last_error()
    assert L.pp_ciede(ctx, 0, 8, 8, None, None, None, 1, 1, 1.0, 1.0, 1.0, None, None) == -1
    for packed in ("uyvy422", "v210"):
        assert _call(ctx, fmt=packed) == -1 and b"planar" in L.pp_last_error()
    assert L.pp_ciede(ctx, 99, 8, 8, ctypes.byref(_frames()), ctypes.byref(_frames()), None, 1, 1, 1.0, 1.0, 1.0,
                      ctypes.addressof((ctypes.c_double * 2)()), None) == -1
    assert _call(ctx, w=0) == -1 and b"frame" in L.pp_last_error()
    assert _call(ctx, h=-1) == -1 and b"frame" in L.pp_last_error()
    assert _call(ctx, ndist=-1) == -1 and b"ndist" in L.pp_last_error()
    assert _call(ctx, nref=-1) == -1 and b"nref" in L.pp_last_error()
    for wts in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, math.inf), (math.nan, 1.0, 1.0)):
        assert _call(ctx, weights=wts) == -1 and b"weights" in L.pp_last_error()
    assert _call(ctx, ref=_frames(planes=(True, False, True))) == -1 and b"ref plane 1: null data" in L.pp_last_error()
    assert _call(ctx, dist=_frames(planes=(True, True, False))) == -1 and b"dist plane 2: null data" in L.pp_last_error()
    assert _call(ctx, ref=_frames(ls=(19, 16, 16))) == -1 and b"ref plane 0: linesize" in L.pp_last_error()
    assert _call(ctx, dist=_frames(ls=(32, 9, 16))) == -1 and b"dist plane 1: linesize" in L.pp_last_error()
    # odd width: the chroma row is the ceil-sized one (21 -> 11 samples)
    assert _call(ctx, w=21, dist=_frames(ls=(32, 16, 10))) == -1 and b"dist plane 2: linesize" in L.pp_last_error()
    assert _call(ctx, fmt="yuv420p10le", ref=_frames(ls=(41, 20, 20))) == -1 and b"2-byte grid" in L.pp_last_error()
    assert _call(ctx, idx=[0, 2]) == -1 and b"ref_index[1] = 2" in L.pp_last_error()
    assert _call(ctx, idx=[-1, 0]) == -1 and b"ref_index[0] = -1" in L.pp_last_error()
    assert _call(ctx, nref=1) == -1 and b"without ref_index" in L.pp_last_error()
    assert _call(ctx, h=64, dist=_frames(ls=(1 << 25, 16, 16))) == -4 and b"2 GiB buffer range" in L.pp_last_error()
    assert _call(ctx, ndist=0) == 0 and _call(ctx, ndist=0, nref=0) == 0  # nothing to do: no HIP call
