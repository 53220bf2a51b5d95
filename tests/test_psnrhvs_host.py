"""Host side of PP-HVS-1 without a GPU: the tables and the DCT matrix, closed
forms of the numpy restatement (tests/psnrhvs_ref.py), the block geometry, the
pooling (pixpath/psnrhvs.py), the report and `cli metrics --psnr-hvs`, and the
argument checks of pp_psnr_hvs that are made before any HIP call."""
import ctypes
import json
import math

import numpy as np
import pytest

import psnrhvs_ref
from pixpath import _native, cli, formats, metrics, psnrhvs

CSF_ROW0 = [1.608443, 2.339554, 2.573509, 1.608443, 1.072295, 0.643377, 0.504610, 0.421887]
MASK_ROW0 = [0.390625, 0.826446, 1.0, 0.390625, 0.173611, 0.0625, 0.038447, 0.026874]


def test_csf_reproduces_the_published_row():
    """CSF is the published six-decimal table.  Its first row is pinned to the
    published one to 5e-7.  The quotient 25.735088 / Q restates the table: it
    rounds to it at six decimals in 63 entries and is 5.45e-7 away at [0][1]
    (25.735088 / 11 = 2.3395535 against the published 2.339554), which is why the
    table and not the quotient is what the kernel and the restatement use."""
    for csf in (psnrhvs.CSF, psnrhvs_ref.CSF):
        np.testing.assert_allclose(csf[0], CSF_ROW0, rtol=0, atol=5e-7)
        quotient = 25.735088 / psnrhvs.Q
        off = np.round(quotient, 6) != csf
        assert np.argwhere(off).tolist() == [[0, 1]]
        assert np.abs(quotient - csf)[~off].max() <= 5e-7 and abs(quotient[0, 1] - csf[0, 1]) < 5.5e-7
        assert np.array_equal(csf, np.round(csf, 6)) and csf[0, 0] == 25.735088 / 16.0
        # the same Q, the same entry: the table is a function of Q
        for q in np.unique(psnrhvs.Q):
            assert len(np.unique(csf[psnrhvs.Q == q])) == 1


def test_tables_reproduce_the_published_rows():
    for mod_csf, mod_mask in ((psnrhvs.CSF, psnrhvs.MASK), (psnrhvs_ref.CSF, psnrhvs_ref.M)):
        assert mod_csf.shape == (8, 8) and mod_mask.shape == (8, 8)
        np.testing.assert_allclose(mod_mask[0], MASK_ROW0, rtol=0, atol=5e-7)
    assert np.array_equal(psnrhvs.Q, psnrhvs_ref.Q) and psnrhvs.Q[7, 7] == 99 and psnrhvs.Q[3, 5] == 87
    assert np.array_equal(psnrhvs.CSF, psnrhvs_ref.CSF)
    np.testing.assert_allclose(psnrhvs.MASK, psnrhvs_ref.M, rtol=4e-16, atol=0)
    assert "PP-HVS-1" in psnrhvs.SPEC and "unpinned" in psnrhvs.SPEC and psnrhvs.STEPS == (8, 7)


def test_dct_matrix_is_orthonormal():
    for C in (psnrhvs.dct_matrix(), psnrhvs_ref.C):
        assert np.abs(C @ C.T - np.eye(8)).max() <= 1e-15
        assert np.abs(C.T @ C - np.eye(8)).max() <= 1e-15
        assert C[0, 0] == math.sqrt(1.0 / 8.0) and C[1, 0] == pytest.approx(0.5 * math.cos(math.pi / 16), rel=1e-15)
    # rows first, then columns: a picture constant along a row has energy in column 0 of D alone
    x = np.repeat(np.arange(8)[:, None] ** 2, 8, axis=1)
    d = psnrhvs_ref.dct2(x)
    assert np.abs(d[:, 1:]).max() < 1e-12 and np.abs(d[1:, 0]).max() > 1


def _noise(fmt, w, h, n, seed):
    rng = np.random.default_rng(seed)
    f = formats.fmt(fmt)
    dt = np.uint16 if f.depth > 8 else np.uint8
    return [rng.integers(0, 1 << f.depth, (n, r, c)).astype(dt) for r, c in formats.plane_shapes(f, w, h)]


@pytest.mark.parametrize("fmt,c", [("yuv420p", 3), ("yuv422p10le", 11), ("yuv444p", 1)])
@pytest.mark.parametrize("step", psnrhvs.STEPS)
def test_constant_offset_closed_form(fmt, c, step):
    """B = A + c: only DC differs, and DC is never masked: mse_hvs = mse_hvsm = c^2 CSF[0][0]^2."""
    w, h = 41, 35
    f = formats.fmt(fmt)
    peak = (1 << f.depth) - 1
    ref = [(p // 2).astype(p.dtype) for p in _noise(fmt, w, h, 2, 3)]  # room for + c
    dist = [(p + c).astype(p.dtype) for p in ref]
    res = psnrhvs.summarize(psnrhvs_ref.psnr_hvs(ref, dist, step), w, h, None, fmt, step)
    want = c * c * (25.735088 / 16.0) ** 2
    assert repr((25.735088 / 16.0) ** 2).startswith("2.587088")
    for kind in psnrhvs.KINDS:
        for name in ("y", "u", "v", "all"):
            np.testing.assert_allclose(res["mse_%s_%s" % (kind, name)], want, rtol=1e-12, atol=0)
            np.testing.assert_allclose(res["psnr_%s_%s" % (kind, name)], 10 * math.log10(peak * peak / want), rtol=1e-12)
            assert res["mean"]["mse_%s_%s" % (kind, name)] == pytest.approx(want, rel=1e-12)


def test_masked_sum_is_never_above_the_plain_one():
    rng = np.random.default_rng(5)
    for step in psnrhvs.STEPS:
        a = rng.integers(0, 256, (40, 52))
        b = np.clip(a + rng.integers(-9, 10, a.shape), 0, 255)
        s, sm, n = psnrhvs_ref.plane_sums(a, b, step)
        assert 0 < sm < s and n == psnrhvs.blocks_axis(40, step) * psnrhvs.blocks_axis(52, step)
        # two flat blocks: no variance, no mask: equality
        s, sm, _ = psnrhvs_ref.plane_sums(np.full((8, 8), 10), np.full((8, 8), 17), step)
        assert s == sm == pytest.approx(64 * 49 * (25.735088 / 16.0) ** 2, rel=1e-12)
        # 16-bit samples above 1023 as stored: the integers of the variance ratio stay exact
        hi = rng.integers(60000, 65536, (16, 16))
        s, sm, _ = psnrhvs_ref.plane_sums(hi, hi[::-1], step)
        assert 0 <= sm <= s and s > 0


def test_identical_planes_give_exactly_zero():
    a = np.random.default_rng(6).integers(0, 1024, (33, 47))
    for step in psnrhvs.STEPS:
        assert psnrhvs_ref.plane_sums(a, a.copy(), step)[:2] == (0.0, 0.0)
    res = psnrhvs.summarize(np.zeros((2, 3, 2)), 47, 33, None, "yuv444p10le", 8)
    assert (res["mse_hvs_all"] == 0).all() and np.isnan(res["psnr_hvs_all"]).all() and np.isnan(res["psnr_hvsm_y"]).all()
    assert res["mean"]["mse_hvsm_all"] == 0.0 and math.isnan(res["mean"]["psnr_hvsm_all"])


def test_blocks_of_an_axis():
    want = {8: {7: 0, 8: 1, 14: 1, 15: 1, 16: 2, 22: 2, 23: 2}, 7: {7: 0, 8: 1, 14: 1, 15: 2, 16: 2, 22: 3, 23: 3}}
    for step in psnrhvs.STEPS:
        for n, nb in want[step].items():
            assert psnrhvs.blocks_axis(n, step) == nb == psnrhvs_ref.nb(n, step), (step, n)
            assert psnrhvs.blocks("yuv444p", n, 23, step) == (nb * want[step][23],) * 3
    assert psnrhvs.blocks("yuv420p", 64, 48) == (48, 12, 12) and psnrhvs.blocks("yuv420p", 64, 48, 7) == (54, 12, 12)
    assert psnrhvs.blocks("yuv422p10le", 1920, 1080) == (240 * 135, 120 * 135, 120 * 135)
    assert (psnrhvs.tile_width(8), psnrhvs.tile_width(7)) == (256, 225)
    assert (psnrhvs.GROUP_BLOCKS, psnrhvs.BLOCK_LANES, psnrhvs.FRAMES_PER_LAUNCH) == (32, 8, 256)
    for bad in (6, 9, 0, 7.5):
        with pytest.raises(ValueError):
            psnrhvs.blocks_axis(16, bad)


@pytest.mark.parametrize("w,h", [(14, 14), (13, 14)])
def test_a_420_frame_with_luma_blocks_and_no_chroma_block(w, h):
    """A 4:2:0 frame whose chroma planes are 7 x 7 has luma blocks and no chroma
    block: `*_u`, `*_v` and `*_all` are NaN.  (15 x 15 is not such a frame here:
    its chroma planes are the ceil-sized 8 x 8 of pp_plane_bytes and hold one
    block; test_a_420_frame_of_15_by_15.)"""
    fmt = "yuv420p"
    ref, dist = _noise(fmt, w, h, 2, 7), _noise(fmt, w, h, 2, 8)
    for step, nb in ((8, 1), (7, 1)):
        assert psnrhvs.blocks(fmt, w, h, step) == (nb, 0, 0)
        t = psnrhvs_ref.psnr_hvs(ref, dist, step)
        assert (t[:, 0] > 0).all() and (t[:, 1:] == 0).all()
        res = psnrhvs.summarize(t, w, h, None, fmt, step)
        for kind in psnrhvs.KINDS:
            assert (res["mse_%s_y" % kind] > 0).all() and (res["psnr_%s_y" % kind] > 0).all()
            for name in ("u", "v", "all"):
                assert np.isnan(res["mse_%s_%s" % (kind, name)]).all() and np.isnan(res["psnr_%s_%s" % (kind, name)]).all()
                assert math.isnan(res["mean"]["mse_%s_%s" % (kind, name)])
    assert psnrhvs.blocks(fmt, 22, 14, 7) == (3, 0, 0) and psnrhvs.blocks(fmt, 22, 14, 8) == (2, 0, 0)
    # under 8 rows: nothing at all
    assert psnrhvs.blocks(fmt, 64, 7) == (0, 0, 0)
    assert all(math.isnan(res_v) for k, res_v in psnrhvs.summarize(np.zeros((1, 3, 2)), 64, 7, None, fmt, 8)["mean"].items()
               if k.startswith(("mse", "psnr")))


def test_a_420_frame_of_15_by_15():
    """15 x 15 as 4:2:0: four luma blocks at step 7, one at step 8, and one block
    in each of the ceil-sized 8 x 8 chroma planes, so every value exists."""
    fmt, w, h = "yuv420p", 15, 15
    ref, dist = _noise(fmt, w, h, 2, 7), _noise(fmt, w, h, 2, 8)
    assert [p.shape[1:] for p in ref] == [(15, 15), (8, 8), (8, 8)]
    for step, nb in ((8, 1), (7, 4)):
        assert psnrhvs.blocks(fmt, w, h, step) == (nb, 1, 1)
        res = psnrhvs.summarize(psnrhvs_ref.psnr_hvs(ref, dist, step), w, h, None, fmt, step)
        assert all(np.isfinite(res[key]).all() for key in psnrhvs.KEYS)
        np.testing.assert_allclose(res["mse_hvs_all"], 0.8 * res["mse_hvs_y"] + 0.1 * (res["mse_hvs_u"] + res["mse_hvs_v"]),
                                   rtol=1e-15)


def _terms():
    t = np.zeros((3, 3, 2))
    t[1] = [[64 * 48 * 4.0, 64 * 48 * 2.0], [64 * 12 * 1.0, 64 * 12 * 0.5], [64 * 12 * 3.0, 64 * 12 * 1.0]]
    t[2] = 2 * t[1]
    return t


def test_summarize_pool_and_matched():
    t = _terms()
    res = psnrhvs.summarize(t, 64, 48, None, "yuv420p", 8)
    assert list(res) == list(psnrhvs.KEYS) + ["mean"] and len(psnrhvs.KEYS) == 16
    assert res["mse_hvs_y"].tolist() == [0.0, 4.0, 8.0] and res["mse_hvsm_v"].tolist() == [0.0, 1.0, 2.0]
    assert res["mse_hvs_all"][1] == pytest.approx(0.8 * 4 + 0.1 * (1 + 3)) and res["mse_hvsm_all"][1] == pytest.approx(1.75)
    assert math.isnan(res["psnr_hvs_y"][0]) and res["psnr_hvs_y"][1] == pytest.approx(10 * math.log10(255 * 255 / 4.0))
    mean = res["mean"]
    assert mean["mse_hvs_y"] == pytest.approx(4.0) and mean["psnr_hvs_y"] == pytest.approx(10 * math.log10(255 * 255 / 4.0))
    assert mean["hvs_step"] == 8 and mean["hvs_blocks"] == [48, 12, 12]
    res = psnrhvs.summarize(t, 64, 48, [True, False, True], "yuv420p", 8)
    assert np.isnan(res["mse_hvs_y"][1]) and np.isnan(res["psnr_hvsm_all"][1])
    assert res["mean"]["mse_hvs_y"] == pytest.approx(4.0) and res["mean"]["mse_hvsm_u"] == pytest.approx(0.5)
    ten = psnrhvs.summarize(t, 64, 48, None, "yuv420p10le", 8)
    assert ten["psnr_hvs_y"][1] == pytest.approx(10 * math.log10(1023 * 1023 / 4.0))
    none = psnrhvs.summarize(np.zeros((0, 3, 2)), 64, 48, None, "yuv420p", 7)
    assert none["mse_hvs_y"].shape == (0,) and math.isnan(none["mean"]["mse_hvs_all"]) and none["mean"]["hvs_step"] == 7
    p = psnrhvs.pool(t, "yuv420p", 64, 48, 7)  # the same sums over step 7's block counts
    assert p["mse_hvs_y"][1] == pytest.approx(4.0 * 48 / 54) and p["mse_hvs_u"][1] == pytest.approx(1.0)


def test_json_keys_only_when_asked(monkeypatch, capsys):
    sse = np.array([[0, 0, 0], [10, 5, 5], [20, 2, 2]])
    ssim = np.array([[1.0, 1.0, 1.0], [0.9, 0.95, 0.95], [0.8, 0.9, 0.9]])
    t = _terms()
    seen = []

    def before(ref, dist, batch=32, flags="bicubic"):  # what `cli metrics` called before PP-HVS-1
        return metrics.summarize(sse, ssim, "yuv420p", 64, 48)

    def scored(ref, dist, **kw):
        seen.append(kw)
        return metrics.summarize(sse, ssim, "yuv420p", 64, 48, hvs_terms=t if kw.get("psnr_hvs") else None,
                                 hvs_step=kw.get("hvs_step"),
                                 vif_terms=np.ones((3, 4, 2)) if kw.get("vif") else None,
                                 adm_terms=np.ones((3, 4, 6)) if kw.get("adm") else None,
                                 motion_terms=np.zeros(3, np.uint64) if kw.get("motion") else None)

    base = ["metrics", "--ref", "r.y4m", "--input", "d.y4m"]
    monkeypatch.setattr(metrics, "metrics_of_files", before)
    assert cli.main(base + ["--per-frame"]) == 0
    old = capsys.readouterr().out
    monkeypatch.setattr(metrics, "metrics_of_files", scored)
    assert cli.main(base + ["--per-frame"]) == 0
    assert capsys.readouterr().out == old and "psnr_hvs" not in seen[-1]  # unchanged to the byte without the flag
    assert not [k for k in json.loads(old) if "hvs" in k]

    assert cli.main(base + ["--psnr-hvs", "--batch", "5"]) == 0
    assert seen[-1] == {"batch": 5, "flags": "bicubic", "psnr_hvs": True}
    d = json.loads(capsys.readouterr().out)
    assert d["mse_hvs_y"] == pytest.approx(4.0) and d["psnr_hvsm_y"] == pytest.approx(10 * math.log10(255 * 255 / 2.0))
    assert d["hvs_step"] == 8 and d["hvs_blocks"] == [48, 12, 12]
    assert set(psnrhvs.KEYS) <= set(d) and not [k for k in d if k.endswith("_frames")]
    for k, v in json.loads(old).items():
        if not k.endswith("_frames"):
            assert d[k] == v

    assert cli.main(base + ["--psnr-hvs", "--hvs-step", "7", "--per-frame"]) == 0
    assert seen[-1] == {"batch": 32, "flags": "bicubic", "psnr_hvs": True, "hvs_step": 7}
    d = json.loads(capsys.readouterr().out)
    assert d["hvs_step"] == 7 and d["hvs_blocks"] == [54, 12, 12]
    assert d["mse_hvs_y_frames"] == pytest.approx([0.0, 4.0 * 48 / 54, 8.0 * 48 / 54])
    assert d["psnr_hvs_y_frames"][0] is None and all(len(d[k + "_frames"]) == 3 for k in psnrhvs.KEYS)

    # --vmaf-features does not imply it
    assert cli.main(base + ["--vmaf-features"]) == 0
    assert "psnr_hvs" not in seen[-1] and not [k for k in json.loads(capsys.readouterr().out) if "hvs" in k]
    assert cli.main(base + ["--vmaf-features", "--psnr-hvs"]) == 0
    d = json.loads(capsys.readouterr().out)
    assert "vmaf_features" in d and d["mse_hvs_v"] == pytest.approx(3.0)

    for bad in (["--hvs-step", "7"], ["--psnr-hvs", "--hvs-step", "6"], ["--psnr-hvs", "--hvs-step", "x"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + bad)
        assert e.value.code not in (0, None)
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        cli.main(base + ["--hvs-step", "8"])
    assert "--hvs-step needs --psnr-hvs" in str(e.value)

    # an unmatched frame of an explicit map is null in the lists and left out of the clip values
    res = metrics.summarize(sse, ssim, "yuv420p", 64, 48, matched=[True, False, True], hvs_terms=t)
    r = metrics.report(res, "r", "d", per_frame=True)
    assert r["mse_hvs_y_frames"] == [0.0, None, 8.0] and r["mse_hvs_y"] == 4.0 and r["psnr_hvs_all_frames"][1] is None
    with pytest.raises(ValueError):
        metrics.metrics_of_files("r.y4m", "d.y4m", psnr_hvs=True, hvs_step=9)


def test_the_feature_table_has_the_row():
    row = metrics.FEATURES[-1]
    assert (row.name, row.terms, row.flat, row.rows) == ("psnr_hvs", "hvs_terms", psnrhvs.KEYS, ())
    assert metrics.FEATURES[-2].name == "ciede" and row.empty == (((3, 2), np.float64),)


def _frames(planes=(True, True, True), ls=(32, 16, 16), fs=1024):
    buf = (ctypes.c_uint8 * 64)()  # never read: every call below is refused, or has nothing to do, first
    fr = _native.pp_frames()
    for p in range(3):
        fr.data[p] = ctypes.addressof(buf) if planes[p] else None
        fr.linesize[p] = ls[p]
        fr.frame_stride[p] = fs
    fr._keep = buf
    return fr


def _call(ctx, fmt="yuv420p", w=20, h=15, ref=None, dist=None, idx=None, nref=2, ndist=2, step=8, out=True):
    L = _native.lib()
    ref, dist = ref or _frames(), dist or _frames()
    ix = None if idx is None else (ctypes.c_int32 * len(idx))(*idx)
    o = (ctypes.c_double * 24)()
    return L.pp_psnr_hvs(ctx, formats.fmt(fmt).id, w, h, ctypes.byref(ref), ctypes.byref(dist),
                         None if ix is None else ctypes.addressof(ix), nref, ndist, step,
                         ctypes.addressof(o) if out else None, None)


def test_pp_psnr_hvs_argument_checks_need_no_gpu():
    L = _native.lib()
    assert "pp_psnr_hvs" in _native.EXPORTS and L.pp_abi_version() == 7
    ctx = (ctypes.c_uint8 * 256)()  # never dereferenced
    assert _call(None) == -1 and b"null" in L.pp_last_error()
    assert _call(ctx, out=False) == -1 and b"null" in L.pp_last_error()
    assert L.pp_psnr_hvs(ctx, 0, 8, 8, None, None, None, 1, 1, 8, None, None) == -1 and b"null" in L.pp_last_error()
    for packed in ("uyvy422", "v210"):
        assert _call(ctx, fmt=packed) == -1 and b"planar" in L.pp_last_error()
    assert L.pp_psnr_hvs(ctx, 99, 8, 8, ctypes.byref(_frames()), ctypes.byref(_frames()), None, 1, 1, 8,
                         ctypes.addressof((ctypes.c_double * 6)()), None) == -1
    assert _call(ctx, w=0) == -1 and b"frame" in L.pp_last_error()
    assert _call(ctx, h=-1) == -1 and b"frame" in L.pp_last_error()
    assert _call(ctx, ndist=-1) == -1 and b"ndist" in L.pp_last_error()
    assert _call(ctx, nref=-1) == -1 and b"nref" in L.pp_last_error()
    for step in (6, 9, 0, -8, 16):
        assert _call(ctx, step=step) == -1 and b"step" in L.pp_last_error() and b"7 or 8" in L.pp_last_error()
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
    for step in psnrhvs.STEPS:
        assert _call(ctx, ndist=0, step=step) == 0 and _call(ctx, ndist=0, nref=0, step=step) == 0  # nothing to do: no HIP call
