"""Host side of the signal statistics (spec PP-STATS-1), no GPU: summarize on
hand-made histograms with closed-form answers, the numpy reference's own
identity, the argument checks of pp_frame_stats and `cli stats`."""
import ctypes
import json
import math

import numpy as np
import pytest

import stats_ref
from pixpath import _native, formats, stats

PLANAR = ("yuv420p", "yuv422p", "yuv444p", "yuv420p10le", "yuv422p10le", "yuv444p10le")
ABSENT = (1 << 64) - 1


def _hist(fmt, frames):
    """[N, 3, bins] from a list of frames, each three {value: count} dicts."""
    bins = 1 << formats.fmt(fmt).depth
    h = np.zeros((len(frames), 3, bins), np.int32)
    for k, fr in enumerate(frames):
        for p, d in enumerate(fr):
            for v, c in d.items():
                h[k, p, v] = c
    return h


def _zero(n):
    return np.zeros((n, 3), np.int32)


# ------------------------------------------------------------------ summarize
def test_a_single_bin():
    h = _hist("yuv444p", [[{50: 100}, {128: 100}, {255: 100}]])
    r = stats.summarize(h, np.full((1, 3), 700, np.uint64), _zero(1), "yuv444p", 10, 10)
    assert r["frames"] == 1
    for key in ("min", "max", "avg", "low", "high"):
        assert r[key + "_y"].tolist() == [50.0] and r[key + "_u"].tolist() == [128.0] and r[key + "_v"].tolist() == [255.0]
    assert r["bitdepth_y"].tolist() == [3] and r["bitdepth_u"].tolist() == [1] and r["bitdepth_v"].tolist() == [8]
    assert r["out_of_range_y"].tolist() == [0] and r["out_of_range_v"].tolist() == [100]  # 255 > 240
    assert r["dif_y"].tolist() == [7.0]
    assert r["black"].tolist() == [False] and r["repeat"].tolist() == [False]
    c = r["clip"]
    assert (c["min_y"], c["max_y"], c["avg_y"], c["dif_y"], c["bitdepth_v"]) == (50.0, 50.0, 50.0, 7.0, 8)
    assert c["black_frames"] == [] and c["repeat_frames"] == [] and "histogram_y" not in c


def test_percentiles_on_two_bins():
    fr = [[{20: 10, 200: 90}] * 3, [{20: 9, 200: 91}] * 3, [{20: 90, 200: 10}] * 3, [{20: 89, 200: 11}] * 3]
    r = stats.summarize(_hist("yuv444p", fr), None, _zero(4), "yuv444p", 10, 10)
    assert r["low_y"].tolist() == [20.0, 200.0, 20.0, 20.0]   # the 10th sample
    assert r["high_y"].tolist() == [200.0, 200.0, 20.0, 200.0]  # the 90th sample
    assert r["avg_u"].tolist() == [182.0, 183.8, 38.0, 39.8]
    assert r["min_v"].tolist() == [20.0] * 4 and r["max_v"].tolist() == [200.0] * 4
    assert all(math.isnan(v) for v in r["dif_y"]) and r["repeat"].tolist() == [False] * 4


def test_percentile_ties_round_half_to_even():
    # 25 samples: 0.10 * 25 = 2.5 -> 2, 0.90 * 25 = 22.5 -> 22
    assert np.rint(0.10 * 25) == 2 and np.rint(0.90 * 25) == 22
    fr = [[{30: 2, 100: 23}] * 3, [{30: 22, 100: 3}] * 3]
    r = stats.summarize(_hist("yuv444p", fr), None, _zero(2), "yuv444p", 5, 5)
    assert r["low_y"].tolist() == [30.0, 30.0]   # half up (3) would give 100 on frame 0
    assert r["high_y"].tolist() == [100.0, 30.0]  # half up (23) would give 100 on frame 1
    # 15 samples: 1.5 -> 2, 13.5 -> 14
    assert np.rint(0.10 * 15) == 2 and np.rint(0.90 * 15) == 14
    r = stats.summarize(_hist("yuv444p", [[{30: 1, 100: 14}] * 3, [{30: 14, 100: 1}] * 3]), None, _zero(2),
                        "yuv444p", 5, 3)
    assert r["low_y"].tolist() == [100.0, 30.0]  # rounding down (1) would give 30 on frame 0
    assert r["high_y"].tolist() == [100.0, 30.0]


def test_bitdepth_of_shifted_8_bit_content():
    fr = [[{256: 50, 512: 30, 1020: 20}, {512: 100}, {4: 1, 8: 99}]]
    r = stats.summarize(_hist("yuv444p10le", fr), None, _zero(1), "yuv444p10le", 10, 10)
    assert r["bitdepth_y"].tolist() == [8]  # 0b1111111100
    assert r["bitdepth_u"].tolist() == [1] and r["bitdepth_v"].tolist() == [2]
    assert r["clip"]["bitdepth_y"] == 8
    # one sample with bit 0 set makes it 9 bits, with bit 1 too 10
    r = stats.summarize(_hist("yuv444p10le", [[{1020: 98, 1: 1, 2: 1}] * 3]), None, _zero(1), "yuv444p10le", 10, 10)
    assert r["bitdepth_y"].tolist() == [10]
    # limited range at 10 bits: 64 .. 940 luma, .. 960 chroma
    fr = [[{63: 1, 64: 1, 940: 1, 941: 97}, {63: 2, 960: 1, 961: 97}, {64: 50, 960: 50}]]
    r = stats.summarize(_hist("yuv444p10le", fr), None, np.array([[0, 5, 0]]), "yuv444p10le", 10, 10)
    assert r["out_of_range_y"].tolist() == [98] and r["out_of_range_u"].tolist() == [99 + 5]
    assert r["out_of_range_v"].tolist() == [0] and r["over_u"].tolist() == [5]
    assert r["clip"]["out_of_range_u"] == 104 and r["clip"]["over_u"] == 5 and r["clip"]["over_y"] == 0


def test_samples_only_in_over():
    h = _hist("yuv422p10le", [[{}, {}, {}]])
    over = np.array([[64, 32, 32]])
    r = stats.summarize(h, None, over, "yuv422p10le", 8, 8, histogram=True)
    for key in ("min", "max", "avg", "low", "high"):
        assert math.isnan(r[key + "_y"][0]) and math.isnan(r[key + "_u"][0])
    assert r["out_of_range_y"].tolist() == [64] and r["out_of_range_u"].tolist() == [32]
    assert r["over_y"].tolist() == [64] and r["bitdepth_y"].tolist() == [0]
    assert r["black"].tolist() == [False]
    assert math.isnan(r["clip"]["min_y"]) and r["clip"]["over_v"] == 32
    assert r["clip"]["histogram_y"] == [0] * 1024
    # half in the bins: the 10 % point is reached, the 90 % point never is
    r = stats.summarize(_hist("yuv422p10le", [[{100: 32}, {100: 16}, {100: 16}]]), None, over // 2, "yuv422p10le", 8, 8)
    assert r["low_y"].tolist() == [100.0] and math.isnan(r["high_y"][0])


def test_the_sentinel_sad_is_a_null_dif():
    h = _hist("yuv444p", [[{50: 100}] * 3] * 3)
    sad = np.array([[ABSENT] * 3, [0, 0, 0], [100, 0, 250]], np.uint64)
    r = stats.summarize(h, sad, _zero(3), "yuv444p", 10, 10)
    assert math.isnan(r["dif_y"][0]) and r["dif_y"].tolist()[1:] == [0.0, 1.0] and r["dif_v"].tolist()[1:] == [0.0, 2.5]
    assert r["repeat"].tolist() == [False, True, False]
    assert r["clip"]["dif_y"] == 0.5 and r["clip"]["repeat_frames"] == [[1, 1]]
    # the same bits as the int64 tensor ops.frame_stats returns
    r2 = stats.summarize(h, sad.view(np.int64), _zero(3), "yuv444p", 10, 10)
    assert math.isnan(r2["dif_y"][0]) and r2["dif_v"].tolist()[1:] == [0.0, 2.5]
    rep = stats.report(r, "/some/dir/x.avi", per_frame=True)
    assert rep["dif_y_frames"] == [None, 0.0, 1.0] and rep["file"] == "x.avi" and rep["spec"] == "PP-STATS-1"
    assert "NaN" not in json.dumps(rep)
    one = stats.summarize(h[:1], sad[:1], _zero(1), "yuv444p", 10, 10)
    assert stats.report(one, "x")["dif_y"] is None  # a one-frame clip has no difference at all


def test_the_black_threshold_at_both_depths():
    # 8 bits: 16 + 0.10 * 219 = 37.9: black up to 37; 98 of 100 samples are enough
    fr = [[{37: 98, 200: 2}, {128: 100}, {128: 100}], [{37: 97, 200: 3}, {128: 100}, {128: 100}],
          [{38: 100}, {128: 100}, {128: 100}], [{16: 100}, {128: 100}, {128: 100}]]
    r = stats.summarize(_hist("yuv444p", fr), None, _zero(4), "yuv444p", 10, 10)
    assert r["black"].tolist() == [True, False, False, True]
    assert r["clip"]["black_frames"] == [[0, 0], [3, 3]]
    # 10 bits: 64 + 0.10 * 876 = 151.6: black up to 151
    fr = [[{151: 98, 900: 2}, {512: 100}, {512: 100}], [{152: 100}, {512: 100}, {512: 100}],
          [{64: 97, 152: 3}, {512: 100}, {512: 100}]]
    r = stats.summarize(_hist("yuv444p10le", fr), None, _zero(3), "yuv444p10le", 10, 10)
    assert r["black"].tolist() == [True, False, False]
    # both thresholds are parameters
    r = stats.summarize(_hist("yuv444p10le", fr), None, _zero(3), "yuv444p10le", 10, 10, pix_th=0.11, pic_th=0.97)
    assert r["black"].tolist() == [True, True, True]  # 64 + 96.36: up to 160
    # chroma is 4:2:0 here: the share is of the luma samples
    r = stats.summarize(_hist("yuv420p", [[{16: 98, 99: 2}, {128: 25}, {128: 25}]]), None, _zero(1), "yuv420p", 10, 10)
    assert r["black"].tolist() == [True]


def test_runs_of_repeated_frames():
    n = 11
    h = _hist("yuv444p", [[{50: 100}] * 3] * n)
    sad = np.full((n, 3), 5, np.uint64)
    sad[0] = ABSENT
    for k in (1, 2, 4, 7, 8, 9):
        sad[k] = 0
    sad[5] = (0, 0, 1)  # one plane differs: no repeat
    r = stats.summarize(h, sad, _zero(n), "yuv444p", 10, 10)
    assert r["clip"]["repeat_frames"] == [[1, 2], [4, 4], [7, 9]]
    sad[10] = 0
    assert stats.summarize(h, sad, _zero(n), "yuv444p", 10, 10)["clip"]["repeat_frames"] == [[1, 2], [4, 4], [7, 10]]
    assert stats.summarize(h[:0], sad[:0], _zero(0), "yuv444p", 10, 10)["clip"]["repeat_frames"] == []


# -------------------------------------------------------------- the reference
@pytest.mark.parametrize("fmt", PLANAR)
def test_reference_identity_on_pitched_planes(fmt):
    f = formats.fmt(fmt)
    rng = np.random.default_rng(len(fmt))
    for w, h in ((1, 1), (17, 3), (130, 67)):
        dt = np.uint16 if f.depth > 8 else np.uint8
        arrs = [rng.integers(0, 1 << (16 if f.depth > 8 else 8), (3, r + 2, c + 5)).astype(dt)
                for r, c in formats.plane_shapes(f, w, h)]
        hist, sad, over = stats_ref.batch_arrays(fmt, w, h, arrs)
        size = np.array([r * c for r, c in formats.plane_shapes(f, w, h)])
        assert np.array_equal(hist.sum(axis=2) + over, np.broadcast_to(size, (3, 3)))
        assert (sad[0] == stats_ref.SAD_ABSENT).all() and (sad[1:] != stats_ref.SAD_ABSENT).all()
        if f.depth == 8:
            assert not over.any()
        elif w > 1:
            assert over.any()
        # padding plays no part
        arrs2 = [a.copy() for a in arrs]
        for a, (r, c) in zip(arrs2, formats.plane_shapes(f, w, h)):
            a[:, r:, :] ^= 1
            a[:, :, c:] ^= 1
        for x, y in zip(stats_ref.batch_arrays(fmt, w, h, arrs2), (hist, sad, over)):
            assert np.array_equal(x, y)


def test_reference_known_answers():
    y = np.array([[1, 2, 9], [2, 300, 9]], np.uint16)
    c = np.array([[1023, 9], [1024, 9]], np.uint16)
    hist, sad, over = stats_ref.frame_arrays("yuv422p10le", 2, 2, [y, c, c], prev=[y + 3, c, c[::-1]])
    assert hist[0, 1] == 1 and hist[0, 2] == 2 and hist[0, 300] == 1 and hist[0].sum() == 4
    assert hist[1, 1023] == 1 and hist[1].sum() == 1 and over.tolist() == [0, 1, 1]
    assert sad.tolist() == [12, 0, 2]


# ------------------------------------------------------------ argument checks
def _frames(data=(0x1000, 0x2000, 0x3000), ls=(256, 128, 128)):
    s = _native.pp_frames()
    for p in range(3):
        s.data[p] = data[p]
        s.linesize[p] = ls[p]
        s.frame_stride[p] = ls[p] * 64
    return s


def _call(ctx, fmt, w, h, src, n=1, prev=None, hist=0x4000, sad=0x5000, over=0x6000):
    L = _native.lib()
    return L.pp_frame_stats(ctx, fmt, w, h, None if src is None else ctypes.byref(src), n,
                            None if prev is None else ctypes.byref(prev), ctypes.c_void_p(hist), ctypes.c_void_p(sad),
                            ctypes.c_void_p(over), None)


def test_pp_frame_stats_argument_checks_need_no_gpu():
    L = _native.lib()
    ctx = (ctypes.c_uint8 * 256)()  # never dereferenced: every call below is refused first
    P8, P10 = formats.YUV422P, formats.YUV422P10LE
    src = _frames()
    assert _call(None, P8, 48, 8, src) == -1 and b"null" in L.pp_last_error()
    assert _call(ctx, P8, 48, 8, None) == -1
    assert _call(ctx, P8, 48, 8, src, hist=None) == -1
    assert _call(ctx, P8, 48, 8, src, over=None) == -1
    for bad in (-1, 8, 99):
        assert _call(ctx, bad, 48, 8, src) == -1 and b"format" in L.pp_last_error()
    for packed in (formats.UYVY422, formats.V210):
        assert _call(ctx, packed, 48, 8, src) == -1 and b"packed" in L.pp_last_error()
        assert _call(ctx, packed, 48, 8, src, n=0) == -1
    assert _call(ctx, P8, 0, 8, src) == -1 and b"0x8" in L.pp_last_error()
    assert _call(ctx, P8, 48, 0, src) == -1
    assert _call(ctx, P8, 48, 8, src, n=-1) == -1 and b"nframes" in L.pp_last_error()
    assert _call(ctx, P8, 300, 8, src) == -1 and b"linesize" in L.pp_last_error()
    assert _call(ctx, P8, 48, 8, _frames(ls=(256, 23, 128))) == -1 and b"plane 1" in L.pp_last_error()
    assert _call(ctx, P10, 48, 8, _frames(ls=(95, 128, 128))) == -1
    assert _call(ctx, P8, 48, 8, _frames(data=(0x1000, 0, 0x3000))) == -1 and b"null" in L.pp_last_error()
    # prev is checked like src, but only when the differences are asked for
    assert _call(ctx, P8, 48, 8, src, prev=_frames(ls=(47, 128, 128))) == -1 and b"prev" in L.pp_last_error()
    assert _call(ctx, P8, 48, 8, src, prev=_frames(data=(0x1000, 0x2000, 0))) == -1
    assert _call(ctx, P8, 48, 8, src, prev=_frames(ls=(47, 128, 128)), sad=None, n=0) == 0
    # a bin is 32 bits: a plane of 2^31 samples; and the 2 GiB buffer range
    big = _frames(ls=(1 << 16, 1 << 15, 1 << 15))
    assert _call(ctx, formats.YUV420P, 1 << 16, 1 << 15, big) == -4 and b"2^31" in L.pp_last_error()
    assert _call(ctx, formats.YUV420P, 1 << 15, 1 << 15, big) == -4 and b"2 GiB" in L.pp_last_error()
    assert _call(ctx, formats.YUV420P, 1 << 15, 1 << 14, big, n=0) == 0
    # accepted geometry with nothing to do: OK without touching the context
    assert _call(ctx, P8, 47, 7, src, n=0) == 0
    assert _call(ctx, P10, 47, 7, src, n=0, sad=None) == 0


def test_frame_stats_is_exported_without_an_abi_bump():
    assert "pp_frame_stats" in _native.EXPORTS
    assert _native.lib().pp_abi_version() == 7


def test_geometry_constants_match_the_kernel():
    import os
    src = open(os.path.join(os.path.dirname(_native.__file__), "..", "csrc", "stats.hip")).read()
    assert "kStLaneBytes = %d;" % stats.LANE_BYTES in src and "kStLaneRows = %d;" % stats.WAVE_ROWS in src
    assert "kStFrames = %d;" % stats.FRAMES_PER_WORKGROUP in src and "kStLanes = 64;" in src and "kStWaves = 4;" in src
    assert stats.TILE_BYTES == 64 * stats.LANE_BYTES and stats.TILE_ROWS == 4 * stats.WAVE_ROWS


# ------------------------------------------------------------------ cli stats
def test_cli_stats_options(monkeypatch, capsys):
    from pixpath import cli
    seen = {}
    h = _hist("yuv420p", [[{16: 16}, {128: 4}, {128: 4}], [{16: 15, 235: 1}, {128: 4}, {100: 4}]])
    sad = np.array([[ABSENT] * 3, [219, 0, 112]], np.uint64)
    res = stats.summarize(h, sad, _zero(2), "yuv420p", 4, 4, histogram=True)
    res.update({"fmt": "yuv420p", "w": 4, "h": 4})

    def stub(path, **kw):
        seen.clear()
        seen.update(kw, path=path)
        return res

    monkeypatch.setattr(stats, "stats_of_file", stub)
    assert cli.main(["stats", "dir/x.avi"]) == 0
    assert seen == {"path": "dir/x.avi", "batch": 32, "pix_th": 0.10, "pic_th": 0.98, "histogram": False}
    line = capsys.readouterr().out
    assert line.count("\n") == 1 and "NaN" not in line
    d = json.loads(line)
    assert d["spec"] == "PP-STATS-1" and d["file"] == "x.avi" and d["frames"] == 2
    assert (d["fmt"], d["w"], d["h"]) == ("yuv420p", 4, 4)
    assert d["min_y"] == 16.0 and d["max_y"] == 235.0 and d["bitdepth_y"] == 7 and d["out_of_range_y"] == 0
    assert d["dif_y"] == 219 / 16 and d["dif_u"] == 0.0 and d["avg_v"] == 114.0
    assert d["black_frames"] == [[0, 0]] and d["repeat_frames"] == []
    assert d["histogram_u"][128] == 8 and len(d["histogram_y"]) == 256
    assert "min_y_frames" not in d and "black" not in d
    assert cli.main(["stats", "x.avi", "--per-frame", "--histogram", "--crop", "64x48", "--avpvs-pix-fmt", "yuv420p",
                     "--black-pix-th", "0.2", "--black-pic-th", "0.5", "--batch", "7"]) == 0
    assert seen == {"path": "x.avi", "batch": 7, "pix_th": 0.2, "pic_th": 0.5, "histogram": True,
                    "crop": (64, 48), "crop_from": "yuv420p"}
    d = json.loads(capsys.readouterr().out)
    assert d["dif_y_frames"] == [None, 219 / 16] and d["max_y_frames"] == [16.0, 235.0]
    assert d["black"] == [True, False] and d["repeat"] == [False, False]
    assert d["over_v_frames"] == [0, 0] and d["high_v_frames"] == [128.0, 100.0]
    assert d["low_v_frames"] == [0.0, 0.0]  # rint(0.10 * 4) = 0 samples are reached at bin 0: the rule as written
    with pytest.raises(SystemExit):
        cli.main(["stats", "x.avi", "--avpvs-pix-fmt", "yuv420p"])
