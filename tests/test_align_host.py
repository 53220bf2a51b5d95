"""The host rule of PP-ALIGN-1 (pixpath.align.track / events) on the CPU,
against the independent restatement (align_ref.track_ref / events_ref) and
against hand-written maps; then the `align` and `metrics --align` argument
parsers.  The SSE matrices come from align_ref.sse_band_ref on seeded 48 x 32
frames of uniform noise in the legal range: two independent ones sit near
9 dB, five below the 14 dB threshold (checked below)."""
import json
import math

import numpy as np
import pytest

import align_ref
from pixpath import align, cli, metrics

W, H, DEPTH = 48, 32, 8
BLACK = 16


def _noise(n, seed):
    return np.random.default_rng(seed).integers(16, 236, (n, H, W)).astype(np.uint8)


def _psnr(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return 10 * math.log10(255 * 255 * d.size / int((d * d).sum()))


def _both(dist, ref, advance=None, batch=8, lookahead=64, min_psnr=14.0):
    """The clip through align.track and through track_ref: equal maps, equal
    winning SSEs, equal events.  Returns (map, events, launches)."""
    adv = [0] + [1] * (len(dist) - 1) if advance is None else [int(v) for v in advance]
    got = align_ref.walk(align.track, dist, ref, adv, batch, lookahead, min_psnr, DEPTH)
    want = align_ref.walk(align_ref.track_ref, dist, ref, adv, batch, lookahead, min_psnr, DEPTH)
    assert got == want
    ev = align.events(got[0], adv)
    assert ev == align_ref.events_ref(got[0], adv)
    return got[0], ev, got[2]


def test_independent_noise_is_far_below_the_threshold():
    f = _noise(6, 1)
    worst = max(_psnr(f[i], f[j]) for i in range(6) for j in range(i))
    print("independent noise frames: at most %.2f dB" % worst)
    assert 8.5 < worst < 9.6
    assert _psnr(np.full((H, W), BLACK, np.uint8), f[0]) < 7.0  # a black frame against noise
    assert align.threshold(W, H, DEPTH, 14.0) == align_ref.threshold_ref(W, H, DEPTH, 14.0) == \
        math.floor(W * H * 65025 * 10 ** -1.4)
    assert align.LOOKAHEAD == 64 and align.MIN_PSNR == 14.0


def test_identity():
    ref = _noise(40, 2)
    m, ev, launches = _both(ref, ref)
    assert m == list(range(40))
    assert ev == {"holds": [], "skips": [], "unmatched": []}
    assert launches == 5


def test_hold_with_a_spinner_like_patch():
    ref = _noise(30, 3)
    src = list(range(10)) + [9] * 5 + list(range(10, 30))
    dist = ref[src].copy()
    dist[10:15, 8:24, 16:32] = _noise(5, 30)[:, :16, :16]  # a 16 x 16 patch overwritten
    margin = min(_psnr(dist[k], ref[9]) for k in range(10, 15))
    print("held frames with the patch: at least %.2f dB" % margin)
    assert margin > 16.0
    m, ev, _ = _both(dist, ref)
    assert m == src
    assert ev == {"holds": [[10, 5, 9]], "skips": [], "unmatched": []}


def test_black_frames_first():
    ref = _noise(20, 4)
    dist = np.concatenate([np.full((3, H, W), BLACK, np.uint8), ref])
    m, ev, _ = _both(dist, ref)
    assert m == [-1, -1, -1] + list(range(20))  # the cursor stayed at 0: frame 3 found reference frame 0
    assert ev == {"holds": [], "skips": [], "unmatched": [[0, 3]]}


def test_skipping_freeze():
    ref = _noise(30, 5)
    src = list(range(10)) + [9] * 4 + list(range(14, 30))  # hold 4 frames, then jump ahead 4
    m, ev, _ = _both(ref[src], ref)
    assert m == src
    assert ev == {"holds": [[10, 4, 9]], "skips": [[14, 9, 14]], "unmatched": []}
    rep = align.report({"map": np.array(m), "sse": np.zeros(30, np.int64), "advance": np.array([0] + [1] * 29),
                        "frames": 30, "w": W, "h": H, "depth": 8, **ev}, "/a/src.y4m", "/b/pvs.avi", per_frame=True)
    assert (rep["held_frames"], rep["skipped_ref_frames"], rep["matched"], rep["unmatched"]) == (4, 4, 30, 0)
    assert rep["map"] == src and rep["psnr_y_frames"] == [None] * 30 and rep["spec"] == "PP-ALIGN-1"


@pytest.mark.parametrize("in_rate,out_rate,n_ref", [(30, 60, 20), (60, 30, 40)])
def test_rate_conversion(in_rate, out_rate, n_ref):
    from pixpath import ops
    ref = _noise(n_ref, 6)
    nom = ops.fps_map(n_ref, in_rate, out_rate).tolist()
    adv = align.nominal_advances(0, len(nom), in_rate, out_rate).tolist()
    assert adv == [0] + [b - a for a, b in zip(nom, nom[1:])]
    split = align.nominal_advances(0, 7, in_rate, out_rate).tolist() + \
        align.nominal_advances(7, len(nom) - 7, in_rate, out_rate).tolist()
    assert split == adv
    m, ev, _ = _both(ref[nom], ref, advance=adv)
    assert m == nom
    assert ev == {"holds": [], "skips": [], "unmatched": []}  # repeats at d_k = 0 are no holds, d_k = 2 no skip


def test_static_run_longer_than_the_lookahead():
    a, s, b = _noise(5, 7), _noise(1, 8), _noise(10, 9)
    ref = np.concatenate([a, np.repeat(s, 80, axis=0), b])
    m, ev, _ = _both(ref, ref, lookahead=64)
    assert m == list(range(95))  # the ties follow d_k: neither lagging nor running ahead, B found at the end
    assert ev == {"holds": [], "skips": [], "unmatched": []}
    # a stall inside the static run cannot be seen; the tracker runs ahead of it and still finds B
    src = list(range(40)) + [39] * 10 + list(range(40, 95))
    m, ev, _ = _both(ref[src], ref, lookahead=64)
    assert m[:85] == list(range(85)) and m[-10:] == list(range(85, 95))


def test_lookahead_limit():
    ref = _noise(40, 10)
    L = 8
    src = [0, 1, 2] + list(range(2 + L - 1, 30))  # a jump of lookahead - 1
    m, ev, _ = _both(ref[src], ref, lookahead=L)
    assert m == src and ev["skips"] == [[3, 2, 2 + L - 1]]
    src = [0, 1, 2] + list(range(2 + L, 30))      # a jump of lookahead: outside the candidates for good
    m, ev, _ = _both(ref[src], ref, lookahead=L)
    assert m == [0, 1, 2] + [-1] * (len(src) - 3)
    assert ev == {"holds": [], "skips": [], "unmatched": [[3, len(src) - 3]]}


def test_skips_past_the_band_relaunch():
    ref = _noise(60, 11)
    src = [0, 7, 14, 21, 28, 29, 30, 31]  # four jumps of lookahead - 1 inside one batch of 8: band 8 + 7
    m, ev, launches = _both(ref[src], ref, batch=8, lookahead=8)
    assert m == src and launches > 1
    assert ev["skips"] == [[1, 0, 7], [2, 7, 14], [3, 14, 21], [4, 21, 28]]


def _rows(*rows):
    return np.array(rows, dtype=np.uint64)


def test_threshold_is_inclusive():
    thr = align.threshold(W, H, DEPTH, 14.0)
    for tr in (align.track, align_ref.track_ref):
        args = ([0, 0], [0, 1], 100, 4, 14.0, W, H, DEPTH, 0)
        mp, ss, c = tr(_rows([thr + 5, thr, thr + 9, thr + 7, 0], [0, thr + 3, thr + 1, thr + 2, thr + 9]), *args)
        assert list(mp) == [1, -1] and list(ss) == [thr, -1] and c == 1


def test_absent_entries_are_never_chosen():
    A = align_ref.ABSENT
    for tr in (align.track, align_ref.track_ref):
        rows = _rows([A, A, 5, 9, 0, 0], [0, 0, A, A, A, A])  # the zeros lie outside the candidates
        mp, ss, c = tr(rows, [0, 0], [0, 1], 100, 4, 14.0, W, H, DEPTH, 0)
        assert list(mp) == [2, -1] and list(ss) == [5, -1] and c == 2
        # the same rows as the int64 view the wrapper returns
        mp, _, _ = tr(rows.view(np.int64), [0, 0], [0, 1], 100, 4, 14.0, W, H, DEPTH, 0)
        assert list(mp) == [2, -1]
        # a row that does not hold every candidate ends the walk
        mp, _, c = tr(_rows([0, 7, 7, 7], [7, 7, 7, 7]), [0, 0], [0, 3], 100, 4, 14.0, W, H, DEPTH, 1)
        assert list(mp) == [] and c == 1


def test_ties_go_to_the_nominal_advance_then_to_the_smaller_index():
    for tr in (align.track, align_ref.track_ref):
        for adv, want in ((0, 0), (1, 1), (2, 2), (3, 2)):
            mp, _, _ = tr(_rows([3, 3, 3, 9, 1]), [0], [adv], 100, 4, 14.0, W, H, DEPTH, 0)
            assert list(mp) == [want]
        mp, _, _ = tr(_rows([3, 9, 3, 9]), [0], [1], 100, 4, 14.0, W, H, DEPTH, 0)
        assert list(mp) == [0]  # both one away from cursor + 1: the smaller


def _fake_align():
    adv = np.array([0, 1, 1, 1], np.int64)
    res = {"map": np.array([-1, 0, 0, 3], np.int32), "sse": np.array([-1, 0, 640, 0], np.int64), "advance": adv,
           "w": 16, "h": 16, "depth": 8, "frames": 4}
    res.update(align.events(res["map"], adv))
    return res


def test_cli_align_json(monkeypatch, capsys):
    seen = {}

    def stub(ref, dist, **kw):
        seen.update(ref=ref, dist=dist, **kw)
        return _fake_align()

    monkeypatch.setattr(align, "align_files", stub)
    assert cli.main(["align", "--ref", "/a/src.y4m", "--input", "/b/pvs.avi"]) == 0
    assert seen == {"ref": "/a/src.y4m", "dist": "/b/pvs.avi", "batch": 32, "flags": "bicubic"}
    line = capsys.readouterr().out.strip()
    assert "\n" not in line and "NaN" not in line
    d = json.loads(line)
    assert d == {"ref": "src.y4m", "file": "pvs.avi", "spec": "PP-ALIGN-1", "frames": 4, "matched": 3, "unmatched": 1,
                 "unmatched_runs": [[0, 1]], "holds": [[2, 1, 0]], "skips": [[3, 0, 3]], "held_frames": 1,
                 "skipped_ref_frames": 2}
    seen.clear()
    assert cli.main(["align", "--ref", "r.y4m", "--input", "d.avi", "--per-frame", "--lookahead", "9", "--min-psnr",
                     "20.5", "--crop", "64x48", "--avpvs-pix-fmt", "yuv420p", "--flags", "lanczos", "--batch", "5"]) == 0
    assert seen == {"ref": "r.y4m", "dist": "d.avi", "batch": 5, "flags": "lanczos", "lookahead": 9, "min_psnr": 20.5,
                    "crop": (64, 48), "crop_from": "yuv420p"}
    d = json.loads(capsys.readouterr().out)
    assert d["map"] == [-1, 0, 0, 3]
    assert d["psnr_y_frames"] == [None, None, pytest.approx(10 * math.log10(65025 * 256 / 640)), None]
    with pytest.raises(SystemExit):
        cli.main(["align", "--input", "d.y4m"])


def test_cli_metrics_align(monkeypatch, capsys):
    calls = []

    def old_signature(ref, dist, batch=32, flags="bicubic"):  # what `cli metrics` called before PP-ALIGN-1
        calls.append((ref, dist, batch, flags))
        return metrics.summarize(np.array([[640, 0, 16], [0, 0, 0]]), np.array([[.75, np.nan, .5], [1, np.nan, 1]]),
                                 "yuv420p", 16, 16)

    monkeypatch.setattr(metrics, "metrics_of_files", old_signature)
    monkeypatch.setattr(align, "align_files", lambda *a, **k: pytest.fail("aligned without --align"))
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--batch", "7"]) == 0
    assert calls == [("r.y4m", "d.y4m", 7, "bicubic")]
    plain = json.loads(capsys.readouterr().out)
    assert "aligned" not in plain and "unmatched" not in plain
    with pytest.raises(SystemExit):
        cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--lookahead", "3"])

    seen = {}

    def scored(ref, dist, **kw):
        seen.update(kw)
        m = kw["ref_index"]
        return metrics.summarize(np.zeros((4, 3), np.int64), np.ones((4, 3)), "yuv420p", 16, 16, matched=m >= 0)

    monkeypatch.setattr(metrics, "metrics_of_files", scored)
    monkeypatch.setattr(align, "align_files", lambda ref, dist, **kw: seen.update(align_kw=kw) or _fake_align())
    assert cli.main(["metrics", "--ref", "r.y4m", "--input", "d.y4m", "--align", "--min-psnr", "11", "--per-frame"]) == 0
    assert seen["align_kw"] == {"batch": 32, "flags": "bicubic", "min_psnr": 11.0}
    assert seen["ref_index"].tolist() == [-1, 0, 0, 3] and seen["batch"] == 32
    d = json.loads(capsys.readouterr().out)
    assert d["aligned"] is True and d["unmatched"] == 1 and d["frames"] == 4
    assert d["mse_y_frames"] == [None, 0.0, 0.0, 0.0] and d["ssim_y_frames"] == [None, 1.0, 1.0, 1.0]
    assert d["mse_y"] == 0.0 and d["ssim_all"] == 1.0


def test_summarize_leaves_unmatched_frames_out():
    sse = np.array([[640, 64, 16], [9999, 9999, 9999], [0, 0, 0]], np.int64)
    ssim = np.array([[0.75, 0.5, 0.5], [0.1, 0.1, 0.1], [1.0, 1.0, 1.0]])
    res = metrics.summarize(sse, ssim, "yuv420p", 16, 16, matched=[True, False, True])
    two = metrics.summarize(sse[[0, 2]], ssim[[0, 2]], "yuv420p", 16, 16)
    assert res["mean"] == two["mean"] and res["frames"] == 3
    for key in ("mse_y", "psnr_all", "ssim_v"):
        assert np.isnan(res[key][1]) and np.array_equal(res[key][[0, 2]], two[key], equal_nan=True)
    same = metrics.summarize(sse, ssim, "yuv420p", 16, 16)
    assert not np.isnan(same["mse_y"]).any() and same["frames"] == 3
