"""PP-ALIGN-1 end to end: a 40-frame 64 x 48 AVPVS goes through `cli stall`
(one stall at t = 0 with --black-frame and one mid-clip; then a --skipping
freeze) and `cli align` must report the map PP-STALL-1's own schedule gives,
`cli metrics --align` must score every pass-through frame against its own
source frame, and plain `cli metrics` must stay what it was.

Margins (checked on the CPU below, with align_ref.track_ref): the frames are
seeded noise, so two different ones sit near 9 dB and a black frame against
any of them near 6 dB, while a 64 x 48 frame shows only the middle of the
128 x 128 spinner, which is almost transparent: the stall frames keep more than
40 dB against the frame they hold.  The 14 dB default separates the two by
5 dB on one side and 26 dB on the other, so the defaults are used as they are."""
import json
import math
import os

import numpy as np
import pytest

import align_ref
import pyoracle as po
import synth
from file_clips import last_line as _line, write_y4m

pytestmark = pytest.mark.gpu
GOLDEN_SPINNER = os.path.join(os.path.dirname(__file__), "golden", "spinner-128-white.png")
FMT, W, H, N, RATE = "yuv422p10le", 64, 48, 40, 60
STALLS = [[0, 0.05], [0.25, 0.1]]  # 3 black frames first; 6 frames on frame 14
FREEZE = [[0.25, 0.1]]             # frames 15..20 show frame 14


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    d = tmp_path_factory.mktemp("align")
    rng = np.random.default_rng(40)
    frames = [synth.noise_frame(rng, po.YUV422P10LE, W, H) for _ in range(N)]
    return {"dir": d, "path": write_y4m(d / "wo_buffer.y4m", FMT, RATE, synth.batch(frames)), "frames": frames}


def _psnr(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    s = int((d * d).sum())
    return math.inf if s == 0 else 10 * math.log10(1023 * 1023 * d.size / s)


def test_stalled_clip(gpu, clip, capsys):
    from pixpath import cli, spinner
    from pixpath.stall import stall_schedule
    out = str(clip["dir"] / "pvs.y4m")
    assert cli.main(["stall", "-y", "--input", clip["path"], "--buffer", json.dumps(STALLS), "--spinner", GOLDEN_SPINNER,
                     "--black-frame", out]) == 0
    anim, delays = spinner.load_apng(GOLDEN_SPINNER)
    seq = stall_schedule(STALLS, RATE, N, False, delays)
    want = [s for s, _ in seq]
    assert want == [-1] * 3 + list(range(15)) + [14] * 6 + list(range(15, 40))

    # the margins, on the CPU: the expected luma of every output frame through track_ref
    frames = clip["frames"]
    black = [np.full((H, W), 64, np.uint16), np.full((H, W // 2), 512, np.uint16), np.full((H, W // 2), 512, np.uint16)]
    luma = []
    for s, sp in seq:
        base = black if s < 0 else frames[s]
        luma.append((base if sp < 0 else po.overlay_spinner(po.YUV422P10LE, base, po.spinner_to_yuva(
            anim[sp], po.YUV422P10LE)))[0])
    ref = np.stack([f[0] for f in frames])
    held = min(_psnr(luma[k], ref[14]) for k in range(18, 24))
    other = max(_psnr(ref[i], ref[j]) for i in range(N) for j in range(i))
    dark = max(_psnr(luma[k], ref[j]) for k in range(3) for j in range(N))
    print("held stall frames >= %.1f dB, different frames <= %.1f dB, black frames <= %.1f dB" % (held, other, dark))
    assert held > 40.0 and other < 10.0 and dark < 8.0
    adv = [0] + [1] * (len(seq) - 1)
    cpu_map, _, _ = align_ref.walk(align_ref.track_ref, np.stack(luma), ref, adv, 32, 64, 14.0, 10)
    assert cpu_map == want

    capsys.readouterr()
    assert cli.main(["align", "--ref", clip["path"], "--input", out, "--per-frame"]) == 0
    d = _line(capsys)
    assert d["spec"] == "PP-ALIGN-1" and d["frames"] == 49 and d["map"] == want
    assert d["holds"] == [[18, 6, 14]] and d["skips"] == [] and d["unmatched_runs"] == [[0, 3]]
    assert (d["matched"], d["unmatched"], d["held_frames"], d["skipped_ref_frames"]) == (46, 3, 6, 0)
    psnr = d["psnr_y_frames"]
    assert psnr[:3] == [None] * 3 and all(v is None for k, v in enumerate(psnr) if seq[k][1] < 0)  # identical: no PSNR
    assert all(v is not None and v > 40.0 for v in psnr[18:24])
    assert cli.main(["align", "--ref", clip["path"], "--input", out, "--batch", "5", "--lookahead", "7"]) == 0
    assert _line(capsys)["holds"] == [[18, 6, 14]]  # several batches, a short band

    assert cli.main(["metrics", "--ref", clip["path"], "--input", out, "--align", "--per-frame"]) == 0
    a = _line(capsys)
    assert a["aligned"] is True and a["unmatched"] == 3 and a["frames"] == 49
    through = [k for k, (s, sp) in enumerate(seq) if s >= 0 and sp < 0]
    assert len(through) == 40
    for name in ("y", "u", "v", "all"):
        assert all(a["mse_%s_frames" % name][k] == 0.0 for k in through)
        assert all(a["psnr_%s_frames" % name][k] is None for k in through)  # MSE 0: no finite PSNR
        assert a["mse_%s_frames" % name][:3] == [None] * 3
    assert all(0 < a["mse_y_frames"][k] for k in range(18, 24))  # the spinner's pixels
    assert cli.main(["metrics", "--ref", clip["path"], "--input", out, "--per-frame"]) == 0
    p = _line(capsys)
    assert "aligned" not in p and p["frames"] == 40
    assert all(p["mse_y_frames"][k] > 0 for k in range(40))  # paired by the nominal map: never its own frame
    assert a["mse_y"] < p["mse_y"] / 100


def test_skipping_freeze(gpu, clip, capsys):
    from pixpath import cli
    from pixpath.stall import stall_schedule
    out = str(clip["dir"] / "pvs_freeze.y4m")
    assert cli.main(["stall", "-y", "--input", clip["path"], "--buffer", json.dumps(FREEZE), "--skipping", out]) == 0
    want = [s for s, _ in stall_schedule(FREEZE, RATE, N, True)]
    assert want == list(range(15)) + [14] * 6 + list(range(21, 40))
    capsys.readouterr()
    assert cli.main(["align", "--ref", clip["path"], "--input", out, "--per-frame", "--batch", "16"]) == 0
    d = _line(capsys)
    assert d["map"] == want and d["holds"] == [[15, 6, 14]] and d["skips"] == [[21, 14, 21]]
    assert (d["matched"], d["unmatched"], d["unmatched_runs"], d["held_frames"], d["skipped_ref_frames"]) == \
        (40, 0, [], 6, 6)
    assert cli.main(["metrics", "--ref", clip["path"], "--input", out, "--align", "--per-frame"]) == 0
    a = _line(capsys)
    assert a["frames"] == 40 and a["unmatched"] == 0 and a["mse_all_frames"] == [0.0] * 40 and a["mse_all"] == 0.0
    assert cli.main(["metrics", "--ref", clip["path"], "--input", out, "--per-frame"]) == 0
    p = _line(capsys)
    assert [v > 0 for v in p["mse_y_frames"]] == [False] * 15 + [True] * 6 + [False] * 19


def test_plain_metrics_unchanged(gpu, clip, capsys):
    """Without --align `cli metrics` prints what metrics_of_files, called as
    before, gives; an identity map gives the same numbers."""
    from pixpath import align, cli, metrics
    rng = np.random.default_rng(41)
    frames = [synth.noise_frame(rng, po.YUV422P10LE, W, H) for _ in range(N)]
    other = write_y4m(clip["dir"] / "noisy.y4m", FMT, RATE, synth.batch(frames))
    res = metrics.metrics_of_files(clip["path"], other, batch=32, flags="bicubic")
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clip["path"], "--input", other, "--per-frame"]) == 0
    line = capsys.readouterr().out.strip()
    assert line == json.dumps(metrics.report(res, clip["path"], other, per_frame=True))
    same = metrics.metrics_of_files(clip["path"], other, ref_index=np.arange(N))
    for key in ("mse_y", "mse_all", "ssim_y", "psnr_v"):
        assert np.array_equal(same[key], res[key], equal_nan=True)
    assert same["mean"] == res["mean"]
    with pytest.raises(ValueError):
        metrics.metrics_of_files(clip["path"], other, ref_index=[3, 2, 1])
    # unrelated clips: nothing matches, and the result says so
    al = align.align_files(clip["path"], other)
    assert (al["map"] == -1).all() and al["unmatched"] == [[0, N]] and al["holds"] == [] and al["skips"] == []
