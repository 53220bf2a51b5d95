"""PP-MSSSIM-1 end to end: `cli metrics --ms-ssim` on a small Y4M pair must
print what msssim_ref.terms and its pool give for the files' luma; with
`--align` on a clip `cli stall --skipping` froze (no spinner) every frame, the
held ones included, scores exactly 1.0 against the frame it shows; and without
the flag the line is what it was."""
import json
import math
import os

import numpy as np
import pytest

import msssim_ref as R
import synth
from file_clips import growing_error_pair, last_line as _line, write_y4m

pytestmark = pytest.mark.gpu
GOLDEN_SPINNER = os.path.join(os.path.dirname(__file__), "golden", "spinner-128-white.png")
FMT, W, H, N, RATE = "yuv422p10le", 180, 176, 24, 60
FREEZE = [[0.2, 0.1]]  # frames 12..17 show frame 11


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("msssim")
    # the luma gets an error growing with k; frame 0 stays identical
    src, pvs = growing_error_pair(50, FMT, W, H, N, error=lambda k: 3 * k)
    paths = {"src": write_y4m(d / "src.y4m", FMT, RATE, synth.batch(src)),
             "pvs": write_y4m(d / "pvs.y4m", FMT, RATE, synth.batch(pvs)), "dir": d}
    paths["want"] = np.stack([R.terms(src[k][0], pvs[k][0], 10) for k in range(N)])
    return paths


def test_cli_metrics_ms_ssim(gpu, clips, capsys):
    from pixpath import cli
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--ms-ssim", "--per-frame", "--batch",
                     "7"]) == 0
    d = _line(capsys)
    want = clips["want"]
    assert d["frames"] == N and d["spec"] == "PP-METRIC-1"
    assert np.abs(np.array(d["cs_scales_y_frames"]) - want[:, :, 0]).max() <= 1e-9
    assert np.abs(np.array(d["ssim_scales_y_frames"]) - want[:, :, 1]).max() <= 1e-9
    assert np.abs(np.array(d["ssim_gauss_y_frames"]) - want[:, 0, 1]).max() <= 1e-9
    pooled = np.array([R.pool(t) for t in want])
    assert pooled.min() > 0.05  # away from 0, where x^0.0448 amplifies without bound
    assert np.abs(np.array(d["ms_ssim_y_frames"]) - pooled).max() <= 1e-8
    assert d["ms_ssim_y_frames"][0] == 1.0 and d["ssim_gauss_y_frames"][0] == 1.0
    assert d["ms_ssim_y"] == pytest.approx(pooled.mean(), abs=1e-8)
    assert d["ssim_gauss_y"] == pytest.approx(want[:, 0, 1].mean(), abs=1e-9)
    ms = d["ms_ssim_y_frames"]
    assert ms[0] > ms[1] > ms[N // 2] > ms[N - 1]  # the error grows
    # one batch gives the same numbers
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--ms-ssim", "--per-frame"]) == 0
    assert _line(capsys) == d


def test_without_the_flag_the_line_is_unchanged(gpu, clips, capsys):
    from pixpath import cli, metrics
    res = metrics.metrics_of_files(clips["src"], clips["pvs"], batch=32, flags="bicubic")
    assert not [k for k in list(res) + list(res["mean"]) if "ms_ssim" in k or "gauss" in k or "scales" in k]
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--per-frame"]) == 0
    line = capsys.readouterr().out.strip()
    assert line == json.dumps(metrics.report(res, clips["src"], clips["pvs"], per_frame=True))
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--ms-ssim", "--per-frame"]) == 0
    with_flag = _line(capsys)
    for k, v in json.loads(line).items():  # the flag only adds keys
        assert with_flag[k] == v
    assert set(with_flag) - set(json.loads(line)) == {
        "ms_ssim_y", "ssim_gauss_y", "ms_ssim_y_frames", "ssim_gauss_y_frames", "cs_scales_y_frames",
        "ssim_scales_y_frames"}


def test_aligned_freeze_scores_one(gpu, clips, capsys):
    from pixpath import cli
    from pixpath.stall import stall_schedule
    out = str(clips["dir"] / "freeze.y4m")
    assert cli.main(["stall", "-y", "--input", clips["src"], "--buffer", json.dumps(FREEZE), "--skipping", out]) == 0
    want = [s for s, _ in stall_schedule(FREEZE, RATE, N, True)]
    assert want == list(range(12)) + [11] * 6 + list(range(18, 24))
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", out, "--align", "--ms-ssim", "--per-frame"]) == 0
    a = _line(capsys)
    assert a["aligned"] is True and a["unmatched"] == 0 and a["frames"] == N
    assert a["ms_ssim_y_frames"] == [1.0] * N and a["ssim_gauss_y_frames"] == [1.0] * N
    assert a["cs_scales_y_frames"] == [[1.0] * 5] * N and a["ms_ssim_y"] == 1.0
    assert cli.main(["metrics", "--ref", clips["src"], "--input", out, "--ms-ssim", "--per-frame"]) == 0
    p = _line(capsys)
    assert [v == 1.0 for v in p["ms_ssim_y_frames"]] == [True] * 12 + [False] * 6 + [True] * 6
    assert max(p["ms_ssim_y_frames"][12:18]) < 0.5
    # a black lead-in has no reference frame: null, and left out of the clip value
    lead = str(clips["dir"] / "lead.y4m")
    assert cli.main(["stall", "-y", "--input", clips["src"], "--buffer", json.dumps([[0, 0.05]]), "--spinner",
                     GOLDEN_SPINNER, "--black-frame", lead]) == 0
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", lead, "--align", "--ms-ssim", "--per-frame"]) == 0
    b = _line(capsys)
    assert b["unmatched"] == 3 and b["ms_ssim_y_frames"] == [None] * 3 + [1.0] * N and b["ms_ssim_y"] == 1.0
    assert b["cs_scales_y_frames"][0] == [None] * 5 and not math.isnan(b["ssim_gauss_y"])
