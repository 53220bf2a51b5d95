"""PP-ADM-1 end to end: `metrics_of_files(adm=True)` and `cli metrics --adm` on
two small written clips must give what adm_ref.terms and its pool give for the
files' luma, with and without `--align`, `--crop`, `--per-frame`, `--vif` and
`--ms-ssim`; and without the flag the line is what it was.  The bar on the sums
is test_gpu_adm's; a pooled value adds cube roots of such sums to 3c and
divides two of those, so it is within twice that."""
import json

import numpy as np
import pytest

import adm_ref as R
import synth
from file_clips import growing_error_pair, last_line as _line, write_cpvs, write_y4m
from test_gpu_adm import REL

pytestmark = pytest.mark.gpu
FMT, W, H, N, RATE = "yuv422p10le", 64, 36, 12, 60
FREEZE = [[0.1, 0.05]]  # frames 6..8 show frame 5
ADM_KEYS = {"adm2_y", "adm_scales_y", "adm2_y_frames", "adm_scales_y_frames"}


def _want(ref, dist):
    """adm_ref.terms of every luma pair, none with a position within reach of the angle branch."""
    for a, b in zip(ref, dist):
        assert not any(R.near_branch(a, b, 10))
    return np.stack([R.terms(a, b, 10) for a, b in zip(ref, dist)])


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("adm")
    src, pvs = growing_error_pair(51, FMT, W, H, N)  # the luma gets an error growing with k
    paths = {"src": write_y4m(d / "src.y4m", FMT, RATE, synth.batch(src)), "dir": d, "src_y": [f[0] for f in src],
             "pvs_planes": synth.batch(pvs)}
    paths["pvs"] = write_y4m(d / "pvs.y4m", FMT, RATE, paths["pvs_planes"])
    paths["want"] = _want([f[0] for f in src], [f[0] for f in pvs])
    return paths


def _compare(d, want):
    """The per-frame lists and clip values of a report against the restatement's sums."""
    scales = np.array([R.pool(t, W, H)[0] for t in want])
    v = np.array([R.pool(t, W, H)[1] for t in want])
    got_s, got_v = np.array(d["adm_scales_y_frames"], dtype=np.float64), np.array(d["adm2_y_frames"], dtype=np.float64)
    print("worst relative: scales %.3e adm2 %.3e" % (np.abs(got_s / scales - 1).max(), np.abs(got_v / v - 1).max()))
    assert np.abs(got_s / scales - 1).max() <= 2 * REL and np.abs(got_v / v - 1).max() <= 2 * REL
    assert d["adm2_y"] == pytest.approx(v.mean(), rel=2 * REL)
    assert d["adm_scales_y"] == pytest.approx(scales.mean(axis=0).tolist(), rel=2 * REL)


def test_metrics_of_files_and_cli(gpu, clips, capsys):
    from pixpath import adm, cli, metrics
    res = metrics.metrics_of_files(clips["src"], clips["pvs"], batch=5, adm=True)
    want = clips["want"]
    assert res["frames"] == N and res["adm_scales_y"].shape == (N, 4) and res["adm2_y"].shape == (N,)
    scales, v = adm.pool(want, W, H)
    assert np.abs(res["adm_scales_y"] / scales - 1).max() <= 2 * REL and np.abs(res["adm2_y"] / v - 1).max() <= 2 * REL
    assert res["mean"]["adm2_y"] == pytest.approx(v.mean(), rel=2 * REL)
    # the error grows; the first frame's is small enough to score just above 1 (r = t may exceed o in the angle branch)
    assert 0.9 < res["adm2_y"][-1] < res["adm2_y"][N // 2] < res["adm2_y"][0] < 1.01
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--adm", "--per-frame", "--batch", "5"]) == 0
    d = _line(capsys)
    assert d["frames"] == N and d["spec"] == "PP-METRIC-1"
    _compare(d, want)
    assert d["adm2_y_frames"] == [float(x) for x in res["adm2_y"]]
    # one batch gives the same numbers; without --per-frame only the clip values
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--adm", "--per-frame"]) == 0
    assert _line(capsys) == d
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--adm"]) == 0
    short = _line(capsys)
    assert short["adm2_y"] == d["adm2_y"] and short["adm_scales_y"] == d["adm_scales_y"]
    assert not [k for k in short if k.endswith("_frames")]


def test_without_the_flag_the_line_is_unchanged(gpu, clips, capsys):
    from pixpath import cli, metrics
    res = metrics.metrics_of_files(clips["src"], clips["pvs"], batch=32, flags="bicubic")
    assert not [k for k in list(res) + list(res["mean"]) if "adm" in k]
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--per-frame"]) == 0
    line = capsys.readouterr().out.strip()
    assert line == json.dumps(metrics.report(res, clips["src"], clips["pvs"], per_frame=True))
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--adm", "--per-frame"]) == 0
    with_flag = _line(capsys)
    for k, v in json.loads(line).items():  # the flag only adds keys
        assert with_flag[k] == v
    assert set(with_flag) - set(json.loads(line)) == ADM_KEYS
    # next to --vif and --ms-ssim: every set of keys, each as on its own
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--vif", "--ms-ssim", "--per-frame"]) == 0
    other = _line(capsys)
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--adm", "--vif", "--ms-ssim", "--per-frame"]) == 0
    both = _line(capsys)
    assert set(both) == set(other) | ADM_KEYS
    for k in both:
        assert both[k] == (with_flag[k] if k in ADM_KEYS else other[k])


def test_aligned_freeze(gpu, clips, capsys):
    from pixpath import cli
    from pixpath.stall import stall_schedule
    out = str(clips["dir"] / "freeze.y4m")
    assert cli.main(["stall", "-y", "--input", clips["src"], "--buffer", json.dumps(FREEZE), "--skipping", out]) == 0
    shown = [s for s, _ in stall_schedule(FREEZE, RATE, N, True)]
    assert shown == list(range(6)) + [5] * 3 + list(range(9, 12))
    y = clips["src_y"]
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", out, "--align", "--adm", "--per-frame"]) == 0
    a = _line(capsys)
    assert a["aligned"] is True and a["unmatched"] == 0 and a["frames"] == N
    assert a["adm2_y_frames"] == [1.0] * N and a["adm_scales_y"] == [1.0] * 4  # every frame against the one it shows
    assert cli.main(["metrics", "--ref", clips["src"], "--input", out, "--adm", "--per-frame"]) == 0
    p = _line(capsys)
    _compare(p, _want(y, [y[s] for s in shown]))  # the vf_fps map: frames 6..8 against another picture
    assert [v == 1.0 for v in p["adm2_y_frames"]] == [s == k for k, s in enumerate(shown)]
    assert max(p["adm2_y_frames"][6:9]) < 0.6


def test_crop_of_a_cpvs_canvas(gpu, clips, capsys, tmp_path):
    """The PVS padded onto a 64 x 48 v210 canvas: --crop 64x36 scores the picture inside it, as the PVS itself."""
    from pixpath import cli, metrics
    path = str(tmp_path / "cpvs.avi")
    write_cpvs(path, gpu, FMT, clips["pvs_planes"], 64, 48, RATE)
    res = metrics.metrics_of_files(clips["src"], path, crop=(W, H), adm=True, batch=7)
    plain = metrics.metrics_of_files(clips["src"], clips["pvs"], adm=True)
    assert res["frames"] == N
    assert np.array_equal(res["adm_scales_y"], plain["adm_scales_y"]) and np.array_equal(res["adm2_y"], plain["adm2_y"])
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", path, "--crop", "%dx%d" % (W, H), "--adm",
                     "--per-frame"]) == 0
    _compare(_line(capsys), clips["want"])
