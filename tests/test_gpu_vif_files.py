"""PP-VIF-1 end to end: `metrics_of_files(vif=True)` and `cli metrics --vif` on
two small written clips must give what vif_ref.terms and its pool give for the
files' luma, with and without `--align`, `--crop`, `--per-frame` and
`--ms-ssim`; and without the flag the line is what it was.  The bar on the sums
is test_gpu_vif's; a ratio of two such sums is within twice that."""
import json

import numpy as np
import pytest

import synth
from file_clips import growing_error_pair, last_line as _line, write_cpvs, write_y4m
import vif_ref as R
from test_gpu_vif import BAR

pytestmark = pytest.mark.gpu
FMT, W, H, N, RATE = "yuv422p10le", 64, 36, 12, 60
FREEZE = [[0.1, 0.05]]  # frames 6..8 show frame 5
VIF_KEYS = {"vif_y", "vif_scales_y", "vif_y_frames", "vif_scales_y_frames"}


def _want(ref, dist):
    """vif_ref.terms of every luma pair, none with a position on a branch."""
    for a, b in zip(ref, dist):
        assert not any(R.near_branch(a, b, 10))
    return np.stack([R.terms(a, b, 10) for a, b in zip(ref, dist)])


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("vif")
    src, pvs = growing_error_pair(51, FMT, W, H, N)  # the luma gets an error growing with k
    paths = {"src": write_y4m(d / "src.y4m", FMT, RATE, synth.batch(src)), "dir": d, "src_y": [f[0] for f in src],
             "pvs_planes": synth.batch(pvs)}
    paths["pvs"] = write_y4m(d / "pvs.y4m", FMT, RATE, paths["pvs_planes"])
    paths["want"] = _want([f[0] for f in src], [f[0] for f in pvs])
    return paths


def _compare(d, want):
    """The per-frame lists and clip values of a report against the restatement's sums."""
    scales = np.array([R.pool(t)[0] for t in want])
    v = np.array([R.pool(t)[1] for t in want])
    got_s, got_v = np.array(d["vif_scales_y_frames"], dtype=np.float64), np.array(d["vif_y_frames"], dtype=np.float64)
    print("worst relative: scales %.3e vif %.3e" % (np.abs(got_s / scales - 1).max(), np.abs(got_v / v - 1).max()))
    assert np.abs(got_s / scales - 1).max() <= 2 * BAR and np.abs(got_v / v - 1).max() <= 2 * BAR
    assert d["vif_y"] == pytest.approx(v.mean(), rel=2 * BAR)
    assert d["vif_scales_y"] == pytest.approx(scales.mean(axis=0).tolist(), rel=2 * BAR)


def test_metrics_of_files_and_cli(gpu, clips, capsys):
    from pixpath import cli, metrics, vif
    res = metrics.metrics_of_files(clips["src"], clips["pvs"], batch=5, vif=True)
    want = clips["want"]
    assert res["frames"] == N and res["vif_scales_y"].shape == (N, 4) and res["vif_y"].shape == (N,)
    scales, v = vif.pool(want)
    assert np.abs(res["vif_scales_y"] / scales - 1).max() <= 2 * BAR and np.abs(res["vif_y"] / v - 1).max() <= 2 * BAR
    assert res["mean"]["vif_y"] == pytest.approx(v.mean(), rel=2 * BAR)
    assert (np.diff(res["vif_y"]) < 0).all() and 0 < res["vif_y"][-1] < res["vif_y"][0] < 1  # the error grows
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--vif", "--per-frame", "--batch", "5"]) == 0
    d = _line(capsys)
    assert d["frames"] == N and d["spec"] == "PP-METRIC-1"
    _compare(d, want)
    assert d["vif_y_frames"] == [float(x) for x in res["vif_y"]]
    # one batch gives the same numbers; without --per-frame only the clip values
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--vif", "--per-frame"]) == 0
    assert _line(capsys) == d
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--vif"]) == 0
    short = _line(capsys)
    assert short["vif_y"] == d["vif_y"] and short["vif_scales_y"] == d["vif_scales_y"]
    assert not [k for k in short if k.endswith("_frames")]


def test_without_the_flag_the_line_is_unchanged(gpu, clips, capsys):
    from pixpath import cli, metrics
    res = metrics.metrics_of_files(clips["src"], clips["pvs"], batch=32, flags="bicubic")
    assert not [k for k in list(res) + list(res["mean"]) if "vif" in k]
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--per-frame"]) == 0
    line = capsys.readouterr().out.strip()
    assert line == json.dumps(metrics.report(res, clips["src"], clips["pvs"], per_frame=True))
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--vif", "--per-frame"]) == 0
    with_flag = _line(capsys)
    for k, v in json.loads(line).items():  # the flag only adds keys
        assert with_flag[k] == v
    assert set(with_flag) - set(json.loads(line)) == VIF_KEYS
    # next to --ms-ssim: both sets of keys, each as on its own
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--ms-ssim", "--per-frame"]) == 0
    ms = _line(capsys)
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--vif", "--ms-ssim", "--per-frame"]) == 0
    both = _line(capsys)
    assert set(both) == set(ms) | VIF_KEYS
    for k in both:
        assert both[k] == (with_flag[k] if k in VIF_KEYS else ms[k])


def test_aligned_freeze(gpu, clips, capsys):
    from pixpath import cli
    from pixpath.stall import stall_schedule
    out = str(clips["dir"] / "freeze.y4m")
    assert cli.main(["stall", "-y", "--input", clips["src"], "--buffer", json.dumps(FREEZE), "--skipping", out]) == 0
    shown = [s for s, _ in stall_schedule(FREEZE, RATE, N, True)]
    assert shown == list(range(6)) + [5] * 3 + list(range(9, 12))
    y = clips["src_y"]
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", out, "--align", "--vif", "--per-frame"]) == 0
    a = _line(capsys)
    assert a["aligned"] is True and a["unmatched"] == 0 and a["frames"] == N
    _compare(a, _want([y[s] for s in shown], [y[s] for s in shown]))  # every frame against the one it shows
    assert min(a["vif_y_frames"]) > 0.99
    assert cli.main(["metrics", "--ref", clips["src"], "--input", out, "--vif", "--per-frame"]) == 0
    p = _line(capsys)
    _compare(p, _want(y, [y[s] for s in shown]))  # the vf_fps map: frames 6..8 against another picture
    assert [v > 0.99 for v in p["vif_y_frames"]] == [s == k for k, s in enumerate(shown)]
    assert max(p["vif_y_frames"][6:9]) < 0.1


def test_crop_of_a_cpvs_canvas(gpu, clips, capsys, tmp_path):
    """The PVS padded onto a 64 x 48 v210 canvas: --crop 64x36 scores the picture inside it, as the PVS itself."""
    from pixpath import cli, metrics
    path = str(tmp_path / "cpvs.avi")
    write_cpvs(path, gpu, FMT, clips["pvs_planes"], 64, 48, RATE)
    res = metrics.metrics_of_files(clips["src"], path, crop=(W, H), vif=True, batch=7)
    plain = metrics.metrics_of_files(clips["src"], clips["pvs"], vif=True)
    assert res["frames"] == N
    assert np.array_equal(res["vif_scales_y"], plain["vif_scales_y"]) and np.array_equal(res["vif_y"], plain["vif_y"])
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", path, "--crop", "%dx%d" % (W, H), "--vif",
                     "--per-frame"]) == 0
    _compare(_line(capsys), clips["want"])
