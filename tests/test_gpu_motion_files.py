"""PP-MOTION-1 end to end on small written clips: `metrics_of_files(motion=True)`,
`motion.motion_of_file` and `cli metrics --motion / --vmaf-features` must give
what motion_ref gives for the reference frames as shown, across batch seams,
window rebuilds, a rate change, the scaler and an explicit map with unmatched
frames; and without the new flags the line is what it was.  The sums are
integers and the host arithmetic is the same few float64 operations on both
sides: every comparison is exact."""
import json
import math

import numpy as np
import pytest

import motion_ref as R
import pyoracle as po
import synth
from file_clips import last_line as _line, write_y4m

pytestmark = pytest.mark.gpu
FMT, W, H, N, RATE = "yuv422p10le", 64, 36, 12, 60
MOTION_KEYS = {"motion_y", "motion2_y", "motion_y_frames", "motion2_y_frames"}
BASE_KEYS = {"ref", "file", "frames", "spec"} | {"%s_%s%s" % (kind, name, tail) for kind in ("mse", "psnr", "ssim")
                                                  for name in ("y", "u", "v", "all") for tail in ("", "_frames")}


def _write(path, frames, rate=RATE):
    write_y4m(path, FMT, rate, synth.batch(frames))


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("motion")
    rng = np.random.default_rng(61)
    src = [synth.noise_frame(rng, po.YUV422P10LE, W, H) for _ in range(N)]
    src[4] = [p.copy() for p in src[3]]  # a repeated picture inside the clip
    pvs = [[np.clip(f[0].astype(np.int64) + rng.integers(-9, 10, f[0].shape), 0, 1023).astype(np.uint16), f[1], f[2]]
           for f in src]
    paths = {"src": str(d / "src.y4m"), "pvs": str(d / "pvs.y4m"), "dir": d, "src_y": np.stack([f[0] for f in src]),
             "src_frames": src}
    _write(paths["src"], src)
    _write(paths["pvs"], pvs)
    paths["sad"] = R.sad(paths["src_y"], 10)
    paths["motion"] = R.motion(paths["sad"], W, H)
    return paths


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def test_batches_and_motion_of_file_agree(gpu, clips):
    """Batch 3, 7 and 32: the carried prev across batch seams and window rebuilds changes nothing."""
    from pixpath import metrics, motion
    m, m2 = clips["motion"]
    assert m[0] == 0.0 and m[4] == 0.0 and min(m[1:4] + m[5:]) > 1.0  # frame 4 repeats frame 3
    for batch in (3, 7, 32):
        res = metrics.metrics_of_files(clips["src"], clips["pvs"], batch=batch, motion=True)
        own = motion.motion_of_file(clips["src"], batch=batch)
        assert res["frames"] == N == own["frames"] and (own["w"], own["h"]) == (W, H)
        for got in (res, own):
            assert got["motion_y"].tolist() == m and got["motion2_y"].tolist() == m2, batch
        assert res["mean"]["motion_y"] == own["mean"]["motion_y"] == float(np.mean(m))
        assert res["mean"]["motion2_y"] == own["mean"]["motion2_y"] == float(np.mean(m2))


def test_half_rate_reference_repeats_give_exact_zeros(gpu, clips, tmp_path):
    from pixpath import metrics, ops
    ref = str(tmp_path / "ref30.y4m")
    _write(ref, clips["src_frames"][:6], rate=RATE // 2)
    shown = [int(v) for v in ops.fps_map(6, RATE // 2, RATE)][:N]
    assert len(set(shown)) == 6 and len(shown) > 6  # every reference frame is shown, some twice
    want = R.motion(R.sad(clips["src_y"][:6], 10, index=shown), W, H)
    for batch in (5, 32):
        res = metrics.metrics_of_files(ref, clips["pvs"], batch=batch, motion=True)
        assert res["frames"] == len(shown)
        assert res["motion_y"].tolist() == want[0] and res["motion2_y"].tolist() == want[1]
        zeros = [k for k in range(1, len(shown)) if shown[k] == shown[k - 1]]
        assert zeros and all(res["motion_y"][k] == 0.0 for k in zeros)


def test_reference_of_another_size_goes_through_the_scaler(gpu, clips, tmp_path):
    import torch
    from pixpath import metrics, ops
    from pixpath.frames import FrameBatch
    rng = np.random.default_rng(62)
    big = [synth.smooth_frame(t, po.YUV422P10LE, 2 * W, 2 * H) for t in range(N)]
    ref = str(tmp_path / "big.y4m")
    _write(ref, big)
    scaled = ops.Scaler(FMT, 2 * W, 2 * H, FMT, W, H, flags="bicubic")(
        FrameBatch.from_numpy(FMT, synth.batch(big), device=gpu))
    torch.cuda.synchronize(gpu)
    luma = scaled.to_numpy()[0]
    want = R.motion(R.sad(luma, 10), W, H)
    res = metrics.metrics_of_files(ref, clips["pvs"], batch=5, motion=True)
    assert res["frames"] == N and res["motion_y"].tolist() == want[0] and res["motion2_y"].tolist() == want[1]
    assert max(want[0]) > 0.0


def test_explicit_map_with_unmatched_frames(gpu, clips, capsys):
    from pixpath import metrics
    idx = [0, 1, -1, -1, 2, 3, 5, -1, 6, 8, 9, 11]
    shown, last = [], 0
    for v in idx:
        last = last if v < 0 else v
        shown.append(last)
    m, m2 = R.motion(R.sad(clips["src_y"], 10, index=shown), W, H)
    assert m[2] == m[3] == m[7] == 0.0  # read against the held frame
    un = [k for k, v in enumerate(idx) if v < 0]
    want_m = [float("nan") if k in un else v for k, v in enumerate(m)]
    want_m2 = [float("nan") if k in un else v for k, v in enumerate(m2)]
    for batch in (4, 32):
        res = metrics.metrics_of_files(clips["src"], clips["pvs"], batch=batch, ref_index=idx, motion=True)
        assert _same(res["motion_y"], want_m) and _same(res["motion2_y"], want_m2)
        assert res["mean"]["motion_y"] == float(np.mean([v for v in want_m if not math.isnan(v)]))
        assert res["mean"]["motion2_y"] == float(np.mean([v for v in want_m2 if not math.isnan(v)]))
    out = metrics.report(res, clips["src"], clips["pvs"], per_frame=True)
    assert [k for k, v in enumerate(out["motion_y_frames"]) if v is None] == un
    assert [k for k, v in enumerate(out["motion2_y_frames"]) if v is None] == un


def test_vmaf_features_equal_the_flags_run_separately(gpu, clips, capsys):
    from pixpath import cli
    base = ["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--per-frame", "--batch", "5"]
    capsys.readouterr()
    assert cli.main(base + ["--vmaf-features"]) == 0
    d = _line(capsys)
    assert d["vmaf_feature_names"] == ["adm2", "motion2", "vif_scale0", "vif_scale1", "vif_scale2", "vif_scale3"]
    assert cli.main(base + ["--vif"]) == 0
    v = _line(capsys)
    assert cli.main(base + ["--adm"]) == 0
    a = _line(capsys)
    assert cli.main(base + ["--motion"]) == 0
    m = _line(capsys)
    assert m["motion_y_frames"] == clips["motion"][0] and m["motion2_y_frames"] == clips["motion"][1]
    rows = d["vmaf_features_frames"]
    assert len(rows) == N and all(len(r) == 6 for r in rows)
    for k, r in enumerate(rows):
        assert r == [a["adm2_y_frames"][k], m["motion2_y_frames"][k]] + v["vif_scales_y_frames"][k]
    assert d["vmaf_features"] == [a["adm2_y"], m["motion2_y"]] + v["vif_scales_y"]
    for other in (v, a, m):  # --vmaf-features implies the three: each one's keys as on its own
        for key, val in other.items():
            assert d[key] == val
    assert set(d) == set(v) | set(a) | set(m) | {"vmaf_features", "vmaf_feature_names", "vmaf_features_frames"}
    assert cli.main(base[:-3] + ["--vmaf-features"]) == 0  # without --per-frame: the clip values only
    short = _line(capsys)
    assert short["vmaf_features"] == d["vmaf_features"] and not [k for k in short if k.endswith("_frames")]


def test_without_the_flags_the_line_is_unchanged(gpu, clips, capsys):
    from pixpath import cli, metrics
    res = metrics.metrics_of_files(clips["src"], clips["pvs"], batch=32, flags="bicubic")
    assert not [k for k in list(res) + list(res["mean"]) if "motion" in k or "vmaf" in k]
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--per-frame"]) == 0
    line = capsys.readouterr().out.strip()
    assert line == json.dumps(metrics.report(res, clips["src"], clips["pvs"], per_frame=True))
    assert set(json.loads(line)) == BASE_KEYS  # exactly the keys of PP-METRIC-1
    assert cli.main(["metrics", "--ref", clips["src"], "--input", clips["pvs"], "--motion", "--per-frame"]) == 0
    with_flag = _line(capsys)
    for k, v in json.loads(line).items():  # the flag only adds keys
        assert with_flag[k] == v
    assert set(with_flag) - set(json.loads(line)) == MOTION_KEYS
