"""PP-CIEDE-1 end to end: `metrics_of_files(ciede=True)` and `cli metrics
--ciede` on two small written clips must give what ops.ciede gives on the same
frames and what the restatement gives for them (test_gpu_ciede's bound on the
sums; delta_e is a sum over w h, so the same bound), with `--align`, `--crop`,
`--per-frame` and `--ciede-weights`; and without the flag the line is what it
was."""
import json

import numpy as np
import pytest

import ciede_ref
import pyoracle as po
import synth
from file_clips import last_line as _line, write_cpvs, write_y4m
from test_gpu_ciede import MARGIN, RTOL

pytestmark = pytest.mark.gpu
FMT, W, H, N, RATE = "yuv422p10le", 64, 36, 12, 60
FREEZE = [[0.1, 0.05]]  # frames 6..8 show frame 5
CIEDE_KEYS = {"delta_e", "delta_e_max", "ciede2000", "delta_e_frames", "delta_e_max_frames", "ciede2000_frames"}


def _want(ref, dist, weights=(1.0, 1.0, 1.0)):
    """The restatement's [n, 2] of two lists of frames, every sample away from the branch boundaries."""
    out, far = ciede_ref.ciede(synth.batch(ref), synth.batch(dist), 10, 1, 0, weights=weights)
    assert far > MARGIN
    return out


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("ciede")
    rng = np.random.default_rng(52)
    src = [synth.noise_frame(rng, po.YUV422P10LE, W, H) for _ in range(N)]
    pvs = []
    for k, f in enumerate(src):  # the chroma gets an error growing with k, the luma a small one
        e = 2 * (k + 1)
        pvs.append([np.clip(p.astype(np.int64) + rng.integers(-(e if i else 1), (e if i else 1) + 1, p.shape), 0, 1023)
                    .astype(np.uint16) for i, p in enumerate(f)])
    paths = {"src": write_y4m(d / "src.y4m", FMT, RATE, synth.batch(src)),
             "pvs": write_y4m(d / "pvs.y4m", FMT, RATE, synth.batch(pvs)), "dir": d, "src_frames": src,
             "pvs_frames": pvs}
    paths["want"] = _want(src, pvs)
    return paths


def _compare(d, want):
    """The per-frame lists and clip values of a report against the restatement's sums."""
    de, mx = want[:, 0] / (W * H), want[:, 1]
    score = np.minimum(45.0 - 20.0 * np.log10(de), 100.0)
    np.testing.assert_allclose(d["delta_e_frames"], de, rtol=RTOL, atol=0)
    np.testing.assert_allclose(d["delta_e_max_frames"], mx, rtol=RTOL, atol=0)
    np.testing.assert_allclose(d["ciede2000_frames"], score, rtol=0, atol=20 * RTOL)  # 20 log10(1 + r) < 8.7 r
    assert d["delta_e"] == pytest.approx(de.mean(), rel=RTOL) and d["delta_e_max"] == pytest.approx(mx.max(), rel=RTOL)
    assert d["ciede2000"] == pytest.approx(score.mean(), abs=20 * RTOL)


def test_metrics_of_files_cli_and_ops(gpu, clips, capsys):
    import torch
    from pixpath import ciede, cli, metrics, ops
    from pixpath.frames import FrameBatch
    res = metrics.metrics_of_files(clips["src"], clips["pvs"], batch=5, ciede=True)
    want = clips["want"]
    assert res["frames"] == N and all(res[k].shape == (N,) for k in ciede.KEYS)
    # equal to ops.ciede on the same frames, to the bit
    out = ops.ciede(FrameBatch.from_numpy(FMT, synth.batch(clips["src_frames"]), device=gpu),
                    FrameBatch.from_numpy(FMT, synth.batch(clips["pvs_frames"]), device=gpu), FMT)
    torch.cuda.synchronize()
    de, mx, score = ciede.pool(out.cpu().numpy(), W, H)
    assert np.array_equal(res["delta_e"], de) and np.array_equal(res["delta_e_max"], mx) and np.array_equal(res["ciede2000"], score)
    assert (np.diff(res["delta_e"]) > 0).all() and res["delta_e"][0] > 0  # the error grows
    capsys.readouterr()
    base = ["metrics", "--ref", clips["src"], "--input", clips["pvs"]]
    assert cli.main(base + ["--ciede", "--per-frame", "--batch", "5"]) == 0
    d = _line(capsys)
    assert d["frames"] == N and d["spec"] == "PP-METRIC-1"
    assert all(len(d[k + "_frames"]) == N for k in ciede.KEYS)
    _compare(d, want)
    assert d["delta_e_frames"] == [float(x) for x in res["delta_e"]]
    # one batch gives the same numbers; without --per-frame only the clip values
    assert cli.main(base + ["--ciede", "--per-frame"]) == 0
    assert _line(capsys) == d
    assert cli.main(base + ["--ciede"]) == 0
    short = _line(capsys)
    assert all(short[k] == d[k] for k in ciede.KEYS) and not [k for k in short if k.endswith("_frames")]
    # other weights
    assert cli.main(base + ["--ciede", "--ciede-weights", "2,1,0.5", "--per-frame"]) == 0
    _compare(_line(capsys), _want(clips["src_frames"], clips["pvs_frames"], (2.0, 1.0, 0.5)))


def test_without_the_flag_the_line_is_unchanged(gpu, clips, capsys):
    from pixpath import cli, metrics
    res = metrics.metrics_of_files(clips["src"], clips["pvs"], batch=32, flags="bicubic")
    assert not [k for k in list(res) + list(res["mean"]) if "delta_e" in k or "ciede" in k]
    capsys.readouterr()
    base = ["metrics", "--ref", clips["src"], "--input", clips["pvs"]]
    assert cli.main(base + ["--per-frame"]) == 0
    line = capsys.readouterr().out.strip()
    assert line == json.dumps(metrics.report(res, clips["src"], clips["pvs"], per_frame=True))
    assert cli.main(base + ["--ciede", "--per-frame"]) == 0
    with_flag = _line(capsys)
    for k, v in json.loads(line).items():  # the flag only adds keys
        assert with_flag[k] == v
    assert set(with_flag) - set(json.loads(line)) == CIEDE_KEYS
    # next to the other switches: every set of keys, each as on its own; --vmaf-features does not imply it
    assert cli.main(base + ["--vmaf-features", "--ms-ssim", "--per-frame"]) == 0
    other = _line(capsys)
    assert not set(other) & CIEDE_KEYS
    assert cli.main(base + ["--vmaf-features", "--ms-ssim", "--ciede", "--per-frame"]) == 0
    both = _line(capsys)
    assert set(both) == set(other) | CIEDE_KEYS
    for k in both:
        assert both[k] == (with_flag[k] if k in CIEDE_KEYS else other[k])


def test_aligned_stall(gpu, clips, capsys):
    from pixpath import cli
    from pixpath.stall import stall_schedule
    out = str(clips["dir"] / "freeze.y4m")
    assert cli.main(["stall", "-y", "--input", clips["src"], "--buffer", json.dumps(FREEZE), "--skipping", out]) == 0
    shown = [s for s, _ in stall_schedule(FREEZE, RATE, N, True)]
    assert shown == list(range(6)) + [5] * 3 + list(range(9, 12))
    src = clips["src_frames"]
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", out, "--align", "--ciede", "--per-frame"]) == 0
    a = _line(capsys)
    assert a["aligned"] is True and a["unmatched"] == 0 and a["frames"] == N
    # every frame against the one it shows: no colour difference at all
    assert a["delta_e_frames"] == [0.0] * N and a["delta_e_max"] == 0.0 and a["ciede2000_frames"] == [100.0] * N
    assert cli.main(["metrics", "--ref", clips["src"], "--input", out, "--ciede", "--per-frame"]) == 0
    p = _line(capsys)  # the vf_fps map: frames 6..8 against another picture
    want = _want(src, [src[s] for s in shown])
    np.testing.assert_allclose(p["delta_e_frames"], want[:, 0] / (W * H), rtol=RTOL, atol=0)
    assert [v == 0.0 for v in p["delta_e_frames"]] == [s == k for k, s in enumerate(shown)]
    assert min(p["delta_e_frames"][6:9]) > 10 and len(p["delta_e_max_frames"]) == N


def test_crop_of_a_v210_cpvs(gpu, clips, capsys, tmp_path):
    """The PVS padded onto a 64 x 48 v210 canvas: --crop 64x36 scores the picture inside it, as the PVS itself."""
    from pixpath import cli, metrics
    path = str(tmp_path / "cpvs.avi")
    write_cpvs(path, gpu, FMT, synth.batch(clips["pvs_frames"]), 64, 48, RATE)
    res = metrics.metrics_of_files(clips["src"], path, crop=(W, H), ciede=True, batch=7)
    plain = metrics.metrics_of_files(clips["src"], clips["pvs"], ciede=True)
    assert res["frames"] == N
    assert np.array_equal(res["delta_e"], plain["delta_e"]) and np.array_equal(res["delta_e_max"], plain["delta_e_max"])
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", clips["src"], "--input", path, "--crop", "%dx%d" % (W, H), "--ciede",
                     "--per-frame"]) == 0
    _compare(_line(capsys), clips["want"])
