"""PP-BAND-1 end to end on small written clips: `banding.banding_of_file` on an
FFV1 AVI and on a v210 CPVS with --crop, `cli banding`, and `cli metrics
--banding` must give what banding_ref gives on the decoded frames; the chain's
8-bit truncation of a 10-bit ramp adds banding; and without the flag the
metrics line is what it was.  The histograms are integers and the pooling is
the same float64 arithmetic on both sides: every comparison is exact."""
import json

import numpy as np
import pytest

import banding_ref as R
import pyoracle as po
import synth
from file_clips import last_line, write_packed_avi, write_y4m

pytestmark = pytest.mark.gpu
FMT, W, H, CW, CH, N = "yuv422p10le", 64, 48, 64, 60, 5
BAND_KEYS = {"banding_y", "banding_ref_y", "banding_added_y"}
BASE_KEYS = {"ref", "file", "frames", "spec"} | {"%s_%s%s" % (kind, name, tail) for kind in ("mse", "psnr", "ssim")
                                                  for name in ("y", "u", "v", "all") for tail in ("", "_frames")}


def _chroma(n=1):
    return np.full((H, W // 2), 512, np.uint16)


def _write_y4m(path, lumas):
    write_y4m(path, FMT, 60, synth.batch([[y, _chroma(), _chroma()] for y in lumas]))


@pytest.fixture(scope="module")
def clip():
    luma = R.content(10, N, W, H, seed=31)
    frames = [[luma[k], _chroma(), _chroma()] for k in range(N)]
    return luma, frames


def _pooled(luma, window):
    from pixpath import banding
    return banding.summarize(R.hist(luma, 10, window))


def _same(res, want):
    assert res["banding_y"].tolist() == want["banding_y"].tolist()
    assert res["banding_scales_y"].tolist() == want["banding_scales_y"].tolist()
    assert res["mean"] == want["mean"]


def test_ffv1_avi(gpu, clip, tmp_path, capsys):
    import torch
    from pixpath import banding, cli, ffv1
    from pixpath.frames import FrameBatch
    luma, frames = clip
    path = str(tmp_path / "a.avi")
    wr = ffv1.Ffv1AviWriter(path, FMT, W, H, 60, slices=(2, 2), batch=16, device=gpu)
    src = FrameBatch.interleaved(FMT, W, H, N, device=gpu)
    for i, f in enumerate(frames):
        for p in range(3):
            src.view(p)[i].copy_(torch.from_numpy(f[p]))
    wr.write_device(src)
    wr.close()
    assert banding.default_window(W, H) == 3
    for batch, window in ((2, None), (32, 9)):  # 2: two batch seams
        got = banding.banding_of_file(path, batch=batch, window=window)
        assert (got["frames"], got["w"], got["h"], got["window"]) == (N, W, H, window or 3)
        _same(got, _pooled(luma, window or 3))
    assert _pooled(luma, 9)["mean"]["banding_y"] > 0.0
    with pytest.raises(ValueError):
        banding.banding_of_file(path, crop=(32, 24))  # crop is for a packed canvas
    capsys.readouterr()
    assert cli.main(["banding", path, "--window", "9", "--per-frame", "--batch", "3"]) == 0
    d = json.loads(capsys.readouterr().out)
    want = _pooled(luma, 9)
    assert set(d) == {"file", "frames", "w", "h", "spec", "window", "banding_y", "banding_max_y", "banding_scales_y",
                      "banding_y_frames", "banding_scales_y_frames"}
    assert d["spec"] == "PP-BAND-1" and d["window"] == 9 and d["frames"] == N
    assert d["banding_y"] == want["mean"]["banding_y"] and d["banding_max_y"] == want["mean"]["banding_max_y"]
    assert d["banding_y_frames"] == want["banding_y"].tolist() and d["banding_scales_y"] == want["mean"]["banding_scales_y"]


def test_v210_cpvs_with_and_without_crop(gpu, clip, tmp_path, capsys):
    from pixpath import banding, cli
    luma, frames = clip
    padded = [po.pad(po.YUV422P10LE, f, CW, CH, 0, 6) for f in frames]
    path = write_packed_avi(tmp_path / "cpvs.avi", b"v210", CW, CH, 60, [po.v210_pack(f) for f in padded])
    got = banding.banding_of_file(path, batch=4, window=7)
    assert (got["w"], got["h"]) == (CW, CH)
    _same(got, _pooled(np.stack([f[0] for f in padded]), 7))
    got = banding.banding_of_file(path, batch=4, window=7, crop=(W, H))
    assert (got["w"], got["h"], got["frames"]) == (W, H, N)
    _same(got, _pooled(luma, 7))
    capsys.readouterr()
    assert cli.main(["banding", path, "--crop", "%dx%d" % (W, H), "--window", "7"]) == 0
    d = json.loads(capsys.readouterr().out)
    assert d["banding_y"] == _pooled(luma, 7)["mean"]["banding_y"] and (d["w"], d["h"]) == (W, H)
    assert not [k for k in d if k.endswith("_frames")]


def test_metrics_banding_of_a_truncated_ramp(gpu, tmp_path, capsys):
    """A 10-bit ramp against its copy with the two low bits dropped (what the
    8-bit CPVS conversion does): the copy bands, the difference is what the
    chain added."""
    from pixpath import banding, cli, metrics
    ramp = np.stack([np.tile(300 + (np.arange(W) + k) // 3, (H, 1)).astype(np.uint16) for k in range(N)])
    cut = (ramp >> 2) << 2
    ref, dist = str(tmp_path / "ramp.y4m"), str(tmp_path / "cut.y4m")
    _write_y4m(ref, ramp)
    _write_y4m(dist, cut)
    win = banding.default_window(W, H)
    want_d, want_r = (banding.pool(R.hist(a, 10, win))[0] for a in (cut, ramp))
    for batch in (2, 32):
        res = metrics.metrics_of_files(ref, dist, batch=batch, banding=True)
        assert res["banding_y"].tolist() == want_d.tolist() and res["banding_ref_y"].tolist() == want_r.tolist()
        assert res["banding_added_y"].tolist() == (want_d - want_r).tolist()
        assert res["mean"]["banding_added_y"] > 0.0
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", ref, "--input", dist, "--banding"]) == 0
    d = json.loads(capsys.readouterr().out)
    assert BAND_KEYS <= set(d) and d["banding_added_y"] > 0.0 and d["banding_y"] == float(want_d.mean())
    assert d["banding_ref_y"] == float(want_r.mean()) and not [k for k in d if k.endswith("_frames")]
    # a map with an unmatched frame: its values are null, the reference frames follow the map
    res = metrics.metrics_of_files(ref, dist, ref_index=[0, 1, -1, 3, 4], banding=True)
    assert np.isnan(res["banding_y"][2]) and res["banding_ref_y"][3] == want_r[3]


def test_without_the_flag_the_line_is_unchanged(gpu, clip, tmp_path, capsys):
    from pixpath import cli, metrics
    luma, _ = clip
    ref, dist = str(tmp_path / "r.y4m"), str(tmp_path / "d.y4m")
    _write_y4m(ref, luma)
    _write_y4m(dist, np.minimum(luma + 3, 1023).astype(np.uint16))
    res = metrics.metrics_of_files(ref, dist, batch=32, flags="bicubic")
    assert not [k for k in list(res) + list(res["mean"]) if "banding" in k]
    capsys.readouterr()
    assert cli.main(["metrics", "--ref", ref, "--input", dist, "--per-frame"]) == 0
    line = capsys.readouterr().out.strip()
    assert line == json.dumps(metrics.report(res, ref, dist, per_frame=True))
    assert set(json.loads(line)) == BASE_KEYS  # exactly the keys of PP-METRIC-1
    assert cli.main(["metrics", "--ref", ref, "--input", dist, "--banding", "--per-frame"]) == 0
    with_flag = last_line(capsys)
    for k, v in json.loads(line).items():  # the flag only adds keys
        assert with_flag[k] == v
    assert set(with_flag) - set(json.loads(line)) == BAND_KEYS | {k + "_frames" for k in BAND_KEYS}
