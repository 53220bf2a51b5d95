"""PP-HVS-1 end to end: `metrics_of_files(psnr_hvs=True)` and `cli metrics
--psnr-hvs --per-frame` on two small written clips (64 x 48, 7 distorted
frames, batch 3, a reference at half the rate, as the all-features test builds
them) must print what psnrhvs.summarize gives for the restatement's sums of the
same frame pairs (test_gpu_psnrhvs' bound on the sums; an MSE is a sum over a
constant, a PSNR 10 log10 of it); an explicit map with an unmatched frame
prints null there; `--hvs-step 7` changes the blocks and the values; without
the flag the line is what it was."""
import json

import numpy as np
import pytest

import psnrhvs_ref
import pyoracle as po
import synth
from file_clips import last_line as _line, write_y4m
from pixpath import psnrhvs
from test_gpu_psnrhvs import RTOL

pytestmark = pytest.mark.gpu
FMT, W, H = "yuv420p", 64, 48
N_REF, REF_RATE, N_DIST, DIST_RATE, BATCH = 4, 15, 7, 30, 3
EXPLICIT = [0, 0, -1, 1, 2, 2, 3]  # one unmatched frame, never going back
HVS_KEYS = set(psnrhvs.KEYS) | {"hvs_step", "hvs_blocks"} | {k + "_frames" for k in psnrhvs.KEYS}


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("psnrhvs")
    rng = np.random.default_rng(78)
    src = [synth.smooth_frame(3 * t, po.YUV420P, W, H) for t in range(N_REF)]
    pvs = [[np.clip(p.astype(np.int64) + rng.integers(-6, 7, p.shape), 0, 255).astype(np.uint8) for p in src[k // 2]]
           for k in range(N_DIST)]
    return {"src": write_y4m(d / "src.y4m", FMT, REF_RATE, synth.batch(src)),
            "pvs": write_y4m(d / "pvs.y4m", FMT, DIST_RATE, synth.batch(pvs)), "src_frames": src, "pvs_frames": pvs}


def _want(clips, ref_index, step):
    """psnrhvs.summarize of the restatement's sums: dist frame k against ref frame ref_index[k] (< 0: none)."""
    idx = np.asarray(ref_index)
    sums = psnrhvs_ref.psnr_hvs(synth.batch(clips["src_frames"]), synth.batch(clips["pvs_frames"]), step,
                                np.maximum(idx, 0))
    return psnrhvs.summarize(sums, W, H, idx >= 0, FMT, step)


def _compare(d, want):
    """The per-frame lists and clip values of a printed report against `want`: null where NaN."""
    for key in psnrhvs.KEYS:
        # |d psnr| = 10 log10(1 + r) < 4.35 r; the all value is a positive combination of the planes'
        tol = {"rtol": RTOL, "atol": 0} if key.startswith("mse") else {"rtol": 0, "atol": 5 * RTOL}
        for got, exp in zip(d[key + "_frames"] + [d[key]], list(want[key]) + [want["mean"][key]]):
            if np.isnan(exp):
                assert got is None, key
            else:
                np.testing.assert_allclose(got, exp, err_msg=key, **tol)
    assert d["hvs_step"] == want["mean"]["hvs_step"] and d["hvs_blocks"] == want["mean"]["hvs_blocks"]


def test_metrics_of_files_cli_and_ops(gpu, clips, capsys):
    import torch
    from pixpath import cli, metrics, ops
    from pixpath.frames import FrameBatch
    fmap = [int(v) for v in ops.fps_map(N_REF, REF_RATE, DIST_RATE)[:N_DIST]]
    assert fmap != list(range(N_DIST)) and fmap == [k // 2 for k in range(N_DIST)]
    res = metrics.metrics_of_files(clips["src"], clips["pvs"], batch=BATCH, psnr_hvs=True)
    assert res["frames"] == N_DIST and all(res[k].shape == (N_DIST,) for k in psnrhvs.KEYS)
    # equal to ops.psnr_hvs on the same frames, to the bit
    out = ops.psnr_hvs(FrameBatch.from_numpy(FMT, synth.batch(clips["src_frames"]), device=gpu),
                       FrameBatch.from_numpy(FMT, synth.batch(clips["pvs_frames"]), device=gpu), ref_index=fmap)
    torch.cuda.synchronize()
    pooled = psnrhvs.pool(out.cpu().numpy(), FMT, W, H)
    assert all(np.array_equal(res[k], pooled[k]) for k in psnrhvs.KEYS)
    assert (res["mse_hvsm_y"] < res["mse_hvs_y"]).all() and (res["mse_hvsm_y"] > 0).all()
    assert (res["psnr_hvsm_all"] > res["psnr_hvs_all"]).all()

    capsys.readouterr()
    base = ["metrics", "--ref", clips["src"], "--input", clips["pvs"]]
    assert cli.main(base + ["--psnr-hvs", "--per-frame", "--batch", str(BATCH)]) == 0
    d = _line(capsys)
    assert d["frames"] == N_DIST and d["spec"] == "PP-METRIC-1" and d["hvs_blocks"] == [48, 12, 12]
    _compare(d, _want(clips, fmap, 8))
    assert d["mse_hvs_y_frames"] == [float(x) for x in res["mse_hvs_y"]]
    # one batch gives the same numbers; without --per-frame only the clip values
    assert cli.main(base + ["--psnr-hvs", "--per-frame"]) == 0
    assert _line(capsys) == d
    assert cli.main(base + ["--psnr-hvs"]) == 0
    short = _line(capsys)
    assert all(short[k] == d[k] for k in psnrhvs.KEYS) and not [k for k in short if k.endswith("_frames")]
    # step 7: other blocks, other values
    assert cli.main(base + ["--psnr-hvs", "--hvs-step", "7", "--per-frame", "--batch", str(BATCH)]) == 0
    d7 = _line(capsys)
    assert d7["hvs_step"] == 7 and d7["hvs_blocks"] == [54, 12, 12] and d["hvs_step"] == 8
    _compare(d7, _want(clips, fmap, 7))
    assert all(d7[k] != d[k] for k in psnrhvs.KEYS)
    # without the flag the line has none of the keys, and the flag only adds keys
    assert cli.main(base + ["--per-frame", "--batch", str(BATCH)]) == 0
    plain = _line(capsys)
    assert set(d) - set(plain) == HVS_KEYS and all(d[k] == v for k, v in plain.items())
    assert cli.main(base + ["--vmaf-features"]) == 0
    assert not set(_line(capsys)) & HVS_KEYS  # --vmaf-features does not imply it


def test_explicit_map_with_an_unmatched_frame(gpu, clips):
    from pixpath import metrics
    for step in psnrhvs.STEPS:
        res = metrics.metrics_of_files(clips["src"], clips["pvs"], batch=BATCH, ref_index=EXPLICIT, psnr_hvs=True,
                                       hvs_step=step)
        d = json.loads(json.dumps(metrics.report(res, clips["src"], clips["pvs"], per_frame=True)))
        _compare(d, _want(clips, EXPLICIT, step))
        un = EXPLICIT.index(-1)
        for key in psnrhvs.KEYS:
            assert d[key + "_frames"][un] is None and d[key + "_frames"][un + 1] is not None, key
