"""`metrics_of_files` with every optional measurement at once against one at a
time: each key of the one-flag report has the identical value in the all-flags
report.  The clips make the driver do all it can between two batches: a
reference at half the rate (the vf_fps map is no identity), batch 3 of 7 frames
(the reference window is rebuilt, motion's held frame crosses a seam), and an
explicit map with an unmatched frame.  The kernels are run-to-run identical and
the host arithmetic is the same on both sides: the printed values are compared
as printed, NaN as null."""
import json

import numpy as np
import pytest

import pyoracle as po
import synth

pytestmark = pytest.mark.gpu
FMT, W, H = "yuv420p", 64, 48
N_REF, REF_RATE, N_DIST, DIST_RATE, BATCH = 4, 15, 7, 30, 3
FLAGS = ("ms_ssim", "vif", "adm", "motion", "banding", "ciede")
EXPLICIT = [0, 0, -1, 1, 2, 2, 3]  # one unmatched frame, never going back


def _write(path, frames, rate):
    from pixpath import io as pio
    wr = pio.Y4MWriter(path, FMT, W, H, rate)
    wr.write(pio.join_planes(synth.batch(frames)))
    wr.close()


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    d = tmp_path_factory.mktemp("allfeatures")
    rng = np.random.default_rng(77)
    src = [synth.smooth_frame(3 * t, po.YUV420P, W, H) for t in range(N_REF)]
    pvs = [[np.clip(p.astype(np.int64) + rng.integers(-6, 7, p.shape), 0, 255).astype(np.uint8) for p in src[k // 2]]
           for k in range(N_DIST)]
    ref, dist = str(d / "src.y4m"), str(d / "pvs.y4m")
    _write(ref, src, REF_RATE)
    _write(dist, pvs, DIST_RATE)
    return ref, dist


def _report(clips, **kw):
    from pixpath import metrics
    ref, dist = clips
    return metrics.report(metrics.metrics_of_files(ref, dist, batch=BATCH, **kw), ref, dist, per_frame=True)


@pytest.mark.parametrize("ref_index", [None, EXPLICIT], ids=["vf_fps", "explicit"])
def test_all_at_once_equals_each_alone(gpu, clips, ref_index):
    from pixpath import ops
    assert [int(v) for v in ops.fps_map(N_REF, REF_RATE, DIST_RATE)[:N_DIST]] != list(range(N_DIST))
    kw = {} if ref_index is None else {"ref_index": ref_index}
    base = _report(clips, **kw)
    both = _report(clips, **kw, **{flag: True for flag in FLAGS})
    assert both["frames"] == N_DIST == base["frames"]
    seen = set(base)
    for flag in FLAGS:
        one = _report(clips, **kw, **{flag: True})
        assert set(one) > set(base), flag  # the flag adds keys of its own
        assert not (set(one) - set(base)) & (seen - set(base)), flag
        for key, v in one.items():
            assert json.dumps(both[key]) == json.dumps(v), (flag, key)
        seen |= set(one)
    assert seen == set(both)  # no measurement is left out of the comparison
    if ref_index is not None:
        un = EXPLICIT.index(-1)
        for key, v in both.items():
            if key.endswith("_frames"):
                assert v[un] is None or v[un] == [None] * len(v[un]), key
