"""strip_kernel's V-pass last-pair skip against the oracle -- bit-exact, every
plane of every frame.

Which rows skip is restated from the plan's filters (strip_plan_ref); every
case asserts the mix of rows it is meant to run before it runs.

Shapes: 344x100 -> 516x150 is the smallest 3:2 plan with 3 luma strips (the
last 4 columns wide) and 2 chroma strips (258 columns: ragged, per-lane V
stores); one 160-row segment of five 32-row chunks, the last 22 rows tall, so
kept row pairs carry from chunk to chunk.  400x100 -> 600x150 is the same with
every plane width a multiple of 4 (the clamped V-pass copy).
"""
import numpy as np
import pytest

import pyoracle as po
import strip_plan_ref as ref
import synth

pytestmark = pytest.mark.gpu

N = 3
P10, P8 = po.YUV422P10LE, po.YUV422P


def _run(gpu, sf, sw, sh, df, dw, dh, flags, frames):
    import torch
    from pixpath import ops
    from pixpath.frames import FrameBatch
    src = FrameBatch.from_numpy(sf, synth.batch(frames), device=gpu)
    out = ops.Scaler(sf, sw, sh, df, dw, dh, flags=flags)(src).to_numpy()
    torch.cuda.synchronize()
    for i, f in enumerate(frames):
        want = po.scale(sf, f, df, dw, dh, flags)
        for p, r in enumerate(want):
            got = out[p][i]
            if not np.array_equal(got, r):
                bad = np.argwhere(got != r)
                pytest.fail("frame %d plane %d: %d mismatches, first at %s got %d want %d" % (
                    i, p, len(bad), tuple(bad[0]), got[tuple(bad[0])], r[tuple(bad[0])]))


def _plan(sf, sw, sh, df, dw, dh, flags):
    from pixpath import ops
    return ops.Scaler(sf, sw, sh, df, dw, dh, flags=flags, host_only=True)


def _noise(fmt, w, h, seed):
    rng = np.random.default_rng(seed)
    return [synth.noise_frame(rng, fmt, w, h) for _ in range(N)]


@pytest.mark.parametrize("sf,sw,dw", [(P10, 344, 516), (P10, 400, 600), (P8, 344, 516)],
                         ids=["10bit-ragged", "10bit-clamped", "8bit-source"])
def test_skip_multi_strip_multi_chunk(gpu, sf, sw, dw):
    """3:2 lanczos (config 2's instance, 4 tap pairs), skipping and full rows
    in one row group of a wave: 3 luma strips with a ragged last one, 2 chroma
    strips, five chunks per segment, 150 rows."""
    sc = _plan(sf, sw, 100, P10, dw, 150, po.SWS_LANCZOS)
    st = sc.stats
    assert sc.kernel_path == 6
    assert -(-dw // 256) >= 3 and dw % 256 and -(-(dw // 2) // 256) >= 2
    assert st["seg_rows"] >= 2 * st["cho"] and 150 % st["cho"]
    for which in (2, 3):
        vtp, zero = ref.last_pair_zero(sc, which)
        assert vtp == 4 and ref.mixed_row_group(zero, st["cho"])
    _run(gpu, sf, sw, 100, P10, dw, 150, po.SWS_LANCZOS, _noise(sf, sw, 100, 71))


def test_skip_three_pair_arm(gpu):
    """Bicubic 3:2 at the same size: the 3-pair arm, two thirds of its rows skip."""
    sc = _plan(P10, 344, 100, P10, 516, 150, po.SWS_BICUBIC)
    assert sc.kernel_path == 4
    vtp, zero = ref.last_pair_zero(sc, 2)
    assert vtp == 3 and ref.mixed_row_group(zero, sc.stats["cho"]) and 2 * zero.sum() > len(zero)
    _run(gpu, P10, 344, 100, P10, 516, 150, po.SWS_BICUBIC, _noise(P10, 344, 100, 72))


def test_downscale_full_rows(gpu):
    """A 2:1 bicubic downscale, 5 tap pairs: every interior row uses its last
    pair.  (swscale folds the taps that fall off the picture into the edge
    rows, so the two first and two last rows of any 2:1 plan do have a zero
    last pair; no such plan is free of them.)"""
    sc = _plan(P10, 1040, 122, P10, 520, 61, po.SWS_BICUBIC)
    assert sc.kernel_path == 8
    for which in (2, 3):
        vtp, zero = ref.last_pair_zero(sc, which)
        assert vtp == 5 and not zero[2:-2].any()
    _run(gpu, P10, 1040, 122, P10, 520, 61, po.SWS_BICUBIC, _noise(P10, 1040, 122, 73))


@pytest.mark.parametrize("value", [0, 1023])
def test_full_range_extremes(gpu, value):
    """All-0 and all-1023 frames through the 3:2 lanczos plan."""
    sc = _plan(P10, 344, 100, P10, 516, 150, po.SWS_LANCZOS)
    assert sc.kernel_path == 6
    frames = [[np.full(s, value, dtype=np.uint16) for s in po.plane_shapes(P10, 344, 100)] for _ in range(N)]
    _run(gpu, P10, 344, 100, P10, 516, 150, po.SWS_LANCZOS, frames)
