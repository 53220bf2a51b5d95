"""Every arm of the SI/TI kernel (csrc/siti.hip) at the smallest clips that
reach it, against oracle/siti_ref.py (float64 / int64).

The production planner gives these clips one frame per chunk on a whole
device, so the software-pipelined frame loop (next frame's rows reloaded into
the window, the previous band carried in registers, frame f reduced in the
middle of frame f + 1, the zero-byte descriptor after the last frame), the
grid-stride loop and the halo of a later chunk would run once or not at all.
Each case of siti_arms.CASES therefore forces its slot count
(ops.siti(..., slots=)); test_siti_plan_host.py proves on the CPU that the
cases plan to their arms.  Content is seeded uniform noise over the full code
range (smooth content hides indexing errors); bytes outside the frames are 7.

Tolerances are the project's (test_gpu_siti.py): SI rtol 1e-4, atol 1e-9; TI,
whose moments are exact integers, rtol 1e-12, atol 1e-12; ti[0] is NaN exactly
when no `prev` is given.  Results at different slot counts are compared bit for
bit: the plan decides which workgroup computes a (frame, band, wave) partial,
never its arithmetic, and siti_finalize reduces in a fixed order.
"""
import numpy as np
import pytest

import siti_arms
import siti_ref

pytestmark = pytest.mark.gpu
SI_TOL = dict(rtol=1e-4, atol=1e-9)
TI_TOL = dict(rtol=1e-12, atol=1e-12)

_reference = {}


def _ref(c):
    """Frames, prev and the reference (si, ti) of a case, computed once."""
    if c.id not in _reference:
        frames, prev = siti_arms.frames_of(c)
        _reference[c.id] = (frames, prev) + siti_ref.siti(frames, prev=prev)
        for a in _reference[c.id][2:]:
            a.setflags(write=False)
    return _reference[c.id]


def _run_case(c, gpu, slots):
    import torch
    from pixpath import ops
    frames, prev = _ref(c)[:2]
    big, pbig, view = siti_arms.place(c, frames, prev)
    t = view(torch.from_numpy(big).to(gpu))
    pt = None if pbig is None else view(torch.from_numpy(pbig).to(gpu))[0]
    assert tuple(t.shape) == frames.shape and t.element_size() == (2 if c.depth > 8 else 1)
    si, ti = ops.siti(t, c.depth, prev=pt, slots=slots)
    torch.cuda.synchronize()
    return si.cpu().numpy(), ti.cpu().numpy()


def _run(frames, depth, gpu, slots=None, prev=None):
    import torch
    from pixpath import ops
    dt = np.uint16 if depth > 8 else np.uint8
    assert frames.min() >= 0 and frames.max() < (1 << depth)
    t = torch.from_numpy(np.ascontiguousarray(frames.astype(dt))).to(gpu)
    pt = None if prev is None else torch.from_numpy(np.ascontiguousarray(prev.astype(dt))).to(gpu)
    si, ti = ops.siti(t, depth, prev=pt, slots=slots)
    torch.cuda.synchronize()
    return si.cpu().numpy(), ti.cpu().numpy()


def _check(si, ti, rsi, rti, has_prev):
    np.testing.assert_allclose(si, rsi, **SI_TOL)
    assert np.isnan(ti[0]) == (not has_prev) and np.isnan(rti[0]) == (not has_prev)
    k = 0 if has_prev else 1
    assert not np.isnan(ti[k:]).any()
    np.testing.assert_allclose(ti[k:], rti[k:], **TI_TOL)


@pytest.mark.parametrize("c", siti_arms.CASES, ids=lambda c: c.id)
def test_siti_arm_case_matches_reference(gpu, c):
    _, _, rsi, rti = _ref(c)
    si, ti = _run_case(c, gpu, c.slots)
    _check(si, ti, rsi, rti, c.prev)


@pytest.mark.parametrize("c", siti_arms.INVARIANT, ids=lambda c: c.id)
def test_siti_is_bit_equal_across_plans(gpu, c):
    """slots 1 (one workgroup walks every unit), 2, one per tile, an odd count
    that leaves a ragged last round, and the device's own count."""
    from pixpath import ops
    ntiles = ops.siti_plan(c.depth, c.w, c.h, c.n, 1).ntiles
    _, _, rsi, rti = _ref(c)
    base = None
    for slots in (1, 2, ntiles, 2 * ntiles + 1, 0):
        si, ti = _run_case(c, gpu, slots)
        if base is None:
            base = (si, ti)
            _check(si, ti, rsi, rti, c.prev)
        np.testing.assert_array_equal(si, base[0], err_msg="slots %d" % slots)
        np.testing.assert_array_equal(ti, base[1], err_msg="slots %d" % slots)  # the NaN position included


def test_siti_slots_none_is_the_device_plan(gpu):
    """ops.siti without slots, pp_siti_ex and pp_siti give the bits of slots == 0."""
    import ctypes
    import torch
    from pixpath import _native, ops
    rng = np.random.default_rng(42)
    frames = rng.integers(0, 1024, (5, 34, 497)).astype(np.uint16)
    pitch = 512
    big = np.zeros((5, 34, pitch), np.uint16)
    big[:, :, :497] = frames
    t = torch.from_numpy(big).to(gpu)[:, :, :497]
    want = [x.cpu().numpy() for x in ops.siti(t, 10, slots=0)]
    got = [x.cpu().numpy() for x in ops.siti(t, 10)]
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    ctx = ops.context(gpu.index)
    for name, extra in (("pp_siti_ex", (0,)), ("pp_siti", ())):
        si = torch.empty(5, dtype=torch.float64, device=gpu)
        ti = torch.empty(5, dtype=torch.float64, device=gpu)
        args = (ctx.handle, 10, 497, 34, ctypes.c_void_p(t.data_ptr()), pitch * 2, 34 * pitch * 2, 5, None,
                ctypes.c_void_p(si.data_ptr()), ctypes.c_void_p(ti.data_ptr())) + extra + (None,)
        torch.cuda.synchronize()
        _native.check(getattr(_native.lib(), name)(*args))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(si.cpu().numpy(), want[0])
        np.testing.assert_array_equal(ti.cpu().numpy(), want[1])


@pytest.mark.parametrize("depth", [8, 10])
def test_siti_no_frames(gpu, depth):
    import torch
    from pixpath import ops
    t = torch.empty((0, 17, 13), dtype=torch.uint16 if depth > 8 else torch.uint8, device=gpu)
    for slots in (None, 3):
        si, ti = ops.siti(t, depth, slots=slots)
        assert si.shape == ti.shape == (0,) and si.dtype == ti.dtype == torch.float64


def test_siti_negative_slots_is_refused(gpu):
    import torch
    from pixpath import _native, ops
    t = torch.zeros((2, 17, 16), dtype=torch.uint8, device=gpu)
    with pytest.raises(_native.PixpathError) as e:
        ops.siti(t, 8, slots=-1)
    assert e.value.code == -1 and "siti slots -1" in str(e.value)


# ---- the documented limits -----------------------------------------------------
def _binary(depth, seed, shape):
    return np.random.default_rng(seed).integers(0, 2, shape) * ((1 << depth) - 1)


@pytest.mark.parametrize("depth", [8, 10])
def test_siti_worst_case_ti_and_si(gpu, depth):
    """Every |d| is full scale: frame 1 is the complement of a random
    {0, max} frame 0 and frame 2 is frame 0 again.  wave_sum_u32_wide adds
    the d^2 of 32 lanes in 32 bits; its documented bound is 32 lanes x 16 rows
    x 8 px x 1023^2 = 4 286 582 784, 2^32 less 8 384 512.  A half wave has 31
    pixel lanes beside its halo lane, so a full band of full-scale differences
    reaches 31 x 16 x 8 x 1023^2 = 4 152 627 072: the nearest a frame can come.
    The Sobel gradients reach +-4092 and gx^2 + gy^2 passes 2^24, beyond
    fp32's exact integers.  512 x 32: two full bands of one full wave and the
    16-px start of the next; slots 2 and 1 walk all three frames in one chunk."""
    mx = (1 << depth) - 1
    f0 = _binary(depth, 7, (32, 512))
    frames = np.stack([f0, mx - f0, f0])
    rsi, rti = siti_ref.siti(frames)
    assert rti[1] == rti[2] and rti[1] > 0  # d = +-max everywhere
    gx, gy = siti_ref.sobel_valid(frames[0])
    assert depth == 8 or (np.abs(gx).max() > 3000 and (gx * gx + gy * gy).max() > 1 << 24)
    for slots in (2, 1, None):
        si, ti = _run(frames, depth, gpu, slots=slots)
        _check(si, ti, rsi, rti, False)


@pytest.mark.parametrize("depth", [8, 10])
def test_siti_largest_difference_sum(gpu, depth):
    """Frame 0 all 0, frame 1 all max: d = +max on every pixel, the largest
    |sum d| and sum d^2 a wave can hold, and TI = 0 exactly (np sum d^2 equals
    (sum d)^2 as integers); back to 0 for the most negative sum."""
    mx = (1 << depth) - 1
    frames = np.zeros((3, 32, 512), np.int64)
    frames[1] = mx
    si, ti = _run(frames, depth, gpu, slots=2)
    assert np.isnan(ti[0]) and ti[1] == 0 and ti[2] == 0
    assert np.all(si == 0)
    # against a prev of the other extreme too
    si, ti = _run(frames, depth, gpu, slots=1, prev=np.full((32, 512), mx, np.int64))
    rsi, rti = siti_ref.siti(frames, prev=np.full((32, 512), mx, np.int64))
    assert np.all(ti == 0) and np.all(rti == 0)


def _ramp(depth, w, h):
    """A horizontal ramp that never saturates over w: |G| is one constant on the whole valid region."""
    x = np.arange(w)
    row = 2 * x if depth > 8 else x // 2  # 10 bits: gx = 16; 8 bits: v[x+1] - v[x-1] = 1, gx = 4
    assert row.max() < (1 << depth) - 1
    return np.tile(row, (h, 1)).astype(np.int64)


@pytest.mark.parametrize("depth", [8, 10])
def test_siti_pure_ramp_is_exactly_zero(gpu, depth):
    """A constant-magnitude frame gives SI == 0 exactly: the shift K is one of
    the lane's own samples, so every |G| - K is 0 (siti.hip's header)."""
    frames = np.stack([_ramp(depth, 497, 34)] * 3)
    gx, gy = siti_ref.sobel_valid(frames[0])
    assert np.all(gx == gx[0, 0]) and gx[0, 0] > 0 and not gy.any()
    for slots in (3, None):
        si, ti = _run(frames, depth, gpu, slots=slots)
        assert np.all(si == 0), si
        assert np.all(ti[1:] == 0)


@pytest.mark.parametrize("depth", [8, 10])
def test_siti_cancellation_under_a_large_constant_gradient(gpu, depth):
    """The ramp with one pixel in about 64 moved by +-1 (seeded): |G| is the
    ramp's constant nearly everywhere, so the standard deviation is small
    against the mean and E[x^2] - mean^2 in fp32 would lose it; the shifted
    moments must keep the project tolerance.  The reference SI is checked to
    lie well above atol before it is relied on."""
    rng = np.random.default_rng(64 + depth)
    frames = np.stack([_ramp(depth, 497, 34)] * 3)
    hit = rng.random(frames.shape) < 1.0 / 64
    frames = np.clip(frames + hit * rng.choice((-1, 1), frames.shape), 0, (1 << depth) - 1)
    rsi, rti = siti_ref.siti(frames)
    gx, gy = siti_ref.sobel_valid(frames[0])
    mean = np.sqrt((gx * gx + gy * gy).astype(np.float64)).mean()
    assert rsi.min() >= 1e-3 and rsi.max() < mean  # (the reference: std 0.42-0.45 on a mean of 16.0 at 10 bits, 4.0 at 8)
    for slots in (3, None):
        si, ti = _run(frames, depth, gpu, slots=slots)
        _check(si, ti, rsi, rti, False)
