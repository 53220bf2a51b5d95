"""pp_motion / ops.motion on the GPU (spec PP-MOTION-1) against the numpy
restatement (motion_ref.sad).  The sums are integers: the bar is
np.array_equal, no tolerance.

Every call of pp_motion itself writes into a sentinel-filled output two entries
longer than it needs and must change [n] alone; planes carry poisoned pitch
padding (gpu_calls.make).  The shapes are the smallest at which the kernel
can still be wrong: 3 x 3, 3 x 40, 40 x 3, and widths and heights one below, at
and one above each seam it has (a lane's piece of 16 B, a tile's 62 pieces, a
wave's 64 pieces, a wave's 16 rows, a tile's 64 rows), sequences one below, at
and one above the segment of 4 shown frames, both depths, on and off the 16-B
grid, with and without `prev`."""

import numpy as np
import pytest

import motion_ref as R
from gpu_calls import call_sequence, make as _make, prev_args, untouched

pytestmark = pytest.mark.gpu

ABSENT = (1 << 64) - 1
_REF = {}


def _noise(depth, n, w, h, seed=0, full=False):
    """[n, h, w] noise over the depth's range, or (``full``) over the whole container."""
    key = (depth, n, w, h, seed, full)
    if key not in _REF:
        rng = np.random.default_rng(1000 + seed)
        top = (1 << (16 if full and depth > 8 else depth)) - 1
        _REF[key] = rng.integers(0, top + 1, (n, h, w)).astype(np.uint16 if depth > 8 else np.uint8)
    return _REF[key]


def _want(a, depth, idx=None, prev=None):
    key = ("sad", depth, a.shape, a.tobytes(), None if idx is None else tuple(idx), None if prev is None else prev.tobytes())
    if key not in _REF:
        _REF[key] = R.sad(a, depth, idx, prev)
    return _REF[key]


def _call(gpu, depth, w, h, src, idx=None, n=None, nsrc=None, prev=None, sls=None, pls=None, null=()):
    """pp_motion itself on a sentinel-filled output of two entries more than it
    needs; returns (rc, sad as a list of Python ints, untouched: everything else kept the sentinel)."""
    rc, k, (raw,) = call_sequence(gpu, "pp_motion", depth, w, h, src, prev_args(prev, pls), [("sad", (), "int64")],
                                  idx, n, nsrc, sls, null)
    return rc, [int(v) for v in raw[:k]], untouched(raw, k)


def _check(gpu, depth, a, idx=None, prev=None, layout="std", player="std", label=""):
    """a [nsrc, h, w] planes: the call's sums equal motion_ref's; returns them."""
    want = _want(a, depth, idx, prev)  # CPU side first
    nsrc, h, w = a.shape
    src = _make(gpu, depth, a, layout, 1)
    pv = None if prev is None else _make(gpu, depth, prev[None], player, 2)[0:1]
    rc, got, untouched = _call(gpu, depth, w, h, src, idx, prev=pv)
    assert rc == 0 and untouched, (label, rc)
    assert got == want, (label, depth, w, h, layout, got, want)
    return got


def test_geometry_constants():
    from pixpath import motion
    assert (motion.LANE_BYTES, motion.TILE_PIECES, motion.WAVE_PIECES) == (16, 62, 64)
    assert (motion.WAVE_ROWS, motion.TILE_ROWS, motion.SEGMENT, motion.FRAMES_PER_LAUNCH) == (16, 64, 4, 256)
    assert motion.tile_cols(8) == 992 and motion.tile_cols(10) == 496 and motion.MIN_SIZE == 3


@pytest.mark.parametrize("depth", [8, 10])
def test_smallest_planes(gpu, depth):
    for w, h in ((3, 3), (3, 40), (40, 3), (4, 5)):
        a = _noise(depth, 3, w, h, seed=w * 100 + h)
        for layout in ("std", "odd"):
            got = _check(gpu, depth, a, prev=a[2], layout=layout, player=layout, label="small")
            assert max(got) < ABSENT
    for w, h in ((2, 9), (9, 2), (1, 1)):  # one reflection does not suffice: absent, prev or not
        a = _noise(depth, 2, w, h, seed=7)
        assert _check(gpu, depth, a, prev=a[0]) == [ABSENT, ABSENT]
        assert _check(gpu, depth, a, layout="odd") == [ABSENT, ABSENT]


def _seam_widths(depth):
    spp = 16 if depth == 8 else 8
    return [spp - 1, spp, spp + 1, 2 * spp + 1, 62 * spp - 1, 62 * spp, 62 * spp + 1, 62 * spp + 2, 62 * spp + 3,
            64 * spp - 1, 64 * spp, 64 * spp + 1, 124 * spp + 1]


@pytest.mark.parametrize("depth", [8, 10])
def test_width_seams(gpu, depth):
    """A lane's piece, a tile's columns (and the two columns past it that the halo
    serves), a wave's 64 pieces, two tiles and a sample."""
    for w in _seam_widths(depth):
        a = _noise(depth, 2, w, 5, seed=w)
        _check(gpu, depth, a, prev=a[1], label="width")
        _check(gpu, depth, a, prev=a[1], layout="odd", player="odd", label="width odd")


@pytest.mark.parametrize("depth", [8, 10])
def test_height_seams(gpu, depth):
    """A wave's 16 rows and a tile's 64 rows, one below, at and one above, and two tiles and a row."""
    for h in (15, 16, 17, 18, 63, 64, 65, 66, 129):
        a = _noise(depth, 2, 21, h, seed=h)
        _check(gpu, depth, a, prev=a[1], label="height")
        _check(gpu, depth, a, layout="odd", label="height odd")


@pytest.mark.parametrize("depth", [8, 10])
def test_segment_seams_and_index(gpu, depth):
    w, h = 37, 19
    for n in (1, 3, 4, 5, 8, 9):
        a = _noise(depth, n, w, h, seed=n)
        _check(gpu, depth, a, label="n")                      # no prev: entry 0 absent
        assert _check(gpu, depth, a, prev=a[n - 1], player="odd", label="n prev")[0] != ABSENT
    a = _noise(depth, 6, w, h, seed=66)
    # repeats (exact 0), a backward step, entries straddling the seams after shown frames 4 and 8
    idx = [0, 1, 1, 2, 5, 5, 3, 0, 4, 4, 2]
    got = _check(gpu, depth, a, idx=idx, prev=a[0], label="index")
    assert [k for k, v in enumerate(got) if v == 0] == [0, 2, 5, 9]
    assert _check(gpu, depth, a, idx=idx, layout="odd", label="index odd")[1:] == got[1:]
    assert _check(gpu, depth, a, idx=[3], prev=a[3]) == [0] and _check(gpu, depth, a, idx=[3]) == [ABSENT]


def test_layouts_give_equal_results(gpu):
    """Two tiles across and down, every layout of source and prev: one result."""
    for depth, w, h in ((8, 1000, 70), (10, 500, 70)):
        a = _noise(depth, 5, w, h, seed=5)
        p = _noise(depth, 1, w, h, seed=6)[0]
        got = [_check(gpu, depth, a, prev=p, layout=sl, player=pl, label="layout")
               for sl, pl in (("std", "std"), ("odd", "std"), ("std", "odd"), ("odd", "odd"))]
        assert got[0] == got[1] == got[2] == got[3]


def test_clamp_of_the_16_bit_container(gpu):
    """10-bit noise over the whole 16-bit range: a stored sample above 1023 counts as 1023."""
    a = _noise(10, 5, 70, 33, seed=8, full=True)
    assert (a > 1023).mean() > 0.9
    got = _check(gpu, 10, a, prev=a[4], label="clamp")
    _check(gpu, 10, a, prev=a[4], layout="odd", player="odd", label="clamp odd")
    clamped = np.minimum(a, 1023)
    assert _check(gpu, 10, clamped, prev=clamped[4]) == got
    b = _noise(10, 5, 70, 33, seed=9)
    b[1, 5:9, 7:30] = 40000
    _check(gpu, 10, b, label="clamp patch")
    mix = np.where(_noise(10, 5, 70, 33, seed=10) & 1, a, _noise(10, 5, 70, 33, seed=9))  # half in range, half above
    _check(gpu, 10, mix, prev=mix[0], label="clamp mix")


@pytest.mark.parametrize("depth", [8, 10])
def test_full_hd_extremes_exceed_32_bits(gpu, depth):
    """All-0 against all-max at 1920 x 1080: B = c 2^(16-d) exactly, a sum far above 2^32; twice the same bits."""
    top = (1 << depth) - 1
    a = np.zeros((2, 1080, 1920), np.uint16 if depth > 8 else np.uint8)
    a[1] = top
    want = 1920 * 1080 * (top << (16 - depth))
    assert want > 1 << 32
    src = _make(gpu, depth, a, "std", 1)
    rc, got, untouched = _call(gpu, depth, 1920, 1080, src, idx=[0, 1, 1, 0])
    assert rc == 0 and untouched and got == [ABSENT, want, 0, want]
    rc, again, _ = _call(gpu, depth, 1920, 1080, src, idx=[0, 1, 1, 0])
    assert again == got


def test_two_runs_give_equal_bits(gpu):
    a = _noise(10, 6, 530, 67, seed=12)
    src = _make(gpu, 10, a, "std", 1)
    runs = [_call(gpu, 10, 530, 67, src, prev=src[5:6])[1] for _ in range(2)]
    assert runs[0] == runs[1] == _want(a, 10, None, a[5])


def test_more_frames_than_a_launch(gpu):
    """More shown frames than one launch's map holds: the launch seam carries its previous frame."""
    from pixpath import motion
    a = _noise(8, 3, 20, 6, seed=13)
    idx = [(k * 7) % 3 for k in range(motion.FRAMES_PER_LAUNCH + 3)]
    _check(gpu, 8, a, idx=idx, prev=a[1], label="launch")


def test_no_frames_writes_nothing(gpu):
    import torch
    from pixpath import ops
    a = _noise(8, 2, 20, 15)
    src = _make(gpu, 8, a)
    rc, got, untouched = _call(gpu, 8, 20, 15, src, n=0)
    assert rc == 0 and got == [] and untouched
    out = ops.motion(src[:0])
    assert out.dtype == torch.uint64 and tuple(out.shape) == (0,)
    assert tuple(ops.motion(src, index=[]).shape) == (0,)


def test_wrapper(gpu):
    import torch
    from pixpath import _native, motion, ops
    from pixpath.frames import FrameBatch
    for fmt, depth in (("yuv420p", 8), ("yuv422p10le", 10)):
        w, h, n = 44, 36, 5
        a = _noise(depth, n, w, h, seed=21)
        cw, ch = w // 2, (h // 2 if fmt == "yuv420p" else h)
        b = FrameBatch.from_numpy(fmt, [a, np.zeros((n, ch, cw), np.int64), np.zeros((n, ch, cw), np.int64)], device=gpu)
        got = ops.motion(b)
        torch.cuda.synchronize(gpu)
        assert got.dtype == torch.uint64 and tuple(got.shape) == (n,)
        assert [int(v) for v in got.cpu().numpy()] == _want(a, depth)
        luma = b.view(0)
        for prev in (luma[4:5], luma[4], FrameBatch(b.fmt, w, h, 1, planes=[t[4:5] for t in b.planes])):
            got = ops.motion(luma, index=[2, 0, 0, 3], prev=prev).cpu().numpy()
            assert [int(v) for v in got] == _want(a, depth, [2, 0, 0, 3], a[4])
        m, m2 = motion.pool(ops.motion(b).cpu().numpy(), w, h)
        rm, rm2 = R.motion(_want(a, depth), w, h)
        assert m.tolist() == rm and m2.tolist() == rm2 and m[0] == 0.0
        with pytest.raises(ValueError):
            ops.motion(luma, prev=luma[0, :-1])
        with pytest.raises(_native.PixpathError):
            ops.motion(luma, index=[0, n])


def test_return_codes(gpu):
    from pixpath import _native
    L = _native.lib()
    INVALID, UNSUPPORTED = -1, -4
    a = _noise(8, 3, 20, 15)
    src = _make(gpu, 8, a)
    a16 = _noise(10, 3, 20, 15)
    s16 = _make(gpu, 10, a16)

    def bad(code, word, depth=8, w=20, h=15, s=src, **kw):
        L.pp_motion(None, 8, 1, 1, None, 0, 0, 0, None, 0, None, 0, None, None)  # leaves "null argument"
        rc, _, untouched = _call(gpu, depth, w, h, s, **kw)
        msg = L.pp_last_error().decode()
        assert rc == code and word in msg, (rc, msg)
        assert untouched  # nothing was launched

    for name in ("ctx", "src", "sad"):
        rc, _, _ = _call(gpu, 8, 20, 15, src, null=(name,))
        assert rc == INVALID and b"null" in L.pp_last_error()
    bad(INVALID, "frame", w=0)
    bad(INVALID, "frame", h=0)
    bad(INVALID, "n -1", n=-1)
    bad(INVALID, "nsrc", nsrc=-1, n=0)
    bad(INVALID, "bitdepth", depth=9)
    bad(INVALID, "bitdepth", depth=16)
    bad(INVALID, "src plane 0: linesize", sls=19)
    bad(INVALID, "prev plane 0: linesize", prev=src[0:1], pls=19)
    bad(INVALID, "linesize", depth=10, s=s16, sls=39)
    bad(INVALID, "2-byte grid", depth=10, s=s16, sls=41)
    bad(INVALID, "2-byte grid", depth=10, s=s16, prev=s16[0:1], pls=41)
    bad(INVALID, "index[1] = 3", idx=[0, 3])
    bad(INVALID, "index[0] = -1", idx=[-1, 0])
    bad(INVALID, "without index", nsrc=1, n=2)
    bad(UNSUPPORTED, "2 GiB buffer range", h=64, sls=1 << 25)
    bad(UNSUPPORTED, "2 GiB buffer range", h=64, prev=src[0:1], pls=1 << 25)
    rc, got, untouched = _call(gpu, 8, 20, 15, src, idx=[2, 0], prev=src[1:2])  # and the same buffers are fine
    assert rc == 0 and untouched and got == _want(a, 8, [2, 0], a[1])
