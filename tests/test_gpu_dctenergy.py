"""pp_dct_energy / ops.dct_energy on the GPU (spec PP-DCTE-1) against the numpy
restatement (dctenergy_ref).  The sums are integers: the bar is equality, no
tolerance.

Every call of pp_dct_energy itself writes into sentinel-filled outputs two
frames longer than it needs and must change [n] alone; planes carry poisoned
pitch padding (gpu_calls.make).  The shapes are the smallest at which the
kernel can still be wrong: 31 x 40 and 40 x 31 (no block), 32, 33, 63, 64 and
65 in each direction, block counts one below, at and one above each seam it has
(a wave's 2 blocks, a workgroup's 8, the 256 lanes of the finalize kernel),
257 shown frames for the launch seam, both depths, on and off the 16-B grid,
with and without `prev`."""

import numpy as np
import pytest

import dctenergy_ref as R
from gpu_calls import call_sequence, make as _make, prev_args, untouched

pytestmark = pytest.mark.gpu

ABSENT = (1 << 64) - 1
_REF = {}


def _noise(depth, n, w, h, seed=0, full=False):
    """[n, h, w] noise over the depth's range, or (``full``) over the whole container."""
    key = (depth, n, w, h, seed, full)
    if key not in _REF:
        rng = np.random.default_rng(2000 + seed)
        top = (1 << (16 if full and depth > 8 else depth)) - 1
        _REF[key] = rng.integers(0, top + 1, (n, h, w)).astype(np.uint16 if depth > 8 else np.uint8)
    return _REF[key]


def _want(a, depth, idx=None, prev=None):
    """(sums, blocks) of the restatement, computed once per input."""
    key = ("dcte", depth, a.shape, a.tobytes(), None if idx is None else tuple(idx), None if prev is None else prev.tobytes())
    if key not in _REF:
        _REF[key] = (R.sums(a, depth, idx, prev), R.blocks(a, depth, idx, prev))
    return _REF[key]


def _call(gpu, depth, w, h, src, idx=None, n=None, nsrc=None, prev=None, sls=None, pls=None, null=(), blocks=True):
    """pp_dct_energy itself on sentinel-filled outputs of two frames more than
    it needs; returns (rc, out as n rows of Python ints, blocks as n [by][bx]
    lists or None, untouched: everything else kept the sentinel)."""
    bx, by = max(w, 0) // 32, max(h, 0) // 32
    nb = bx * by
    rc, k, (raw, rawb) = call_sequence(gpu, "pp_dct_energy", depth, w, h, src, prev_args(prev, pls),
                                       [("out", (3,), "int64"), ("blocks", (max(nb, 1),), "int64")], idx, n, nsrc, sls,
                                       tuple(null) + (() if blocks else ("blocks",)))
    kb = k if (blocks and nb) else 0
    got_b = None
    if blocks:
        got_b = [[[int(v) for v in rawb[f, j * bx:(j + 1) * bx]] for j in range(by)] if nb else [] for f in range(k)]
    return rc, [[int(v) for v in row] for row in raw[:k]], got_b, untouched(raw, k) and untouched(rawb, kb)


def _check(gpu, depth, a, idx=None, prev=None, layout="std", player="std", label=""):
    """a [nsrc, h, w] planes: the call's sums and map equal the restatement's; returns the sums."""
    want, want_b = _want(a, depth, idx, prev)  # CPU side first
    nsrc, h, w = a.shape
    src = _make(gpu, depth, a, layout, 1)
    pv = None if prev is None else _make(gpu, depth, prev[None], player, 2)[0:1]
    rc, got, got_b, untouched = _call(gpu, depth, w, h, src, idx, prev=pv)
    assert rc == 0 and untouched, (label, rc)
    assert got == want, (label, depth, w, h, layout, got, want)
    assert got_b == want_b, (label, depth, w, h, layout)
    for row, fb in zip(got, got_b):  # the map sums to the energy
        if row[0] != ABSENT:
            assert sum(sum(r) for r in fb) == row[0], label
    return got


def test_geometry_constants():
    from pixpath import dctenergy as D
    assert (D.BLOCK, D.BLOCKS_PER_WAVE, D.BLOCKS_PER_WORKGROUP, D.FINALIZE_LANES, D.FRAMES_PER_LAUNCH) == (32, 2, 8, 256, 256)
    assert (D.ENERGY_SCALE, D.DC_SCALE, D.ABSENT) == (1 << 20, 128, ABSENT)
    assert D.geometry(1920, 1080) == (60, 33) and D.geometry(31, 400) == (0, 12)


@pytest.mark.parametrize("depth", [8, 10])
def test_planes_without_a_block(gpu, depth):
    for w, h in ((31, 40), (40, 31), (1, 1)):
        a = _noise(depth, 2, w, h, seed=w)
        assert _check(gpu, depth, a, prev=a[0]) == [[ABSENT] * 3] * 2
        assert _check(gpu, depth, a, layout="odd") == [[ABSENT] * 3] * 2


@pytest.mark.parametrize("depth", [8, 10])
def test_sizes_around_one_and_two_blocks(gpu, depth):
    """32, 33, 63, 64, 65 in each direction: the ragged remainder never counts."""
    sizes = (32, 33, 63, 64, 65)
    for w in sizes:
        for h in sizes:
            if w != 33 and h != 33 and (w, h) not in ((32, 32), (65, 65), (63, 64), (64, 63)):
                continue  # every size in each direction, the pairs around 33 in full
            a = _noise(depth, 2, w, h, seed=w * 100 + h)
            got = _check(gpu, depth, a, prev=a[1], label="size")
            assert max(max(r) for r in got) < ABSENT
            _check(gpu, depth, a, layout="odd", label="size odd")
    a = _noise(depth, 2, 65, 65, seed=1)
    cut = np.ascontiguousarray(a[:, :64, :64])
    assert _check(gpu, depth, a, prev=a[1]) == _check(gpu, depth, cut, prev=cut[1])


@pytest.mark.parametrize("depth", [8, 10])
def test_block_count_seams(gpu, depth):
    """A wave's 2 blocks and a workgroup's 8, one below, at and one above, across and down, and two rows of blocks
    that split a workgroup."""
    for bx, by in ((1, 1), (2, 1), (3, 1), (7, 1), (8, 1), (9, 1), (1, 7), (1, 8), (1, 9), (3, 3), (5, 5)):
        a = _noise(depth, 2, bx * 32 + 5, by * 32 + 3, seed=bx * 10 + by)
        _check(gpu, depth, a, prev=a[1], label="blocks")
        _check(gpu, depth, a, layout="odd", player="odd", label="blocks odd")


def test_finalize_seams(gpu):
    """255, 256 and 257 blocks a frame: the 256 lanes of the finalize kernel; 513: three turns of its loop."""
    for bx, by in ((15, 17), (16, 16), (257, 1), (27, 19)):
        a = _noise(8, 2, bx * 32, by * 32, seed=bx)
        _check(gpu, 8, a, prev=a[1], label="finalize")


@pytest.mark.parametrize("depth", [8, 10])
def test_index_maps(gpu, depth):
    w, h = 70, 37
    for n in (1, 2, 5):
        a = _noise(depth, n, w, h, seed=n)
        assert _check(gpu, depth, a, label="n")[0][2] == ABSENT       # no prev: tdiff of entry 0 absent
        assert _check(gpu, depth, a, prev=a[n - 1], player="odd", label="n prev")[0][2] != ABSENT
    a = _noise(depth, 6, w, h, seed=66)
    idx = [0, 1, 1, 2, 5, 5, 3, 0, 4, 4, 2]  # repeats (exact 0), a backward step
    got = _check(gpu, depth, a, idx=idx, prev=a[0], label="index")
    assert [k for k, r in enumerate(got) if r[2] == 0] == [0, 2, 5, 9]
    assert _check(gpu, depth, a, idx=idx, layout="odd", label="index odd")[1:] == got[1:]
    assert _check(gpu, depth, a, idx=[3], prev=a[3])[0][2] == 0 and _check(gpu, depth, a, idx=[3])[0][2] == ABSENT


def test_layouts_give_equal_results(gpu):
    for depth, w, h in ((8, 300, 70), (10, 300, 70)):
        a = _noise(depth, 3, w, h, seed=5)
        p = _noise(depth, 1, w, h, seed=6)[0]
        got = [_check(gpu, depth, a, prev=p, layout=sl, player=pl, label="layout")
               for sl, pl in (("std", "std"), ("odd", "std"), ("std", "odd"), ("odd", "odd"))]
        assert got[0] == got[1] == got[2] == got[3]


def test_clamp_of_the_16_bit_container(gpu):
    """10-bit noise over the whole 16-bit range: a stored sample above 1023 counts as 1023."""
    a = _noise(10, 3, 70, 40, seed=8, full=True)
    assert (a > 1023).mean() > 0.9
    got = _check(gpu, 10, a, prev=a[2], label="clamp")
    _check(gpu, 10, a, prev=a[2], layout="odd", player="odd", label="clamp odd")
    clamped = np.minimum(a, 1023)
    assert _check(gpu, 10, clamped, prev=clamped[2]) == got
    mix = np.where(_noise(10, 3, 70, 40, seed=10) & 1, a, _noise(10, 3, 70, 40, seed=9))  # half in range, half above
    _check(gpu, 10, mix, prev=mix[0], label="clamp mix")


def _probe(depth, l, k):
    """The 32 x 32 block that drives Y[l][k] as high as it goes: the maximum where C[k][n] C[l][i] > 0, else 0."""
    top = (1 << depth) - 1
    return np.where(np.outer(R.C[l], R.C[k]) > 0, top, 0).astype(np.uint16 if depth > 8 else np.uint8)


@pytest.mark.parametrize("depth", [8, 10])
def test_overflow_probes(gpu, depth):
    planes = [_probe(depth, l, k) for l, k in ((1, 1), (31, 31), (0, 31))]
    planes.append(np.full((32, 32), (1 << depth) - 1, planes[0].dtype))  # the largest DC as well
    a = np.stack(planes)
    _check(gpu, depth, a, prev=np.zeros_like(a[0]), label="probe")
    _check(gpu, depth, a, layout="odd", label="probe odd")


@pytest.mark.parametrize("depth", [8, 10])
def test_full_hd_sums_exceed_32_bits(gpu, depth):
    """All-zero against the (1, 1) probe tiled over 1920 x 1080: energy and tdiff far above 2^32; twice the same bits."""
    a = np.zeros((2, 1080, 1920), np.uint16 if depth > 8 else np.uint8)
    a[1] = np.tile(_probe(depth, 1, 1), (34, 60))[:1080]
    e = R.frame(a[1, :32, :32], depth)[0][0, 0]
    d = R.frame(a[1, :32, :32], depth)[1][0, 0]
    nb = 60 * 33
    assert nb * e > 1 << 32
    src = _make(gpu, depth, a, "std", 1)
    rc, got, got_b, untouched = _call(gpu, depth, 1920, 1080, src, idx=[0, 1, 1, 0])
    assert rc == 0 and untouched
    assert got == [[0, 0, ABSENT], [nb * e, nb * d, nb * e], [nb * e, nb * d, 0], [0, 0, nb * e]]
    assert got_b[1] == [[e] * 60] * 33
    rc, again, again_b, _ = _call(gpu, depth, 1920, 1080, src, idx=[0, 1, 1, 0])
    assert again == got and again_b == got_b


def test_two_runs_give_equal_bits(gpu):
    a = _noise(10, 4, 330, 67, seed=12)
    src = _make(gpu, 10, a, "std", 1)
    runs = [_call(gpu, 10, 330, 67, src, prev=src[3:4])[1:3] for _ in range(2)]
    assert runs[0] == runs[1]
    assert (runs[0][0], runs[0][1]) == _want(a, 10, None, a[3])


def test_more_frames_than_a_launch(gpu):
    """257 and more shown frames on a 32 x 32 plane: the launch seam carries its previous frame."""
    from pixpath import dctenergy
    a = _noise(8, 3, 32, 32, seed=13)
    for n in (dctenergy.FRAMES_PER_LAUNCH, dctenergy.FRAMES_PER_LAUNCH + 1, dctenergy.FRAMES_PER_LAUNCH + 3):
        idx = [(k * 7) % 3 if k % 5 else (k // 5) % 3 for k in range(n)]  # repeats across the seam among them
        _check(gpu, 8, a, idx=idx, prev=a[1], label="launch")
    idx = [0] * 255 + [1, 1, 2]  # a step exactly at the seam, a repeat right after it
    got = _check(gpu, 8, a, idx=idx, label="launch seam")
    assert got[255][2] > 0 and got[256][2] == 0 and got[257][2] > 0


def test_without_a_map_and_no_frames(gpu):
    import torch
    from pixpath import ops
    a = _noise(8, 2, 40, 35)
    src = _make(gpu, 8, a)
    rc, got, got_b, untouched = _call(gpu, 8, 40, 35, src, blocks=False)  # blocks NULL: out alone
    assert rc == 0 and untouched and got_b is None and got == _want(a, 8)[0]
    rc, got, got_b, untouched = _call(gpu, 8, 40, 35, src, n=0)
    assert rc == 0 and got == [] and untouched
    out = ops.dct_energy(src[:0])
    assert out.dtype == torch.uint64 and tuple(out.shape) == (0, 3)
    out, bl = ops.dct_energy(src, index=[], blocks=True)
    assert tuple(out.shape) == (0, 3) and tuple(bl.shape) == (0, 1, 1)


def test_wrapper(gpu):
    import torch
    from pixpath import _native, dctenergy, ops
    from pixpath.frames import FrameBatch
    for fmt, depth in (("yuv420p", 8), ("yuv422p10le", 10)):
        w, h, n = 76, 68, 4
        a = _noise(depth, n, w, h, seed=21)
        cw, ch = w // 2, (h // 2 if fmt == "yuv420p" else h)
        b = FrameBatch.from_numpy(fmt, [a, np.zeros((n, ch, cw), np.int64), np.zeros((n, ch, cw), np.int64)], device=gpu)
        want, want_b = _want(a, depth)
        got, bl = ops.dct_energy(b, blocks=True)
        torch.cuda.synchronize(gpu)
        assert got.dtype == torch.uint64 and tuple(got.shape) == (n, 3)
        assert bl.dtype == torch.uint64 and tuple(bl.shape) == (n, 2, 2)
        assert [[int(v) for v in r] for r in got.cpu().numpy()] == want
        assert [[[int(v) for v in r] for r in f] for f in bl.cpu().numpy()] == want_b
        luma = b.view(0)
        for prev in (luma[3:4], luma[3], FrameBatch(b.fmt, w, h, 1, planes=[t[3:4] for t in b.planes])):
            got = ops.dct_energy(luma, index=[2, 0, 0, 3], prev=prev).cpu().numpy()
            assert [[int(v) for v in r] for r in got] == _want(a, depth, [2, 0, 0, 3], a[3])[0]
        E, T, L = dctenergy.pool(ops.dct_energy(b).cpu().numpy(), w, h)
        rE, rT, rL = R.pool(want, w, h)
        assert E.tolist() == rE and T.tolist() == rT and L.tolist() == rL and T[0] == 0.0
        with pytest.raises(ValueError):
            ops.dct_energy(luma, prev=luma[0, :-1])
        with pytest.raises(_native.PixpathError):
            ops.dct_energy(luma, index=[0, n])
    small = ops.dct_energy(torch.zeros((2, 20, 40), dtype=torch.uint8, device=gpu), blocks=True)
    assert tuple(small[1].shape) == (2, 0, 1) and [int(v) for v in small[0].cpu().numpy().ravel()] == [ABSENT] * 6


def test_return_codes(gpu):
    from pixpath import _native
    L = _native.lib()
    INVALID, UNSUPPORTED = -1, -4
    a = _noise(8, 3, 40, 35)
    src = _make(gpu, 8, a)
    a16 = _noise(10, 3, 40, 35)
    s16 = _make(gpu, 10, a16)

    def bad(code, word, depth=8, w=40, h=35, s=src, **kw):
        L.pp_dct_energy(None, 8, 1, 1, None, 0, 0, 0, None, 0, None, 0, None, None, None)  # leaves "null argument"
        rc, _, _, untouched = _call(gpu, depth, w, h, s, **kw)
        msg = L.pp_last_error().decode()
        assert rc == code and word in msg, (rc, msg)
        assert untouched  # nothing was launched

    for name in ("ctx", "src", "out"):
        rc, _, _, _ = _call(gpu, 8, 40, 35, src, null=(name,))
        assert rc == INVALID and b"null" in L.pp_last_error()
    bad(INVALID, "frame", w=0)
    bad(INVALID, "frame", h=0)
    bad(INVALID, "n -1", n=-1)
    bad(INVALID, "nsrc", nsrc=-1, n=0)
    bad(INVALID, "bitdepth", depth=9)
    bad(INVALID, "bitdepth", depth=16)
    bad(INVALID, "src plane 0: linesize", sls=39)
    bad(INVALID, "prev plane 0: linesize", prev=src[0:1], pls=39)
    bad(INVALID, "linesize", depth=10, s=s16, sls=79)
    bad(INVALID, "2-byte grid", depth=10, s=s16, sls=81)
    bad(INVALID, "2-byte grid", depth=10, s=s16, prev=s16[0:1], pls=81)
    bad(INVALID, "index[1] = 3", idx=[0, 3])
    bad(INVALID, "index[0] = -1", idx=[-1, 0])
    bad(INVALID, "without index", nsrc=1, n=2)
    bad(UNSUPPORTED, "2 GiB buffer range", h=64, sls=1 << 25)
    bad(UNSUPPORTED, "2 GiB buffer range", h=64, prev=src[0:1], pls=1 << 25)
    rc, got, _, untouched = _call(gpu, 8, 40, 35, src, idx=[2, 0], prev=src[1:2])  # and the same buffers are fine
    assert rc == 0 and untouched and got == _want(a, 8, [2, 0], a[1])[0]
