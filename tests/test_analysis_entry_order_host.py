"""The order in which the analysis entry points report the faults of a call:
every call below carries two faults that adjacent checks look for, and names
the one that is reported.  pp_metrics, pp_ciede, pp_psnr_hvs (planar pair),
pp_ms_ssim, pp_vif, pp_adm (luma pair), pp_motion, pp_banding, pp_dct_energy
(shown sequence).  No GPU: every call is refused, or has nothing to do, before
the first HIP call; nothing but return codes and message text is looked at."""
import ctypes

import pytest

from pixpath import _native, formats

INVALID, UNSUPPORTED = -1, -4
BIG = 1 << 25  # a pitch that puts 64 rows outside the 2 GiB buffer range


def _ptr(buf, on=True):
    return ctypes.c_void_p(ctypes.addressof(buf)) if on else None


def _map(idx):
    return None if idx is None else (ctypes.c_int32 * len(idx))(*idx)


def _frames(ls):
    buf = (ctypes.c_uint8 * 64)()  # never read
    fr = _native.pp_frames()
    for p in range(3):
        fr.data[p] = ctypes.addressof(buf)
        fr.linesize[p] = ls[p]
        fr.frame_stride[p] = 1024
    fr._keep = buf
    return fr


OPTION = {"pp_ciede": (1.0, 1.0, 1.0), "pp_psnr_hvs": (8,), "pp_banding": (3,)}
BAD_OPTION = {"pp_ciede": ((0.0, 1.0, 1.0), b"weights"), "pp_psnr_hvs": ((6,), b"step 6"), "pp_banding": ((4,), b"window 4")}


def _planar(name, fmt="yuv420p", w=20, h=15, rls=None, dls=None, idx=None, nref=2, ndist=2, opt=None):
    """A planar pair of 4:2:0 frames; `fmt` a name or a raw id."""
    L = _native.lib()
    ctx, out = (ctypes.c_uint8 * 256)(), (ctypes.c_uint8 * 256)()  # never dereferenced
    good = (64, 32, 32)
    ref, dist, ix = _frames(rls or good), _frames(dls or good), _map(idx)
    head = (ctx, fmt if isinstance(fmt, int) else formats.fmt(fmt).id, w, h, ctypes.byref(ref), ctypes.byref(dist),
            None if ix is None else ctypes.addressof(ix))
    if name == "pp_metrics":  # no nref: ndist is its nframes
        return L.pp_metrics(*head, ndist, _ptr(out), _ptr(out), None)
    return getattr(L, name)(*head, nref, ndist, *(opt or OPTION[name]), _ptr(out), None)


def _luma(name, depth=8, w=20, h=15, rls=64, dls=64, nref=2, ndist=2, idx=None):
    L = _native.lib()
    ctx, buf, ix = (ctypes.c_uint8 * 256)(), (ctypes.c_uint8 * 64)(), _map(idx)
    return getattr(L, name)(ctx, depth, w, h, _ptr(buf), rls, 1024, nref, _ptr(buf), dls, 1024, ndist,
                            None if ix is None else ctypes.addressof(ix), _ptr(buf), None)


def _seq(name, depth=8, w=20, h=15, sls=64, nsrc=2, n=2, idx=None, prev=False, pls=64, opt=None):
    L = _native.lib()
    ctx, buf, ix = (ctypes.c_uint8 * 256)(), (ctypes.c_uint8 * 64)(), _map(idx)
    head = (ctx, depth, w, h, _ptr(buf), sls, 1024, nsrc, None if ix is None else ctypes.addressof(ix), n)
    if name == "pp_banding":
        return L.pp_banding(*head, *(opt or OPTION[name]), None, _ptr(buf), None)
    tail = (_ptr(buf), None, None) if name == "pp_dct_energy" else (_ptr(buf), None)
    return getattr(L, name)(*head, _ptr(buf, prev), pls, *tail)


def _check(call, name, cases):
    L = _native.lib()
    for kw, rc, needle in cases:
        got = call(name, **kw)
        msg = L.pp_last_error()
        assert got == rc and needle in msg, (name, kw, got, msg)


# rows of 20 samples: 20 bytes at 8 bits, 40 at 10; the 4:2:0 chroma rows hold 10 samples
PLANAR_COMMON = [
    # ref plane 0, dist plane 0, ref plane 1, ..: planes outside, clips inside
    (dict(rls=(64, 9, 32), dls=(19, 32, 32)), INVALID, b"plane 0"),
    (dict(rls=(BIG, 32, 32), dls=(19, 32, 32), h=64), UNSUPPORTED, b"2 GiB buffer range"),
    (dict(rls=(19, 32, 32), dls=(BIG, 32, 32), h=64), INVALID, b"plane 0"),
    # short pitch + off-grid pitch: a plane's grid test follows its own checks and precedes the other clip's
    (dict(fmt="yuv420p10le", rls=(39, 32, 32)), INVALID, b"linesize"),
    (dict(fmt="yuv420p10le", rls=(41, 32, 32), dls=(39, 32, 32)), INVALID, b"plane 0: 16-bit samples off the 2-byte grid"),
    (dict(fmt="yuv420p10le", rls=(64, 19, 32), dls=(41, 32, 32)), INVALID, b"plane 0: 16-bit samples off the 2-byte grid"),
]

PLANAR = {
    "pp_metrics": [
        (dict(fmt=99, w=0), INVALID, b"metrics need a planar format"),
        (dict(w=0, ndist=0), INVALID, b"frame 0x15"),
        (dict(ndist=0, rls=(19, 32, 32)), INVALID, b"nframes 0 < 1"),  # an empty call is refused here
        (dict(idx=[0, -1], rls=(19, 32, 32)), INVALID, b"ref_index[1] = -1 is negative"),
        (dict(rls=(19, 32, 32), dls=(19, 32, 32)), INVALID, b"plane 0: null data or short linesize"),
        (dict(fmt="yuv420p10le", idx=[-1, 0], rls=(41, 32, 32)), INVALID, b"ref_index[0] = -1 is negative"),
    ],
    "pp_ciede": [(dict(fmt=99, w=0), INVALID, b"ciede needs a planar format")],
    "pp_psnr_hvs": [(dict(fmt=99, w=0), INVALID, b"psnr_hvs needs a planar format")],
}
for _name in ("pp_ciede", "pp_psnr_hvs"):
    _bad, _word = BAD_OPTION[_name]
    PLANAR[_name] += [
        (dict(w=0, ndist=-1), INVALID, b"frame 0x15"),
        (dict(ndist=-1, nref=-2), INVALID, b"ndist -1 < 0"),
        (dict(nref=-2, opt=_bad), INVALID, b"nref -2 < 0"),
        (dict(opt=_bad, rls=(19, 32, 32)), INVALID, _word),
        (dict(rls=(19, 32, 32), dls=(19, 32, 32)), INVALID, b"ref plane 0: linesize 19 below the row's 20 bytes"),
        (dict(rls=(64, 9, 32), dls=(19, 32, 32)), INVALID, b"dist plane 0: linesize"),
        (dict(fmt="yuv420p10le", rls=(41, 32, 32), dls=(39, 32, 32)), INVALID, b"ref plane 0: 16-bit"),
        (dict(fmt="yuv420p10le", dls=(64, 32, 21), idx=[0, 2]), INVALID, b"dist plane 2: 16-bit samples off the 2-byte grid"),
        (dict(idx=[0, 2], ndist=2), INVALID, b"ref_index[1] = 2 outside the 2 reference frames"),
        (dict(nref=1), INVALID, b"ndist 2 > nref 1 without ref_index"),
    ]


@pytest.mark.parametrize("name", list(PLANAR))
def test_planar_pair_reports_the_first_fault(name):
    _check(_planar, name, PLANAR[name] + PLANAR_COMMON)


LUMA = [
    (dict(depth=9, w=0), INVALID, b"bitdepth 9 (8 or 10)"),
    (dict(w=0, ndist=-1), INVALID, b"frame 0x15"),
    (dict(ndist=-1, nref=-2), INVALID, b"ndist -1 < 0"),
    (dict(nref=-2, rls=19), INVALID, b"nref -2 < 0"),
    (dict(rls=19, dls=19), INVALID, b"ref plane 0: linesize 19 below the row's 20 bytes"),
    (dict(rls=BIG, dls=19, h=64), UNSUPPORTED, b"2 GiB buffer range"),
    # the grid test follows both planes
    (dict(depth=10, rls=41, dls=39), INVALID, b"dist plane 0: linesize 39 below the row's 40 bytes"),
    (dict(depth=10, rls=39), INVALID, b"ref plane 0: linesize"),
    (dict(depth=10, dls=41, idx=[0, 2]), INVALID, b"16-bit samples off the 2-byte grid"),
    (dict(idx=[0, 2]), INVALID, b"ref_index[1] = 2 outside the 2 reference frames"),
    (dict(nref=1), INVALID, b"ndist 2 > nref 1 without ref_index"),
]


@pytest.mark.parametrize("name", ["pp_ms_ssim", "pp_vif", "pp_adm"])
def test_luma_pair_reports_the_first_fault(name):
    _check(_luma, name, LUMA)


SEQ = [
    (dict(depth=9, w=0), INVALID, b"bitdepth 9 (8 or 10)"),
    (dict(w=0, n=-1), INVALID, b"frame 0x15"),
    (dict(n=-1, nsrc=-2), INVALID, b"n -1 < 0"),
    (dict(nsrc=-2, sls=19), INVALID, b"nsrc -2 < 0"),
    (dict(depth=10, sls=39), INVALID, b"src plane 0: linesize 39 below the row's 40 bytes"),
    (dict(depth=10, sls=41, idx=[0, 2]), INVALID, b"16-bit samples off the 2-byte grid"),
    (dict(idx=[0, 2]), INVALID, b"index[1] = 2 outside the 2 source frames"),
    (dict(nsrc=1), INVALID, b"n 2 > nsrc 1 without index"),
]
WITH_PREV = [
    (dict(sls=19, prev=True, pls=19), INVALID, b"src plane 0: linesize"),
    (dict(sls=BIG, h=64, prev=True, pls=19), UNSUPPORTED, b"2 GiB buffer range"),
    (dict(sls=19, h=64, prev=True, pls=BIG), INVALID, b"src plane 0: linesize"),
    # the grid test follows both planes
    (dict(depth=10, sls=41, prev=True, pls=39), INVALID, b"prev plane 0: linesize 39 below the row's 40 bytes"),
    (dict(depth=10, prev=True, pls=41, idx=[0, 2]), INVALID, b"16-bit samples off the 2-byte grid"),
]
# the window is looked at between nsrc and the plane
WINDOW = [
    (dict(nsrc=-2, opt=BAD_OPTION["pp_banding"][0]), INVALID, b"nsrc -2 < 0"),
    (dict(opt=BAD_OPTION["pp_banding"][0], sls=19), INVALID, b"window 4 (odd, 3 .. "),
]


@pytest.mark.parametrize("name", ["pp_motion", "pp_banding", "pp_dct_energy"])
def test_shown_sequence_reports_the_first_fault(name):
    _check(_seq, name, SEQ + (WINDOW if name == "pp_banding" else WITH_PREV))


def test_an_empty_call_is_ok_without_a_device():
    for name in ("pp_ciede", "pp_psnr_hvs"):
        assert _planar(name, ndist=0) == 0 and _planar(name, ndist=0, nref=0) == 0
        assert _planar(name, ndist=0, idx=[]) == 0 and _planar(name, fmt="yuv420p10le", ndist=0) == 0
    for name in ("pp_ms_ssim", "pp_vif", "pp_adm"):
        assert _luma(name, ndist=0) == 0 and _luma(name, ndist=0, nref=0) == 0 and _luma(name, depth=10, ndist=0) == 0
    for name in ("pp_motion", "pp_banding", "pp_dct_energy"):
        assert _seq(name, n=0) == 0 and _seq(name, n=0, nsrc=0) == 0 and _seq(name, depth=10, n=0) == 0
    assert _seq("pp_motion", n=0, prev=True) == 0 and _seq("pp_dct_energy", n=0, prev=True) == 0
