"""Case table of the pad / stall row kernels and the fused CPVS kernel: small
launches that between them take every arm ops.pack_arms can report
(enum pp_pack_arm, csrc/pack_plan.hpp).

CASES is written by hand: each entry is one launch in one memory layout with
the arms it was built for (`arms`).  tests/pack_arms_table.py records every arm
each case holds (tools/gen_pack_arms.py rewrites it); test_pack_arms.py checks
on the CPU that the record is current, that the cases cover every arm of every
kernel instance, and that each case holds an arm no other case holds;
test_gpu_pack_arms.py runs every case against the oracle.

Layouts (the alignment facts below are what the GPU test allocates):
  source       "pitched"  FrameBatch rows (16-B pitch)
               "dense"    frame-interleaved dense Y|U|V (rows at any offset)
  destination  "guard"    16-B pitch + 16 guard bytes a row + one guard row
               "offset"   the same buffer entered one sample in (unaligned)
"""
import collections

import numpy as np

from pixpath import formats, ops

BASE = 1 << 16  # a 16-B aligned stand-in address
GUARD = 16      # guard bytes after every destination row

Case = collections.namedtuple("Case", "id op fmt w h W H x y n src dst spin src_index spinner_index arms error")


def case(id, op, fmt, w, h, W=None, H=None, x=-1, y=-1, n=1, src="pitched", dst="guard", spin=None,
         src_index=None, spinner_index=None, arms=(), error=None):
    return Case(id, op, fmt, w, h, w if W is None else W, h if H is None else H, x, y, n, src, dst, spin,
                src_index, spinner_index, tuple(arms), error)


def _cpvs(fmt, bits, v420):
    tail = (["cpvs_c8_slow_tail", "cpvs_c8_fast"] if bits == 8 else ["cpvs_v210_tail2", "cpvs_v210_zero"])
    br = ["cpvs_c8_offgrid"] if bits == 8 else ["cpvs_v210_tail4"]
    # second staging pass: more than 512 16-B pieces (4:2:0 stages luma only)
    # (w, W): v210 canvases a multiple of 6 wide, so the tail arms stay with the small cases
    wide, wideW = {(8, True): (8208, 8208), (8, False): (4128, 4128), (10, True): (4116, 4116),
                   (10, False): (16384, 16386)}[bits, v420]
    g = ["cpvs_group_vec"] if v420 else []
    return [
        # flush top-left, odd w / h / H (4:2:0: ch = ceil(h/2), csh = ceil(H/2))
        case(fmt + "-cpvs-flush00-odd", "cpvs", fmt, 21, 5, 26, 7, 0, 0, n=2,
             arms=tail + g + ["cpvs_row_live", "cpvs_row_pad", "cpvs_stage_vec_one"] + (["cpvs_tap_below"] if v420 else [])),
        # flush bottom-right; 8-bit: offset 20 is off the 8-px grid on live, aligned rows
        case(fmt + "-cpvs-flushBR", "cpvs", fmt, 20, 4, 40, 8, 20, 4, n=2, arms=br + (["cpvs_tap_above"] if v420 else [])),
        # odd x and y rounded down to the chroma grid (9, 3 -> 8, 2 for 4:2:0), dense source rows
        case(fmt + "-cpvs-oddxy-dense", "cpvs", fmt, 22, 4, 48, 8, 9, 3, n=3, src="dense",
             arms=["cpvs_stage_samples"] + (["cpvs_group_samples", "cpvs_group_clamped"] if v420 else [])),
        case(fmt + "-cpvs-wide", "cpvs", fmt, wide, 2, wideW, 4 if v420 else 2, 0, 0,
             arms=["cpvs_stage_vec_multi", "cpvs_chunks_gt64"] + (["cpvs_groups_gt64"] if v420 else [])),
        case(fmt + "-cpvs-past-edge", "cpvs", fmt, 20, 4, 40, 8, 22, 0, error=(-1, "exceeds")),
    ]


def _pad(bits):
    s = "" if bits == 8 else "10le"
    wide = 4128 if bits == 8 else 2064  # more than 256 16-B chunks a row, every plane whole chunks
    return [
        case("yuv420p%s-pad-flush00-odd" % s, "pad", "yuv420p" + s, 21, 5, 24, 7, 0, 0, n=2,
             arms=["row_420", "row_src_vec", "row_src_edge", "row_src_null", "row_dst_vec", "row_dst_tail"]),
        case("yuv422p%s-pad-flushBR" % s, "pad", "yuv422p" + s, 32, 4, 48, 8, 16, 4, n=2,
             arms=["row_422", "row_src_vec", "row_src_outside"]),
        case("yuv444p%s-pad-oddxy" % s, "pad", "yuv444p" + s, 20, 4, 40, 8, 7, 3, n=2, arms=["row_444", "row_src_scalar"]),
        case("yuv420p%s-pad-oddxy-dense-offset" % s, "pad", "yuv420p" + s, 22, 6, 40, 10, 7, 3, n=3, src="dense",
             dst="offset", arms=["row_dst_scalar", "row_src_scalar"]),
        case("yuv422p%s-pad-wide" % s, "pad", "yuv422p" + s, wide, 2, wide, 2, 0, 0, arms=["row_chunks_gt256"]),
        case("yuv420p%s-pad-past-edge" % s, "pad", "yuv420p" + s, 20, 4, 40, 8, 22, 0, error=(-1, "exceeds")),
    ]


def _stall(bits):
    s = "" if bits == 8 else "10le"
    wide = 4112 if bits == 8 else 2064
    return [
        case("yuv420p%s-stall-2x2" % s, "stall", "yuv420p" + s, 24, 4, n=2, spin=(2, 2, 2),
             src_index=[0, 1, -1], spinner_index=[0, -1, 1],
             arms=["row_420", "stall_tile_short", "stall_src_change", "stall_black", "stall_no_spinner",
                   "stall_spin_left", "stall_spin_right", "row_src_null", "row_src_edge", "row_dst_tail"]),
        case("yuv444p%s-stall-20x12" % s, "stall", "yuv444p" + s, 40, 12, n=2, spin=(2, 20, 12),
             src_index=[1, 0], spinner_index=[0, 1], arms=["row_444", "stall_spin_left", "stall_spin_right"]),
        case("yuv422p%s-stall-frame-size" % s, "stall", "yuv422p" + s, 32, 4, n=1, spin=(1, 32, 4),
             src_index=[0, 0], spinner_index=[0, 0], arms=["row_422", "stall_spin_inside", "row_src_vec", "row_dst_vec"]),
        case("yuv420p%s-stall-larger" % s, "stall", "yuv420p" + s, 16, 4, n=1, spin=(1, 24, 8),
             src_index=[0], spinner_index=[0], arms=["stall_spin_clipped"]),
        # 13 frames: two whole tiles of G = 6 and a last tile of one, source changes on the tile seams
        case("yuv420p%s-stall-tiles-dense-offset" % s, "stall", "yuv420p" + s, 24, 4, n=3, src="dense", dst="offset",
             spin=(3, 4, 2), src_index=[0] * 6 + [1] * 6 + [2], spinner_index=[k % 3 for k in range(13)],
             arms=["stall_tile_full", "stall_tile_short", "row_src_scalar", "row_dst_scalar"]),
        case("yuv420p%s-stall-260-frames" % s, "stall", "yuv420p" + s, 16, 4, n=2, spin=(2, 4, 2),
             src_index=[k // 7 % 2 for k in range(260)], spinner_index=[k % 2 for k in range(260)],
             arms=["stall_launch_split"]),
        case("yuv420p%s-stall-wide-no-spinner" % s, "stall", "yuv420p" + s, wide, 2, n=1,
             src_index=[0], spinner_index=[-1], arms=["row_chunks_gt256", "stall_no_spinner"]),
    ]


CASES = (
    _cpvs("yuv420p", 8, True) + _cpvs("yuv422p", 8, False) + _cpvs("yuv420p10le", 10, True)
    + _cpvs("yuv422p10le", 10, False)
    + [
        # the LDS row stage holds 64 KiB: 16384 is the widest 10-bit 4:2:2 row it accepts (the wide case above)
        case("yuv422p10le-cpvs-lds-reject", "cpvs", "yuv422p10le", 16392, 2, error=(-4, "LDS")),
        case("yuv422p10le-cpvs-odd-canvas", "cpvs", "yuv422p10le", 20, 4, 27, 8, error=(-1, "even width, not 27")),
        case("v210-20", "v210", "yuv422p10le", 20, 2, n=2, arms=["cpvs_v210_tail2", "cpvs_v210_zero", "cpvs_stage_vec_one"]),
        case("v210-22-dense", "v210", "yuv422p10le", 22, 3, n=3, src="dense", arms=["cpvs_v210_tail4", "cpvs_stage_samples"]),
        case("v210-wide", "v210", "yuv422p10le", 2064, 2, arms=["cpvs_stage_vec_multi", "cpvs_chunks_gt64"]),
        case("v210-odd", "v210", "yuv422p10le", 21, 2, error=(-1, "even width, not 21")),
    ]
    + _pad(8) + _pad(10) + _stall(8) + _stall(10)
)

_CPVS = {"cpvs_row_live", "cpvs_row_pad", "cpvs_stage_vec_one", "cpvs_stage_vec_multi", "cpvs_stage_samples",
         "cpvs_chunks_gt64"}
_C8 = {"cpvs_c8_fast", "cpvs_c8_offgrid", "cpvs_c8_slow_full", "cpvs_c8_slow_tail"}
_C10 = {"cpvs_v210_full", "cpvs_v210_tail2", "cpvs_v210_tail4", "cpvs_v210_zero"}
_G420 = {"cpvs_group_vec", "cpvs_group_samples", "cpvs_group_clamped", "cpvs_tap_above", "cpvs_tap_below",
         "cpvs_groups_gt64"}
_ROW = {"row_src_vec", "row_src_edge", "row_src_scalar", "row_src_null", "row_dst_vec", "row_dst_tail",
        "row_dst_scalar", "row_chunks_gt256", "row_420", "row_422", "row_444"}
_STALL = {a for a in ops.PACK_ARMS if a.startswith("stall_")}
# The arms each kernel instance compiles.  "v210" is pp_v210_pack: the 10-bit
# 4:2:2 instance with the canvas = the frame (no pad rows), kept apart so its
# entry point has cases of its own.  A stall source row is never shifted, so
# no chunk of it lies outside the image.
REQUIRED = {
    "cpvs8_420": _CPVS | _C8 | _G420, "cpvs8_422": _CPVS | _C8, "cpvs10_420": _CPVS | _C10 | _G420,
    "cpvs10_422": _CPVS | _C10, "v210": (_CPVS - {"cpvs_row_pad"}) | _C10,
    "pad8": _ROW | {"row_src_outside"}, "pad16": _ROW | {"row_src_outside"},
    "stall8": _ROW | _STALL, "stall16": _ROW | _STALL,
}
UNREACHED = {
    "cpvs_group_vec_ragged":
        "a vector chroma group past the padded row needs ceil(cw / 8) > cs / 8, but cs is cw rounded up to whole "
        "16-B groups (16 samples at 8 bits, 8 at 10), so cs / 8 >= ceil(cw / 8) for every cw; the kernel's "
        "`g < nfull` term was always true with aligned rows and is deleted",
}


def _pitch(nbytes):
    return (nbytes + 15) // 16 * 16


def out_fmt(c):
    """The destination format of a case."""
    f = formats.fmt(c.fmt)
    if c.op == "v210":
        return formats.fmt(formats.V210)
    if c.op == "cpvs":
        return formats.fmt(formats.UYVY422 if f.depth == 8 else formats.V210)
    return f


def _bps(f):
    return 1 if f.packed else f.bytes_per_sample


def src_facts(c, layout=None):
    f = formats.fmt(c.fmt)
    bps, shapes = _bps(f), formats.plane_shapes(f, c.w, c.h)
    if (layout or c.src) == "dense":
        fb, off, data = formats.frame_bytes(f, c.w, c.h), 0, []
        for r, cols in shapes:
            data.append(BASE + off)
            off += r * cols * bps
        return data, [cols * bps for r, cols in shapes], [fb] * 3
    ls = [_pitch(cols * bps) for r, cols in shapes]
    return [BASE] * 3, ls, [r * l for (r, cols), l in zip(shapes, ls)]


def dst_facts(c, layout=None):
    f = out_fmt(c)
    bps, shapes = _bps(f), formats.plane_shapes(f, c.W, c.H)
    shapes = (list(shapes) * 3)[:3]
    ls = [_pitch(cols * bps) + GUARD for r, cols in shapes]
    off = bps if (layout or c.dst) == "offset" else 0
    return [BASE + off] * 3, ls, [(r + 1) * l for (r, cols), l in zip(shapes, ls)]


def query(c, src=None, dst=None):
    """ops.pack_arms of a case, for its recorded layout or for the given batches / facts."""
    src = src_facts(c) if src is None else src
    dst = dst_facts(c) if dst is None else dst
    if c.op == "stall":
        return ops.pack_arms("stall", c.fmt, c.w, c.h, src, dst, src_index=c.src_index, spinner_index=c.spinner_index,
                             spinner=c.spin or (0, 0, 0))
    return ops.pack_arms(c.op, c.fmt, c.w, c.h, src, dst, W=c.W, H=c.H, x=c.x, y=c.y, nframes=c.n)


def instance(c, inst):
    return "v210" if c.op == "v210" else inst


def keys(c):
    """(instance, arm) pairs of a case, computed now."""
    inst, arms = query(c)
    return {(instance(c, inst), a) for a in arms}


def spinner_rgba(c):
    """Synthetic RGBA animation of a stall case: alpha 0, 255 and values between."""
    n, sw, sh = c.spin
    rng = np.random.default_rng(sw * 131 + sh)
    a = rng.integers(0, 256, (n, sh, sw, 4), dtype=np.uint8)
    sel = rng.integers(0, 3, (n, sh, sw))
    a[..., 3] = np.where(sel == 0, 0, np.where(sel == 1, 255, a[..., 3]))
    return a
