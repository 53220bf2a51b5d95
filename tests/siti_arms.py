"""Case table of the SI/TI kernel (csrc/siti.hip): small clips with a forced
slot count (ops.siti(..., slots=)) that between them reach every arm of the
kernel and of its host code with more than one frame per chunk.

CASES is written by hand: each entry is one launch with the arms it was built
for (`arms`).  test_siti_plan_host.py checks on the CPU, through
ops.siti_plan (pp_siti_plan: the planner pp_siti_slots launches), that every
case still plans to the arms it claims and that the claims of the 8-bit and
of the 10-bit cases each cover REQUIRED; test_gpu_siti_arms.py runs every case
against oracle/siti_ref.py.

Arms (arms_of computes them from the plan and the layout):
  instance   ragged / even      w % 8 != 0 takes the RAGGED kernel instances
                                (u8 / u16 is the case's depth)
  bands      first              band 0 of several: full, not interior
             interior           all 18 window rows in the frame
             last_full          last band of 16 rows (no row below it)
             last_1row          last band of 1 row: no Sobel row, K stays unset
             last_2rows         last band of 2 rows: its first Sobel row is row 3
             single_short       one band of fewer than 16 rows
             single_full        one band of exactly 16 rows
  plan       multi              fchunk >= 2: the pipelined frame loop runs on
             whole              one chunk walks all frames (fchunk == n >= 2)
             chunks             chunks >= 2
             even_split         multi, chunks, every chunk of fchunk frames
             tail_short         multi, chunks, a last chunk shorter than fchunk
             tail_1             ... of exactly 1 frame
             stride             units > groups: a workgroup takes a second unit
             one_group          one workgroup walks every unit in turn
             tiles2             a second tile column
             single_frame       n == 1
  layout     contig             [n, h, w] dense (repacked when w * es is off the load granule)
             pitched            rows padded to a multiple of 64 samples
             offset1            the view [:, :, 1:w+1] of a pitched buffer: repacked
             stride2            every second frame of a pitched buffer
             stride2_offset1    both: repacked frame by frame
             repack             the layout is not on the kernel's load granule
  prev       prev               the frame before frame 0 is given
             prev_later_chunk   ... and chunks >= 2: the halo of chunk 0 is prev, of later chunks a frame
             prev_repack        ... and the layout is repacked (the extra scratch frame)
"X+multi" is arm X held by a case that also holds multi.
"""
import collections

import numpy as np

import siti_plan_ref

Case = collections.namedtuple("Case", "id depth w h n slots layout prev arms")
LAYOUTS = ("contig", "pitched", "offset1", "stride2", "stride2_offset1")

# (w, h, n, slots, layout, prev, arms): every width and height the kernel's
# geometry calls for (w: no straddling lane, a straddling lane in the first and
# in a later wave, the second tile column, w % 8 of 1, 5, 7 and 2; h: one short
# band, one full band, last bands of 1, 2 and 16 rows, interior bands)
_SHAPES = (
    (8, 3, 5, 1, "contig", False, "even single_short multi whole contig"),
    (13, 16, 7, 2, "contig", True, "ragged single_full multi chunks tail_short contig repack prev prev_later_chunk "
                                   "prev_repack"),
    (496, 17, 8, 4, "pitched", False, "even first last_1row multi chunks even_split pitched"),
    (497, 18, 7, 6, "offset1", False, "ragged first last_2rows multi chunks tail_short tail_1 offset1 repack"),
    (503, 32, 9, 3, "offset1", True, "ragged first last_full multi chunks even_split stride offset1 repack prev "
                                     "prev_later_chunk prev_repack"),
    (1984, 33, 8, 6, "stride2", False, "even first interior last_1row multi chunks even_split stride2"),
    (1985, 34, 9, 5, "stride2_offset1", False, "ragged tiles2 first interior last_2rows multi chunks even_split stride "
                                               "stride2_offset1 repack"),
    (2050, 48, 12, 8, "pitched", True, "ragged tiles2 first interior last_full multi chunks even_split stride pitched "
                                       "prev prev_later_chunk"),
    (2050, 50, 7, 6, "contig", False, "ragged tiles2 first interior last_2rows multi chunks tail_short contig repack"),
    (497, 33, 5, 1, "pitched", False, "ragged first interior last_1row multi whole stride one_group pitched"),
    (1984, 16, 3, 1, "contig", False, "even single_full multi whole contig"),
    (13, 17, 1, 2, "pitched", False, "ragged first last_1row single_frame pitched"),
    (13, 17, 1, 2, "offset1", True, "ragged first last_1row single_frame offset1 repack prev prev_repack"),
)

CASES = tuple(
    Case("u%d-%dx%dx%d-s%d-%s%s" % (8 if depth == 8 else 16, w, h, n, slots, layout, "-prev" if prev else ""), depth, w, h,
         n, slots, layout, prev, tuple(arms.split()))
    for depth in (8, 10) for w, h, n, slots, layout, prev, arms in _SHAPES)

# cases run at several slot counts for bit-equal results
INVARIANT = tuple(c for c in CASES if (c.w, c.h) in ((497, 18), (503, 32), (1984, 33), (1985, 34), (2050, 48)))

_SITES = ("ragged", "even", "first", "interior", "last_full", "last_1row", "last_2rows", "single_short", "single_full",
          "tiles2", "chunks", "tail_short", "tail_1", "stride", "one_group", "prev", "prev_later_chunk", "prev_repack",
          "repack") + LAYOUTS
REQUIRED = frozenset(_SITES) | frozenset(s + "+multi" for s in _SITES) | {"multi", "whole", "even_split", "single_frame"}


def geometry(c):
    """(pitch, frame step, column offset, frames allocated) in samples / frames of the buffer the case's luma views."""
    if c.layout == "contig":
        return c.w, 1, 0, c.n
    pitch = (c.w + 2 + 63) // 64 * 64
    step = 2 if c.layout.startswith("stride2") else 1
    return pitch, step, 1 if c.layout.endswith("offset1") else 0, c.n * step


def repacked(c):
    """The layout is off the kernel's load granule (8 samples), given a buffer that starts on it."""
    pitch, step, off, _ = geometry(c)
    return bool(off % 8 or pitch % 8 or (c.n >= 2 and step * c.h * pitch % 8))


def band_kinds(h):
    rows = siti_plan_ref.band_rows(h)
    if len(rows) == 1:
        return {"single_full" if rows[0][1] == 16 else "single_short"}
    kinds = {"first"}
    kinds |= {"interior" for y0, _ in rows[1:] if siti_plan_ref.interior(y0, h)}
    kinds.add({1: "last_1row", 2: "last_2rows", 16: "last_full"}.get(rows[-1][1], "last_short"))
    return kinds


def arms_of(c, plan):
    """The arms case `c` holds under `plan` (ops.siti_plan(c.depth, c.w, c.h, c.n, c.slots))."""
    a = {"ragged" if plan.ragged else "even", c.layout} | band_kinds(c.h)
    multi, chunks, tail = plan.fchunk >= 2, plan.chunks >= 2, c.n % plan.fchunk
    units = plan.ntiles * plan.chunks
    a |= {name for name, held in (
        ("multi", multi), ("whole", multi and plan.chunks == 1), ("chunks", chunks),
        ("even_split", multi and chunks and tail == 0), ("tail_short", multi and chunks and tail > 0),
        ("tail_1", multi and chunks and tail == 1), ("stride", units > plan.groups),
        ("one_group", plan.groups == 1 and units > 1), ("tiles2", plan.tiles_x == 2), ("single_frame", c.n == 1),
        ("repack", repacked(c)), ("prev", c.prev), ("prev_later_chunk", c.prev and chunks),
        ("prev_repack", c.prev and repacked(c))) if held}
    return a


def coverage(cases):
    """The arms the cases claim, with X+multi for every arm of a multi-frame case."""
    held = set()
    for c in cases:
        held |= set(c.arms)
        if "multi" in c.arms:
            held |= {a + "+multi" for a in c.arms if a != "multi"}
    return held


def frames_of(c, seed=0):
    """Seeded uniform noise over the full code range: (frames [n, h, w], prev [h, w] or None)."""
    rng = np.random.default_rng([910, c.depth, c.w, c.h, c.n, seed])
    dt = np.uint16 if c.depth > 8 else np.uint8
    f = rng.integers(0, 1 << c.depth, (c.n + 1, c.h, c.w)).astype(dt)
    return f[1:], (f[0] if c.prev else None)


def place(c, frames, prev):
    """The host buffers of the case's layout, filled with 7 outside the frames:
    (buffer, prev buffer or None, view) with view(buffer) -> the [n, h, w] luma
    and view(prev buffer) -> [1, h, w]; the views keep the buffers' pitch."""
    pitch, step, off, nalloc = geometry(c)
    big = np.full((nalloc, c.h, pitch), 7, frames.dtype)
    big[::step, :, off:off + c.w] = frames
    pbig = None
    if prev is not None:
        pbig = np.full((1, c.h, pitch), 7, frames.dtype)
        pbig[0, :, off:off + c.w] = prev

    def view(t):
        return t[::step, :, off:off + c.w]
    return big, pbig, view
