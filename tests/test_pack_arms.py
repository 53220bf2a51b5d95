"""The arm table of the pad / stall / CPVS kernels (pack_arms.py) is complete
and current -- CPU only, through ops.pack_arms (pp_pack_arms: the kernels' own
predicates of csrc/pack_plan.hpp walked on the host).

* every case still holds the arms recorded for it and the arms it was written
  for (a predicate or geometry change that moves a case off its arm fails
  here instead of silently shrinking what the GPU test runs);
* per kernel instance the cases hold exactly the arms the instance compiles,
  and over all instances the whole enum less UNREACHED, each with its reason;
* every case holds an arm of its instance that no other case holds: deleting
  a case fails here;
* the rejected cases return their codes and messages, odd-width v210 among them;
* the table has the shapes the kernels' thresholds call for.
"""
import collections
import os
import re

import pytest

from pixpath import _native, formats, ops

import pack_arms as pa
import pack_arms_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE = [c for c in pa.CASES if not c.error]


def test_arm_names_are_the_header_enum():
    hdr = open(os.path.join(ROOT, "include", "pixpath.h")).read()
    body = hdr[hdr.index("enum pp_pack_arm {"):hdr.index("PP_ARM_COUNT")]
    names = re.findall(r"^\s*PP_ARM_(\w+)", body, re.M)
    assert tuple(n.lower() for n in names) == ops.PACK_ARMS
    assert len(ops.PACK_ARMS) <= 64
    for kind, names in (("OP", ops.PACK_OPS), ("INST", ops.PACK_INSTANCES)):
        vals = dict(re.findall(r"#define PP_PACK_%s_(\w+) (\d+)" % kind, hdr))
        assert [int(vals[n.upper()]) for n in names] == list(range(len(names)))


def test_kernels_use_the_shared_predicates():
    """cpvs.hip and pack.hip call pack_plan.hpp's functions; the conditions are not spelled in the kernels."""
    csrc = os.path.join(ROOT, "processing-chain_amd", "csrc")
    cpvs, pack = (open(os.path.join(csrc, f)).read() for f in ("cpvs.hip", "pack.hip"))
    for fn in ("row_live", "cpvs_stage_luma", "cpvs_tap_in", "cpvs_group_vec", "cpvs_group_sample", "cpvs_fast8_chunk",
               "uyvy_chunk_full", "v210_chunk", "cpvs_geometry"):
        assert fn + "(" in cpvs, fn
    for fn in ("chunk_src_vec", "chunk_dst_vec", "chunk_sample_stored", "row_live", "row_chunks", "stall_chunk_blends",
               "stall_sample_blends", "pad_geometry", "stall_geometry"):
        assert fn + "(" in pack, fn


def test_table_is_current():
    assert len({c.id for c in pa.CASES}) == len(pa.CASES)
    assert set(pack_arms_table.HELD) == {c.id for c in LIVE}
    for c in LIVE:
        inst, arms = pa.query(c)
        rec_inst, rec = pack_arms_table.HELD[c.id]
        assert (pa.instance(c, inst), sorted(arms)) == (rec_inst, sorted(rec)), c.id
        assert set(c.arms) <= arms, (c.id, set(c.arms) - arms)
        assert c.arms, c.id


def test_every_arm_is_held_and_every_case_is_needed():
    held = collections.defaultdict(set)
    count = collections.Counter()
    for c in LIVE:
        for k in pa.keys(c):
            held[k[0]].add(k[1])
            count[k] += 1
    assert dict(held) == pa.REQUIRED
    union = set().union(*held.values())
    assert union | set(pa.UNREACHED) == set(ops.PACK_ARMS)
    assert not union & set(pa.UNREACHED)
    assert all(len(reason) > 40 for reason in pa.UNREACHED.values())
    spare = [c.id for c in LIVE if not any(count[k] == 1 for k in pa.keys(c))]
    assert not spare, spare


def test_unreached_group_arm_argument():
    """cs / 8 >= ceil(cw / 8) for every width: the LDS chroma stride, in 8-sample
    groups, never falls short of the groups the filter walks (UNREACHED's reason),
    checked through the walker on aligned 4:2:0 sources of every small width."""
    for fmt, es in (("yuv420p", 1), ("yuv420p10le", 2)):
        for w in list(range(2, 200)) + [1023, 1025, 4097]:
            cw = (w + 1) // 2
            cs = (cw * es + 15) // 16 * 16 // es
            assert cs // 8 >= (cw + 7) // 8
            c = pa.case("w%d" % w, "cpvs", fmt, w, 2, w + (w & 1), 2, 0, 0)
            assert "cpvs_group_vec_ragged" not in pa.query(c)[1]


@pytest.mark.parametrize("c", [c for c in pa.CASES if c.error], ids=lambda c: c.id)
def test_rejected_cases_return_their_codes(c):
    code, text = c.error
    with pytest.raises(_native.PixpathError) as e:
        pa.query(c)
    assert e.value.code == code and text in str(e.value), str(e.value)


def test_odd_width_v210_is_rejected_by_the_execute_calls():
    """pp_cpvs_execute and pp_v210_pack check their arguments before any HIP
    call: an odd v210 width is PP_ERR_INVALID with the width in the message
    (FFmpeg: "v210 needs even width"); the even neighbours pass the same check
    and fail later only for want of a GPU context."""
    import ctypes
    L = _native.lib()
    ctx = ctypes.c_void_p(1)  # never dereferenced before the argument checks
    s, d = _native.pp_frames(), _native.pp_frames()
    for p in range(3):
        s.data[p], s.linesize[p], s.frame_stride[p] = pa.BASE, 64, 256
        d.data[p], d.linesize[p], d.frame_stride[p] = pa.BASE, 256, 1024
    for w in (21, 23, 25):
        assert L.pp_v210_pack(ctx, w, 4, ctypes.byref(s), ctypes.byref(d), 1, None) == -1
        assert ("even width, not %d" % w).encode() in L.pp_last_error()
    assert L.pp_cpvs_execute(ctx, formats.YUV420P10LE, 20, 4, ctypes.byref(s), 27, 8, -1, -1, formats.V210,
                             ctypes.byref(d), 1, None) == -1
    assert b"even width, not 27" in L.pp_last_error()
    # nframes = 0 passes every check and launches nothing
    assert L.pp_v210_pack(ctx, 22, 4, ctypes.byref(s), ctypes.byref(d), 0, None) == 0


def test_stall_vector_loads_follow_the_source_extent():
    """One output frame taken from source frame 1 of a batch whose rows are
    aligned but whose frame stride is not: the loads go by samples; from frame
    0, whose rows are aligned, by vectors."""
    f = formats.fmt("yuv422p10le")
    shapes = formats.plane_shapes(f, 24, 4)
    ls = [(c * 2 + 15) // 16 * 16 for r, c in shapes]
    src = ([pa.BASE] * 3, ls, [r * l + 8 for (r, c), l in zip(shapes, ls)])
    c = pa.case("skew", "stall", "yuv422p10le", 24, 4, n=2, src_index=[1], spinner_index=[-1])
    assert "row_src_scalar" in pa.query(c, src=src)[1] and "row_src_vec" not in pa.query(c, src=src)[1]
    c0 = c._replace(src_index=[0])
    assert "row_src_vec" in pa.query(c0, src=src)[1]


def test_table_has_the_threshold_shapes():
    by = {c.id: c for c in pa.CASES}
    # second staging pass: > 512 16-B pieces a row
    for fmt, pieces in (("yuv420p", lambda w: w // 16), ("yuv422p", lambda w: w // 8), ("yuv420p10le", lambda w: w // 8),
                        ("yuv422p10le", lambda w: w // 4)):
        w = by[fmt + "-cpvs-wide"].w
        assert 512 < pieces(w) <= 1024 or fmt == "yuv422p10le"
    assert by["yuv422p10le-cpvs-wide"].w == 16384 and by["yuv422p10le-cpvs-lds-reject"].w == 16392
    # heights 2 to 8 rows except where row position matters; wide cases 2 to 4 rows; frames 1 to 3, 13, 260
    for c in LIVE:
        assert c.H <= 12 and (c.W < 64 or c.H <= 4), c.id
        nout = len(c.src_index) if c.op == "stall" else c.n
        assert nout <= 3 or nout in (13, 260), c.id
    odd = by["yuv420p-cpvs-flush00-odd"]
    assert odd.w & 1 and odd.h & 1 and odd.H & 1 and (odd.x, odd.y) == (0, 0)
    br = by["yuv420p-cpvs-flushBR"]
    assert (br.x, br.y) == (br.W - br.w, br.H - br.h)
    assert {c.spin[1:] for c in LIVE if c.spin} >= {(2, 2), (20, 12), (32, 4), (24, 8)}
