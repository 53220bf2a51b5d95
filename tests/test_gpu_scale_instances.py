"""Every scaler kernel instance the planner can pick, against the oracle --
bit-exact.

The table (scale_instances.py) holds one small case per compiled strip_kernel /
scale_kernel instance and width class: one or two 256-column strips, tens of
rows.  Each case first asserts that the live plan reports the kernels the
table promises (pp_scale_plan_instances: the launchers' own choice), then runs
four distinct frames through the plan and through its PP_PLAN_GENERIC twin
and compares every plane with po.scale (chain plans: po.scale twice).

Also: destination rows that are not 8-B aligned through the strip kernel
(per-lane stores, guard bytes untouched), and the same content at a clamped and
a ragged width (the launcher's `clamped` rule, FUSE 9 / 11 and a plain plan).
"""
import numpy as np
import pytest

import pyoracle as po
import scale_instances as si
import synth

pytestmark = pytest.mark.gpu

FLAGS = {"bicubic": po.SWS_BICUBIC, "lanczos": po.SWS_LANCZOS, "bilinear": po.SWS_BILINEAR}
ROWS = si.load()


def _oracle(case, frame):
    chain, sf, sw, sh, df, dw, dh, fl = case
    s, d = po.FMT_BY_NAME[sf], po.FMT_BY_NAME[df]
    if not chain:
        return po.scale(s, frame, d, dw, dh, FLAGS[fl])
    mid = po.scale(s, frame, po.YUV420P, dw, dh, FLAGS[fl])
    return mid if d == po.YUV420P else po.scale(po.YUV420P, mid, d, dw, dh, po.SWS_BICUBIC)


def _frames(case, keys):
    """Legal-range noise, full-range noise, a 1-px 0/max checkerboard, and 0/max
    steps with seams at the source columns / rows of output column 256 (the
    strip seam; 512 for the chroma planes') and of the chunk boundaries of
    every launch (keys: each launch's rows per chunk)."""
    chain, sf, sw, sh, df, dw, dh, fl = case
    f = po.FMT_BY_NAME[sf]
    rng = np.random.default_rng(sw * 131 + sh * 7 + dw)
    seams_x = [x * sw // dw for x in (256, 512) if x < dw]
    chos = sorted({k[10] for k in keys if k[10]})
    seams_y = sorted({y * sh // dh for cho in chos for y in range(cho, dh, cho)})
    return [synth.noise_frame(rng, f, sw, sh),
            synth.extreme_frame("noise", f, sw, sh, seed=sw + dh),
            synth.extreme_frame("checker", f, sw, sh),
            synth.extreme_frame("steps", f, sw, sh, seams_x=seams_x, seams_y=seams_y)]


def _aligned(batch, a):
    s = batch.frames_struct()
    np_ = len(batch.planes)
    return all(s.data[p] % a == 0 and s.linesize[p] % a == 0 and (batch.n < 2 or s.frame_stride[p] % a == 0)
               for p in range(np_))


def _compare(out, refs, what):
    for f, ref in enumerate(refs):
        for p, r in enumerate(ref):
            got = out[p][f]
            if not np.array_equal(got, r):
                bad = np.argwhere(got != r)
                pytest.fail("%s frame %d plane %d: %d mismatches, first at %s got %d want %d" % (
                    what, f, p, len(bad), tuple(bad[0]), got[tuple(bad[0])], r[tuple(bad[0])]))


def _run(gpu, case, frames, generic=False, want=None):
    from pixpath.frames import FrameBatch
    chain, sf, sw, sh, df, dw, dh, fl = case
    sc = si.plan(case, generic=generic, host_only=False)
    src = FrameBatch.from_numpy(sf, synth.batch(frames), device=gpu)
    dst = FrameBatch(df, dw, dh, len(frames), device=gpu, zero=True)
    keys = sc.instance_keys_for(_aligned(src, 16), _aligned(dst, 4 if dst.bps == 1 else 8))
    if want is not None:
        assert [tuple(k) for k in keys] == [tuple(k) for k in want], "the plan no longer picks the table's kernels"
    return sc, keys, sc(src, dst).to_numpy()


@pytest.mark.parametrize("idx", range(len(ROWS)), ids=[si.case_id(r) for r in ROWS])
def test_instance_matches_oracle(gpu, idx):
    case, keys, gkeys = ROWS[idx]
    frames = _frames(case, keys)
    refs = [_oracle(case, f) for f in frames]
    for generic, want in ((False, keys), (True, gkeys)):
        sc, got, out = _run(gpu, case, frames, generic, want)
        _compare(out, refs, "generic" if generic else "auto")


def _first(pred):
    for row in ROWS:
        if pred(row):
            return row
    raise AssertionError("no such case in the table")


def _has(row, family, sbytes=None, outb=None):
    return any(k[0] == family and sbytes in (None, k[1]) and outb in (None, k[2]) for k in row[1])


UNALIGNED = [("plain", sb, ob) for sb, ob in si.ST_OUTB] + [("packed", 1, 8), ("chain", 2, 10)]


@pytest.mark.parametrize("family,sbytes,outb", UNALIGNED, ids=lambda v: str(v))
def test_unaligned_destination_through_strip_kernel(gpu, family, sbytes, outb):
    """Destination rows 2 bytes off an 8-B boundary (a pitched view into a larger
    tensor): the strip kernel still runs, with per-lane stores (vec_dst == 0),
    the bytes equal the oracle's and the bytes around every row stay untouched."""
    import torch
    from pixpath import formats
    from pixpath.frames import FrameBatch
    case, keys, _ = _first(lambda r: _has(r, family, sbytes, outb))
    chain, sf, sw, sh, df, dw, dh, fl = case
    frames = _frames(case, keys)[2:]
    n = len(frames)
    fm = formats.fmt(df)
    es = 1 if fm.packed else fm.bytes_per_sample
    dtype = torch.uint16 if es == 2 else torch.uint8
    guard = 0xA5A5 if es == 2 else 0xA5
    off = 2 // es
    big, planes = [], []
    for r, c in formats.plane_shapes(fm, dw, dh):
        pitch = (c * es + 15) // 16 * 16 // es + 16 // es
        t = torch.full((n, r + 1, pitch), guard, dtype=torch.int32, device=gpu).to(dtype)
        big.append(t)
        planes.append(t[:, :r, off:off + pitch - 16 // es])
    dst = FrameBatch(fm, dw, dh, n, device=gpu, planes=planes)
    assert not _aligned(dst, 4) and dst.frames_struct().data[0] % 8 == 2
    src = FrameBatch.from_numpy(sf, synth.batch(frames), device=gpu)
    sc = si.plan(case, host_only=False)
    got = sc.instance_keys_for(_aligned(src, 16), False)
    assert all(k.family in si.STRIP_FAMILIES and not k.clamped for k in got)
    assert any(k.family == family for k in got)
    sc(src, dst)
    torch.cuda.synchronize()
    _compare([dst.view(p).cpu().numpy() for p in range(len(planes))], [_oracle(case, f) for f in frames], "unaligned")
    for p, (r, c) in enumerate(dst.shapes):
        whole = big[p].cpu().numpy()
        mask = np.ones(whole.shape, dtype=bool)
        mask[:, :r, off:off + c] = False
        assert (whole[mask] == guard).all(), "plane %d: bytes outside the rows were written" % p


@pytest.mark.parametrize("family", ["chain-luma", "chain-chroma", "plain"])
def test_clamped_and_per_lane_widths(gpu, family):
    """The same content at a width whose every plane is a multiple of 4 and at
    that width + 2: the first runs the clamped V pass (FUSE 9 / 11 exist for it
    alone), the second the per-lane one; both bit-exact."""
    case, keys, _ = _first(lambda r: any(k[0] == family and k[8] and r[0][5] % 8 == 0 for k in r[1]))
    chain, sf, sw, sh, df, dw, dh, fl = case
    frames = _frames(case, keys)
    seen = {}
    for w in (dw, dw + 2):
        c = (chain, sf, sw, sh, df, w, dh, fl)
        sc, got, out = _run(gpu, c, frames)
        _compare(out, [_oracle(c, f) for f in frames], "dw %d" % w)
        seen[w] = got
    assert all(k.clamped for k in seen[dw] if k.family in si.STRIP_FAMILIES)
    assert any(k.family == family for k in seen[dw])
    # ragged planes: no clamped launch, and the chain's own instance in place of FUSE 9 / 11
    assert all(k.family in si.STRIP_FAMILIES and not k.clamped for k in seen[dw + 2])
    want = "plain" if family == "plain" else "chain"
    assert {k.family for k in seen[dw + 2]} == {want}
