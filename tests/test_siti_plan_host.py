"""The SI/TI launch planner (csrc/siti_plan.hpp) through ops.siti_plan
(pp_siti_plan) -- CPU only, no GPU and no context.

* the planner equals the Python re-statement (siti_plan_ref.py) on a grid of
  widths around the 8-px lane, the 496-px wave and the 1984-px tile, heights
  around the 16-row band, frame counts and slot counts, and holds its
  invariants there;
* the argument errors are those of pp_siti_ex;
* every case of the arms table (siti_arms.py) still plans to the arms it
  claims, and the claims of the 8-bit and of the 10-bit cases each cover
  every arm: a planner change that moves a case off its arm fails here
  instead of silently emptying tests/test_gpu_siti_arms.py.
"""
import ctypes
import itertools
import os

import pytest

from pixpath import _native, ops

import siti_arms
import siti_plan_ref as ref

WIDTHS = (3, 8, 495, 496, 497, 498, 1983, 1984, 1985, 1986, 3969)
HEIGHTS = (3, 15, 16, 17, 18, 31, 32, 33, 34, 48, 1080)
FRAMES = (1, 2, 3, 7, 8, 600)
SLOTS = (1, 2, 3, 7, 64, 512, 2048)


def test_planner_matches_the_restatement_and_holds_its_invariants():
    for depth, (w, h, n, slots) in zip(itertools.cycle((8, 10)), itertools.product(WIDTHS, HEIGHTS, FRAMES, SLOTS)):
        p = ops.siti_plan(depth, w, h, n, slots)
        at = (depth, w, h, n, slots, p)
        assert p == ref.plan(w, h, n, slots), at
        assert (p.tiles_x, p.bands, p.ntiles) == (-(-w // 1984), -(-h // 16), p.tiles_x * p.bands), at
        assert 1 <= p.fchunk <= n, at
        assert (p.chunks - 1) * p.fchunk < n <= p.chunks * p.fchunk, at
        assert p.groups == min(slots, p.ntiles * p.chunks) >= 1, at
        assert p.interior_bands == sum(1 for y0 in range(0, h, 16) if y0 >= 1 and y0 + 17 <= h), at
        assert p.ragged is (w % 8 != 0), at


def test_kernel_dispatches_on_the_planners_band_condition():
    """siti_kernel spells siti_band_interior out (siti_plan.hpp says why); the two stay one condition."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "processing-chain_amd", "csrc")
    cond = "y0 >= 1 && y0 + kBand + 1 <= H"
    assert "if (%s)" % cond in open(os.path.join(csrc, "siti.hip")).read()
    assert "return %s;" % cond in open(os.path.join(csrc, "siti_plan.hpp")).read()


def test_plan_does_not_depend_on_the_depth():
    for w, h, n, slots in ((497, 33, 7, 3), (1985, 50, 600, 512), (8, 3, 1, 1)):
        assert ops.siti_plan(8, w, h, n, slots) == ops.siti_plan(10, w, h, n, slots)


def test_no_frames_plan_nothing():
    p = ops.siti_plan(10, 1985, 34, 0, 4)
    assert (p.tiles_x, p.bands, p.ntiles, p.ragged, p.interior_bands) == (2, 3, 6, True, 1)
    assert (p.fchunk, p.chunks, p.groups) == (0, 0, 0)


@pytest.mark.parametrize("args,text", [
    ((9, 64, 64, 4, 8), "bit depth 9 (8 or 10)"), ((12, 64, 64, 4, 8), "bit depth 12 (8 or 10)"),
    ((8, 2, 64, 4, 8), "frame 2x64 too small for Sobel"), ((10, 64, 2, 4, 8), "frame 64x2 too small for Sobel"),
    ((10, 64, 64, -1, 8), "null argument"), ((10, 64, 64, 4, 0), "siti slots 0"), ((10, 64, 64, 4, -3), "siti slots -3"),
])
def test_plan_argument_errors(args, text):
    with pytest.raises(_native.PixpathError) as e:
        ops.siti_plan(*args)
    assert e.value.code == -1 and text in str(e.value), str(e.value)


def test_plan_output_array():
    L = _native.lib()
    out = (ctypes.c_int32 * 10)(*([-7] * 10))
    assert L.pp_siti_plan(10, 1985, 34, 9, 5, None, 8) == -1 and b"null argument" in L.pp_last_error()
    assert L.pp_siti_plan(10, 1985, 34, 9, 5, out, 0) == -1 and b"null argument" in L.pp_last_error()
    assert L.pp_siti_plan(10, 1985, 34, 9, 5, out, 3) == 0
    assert list(out) == [2, 3, 6] + [-7] * 7  # no more than n fields are written
    assert L.pp_siti_plan(10, 1985, 34, 9, 5, out, 10) == 0
    assert list(out) == [2, 3, 6, 1, 1, 3, 3, 5, -7, -7]  # nor more than the plan has


def test_entries_check_their_arguments_before_any_gpu_call():
    """pp_siti_slots refuses what pp_siti_ex refuses, and a negative slot
    count, with the same codes and messages, before it touches the device;
    no frames is no error."""
    L = _native.lib()
    p = ctypes.c_void_p(1 << 16)  # never dereferenced before the argument checks
    for depth, w, h, text in ((9, 64, 64, b"bit depth 9 (8 or 10)"), (8, 2, 64, b"frame 2x64 too small for Sobel")):
        assert L.pp_siti_ex(p, depth, w, h, p, 64, 4096, 1, None, p, p, 0, None) == -1 and text in L.pp_last_error()
        assert L.pp_siti_slots(p, depth, w, h, p, 64, 4096, 1, None, p, p, 0, 4, None) == -1
        assert text in L.pp_last_error()
        assert L.pp_siti_plan(depth, w, h, 1, 4, (ctypes.c_int32 * 8)(), 8) == -1 and text in L.pp_last_error()
    assert L.pp_siti_slots(p, 8, 64, 64, p, 64, 4096, 1, None, p, p, 0, -1, None) == -1
    assert b"siti slots -1" in L.pp_last_error()
    assert L.pp_siti_slots(p, 8, 64, 64, p, 64, 4096, 1, None, p, p, 2, 4, None) == -1
    assert b"siti flags 0x2" in L.pp_last_error()
    assert L.pp_siti_slots(None, 8, 64, 64, p, 64, 4096, 1, None, p, p, 0, 4, None) == -1
    assert b"null argument" in L.pp_last_error()
    assert L.pp_siti_slots(p, 8, 64, 64, p, 64, 4096, 0, None, p, p, 0, 4, None) == 0
    assert L.pp_siti_ex(p, 8, 64, 64, p, 64, 4096, 0, None, p, p, 0, None) == 0


@pytest.mark.parametrize("c", siti_arms.CASES, ids=lambda c: c.id)
def test_case_plans_to_its_claimed_arms(c):
    plan = ops.siti_plan(c.depth, c.w, c.h, c.n, c.slots)
    held = siti_arms.arms_of(c, plan)
    assert c.arms and set(c.arms) <= held, (set(c.arms) - held, plan)
    # the band kinds are a second statement of the planner's interior count
    assert ("interior" in held) == (plan.interior_bands > 0)


@pytest.mark.parametrize("depth", [8, 10])
def test_cases_cover_every_arm(depth):
    cases = [c for c in siti_arms.CASES if c.depth == depth]
    assert siti_arms.REQUIRED - siti_arms.coverage(cases) == set()
    assert len({c.id for c in siti_arms.CASES}) == len(siti_arms.CASES)
    assert {c.layout for c in cases} == set(siti_arms.LAYOUTS)
    # the widths and heights the kernel's geometry calls for, at sizes a test can afford
    assert {c.w for c in cases} == {8, 13, 496, 497, 503, 1984, 1985, 2050}
    assert {c.h for c in cases} >= {3, 16, 17, 18, 32, 33, 34, 48, 50}
    assert all(c.w <= 2050 and c.h <= 50 and c.n <= 12 for c in cases)
    # the plan-invariance runs need several tiles and chunks to differ at all
    inv = [c for c in siti_arms.INVARIANT if c.depth == depth]
    assert len(inv) >= 4 and all({"multi", "chunks"} <= set(c.arms) for c in inv)


def test_required_arms_are_computable():
    """Every required arm is one arms_of can report (a typo in REQUIRED or in a claim cannot hide)."""
    names = set()
    for c in siti_arms.CASES:
        names |= siti_arms.arms_of(c, ops.siti_plan(c.depth, c.w, c.h, c.n, c.slots))
    for c in siti_arms.CASES:
        assert set(c.arms) <= names
    assert {a.split("+")[0] for a in siti_arms.REQUIRED} <= names
