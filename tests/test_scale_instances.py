"""The scaler's kernel-instance table (scale_instances.py) is complete and
current -- CPU only, host-only plans.

* every table case still plans to the kernels recorded for it (planner drift
  fails here instead of silently shrinking what the GPU test runs);
* the recorded keys cover the whole instantiated grid: every plain / packed /
  chain (ST, OUTB, HW, VTM), FUSE 9 and 11 at every narrow window, every H-tap
  bucket of the general kernel at both tile widths -- less an explicit
  UNREACHED list of at most 5 % of the grid;
* the grid's value lists are the dispatch macros' and the planner's buckets;
* both width classes (every plane width a multiple of 4 / ragged) are present
  for every strip instance that compiles the clamped V-pass copy;
* every required slot (scale_instances.slots) is held, and every case holds a
  required slot that no other case holds: deleting a case fails here.
"""
import os
import re

from pixpath import ops

import scale_instances as si

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "processing-chain_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _macro(text, name):
    """Body of a multi-line #define (continuation lines)."""
    m = re.search(r"#define %s\b.*?(?:\\\n.*?)*\n" % re.escape(name), text)
    return m.group(0)


def test_value_lists_are_the_dispatch_macros():
    strip = _src("strip.hpp")
    assert tuple(int(v) for v in re.findall(r"case (\d+): PP_STRIP_VTM", _macro(strip, "PP_STRIP_HW_FT"))) == si.STRIP_HW
    vtm = _macro(strip, "PP_STRIP_VTM")
    assert tuple(int(v) for v in re.findall(r"strip_kernel<ST, OUTB, HW, (\d+), FUSE, TW>", vtm)) == si.STRIP_VTM
    for f in ("strip_u8_fused.hip", "strip_u16_fused.hip"):
        narrow = _macro(_src(f), "PP_STRIP_HW_NARROW_F")
        assert tuple(int(v) for v in re.findall(r"case (\d+): PP_STRIP_VTM", narrow)) == si.STRIP_HW_NARROW
    scale = _src("scale.hip")
    body = scale[scale.index("KernelFn pick_ht_tw(int ht)"):scale.index("KernelFn pick_ht(int ht, bool tw256)")]
    assert tuple(int(v) for v in re.findall(r"case (\d+): return scale_kernel", body)) == si.GENERAL_HT


def test_table_is_current_and_value_lists_are_the_planner_buckets():
    """Every case, planned now, reports the recorded keys; and the windows /
    tap buckets the planner hands out over the table are exactly the lists."""
    rows = si.load()
    assert len({r[0] for r in rows}) == len(rows)
    hw, vtm, ht = set(), set(), set()
    for case, keys, gkeys in rows:
        for generic, want in ((False, keys), (True, gkeys)):
            sc = si.plan(case, generic=generic)
            got = sc.instance_keys
            assert [tuple(k) for k in got] == [tuple(k) for k in want], (case, generic)
            for k in got:
                if k.family in si.STRIP_FAMILIES:
                    hw.add(k.win)
                    vtm.add(k.vtm)
                    assert sc.kernel_path > 0
                elif k.family == "general":
                    ht.add(k.win)
            if generic:
                assert sc.kernel_path == 0
    assert (sorted(hw), sorted(vtm), sorted(ht)) == (sorted(si.STRIP_HW), sorted(si.STRIP_VTM), sorted(si.GENERAL_HT))


def test_table_covers_the_instantiated_grid():
    reached = si.reached()
    have = {i._replace(vtp2=0) for i, cl in reached}
    grid = si.grid()
    assert len(grid) == len(set(grid)) == 2 * 128 + 2 * 64 + 72
    unreached = [u[0] for u in si.UNREACHED]
    assert all(u in grid for u in unreached)
    assert len(si.UNREACHED) + len(si.UNREACHED_VTP2) <= len(grid) // 20
    for u in si.UNREACHED + si.UNREACHED_VTP2:
        assert u[1] and u[2]          # the bounds that failed and the reason
    missing = [i for i in grid if i not in have and i not in unreached]
    assert not missing, missing
    listed_but_reached = [u for u in unreached if u in have]
    assert not listed_but_reached, listed_but_reached
    # 8-bit HW 8 plain is the DIRECT instance, and only it
    assert all(i.direct == int(i.sbytes == 1 and i.win == 8) for i in have if i.family == "plain")
    assert not any(i.direct for i in have if i.family != "plain")
    # the second stage's pass2 arms (strip.hpp: VT2 1, 2, 3)
    arms = {i.vtp2 for i, cl in reached if i.vtp2}
    assert arms | {u[0] for u in si.UNREACHED_VTP2} == {1, 2, 3}
    assert not arms & {u[0] for u in si.UNREACHED_VTP2}


def test_both_width_classes_for_clamp_path_instances():
    by_inst = {}
    clamp_path = set()
    for case, keys, gkeys in si.load():
        for k in keys + gkeys:
            k = ops.InstanceKey(*k)
            if k.family not in si.STRIP_FAMILIES:
                continue
            by_inst.setdefault(si.instance(k)._replace(vtp2=0), set()).add(k.clamped)
            if k.clamp_path:
                clamp_path.add(si.instance(k)._replace(vtp2=0))
            else:
                assert not k.clamped
    assert clamp_path
    for i in sorted(clamp_path):
        # FUSE 9 / 11 compile the clamped copy alone: the launcher never picks them for a ragged plan
        want = {1} if i.family in ("chain-luma", "chain-chroma") else {0, 1}
        assert by_inst[i] == want, (i, by_inst[i])


def test_every_required_slot_is_held_and_every_case_is_needed():
    """The table lists the slots it must hold: every instance in its width
    classes and every second-stage arm of every chain instance, by a launch
    whose planes all walk two or more chunks wherever the search found one.
    Each case holds one of them alone, so no case can go unnoticed."""
    import collections
    rows, need = si.load(), si.required()
    needs = set(need)
    assert len(needs) == len(need)
    cover = collections.Counter(s for row in rows for s in si.row_slots(row) if s in needs)
    missing = [s for s in need if not cover[s]]
    assert not missing, missing[:5]
    spare = [row[0] for row in rows if not any(cover[s] == 1 for s in si.row_slots(row))]
    assert not spare, spare[:5]
    # the required slots are what the coverage tests above count, not a subset of it
    assert {(i, c) for i, c, m in need if c is not None} == {(i._replace(vtp2=0), c) for i, c in si.reached()}
    arms = {i for i, c, m in need if c is None}
    assert arms == {i for i, c in si.reached() if i.vtp2}
    # one-chunk slots only where no multi-chunk case of the instance exists
    assert not [s for s in need if not s[2] and (s[0], s[1], True) in needs]
