#!/usr/bin/env python3
"""Regenerate tests/scale_instances_table.py: the smallest shape found for every
scaler kernel instance the planner can pick.

Searches small shapes with host-only plans (no GPU), asks each plan which
compiled kernels it launches (pp_scale_plan_instances, the launchers' own
choice) and keeps the smallest case per slot (scale_instances.slots: an
instance in each width class, and each second-stage arm of a chain instance,
multi-chunk and one-chunk launches apart), by source pixels, then destination
pixels.  Where a multi-chunk case of a slot exists the one-chunk slot is not
required (a one-chunk case never carries window rows from chunk to chunk).
The table lists the required slots (REQUIRED) and keeps only cases that hold
a required slot no other case holds, so tests/test_scale_instances.py fails
when a case is deleted.

    python tools/gen_scale_instances.py            # rewrite the table
    python tools/gen_scale_instances.py --check    # exit 1 if it would change

Search space (SEARCH below; recorded in the table for the UNREACHED reasons):
destination widths one to two 256-column strips in both width classes (every
plane width a multiple of 4 / ragged), heights 4..96, source : destination
ratios 1:4 .. 5:1 horizontally and vertically, every planar source format,
every destination format of each constructor, the three filters; no source
plane beyond 1300 x 200 samples.  A few narrow widths add the general
kernel's narrow-strip variants.
"""
import argparse
import collections
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "processing-chain_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from pixpath import _native, ops  # noqa: E402

import scale_instances as si  # noqa: E402

SEARCH = {
    "dst_w": [260, 261, 262, 264, 520],
    "dst_w_narrow": [100],                # general kernel, strips narrower than 256
    "dst_h": [4, 6, 8, 24, 40, 72, 96],   # (4, 6: the only heights whose second stage has one tap pair)
    # source : destination, each axis on its own
    "ratio": [(1, 4), (1, 2), (2, 3), (1, 1), (5, 4), (3, 2), (2, 1), (5, 2), (3, 1), (4, 1), (5, 1)],
    "src_fmt": ["yuv420p", "yuv422p", "yuv444p", "yuv420p10le", "yuv422p10le", "yuv444p10le"],
    "dst_fmt_plain": ["yuv420p", "yuv422p", "yuv444p", "yuv420p10le", "yuv422p10le", "yuv444p10le", "uyvy422"],
    "dst_fmt_chain": ["yuv422p", "yuv420p10le", "yuv422p10le"],   # (yuv420p: the plain plan itself)
    "flags": ["bicubic", "lanczos", "bilinear"],
    "max_src": (1300, 200),
}


def shapes():
    for dw, dh, (hn, hd), (vn, vd) in itertools.product(SEARCH["dst_w"] + SEARCH["dst_w_narrow"], SEARCH["dst_h"],
                                                        SEARCH["ratio"], SEARCH["ratio"]):
        sw, sh = (dw * hn + hd // 2) // hd, (dh * vn + vd // 2) // vd
        if 8 <= sw <= SEARCH["max_src"][0] and 8 <= sh <= SEARCH["max_src"][1]:
            yield sw, sh, dw, dh


def rank(case):
    chain, sf, sw, sh, df, dw, dh, fl = case
    return (sw * sh, dw * dh, case)


def search_shape(arg):
    """Best (rank, case) per slot over every format pair and
    filter at one shape, plans and their PP_PLAN_GENERIC twins; rejections."""
    chain, (sw, sh, dw, dh) = arg
    best, rejects = {}, {}
    for sf, df, fl in itertools.product(SEARCH["src_fmt"], SEARCH["dst_fmt_chain" if chain else "dst_fmt_plain"],
                                        SEARCH["flags"]):
        if df == "uyvy422" and dw % 2:
            continue  # a packed 4:2:2 row holds whole pixel pairs
        case = (chain, sf, sw, sh, df, dw, dh, fl)
        for generic in (False, True):
            try:
                sc = si.plan(case, generic=generic)
            except _native.PixpathError as e:
                msg = str(e).split(": ", 1)[-1].split(" of ")[0]
                rejects[msg] = rejects.get(msg, 0) + 1
                break
            keys = sc.instance_keys
            r = rank(case)
            for k in keys:
                for slot in si.slots(k):
                    if slot not in best or r < best[slot][0]:
                        best[slot] = (r, case)
    return best, rejects


def search(jobs=1):
    """{slot: (rank, case)} and {rejection message: count}."""
    args = [(chain, s) for chain in (False, True) for s in shapes() if not (chain and s[2] < 256)]
    if jobs > 1:
        import multiprocessing
        with multiprocessing.Pool(jobs) as pool:
            parts = pool.map(search_shape, args, chunksize=16)
    else:
        parts = map(search_shape, args)
    best, rejects = {}, {}
    for b, rj in parts:
        for slot, v in b.items():
            if slot not in best or v[0] < best[slot][0]:
                best[slot] = v
        for m, c in rj.items():
            rejects[m] = rejects.get(m, 0) + c
    return best, rejects


def render(best, rejects):
    need = sorted((s for s in best if s[2] or (s[0], s[1], True) not in best),
                  key=lambda s: (tuple(s[0]), s[1] is None, s[1] or 0, s[2]))
    rows = []
    for case in sorted({best[s][1] for s in need}):
        rows.append((case, tuple(tuple(k) for k in si.plan(case).instance_keys),
                     tuple(tuple(k) for k in si.plan(case, generic=True).instance_keys)))
    # keep only cases that hold a required slot no other kept case holds
    # (largest sources go first)
    needs = set(need)
    cover = collections.Counter(s for row in rows for s in si.row_slots(row) & needs)
    for row in sorted(rows, key=lambda r: (-r[0][2] * r[0][3], r[0])):
        mine = si.row_slots(row) & needs
        if all(cover[s] > 1 for s in mine):
            rows.remove(row)
            cover.subtract(mine)
    out = ['"""Generated by tools/gen_scale_instances.py -- do not edit by hand.',
           "",
           "CASES: (chain, src fmt, sw, sh, dst fmt, dw, dh, filter), then the InstanceKey tuples",
           "pp_scale_plan_instances reports (aligned batches) for the plan and for its",
           "PP_PLAN_GENERIC twin.",
           "REQUIRED: the slots (scale_instances.slots) the cases must hold: (instance, width class or",
           "None for a second-stage arm, every plane walks two or more chunks).",
           "SEARCH: the generator's search space.  REJECTED: plan-construction errors met in it.",
           '"""',
           "SEARCH = {"]
    for k, v in SEARCH.items():
        out.append("    %r: %r," % (k, v))
    out.append("}")
    out.append("REJECTED = {")
    for k in sorted(rejects):
        out.append("    %r: %d," % (k, rejects[k]))
    out.append("}")
    out.append("REQUIRED = [")
    for i, c, m in need:
        out.append("    (%r, %r, %r)," % (tuple(i), c, m))
    out.append("]")
    out.append("CASES = [")
    for row in rows:
        out.append("    (%r, %r, %r)," % row)
    out.append("]")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("-j", "--jobs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    best, rejects = search(a.jobs)
    text = render(best, rejects)
    path = os.path.join(ROOT, "tests", "scale_instances_table.py")
    if a.check:
        same = os.path.exists(path) and open(path).read() == text
        print("table is %s" % ("current" if same else "STALE"))
        return 0 if same else 1
    open(path, "w").write(text)
    print("%d required slots -> %s" % (text.count("\n    (('"), path))
    return 0


if __name__ == "__main__":
    sys.exit(main())
