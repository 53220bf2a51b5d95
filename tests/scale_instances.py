"""The scaler's kernel-instance matrix: one small case per compiled kernel the
planner can pick (tests/scale_instances_table.py, written by
tools/gen_scale_instances.py), the instantiated grid it must cover, and the
instances no plan reaches.

Used by test_scale_instances.py (CPU: the table is complete and current) and
test_gpu_scale_instances.py (GPU: every entry against the oracle).
"""
import collections

from pixpath import ops

STRIP_FAMILIES = ("plain", "packed", "chain", "chain-luma", "chain-chroma")

# ---- the instantiated grid: the dispatch macros' value lists, stated once ----
STRIP_HW = (3, 4, 5, 6, 8, 10, 12, 16)   # PP_STRIP_HW_FT (strip.hpp) = hw_bucket (scale_plan.cpp)
STRIP_HW_NARROW = (3, 4, 5, 6)           # PP_STRIP_HW_NARROW_F (strip_*_fused.hip): FUSE 9 / 11
STRIP_VTM = (2, 3, 5, 8)                 # PP_STRIP_VTM (strip.hpp) = strip_vtm_bucket
GENERAL_HT = (1, 2, 4, 6, 8, 12, 16, 24, 32)   # pick_ht_tw (scale.hip) = ht_bucket
ST_OUTB = ((1, 8), (1, 10), (2, 8), (2, 10))   # source sample bytes, output bits

# (family, sbytes, outb, win, vtm, direct, tw256): an instance without the
# fuse-2 second-stage arm (vtp2) and the width class
Instance = collections.namedtuple("Instance", "family sbytes outb win vtm direct tw256 vtp2")


def instance(key):
    """The compiled kernel (and pass2 arm) of an ops.InstanceKey."""
    return Instance(*tuple(key)[:8])


def slots(key):
    """What a table case is kept for: the instance in its width class, and the
    pass2 arm (second-stage tap pairs) of a chain instance -- each apart for
    launches whose every plane walks at least two chunks (window rows carried
    from chunk to chunk) and for one-chunk launches."""
    i = instance(key)
    multi = key.chunks >= 2
    out = [(i._replace(vtp2=0), key.clamped if key.clamp_path else 0, multi)]
    if i.vtp2:
        out.append((i, None, multi))
    return out


def row_slots(row):
    return {s for k in tuple(row[1]) + tuple(row[2]) for s in slots(ops.InstanceKey(*k))}


def required():
    """The slots the table must hold (scale_instances_table.REQUIRED): every
    slot the search reached, less the one-chunk slot where a multi-chunk case
    of the same instance exists."""
    import scale_instances_table as t
    return [(Instance(*i), c, m) for i, c, m in t.REQUIRED]


def grid():
    """Every instance the dispatch macros instantiate, as Instance tuples with
    vtp2 = 0 (the pass2 arms of a chain instance are counted apart)."""
    g = []
    for sb, ob in ST_OUTB:
        for hw in STRIP_HW:
            for vtm in STRIP_VTM:
                g.append(Instance("plain", sb, ob, hw, vtm, int(sb == 1 and hw == 8), 1, 0))
                g.append(Instance("chain", sb, ob, hw, vtm, 0, 1, 0))
        for ht in GENERAL_HT:
            for tw256 in (0, 1):
                g.append(Instance("general", sb, ob, ht, 0, 0, tw256, 0))
    for sb in (1, 2):
        for hw in STRIP_HW:
            for vtm in STRIP_VTM:
                g.append(Instance("packed", sb, 8, hw, vtm, 0, 1, 0))
        for hw in STRIP_HW_NARROW:
            for vtm in STRIP_VTM:
                g.append(Instance("chain-luma", sb, 10, hw, vtm, 0, 1, 0))
                g.append(Instance("chain-chroma", sb, 10, hw, vtm, 0, 1, 0))
    return g


def plan(case, generic=False, host_only=True):
    """ops.Scaler of a table case."""
    chain, sf, sw, sh, df, dw, dh, fl = case
    return ops.Scaler(sf, sw, sh, df, dw, dh, flags=fl, chain=chain, generic=generic, host_only=host_only)


def key_id(key):
    k = ops.InstanceKey(*key)
    s = "%s-u%d-o%d-w%d" % (k.family, 8 * k.sbytes, k.outb, k.win)
    if k.family in STRIP_FAMILIES:
        s += "-v%d" % k.vtm
    if k.direct:
        s += "-direct"
    if k.family == "general":
        s += "-tw256" if k.tw256 else "-twn"
    if k.vtp2:
        s += "-p%d" % k.vtp2
    if k.clamped:
        s += "-cl"
    return s


def case_id(row):
    case, keys, gkeys = row
    chain, sf, sw, sh, df, dw, dh, fl = case
    return "%s_%s%dx%d_%s%dx%d_%s" % ("+".join(key_id(k) for k in keys if k[0] != "two-launch") or "two-launch",
                                      sf, sw, sh, df, dw, dh, fl)


def load():
    """The committed table: rows (case, keys, generic keys)."""
    import scale_instances_table as t
    return t.CASES


def reached(rows=None):
    """{(Instance, width class)} over the keys the table records."""
    out = set()
    for case, keys, gkeys in (load() if rows is None else rows):
        for k in tuple(keys) + tuple(gkeys):
            k = ops.InstanceKey(*k)
            out.add((instance(k), k.clamped if k.clamp_path else 0))
    return out


# ---- instances no plan reaches -------------------------------------------------
# (Instance with vtp2 = 0, the search bounds that failed, why -- read from the planner).
# The table's SEARCH space (scale_instances_table.SEARCH) reaches the whole grid.
UNREACHED = []

# (pass2 arm, bounds, why): strip.hpp's VT2 1, 2, 3 arms that no chain plan reaches.
# None either: 3 is the usual count, 2 and 1 come with destinations of 5..10 and
# 4 or 6 rows (plan_stage2: a row pair's taps then span 4 or 2 first-stage rows).
UNREACHED_VTP2 = []
