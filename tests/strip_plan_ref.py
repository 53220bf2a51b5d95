"""Restatement, from a plan's vertical filter alone, of which output rows
strip_kernel's V pass skips a tap pair for (csrc/strip.hpp vpass, VSKIP).

The window ring keeps source rows as (even, odd) pairs, so a row's taps are
regrouped from the even row at or below its first tap (csrc/scale_plan.cpp
pair_rows): a row whose taps start on an odd source row gets a leading zero
tap.  The plan runs as many pairs as its widest row needs; a row that needs
fewer leaves its last pair zero.
"""
import numpy as np


def last_pair_zero(sc, which):
    """(vtp, bool per output row: the row's last V tap pair is zero) of the luma
    (which = 2) or chroma (3) plane of a plan (ops.Scaler)."""
    coef, pos = sc.filter(which)
    need = np.array([((int(pos[y]) & 1) + int(np.flatnonzero(coef[y])[-1]) + 2) // 2 for y in range(len(pos))])
    vtp = int(need.max())
    return vtp, need < vtp


def mixed_row_group(zero, cho):
    """Some wave's row group (rows y0 + rg + 4 i, i < 4, of one chunk of `cho`
    rows) holds both a row with a zero last pair and a full row."""
    for y0 in range(0, len(zero), cho):
        for rg in range(4):
            rows = list(range(y0 + rg, min(y0 + cho, len(zero)), 4))[:4]
            if len(rows) > 1 and zero[rows].any() and not zero[rows].all():
                return True
    return False
