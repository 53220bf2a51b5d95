"""PP-STATS-1 on the host (test helper): the three integer arrays
pp_frame_stats returns, from numpy planes, in a few lines of numpy."""
import numpy as np

from pixpath import formats

SAD_ABSENT = np.uint64((1 << 64) - 1)


def plane(fmt, w, h, p, a):
    """The samples of plane p that count: the first rows x cols of a pitched
    2-D (or [n, rows, pitch]) array, padding dropped."""
    rows, cols = formats.plane_shapes(formats.fmt(fmt), w, h)[p]
    return np.asarray(a)[..., :rows, :cols]


def frame_arrays(fmt, w, h, planes, prev=None):
    """(hist [3, bins] int64, sad [3] uint64, over [3] int64) of one frame:
    planes / prev are the three 2-D arrays (any pitch) of the frame and of the
    frame before it (None: sad is the sentinel)."""
    bins = 1 << formats.fmt(fmt).depth
    hist, sad, over = np.zeros((3, bins), np.int64), np.full(3, SAD_ABSENT, np.uint64), np.zeros(3, np.int64)
    for p in range(3):
        a = plane(fmt, w, h, p, planes[p]).astype(np.int64).reshape(-1)
        hist[p] = np.bincount(a[a < bins], minlength=bins)
        over[p] = int((a >= bins).sum())
        if prev is not None:
            b = plane(fmt, w, h, p, prev[p]).astype(np.int64).reshape(-1)
            sad[p] = np.uint64(int(np.abs(a - b).sum()))
    return hist, sad, over


def batch_arrays(fmt, w, h, arrs, prev=None):
    """The same for a batch: arrs = three [n, rows, pitch] arrays; prev = the
    three 2-D arrays of the frame before frame 0, or None.  Returns hist
    [n, 3, bins], sad [n, 3] uint64, over [n, 3]."""
    n = arrs[0].shape[0]
    out = []
    for k in range(n):
        before = prev if k == 0 else [a[k - 1] for a in arrs]
        out.append(frame_arrays(fmt, w, h, [a[k] for a in arrs], before))
    bins = 1 << formats.fmt(fmt).depth
    if not out:
        return np.zeros((0, 3, bins), np.int64), np.zeros((0, 3), np.uint64), np.zeros((0, 3), np.int64)
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])
