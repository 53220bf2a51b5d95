"""numpy restatement of spec PP-MOTION-1, written from the
spec text: np.pad(mode="reflect"), int64 arithmetic, the vertical pass and its
rounding, the horizontal pass and its rounding, sums in Python ints.  It shares
no code with csrc/motion.hip or pixpath/motion.py."""
import numpy as np

TAPS = (3571, 16004, 26386, 16004, 3571)
ABSENT = (1 << 64) - 1


def blur(plane, bitdepth, bounds=None):
    """B of one [h, w] plane (w, h >= 3), int64.  ``bounds``: a dict that
    receives the largest vertical accumulator, t, horizontal accumulator and B."""
    d = int(bitdepth)
    x = np.minimum(np.asarray(plane).astype(np.int64), (1 << d) - 1)
    h, w = x.shape
    if w < 3 or h < 3:
        raise ValueError("one reflection does not suffice under 3 x 3")
    p = np.pad(x, ((2, 2), (0, 0)), mode="reflect")
    acc = sum(TAPS[k] * p[k:k + h, :] for k in range(5)) + (1 << (d - 1))
    t = acc >> d
    q = np.pad(t, ((0, 0), (2, 2)), mode="reflect")
    acc2 = sum(TAPS[k] * q[:, k:k + w] for k in range(5)) + 32768
    b = acc2 >> 16
    if bounds is not None:
        for key, v in (("vacc", acc), ("t", t), ("hacc", acc2), ("b", b)):
            bounds[key] = max(bounds.get(key, 0), int(v.max()))
    return b


def sad(src, bitdepth, index=None, prev=None):
    """pp_motion's result as a list of Python ints: ``src`` [nsrc, h, w],
    ``index`` the shown sequence (default: every frame in order), ``prev`` one
    [h, w] plane or None."""
    src = np.asarray(src)
    idx = list(range(src.shape[0])) if index is None else [int(i) for i in index]
    h, w = src.shape[1:]
    if w < 3 or h < 3:
        return [ABSENT] * len(idx)
    cache = {}

    def b_of(i):
        if i not in cache:
            cache[i] = blur(src[i], bitdepth)
        return cache[i]
    out = []
    last = None if prev is None else blur(prev, bitdepth)
    for i in idx:
        cur = b_of(i)
        out.append(ABSENT if last is None else int(np.abs(cur - last).sum()))
        last = cur
    return out


def motion(sads, w, h):
    """(motion, motion2) of a whole clip's sums, as lists of floats (NaN: absent)."""
    m = [float("nan") if s == ABSENT else s / 256.0 / (w * h) for s in sads]
    if m:
        m[0] = 0.0
    m2 = [min(m[k], m[k + 1]) if k + 1 < len(m) and m[k] == m[k] and m[k + 1] == m[k + 1]
          else (m[k] if k + 1 == len(m) else float("nan")) for k in range(len(m))]
    return m, m2
