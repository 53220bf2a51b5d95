"""numpy restatement of spec PP-DCTE-1, written from the
spec text: its own tables from the two formulas, int64 arithmetic, both passes
as plain 32 x 32 matrix products with the two roundings, sums in Python ints.
It shares no code with csrc/dctenergy.hip, csrc/dct32_tables.hpp,
tools/gen_dct32_tables.py or pixpath/dctenergy.py."""
import numpy as np

ABSENT = (1 << 64) - 1
B = 32

_n = np.arange(B, dtype=np.float64)
_s = np.where(np.arange(B) == 0, np.sqrt(0.5), 1.0)
C = np.floor(4096.0 * _s[:, None] * np.cos((2.0 * _n[None, :] + 1.0) * _n[:, None] * np.pi / 64.0) + 0.5).astype(np.int64)
W = np.floor(256.0 * np.exp(np.abs((_n[:, None] * _n[None, :] / 1024.0) ** 2 - 1.0)) + 0.5).astype(np.int64)


def geometry(w, h):
    """(bx, by): the whole 32 x 32 blocks across and down."""
    return int(w) // B, int(h) // B


def transform(block, bitdepth, bounds=None):
    """Y [32, 32] int64 of one 32 x 32 block of samples.  ``bounds``: a dict
    that receives the largest |row accumulator|, |T|, |column accumulator|, |Y|."""
    d = int(bitdepth)
    x = np.minimum(np.asarray(block).astype(np.int64), (1 << d) - 1)
    acc = x @ C.T + (1 << (d + 3))          # acc[i][k] = sum_n C[k][n] x[i][n]
    t = acc >> (d + 4)
    acc2 = C @ t + (1 << 13)                # acc2[l][k] = sum_i C[l][i] T[i][k]
    y = acc2 >> 14
    if bounds is not None:
        for key, v in (("racc", acc), ("t", t), ("cacc", acc2), ("y", y)):
            bounds[key] = max(bounds.get(key, 0), int(np.abs(v).max()))
    return y


def frame(plane, bitdepth):
    """(e [by, bx] of Python ints as an object array, dc [by, bx] likewise) of one [h, w] plane."""
    plane = np.asarray(plane)
    h, w = plane.shape
    bx, by = geometry(w, h)
    e = np.zeros((by, bx), dtype=object)
    dc = np.zeros((by, bx), dtype=object)
    for j in range(by):
        for i in range(bx):
            y = transform(plane[j * B:(j + 1) * B, i * B:(i + 1) * B], bitdepth)
            wy = W * np.abs(y)
            e[j, i] = int(wy.sum()) - int(wy[0, 0])
            dc[j, i] = int(y[0, 0])
    return e, dc


def _walk(src, bitdepth, index, prev):
    src = np.asarray(src)
    idx = list(range(src.shape[0])) if index is None else [int(i) for i in index]
    cache = {}

    def of(i):
        if i not in cache:
            cache[i] = frame(src[i], bitdepth)
        return cache[i]
    last = None if prev is None else frame(prev, bitdepth)[0]
    for i in idx:
        e, dc = of(i)
        yield e, dc, last
        last = e


def sums(src, bitdepth, index=None, prev=None):
    """pp_dct_energy's ``out`` as a list of [energy, dc, tdiff] rows of Python
    ints: ``src`` [nsrc, h, w], ``index`` the shown sequence (default: every
    frame in order), ``prev`` one [h, w] plane or None."""
    h, w = np.asarray(src).shape[1:]
    if w < B or h < B:
        n = np.asarray(src).shape[0] if index is None else len(index)
        return [[ABSENT] * 3 for _ in range(n)]
    out = []
    for e, dc, last in _walk(src, bitdepth, index, prev):
        td = ABSENT if last is None else sum(abs(int(a) - int(b)) for a, b in zip(e.ravel(), last.ravel()))
        out.append([sum(int(v) for v in e.ravel()), sum(int(v) for v in dc.ravel()) & ABSENT, td])
    return out


def blocks(src, bitdepth, index=None, prev=None):
    """pp_dct_energy's ``blocks``: a list over shown frames of [by][bx] lists of Python ints."""
    h, w = np.asarray(src).shape[1:]
    if w < B or h < B:
        n = np.asarray(src).shape[0] if index is None else len(index)
        return [[] for _ in range(n)]
    return [[[int(v) for v in row] for row in e] for e, _, _ in _walk(src, bitdepth, index, prev)]


def pool(rows, w, h):
    """(E, h, L) per frame as lists of floats from ``sums``' rows of a whole clip."""
    bx, by = geometry(w, h)
    nb = bx * by
    E = [r[0] / (nb * 1048576.0) for r in rows]
    T = [0.0 if (r[2] == ABSENT and k == 0) else r[2] / (nb * 1048576.0) for k, r in enumerate(rows)]
    L = [r[1] / (nb * 128.0) for r in rows]
    return E, T, L
