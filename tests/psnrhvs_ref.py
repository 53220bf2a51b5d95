"""numpy restatement of spec PP-HVS-1, written from the spec's text
and not from the kernel: the S_hvs and S_hvsm sums of a plane pair, every block
at once.  Floating arithmetic is float64; the variance ratio is taken in exact
int64; the DCT is two matrix products, rows first, then columns (the kernel
folds each 8-point sum by the matrix's symmetry and fuses its multiply-adds:
another order of the same sums, a few 2^-53 relative apart)."""
import numpy as np

N = 8
Q = np.array([[16, 11, 10, 16, 24, 40, 51, 61],
              [12, 12, 14, 19, 26, 58, 60, 55],
              [14, 13, 16, 24, 40, 57, 69, 56],
              [14, 17, 22, 29, 51, 87, 80, 62],
              [18, 22, 37, 56, 68, 109, 103, 77],
              [24, 35, 55, 64, 81, 104, 113, 92],
              [49, 64, 78, 87, 103, 121, 120, 101],
              [72, 92, 95, 98, 112, 100, 103, 99]], dtype=np.float64)
# the published six-decimal table, as DESIGN.md prints it
CSF = np.array([[1.608443, 2.339554, 2.573509, 1.608443, 1.072295, 0.643377, 0.504610, 0.421887],
                [2.144591, 2.144591, 1.838221, 1.354478, 0.989811, 0.443708, 0.428918, 0.467911],
                [1.838221, 1.979622, 1.608443, 1.072295, 0.643377, 0.451493, 0.372972, 0.459555],
                [1.838221, 1.513829, 1.169777, 0.887417, 0.504610, 0.295806, 0.321689, 0.415082],
                [1.429727, 1.169777, 0.695543, 0.459555, 0.378457, 0.236102, 0.249855, 0.334222],
                [1.072295, 0.735288, 0.467911, 0.402111, 0.317717, 0.247453, 0.227744, 0.279729],
                [0.525206, 0.402111, 0.329937, 0.295806, 0.249855, 0.212687, 0.214459, 0.254803],
                [0.357432, 0.279729, 0.270896, 0.262603, 0.229778, 0.257351, 0.249855, 0.259950]])
M = (10.0 / Q) ** 2
NOT_DC = np.ones((N, N), dtype=bool)
NOT_DC[0, 0] = False


def dct_matrix():
    """C[k][n] = c(k) cos((2n + 1) k pi / 16), c(0) = sqrt(1/8), c(k) = 1/2."""
    C = np.zeros((N, N))
    for k in range(N):
        for n in range(N):
            C[k, n] = (np.sqrt(1.0 / 8.0) if k == 0 else 0.5) * np.cos((2 * n + 1) * k * np.pi / 16.0)
    return C


C = dct_matrix()


def nb(n, step):
    return 0 if n < N else (n - N) // step + 1


def _blocks(plane, step):
    """[by, bx, 8, 8] int64: the blocks with origins (i step, j step) wholly inside the plane."""
    h, w = plane.shape
    if h < N or w < N:
        return np.zeros((0, 0, N, N), dtype=np.int64)
    out = np.lib.stride_tricks.sliding_window_view(plane, (N, N))[::step, ::step]  # every origin with origin + 8 <= size
    assert out.shape[:2] == (nb(h, step), nb(w, step))
    return np.ascontiguousarray(out)


def dct2(x):
    """D(X) of every block of [.., 8, 8]: the rows first (X C^T), then the columns (C .)."""
    return np.matmul(C, np.matmul(x.astype(np.float64), C.T))


def _pop(x):
    """21 sum V_q / (5 V) in exact integers, 0 where V = 0; x int64 [.., 8, 8]."""
    S = x.sum(axis=(-1, -2))
    V = 64 * (x * x).sum(axis=(-1, -2)) - S * S
    vq = np.zeros_like(V)
    for r in (0, 4):
        for c in (0, 4):
            q = x[..., r:r + 4, c:c + 4]
            s = q.sum(axis=(-1, -2))
            vq += 16 * (q * q).sum(axis=(-1, -2)) - s * s
    assert (V >= 0).all() and (vq >= 0).all() and (21 * vq < 2 ** 53).all() and (5 * V < 2 ** 53).all()
    safe = np.where(V != 0, 5 * V, 1).astype(np.float64)
    return np.where(V != 0, (21 * vq).astype(np.float64) / safe, 0.0)


def _mask(x, d):
    m = (d * d * M)[..., NOT_DC].sum(axis=-1)
    return np.sqrt(m * _pop(x)) / 32.0


def plane_sums(a, b, step=8):
    """(S_hvs, S_hvsm, blocks) of a reference plane a and a distorted plane b (2-D integer arrays)."""
    assert a.shape == b.shape and step in (7, 8)
    xa, xb = _blocks(np.asarray(a).astype(np.int64), step), _blocks(np.asarray(b).astype(np.int64), step)
    count = xa.shape[0] * xa.shape[1]
    if count == 0:
        return 0.0, 0.0, 0
    da, db = dct2(xa), dct2(xb)
    T = np.maximum(_mask(xa, da), _mask(xb, db))[..., None, None]
    u = np.abs(da - db)
    um = np.where(NOT_DC, np.maximum(u - T / M, 0.0), u)
    return float(((u * CSF) ** 2).sum()), float(((um * CSF) ** 2).sum()), count


def psnr_hvs(ref, dist, step=8, ref_index=None):
    """[ndist, 3, 2] float64: per distorted frame and plane S_hvs and S_hvsm;
    ref, dist: lists of three [n, rows, cols] arrays."""
    n = dist[0].shape[0]
    idx = np.arange(n) if ref_index is None else np.asarray(ref_index)
    out = np.zeros((n, 3, 2))
    for k in range(n):
        for p in range(3):
            out[k, p] = plane_sums(ref[p][idx[k]], dist[p][k], step)[:2]
    return out
