"""Plumbing the GPU tests of the analysis kernels share: the poisoned device
layout of a clip, and callers of the C entry points themselves that hand them
sentinel-filled outputs of two frames more than they need, so that a test can
see that nothing but the result was written."""
import ctypes

import numpy as np

SENTINEL = 0x5A5A5A5A5A5A5A5A


def make(gpu, depth, data, layout="std", seed=0):
    """The planes `data` [n, h, w] on the device as an [n, h, w] view.  Layouts:
    std (pointer, pitch and frame stride on the 16-B grid, at least 16 B of
    pitch padding), odd (one element off the grid, an odd pitch).  The padding
    holds random samples of the whole container: poison."""
    import torch
    rng = np.random.default_rng(seed + 77)
    n, h, w = data.shape
    es = 2 if depth > 8 else 1
    dt = np.uint16 if es == 2 else np.uint8
    top = (1 << (8 * es)) - 1
    if layout == "std":
        rows, cols, x0, y0 = h + 2, ((w * es + 15) // 16 * 16 + 16) // es, 0, 0
        if (rows * cols * es) % 16:
            rows += 1
    else:
        rows, cols, x0, y0 = h + 3, (w + 7) | 1, 1, 1
    big = rng.integers(0, top + 1, (max(n, 1), rows, cols)).astype(dt)
    big[:n, y0:y0 + h, x0:x0 + w] = data
    t = torch.from_numpy(big).to(gpu)[:n, y0:y0 + h, x0:x0 + w]
    on_grid = (t.data_ptr() | t.stride(1) * es | t.stride(0) * es) % 16 == 0
    assert on_grid == (layout == "std")
    return t


def _entry(gpu, symbol, null):
    """(the library's `symbol`, the context or None, name -> pointer or None, the stream)."""
    import torch
    from pixpath import _native, ops
    ctx = None if "ctx" in null else ops.context(gpu.index).handle
    ptr = lambda name, v: None if name in null else ctypes.c_void_p(v)
    return getattr(_native.lib(), symbol), ctx, ptr, ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


def call_pair(gpu, symbol, tail, depth, w, h, ref, dist, idx=None, nd=None, nr=None, rls=None, dls=None, null=()):
    """A luma-pair entry (pp_ms_ssim, pp_vif, pp_adm) itself; returns (rc, out
    [nd, *tail] float64, untouched: everything else kept the sentinel)."""
    import torch
    fn, ctx, ptr, stream = _entry(gpu, symbol, null)
    nd = dist.shape[0] if nd is None else nd
    nr = ref.shape[0] if nr is None else nr
    es = dist.element_size()
    out = torch.full((max(nd, 0) + 2,) + tuple(tail), SENTINEL, dtype=torch.int64, device=gpu)
    ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    rc = fn(ctx, depth, w, h, ptr("ref", ref.data_ptr()), ref.stride(1) * es if rls is None else rls, ref.stride(0) * es, nr,
            ptr("dist", dist.data_ptr()), dist.stride(1) * es if dls is None else dls, dist.stride(0) * es, nd,
            None if ix is None else ix.ctypes.data, ptr("out", out.data_ptr()), stream)
    torch.cuda.synchronize(gpu)
    raw = out.cpu().numpy()
    n = max(nd, 0) if rc == 0 else 0
    return rc, raw[:n].view(np.float64), bool((raw[n:] == SENTINEL).all())


def prev_args(prev, pls=None):
    """(pointer, pitch) of the one frame `prev` [1, h, w] shown before a sequence; (None, 0) without one."""
    if prev is None:
        return None, 0
    return ctypes.c_void_p(prev.data_ptr()), prev.stride(1) * prev.element_size() if pls is None else pls


def call_sequence(gpu, symbol, depth, w, h, src, middle, outs, idx=None, n=None, nsrc=None, sls=None, null=()):
    """A shown-sequence entry (pp_motion, pp_banding, pp_dct_energy) itself.
    `middle`: its arguments between n and the outputs; `outs`: (name, trailing
    shape, dtype name) of each output, NULL where `null` has the name.  Returns
    (rc, k, raws): the k frames it should have written (none unless rc is 0) and
    every output whole, two frames more than n, as unsigned integers (`untouched`)."""
    import torch
    fn, ctx, ptr, stream = _entry(gpu, symbol, null)
    nsrc = src.shape[0] if nsrc is None else nsrc
    ix = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    n = (nsrc if ix is None else len(ix)) if n is None else n
    es = src.element_size()
    bufs = [torch.full((max(n, 0) + 2,) + tuple(tail), sentinel(dt), dtype=getattr(torch, dt), device=gpu) for _, tail, dt in outs]
    rc = fn(ctx, depth, w, h, ptr("src", src.data_ptr()), src.stride(1) * es if sls is None else sls, src.stride(0) * es, nsrc,
            None if ix is None else ix.ctypes.data, n, *middle,
            *[ptr(name, b.data_ptr()) for (name, _, _), b in zip(outs, bufs)], stream)
    torch.cuda.synchronize(gpu)
    raws = [b.cpu().numpy().view(np.uint32 if dt == "int32" else np.uint64) for (_, _, dt), b in zip(outs, bufs)]
    return rc, max(n, 0) if rc == 0 else 0, raws


def sentinel(dt):
    """The sentinel of an output of dtype name `dt` (int32 or int64)."""
    return SENTINEL & 0xFFFFFFFF if dt == "int32" else SENTINEL


def untouched(raw, k):
    """Everything of the output `raw` past its first k frames kept the sentinel."""
    return bool((raw[k:] == sentinel("int32" if raw.dtype == np.uint32 else "int64")).all())
