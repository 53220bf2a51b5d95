"""Host side of the DCT-energy complexity (spec PP-DCTE-1): the block
geometry, the pooling of the sums into E, h and L, the clip values and the
complexity of one file.

pp_dct_energy (ops.dct_energy) gives, per shown frame, the exact sums over the
frame's whole 32 x 32 blocks of the weighted absolute AC coefficients
(``energy``), of the DC coefficients (``dc``) and of the blocks' absolute
energy differences against the frame shown before (``tdiff``).  This module
turns them into the spatial complexity E, the temporal complexity h and the
brightness L, in numpy, importable without a GPU.  The measure is modelled on
the Video Complexity Analyzer (Menon et al., 2022) as recalled and defined by
the spec's text alone: the weight formula is VCA's, the integer transform, its
roundings and the brightness (the mean luma on the 8-bit scale, not VCA's
square root of the DC) are this library's; parity with VCA is unpinned
(DESIGN.md).
"""
import os

import numpy as np

from .clips import json_value, nan_mean

SPEC = "PP-DCTE-1 (32x32 integer DCT-II energy, modelled on VCA, parity unpinned)"
ABSENT = (1 << 64) - 1   # pp_dct_energy's tdiff without a previous frame; everything of a plane under 32 x 32
BLOCK = 32               # rows and columns of a block
ENERGY_SCALE = 1 << 20   # energy and tdiff per block -> E and h
DC_SCALE = 128           # dc per block -> the mean luma on the 8-bit scale
# kernel geometry (csrc/dctenergy.hip), for tests that place sizes on its seams
BLOCKS_PER_WAVE = 2        # a half-wave of 32 lanes owns a block
BLOCKS_PER_WORKGROUP = 8   # kDeBlocks: consecutive blocks (row-major) a workgroup owns
FINALIZE_LANES = 256       # lanes of dct_finalize: a lane adds every 256th block of a frame
FRAMES_PER_LAUNCH = 256    # kFrameMap (csrc/analysis_host.hpp)


def geometry(w, h):
    """(bx, by): the whole blocks across and down a w x h plane."""
    return int(w) // BLOCK, int(h) // BLOCK


def _as_uint64(v):
    a = v if isinstance(v, np.ndarray) else np.array([[int(x) & ABSENT for x in row] for row in v], dtype=np.uint64)
    a = np.ascontiguousarray(a).reshape(-1, 3)
    if a.dtype == np.int64:
        a = a.view(np.uint64)
    elif a.dtype != np.uint64:
        raise ValueError("sums must be uint64 or int64")
    return a


def pool(sums, w, h, first=True):
    """(E [N], h [N], L [N]) of pp_dct_energy's sums [N, 3] of w x h planes,
    float64, with nb = bx by: E = energy / (nb 2^20), h = tdiff / (nb 2^20),
    L = dc / (128 nb); NaN where a sum is absent, but with ``first`` entry 0 is
    the first frame of a clip and an absent tdiff there gives h = 0."""
    s = _as_uint64(sums)
    bx, by = geometry(w, h)
    nb = float(max(bx * by, 1))
    val = np.where(s == np.uint64(ABSENT), np.nan, s.astype(np.float64))
    E = val[:, 0] / (nb * ENERGY_SCALE)
    T = val[:, 2] / (nb * ENERGY_SCALE)
    L = val[:, 1] / (nb * DC_SCALE)
    if first and T.size and np.isnan(T[0]) and not np.isnan(E[0]):
        T[0] = 0.0
    return E, T, L


def summarize(sums, w, h):
    """Per-frame arrays ``dct_energy_y``, ``dct_temporal_y`` and
    ``brightness_y`` (float64 [N]) from pp_dct_energy's output for a whole clip
    (entry 0 its first frame), plus ``mean``: the clip values, the means over
    the frames that have one."""
    E, T, L = pool(sums, w, h)
    res = {"dct_energy_y": E, "dct_temporal_y": T, "brightness_y": L}
    res["mean"] = {k: nan_mean(v) for k, v in res.items()}
    return res


def _host_batches(rd, batch, dev):
    """[n, h, w] device luma tensors of a luma reader, ``batch`` frames each."""
    import torch
    dt = np.uint16 if rd.depth > 8 else np.uint8
    while True:
        host = np.empty((batch, rd.luma_bytes), np.uint8)
        n = rd.read_into(host, batch)
        if n == 0:
            return
        yield torch.from_numpy(host[:n].view(dt).reshape(n, rd.h, rd.w)).to(dev)
        if n < batch:
            return


def _packed_batches(rd, batch, dev, window):
    """The same of a packed reader: packets to the GPU as they are, luma alone unpacked there."""
    from . import clips, ops
    while (b := clips.read_packets(rd, batch, dev)) is not None:
        yield ops.unpack(b, crop=window, luma_only=True)


def dct_energy_of_file(videofile, batch=32, reader=None, crop=None, crop_from="yuv422p"):
    """PP-DCTE-1 of the file ``videofile`` on its own: ``summarize``'s dict
    plus ``frames``, ``w``, ``h``, ``bitdepth`` and ``blocks`` (bx, by).  Luma
    alone is read, as clips.open_luma reads it (``reader``: a full-frame
    pixpath.io reader instead); of a v210 or UYVY AVI, ``crop`` = (w, h) and
    ``crop_from`` give the AVPVS picture inside a CPVS canvas, as
    stats.stats_of_file's.  ``batch`` frames at a time; a copy of the last
    luma plane of a batch is the next call's ``prev``, so only frame 0 of the
    file has no difference."""
    import torch

    from . import clips, ops
    batch = max(1, int(batch))
    dev = torch.device("cuda", torch.cuda.current_device())
    rd, packed = clips.open_luma(videofile, reader)
    try:
        if crop is not None and not packed:
            raise ValueError("crop applies to a packed (v210 / UYVY) clip")
        if packed:
            window = None if crop is None else clips.crop_window(rd.w, rd.h, crop[0], crop[1], crop_from)
            w, h, depth = (rd.w, rd.h) + (rd.fmt.depth,) if window is None else tuple(window[2:]) + (rd.fmt.depth,)
            batches = _packed_batches(rd, batch, dev, window)
        else:
            w, h, depth = rd.w, rd.h, rd.depth
            batches = _host_batches(rd, batch, dev)
        outs, prev = [], None
        for luma in batches:
            outs.append(ops.dct_energy(luma, depth, prev=prev))
            prev = luma[luma.shape[0] - 1:].clone()
        torch.cuda.current_stream().synchronize()
    finally:
        rd.close()
    sums = clips.host_array(outs, (3,), np.uint64)
    res = summarize(sums, w, h)
    res.update({"frames": int(sums.shape[0]), "w": int(w), "h": int(h), "bitdepth": int(depth),
                "blocks": geometry(w, h)})
    return res


def report(res, path, per_frame=False):
    """The JSON object `cli complexity` prints: the clip values, and with
    per_frame the three per-frame lists; NaN becomes null."""
    mean = res["mean"]
    out = {"file": os.path.basename(path), "frames": int(res["frames"]), "w": int(res["w"]), "h": int(res["h"]),
           "spec": SPEC, "blocks": [int(v) for v in res["blocks"]]}
    for key in ("dct_energy_y", "dct_temporal_y", "brightness_y"):
        out[key] = json_value(mean[key])
    if per_frame:
        for key in ("dct_energy_y", "dct_temporal_y", "brightness_y"):
            out[key + "_frames"] = [json_value(v) for v in res[key]]
    return out


def yaml_entry(res):
    """The extra "dct_energy" key of <src>.yaml (siti.analyse_src): the clip
    values, the per-frame lists, the SRC's luma bit depth and the spec string.
    ``res``: dct_energy_of_file's dict, or any dict with the three per-frame
    lists and ``bitdepth``."""
    lists = {k: [json_value(v) for v in np.asarray(res[k], dtype=np.float64)]
             for k in ("dct_energy_y", "dct_temporal_y", "brightness_y")}
    e = {k: json_value(nan_mean(np.asarray(res[k], dtype=np.float64))) for k in lists}
    e.update({k + "_frames": v for k, v in lists.items()})
    if res.get("bitdepth") is not None:
        e["bitdepth"] = int(res["bitdepth"])
    e["spec"] = SPEC
    return e
