"""Host side of the motion feature (spec PP-MOTION-1): the scale of the
difference sums, motion2, the clip values and the motion of one file.

pp_motion (ops.motion) gives, per shown frame, the exact sum of absolute
differences between its blurred luma plane and that of the frame shown before
it.  This module turns the sums into the per-frame ``motion`` and ``motion2``
in the form VMAF uses as its temporal feature, in numpy, importable without a
GPU.  The taps, the roundings and the scale are libvmaf's integer motion as
recalled; parity with libvmaf is unpinned.
"""
import numpy as np

from .clips import nan_mean

SAD_ABSENT = (1 << 64) - 1  # pp_motion's sad without a previous frame, or of a plane under 3 x 3
TAPS = (3571, 16004, 26386, 16004, 3571)  # sum 65536
MIN_SIZE = 3           # the smallest width and height one reflection serves
# kernel geometry (csrc/motion.hip), for tests that place sizes on its seams
LANE_BYTES = 16        # bytes of a row a lane loads: 16 samples at 8 bits, 8 at 10
WAVE_PIECES = 64       # lanes of a wave: pieces of a row it loads, the halo's two among them
TILE_PIECES = 62       # kMoPieces: pieces of a row that are a tile's outputs
WAVE_ROWS = 16         # kMoLaneRows: rows of a tile one wave owns
TILE_ROWS = 64         # kMoTileRows: rows of a tile
SEGMENT = 4            # kMoSeg: shown frames a workgroup walks with the blurred tile in registers
FRAMES_PER_LAUNCH = 256  # kFrameMap (csrc/analysis_host.hpp)


def tile_cols(bitdepth):
    """Output columns of a tile at this bit depth."""
    return TILE_PIECES * LANE_BYTES // (2 if bitdepth > 8 else 1)


def _sad_float(sad):
    """pp_motion's sums as float64, NaN where absent (uint64 2^64-1 or int64 -1)."""
    if not isinstance(sad, np.ndarray):  # Python ints: numpy would make 2^64 - 1 next to a small one a float
        sad = np.array([int(v) & SAD_ABSENT for v in sad], dtype=np.uint64)
    s = np.ascontiguousarray(sad.reshape(-1))
    if s.dtype == np.int64:
        s = s.view(np.uint64)
    elif s.dtype != np.uint64:
        raise ValueError("sad must be uint64 or int64")
    return np.where(s == np.uint64(SAD_ABSENT), np.nan, s.astype(np.float64))


def pool(sad, w, h, first=True):
    """(motion [N], motion2 [N]) of pp_motion's sums of w x h planes, float64:
    motion[k] = sad[k] / 256 / (w h), on the 8-bit scale at both depths, NaN
    where the sum is absent; with ``first`` entry 0 is the first frame of a
    clip and has motion 0.  motion2[k] = min(motion[k], motion[k + 1]), the
    last frame's is its motion; a NaN on either side gives NaN."""
    m = _sad_float(sad) / 256.0 / (float(w) * float(h))
    if first and m.size:
        m[0] = 0.0
    m2 = m.copy()
    if m.size > 1:
        nxt = m[1:]
        m2[:-1] = np.where(np.isnan(m[:-1]) | np.isnan(nxt), np.nan, np.minimum(m[:-1], nxt))
    return m, m2


def summarize(sad, w, h, matched=None):
    """Per-frame arrays ``motion_y`` and ``motion2_y`` (float64 [N]) from
    pp_motion's output for a whole clip (entry 0 its first frame), plus
    ``mean``: the clip values of both, over the frames that have one.
    ``matched`` (bool [N]): the sequence is pooled as shown, then the other
    frames, which have no reference frame of their own, are set to NaN."""
    m, m2 = pool(sad, w, h)
    if matched is not None:
        un = ~np.asarray(matched, dtype=bool).reshape(-1)
        m[un] = np.nan
        m2[un] = np.nan
    res = {"motion_y": m, "motion2_y": m2}
    res["mean"] = {"motion_y": nan_mean(m), "motion2_y": nan_mean(m2)}
    return res


def motion_of_file(path, batch=32, crop=None, crop_from="yuv422p"):
    """PP-MOTION-1 of the file ``path`` on its own: ``summarize``'s dict plus
    ``frames``, ``w`` and ``h``.  The file is opened as stats.stats_of_file
    opens it and streamed ``batch`` frames at a time; a copy of the last luma
    plane of a batch is the next call's ``prev``, so only frame 0 of the file
    has no difference.  ``crop``, ``crop_from``: as stats_of_file's."""
    import torch

    from . import clips, ops
    with clips.clip_batches(path, max(1, int(batch)), crop, crop_from) as (rd, window, batches):
        w, h = (rd.w, rd.h) if window is None else window[2:]
        outs, prev = [], None
        for b in batches:
            outs.append(ops.motion(b, prev=prev))
            prev = b.view(0)[b.n - 1:b.n].clone()
        torch.cuda.current_stream().synchronize()
    sad = clips.host_array(outs, (), np.uint64)
    res = summarize(sad, w, h)
    res.update({"frames": int(sad.shape[0]), "w": int(w), "h": int(h)})
    return res
