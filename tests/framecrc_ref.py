"""PP-HASH-1 on the host (test helper): the byte string of a frame from numpy
planes by plain slicing, and zlib's Adler-32 of it."""
import zlib

import numpy as np

PLANAR = {"yuv420p": (1, 1, 1), "yuv422p": (1, 1, 0), "yuv444p": (1, 0, 0),
          "yuv420p10le": (2, 1, 1), "yuv422p10le": (2, 1, 0), "yuv444p10le": (2, 0, 0)}


def v210_linesize(w):
    return (w + 47) // 48 * 48 * 8 // 3


def frame_string(fmt, w, h, planes):
    """The bytes PP-HASH-1 hashes.  planes: the 2-D arrays of one frame (uint8 /
    uint16; packed formats: the uint8 rows of plane 0), as wide or wider than
    the rows' extent and as high or higher than the plane."""
    if fmt == "uyvy422":
        return np.asarray(planes[0], np.uint8)[:h, :2 * w].tobytes()
    if fmt == "v210":
        return np.asarray(planes[0], np.uint8)[:h, :v210_linesize(w)].tobytes()
    es, hs, vs = PLANAR[fmt]
    out = b""
    for p in range(3):
        pw, ph = (-(-w >> hs), -(-h >> vs)) if p else (w, h)
        out += np.asarray(planes[p])[:ph, :pw].astype("<u2" if es == 2 else np.uint8).tobytes()
    return out


def adler32(fmt, w, h, planes, init=0):
    return zlib.adler32(frame_string(fmt, w, h, planes), init) & 0xffffffff
