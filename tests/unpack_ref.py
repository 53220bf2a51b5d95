"""numpy restatement of the v210 and uyvy422 sample layouts (the reference of
pp_unpack_execute), written from the layouts, not from the oracle's packer.

v210 (libavcodec/v210dec.c): a line is little-endian 32-bit words of three
10-bit fields at bits 0-9, 10-19, 20-29 (bits 30-31 ignored).  Numbering the
fields of a line f = 0, 1, 2, ... (word f // 3, field f % 3), a 16-byte group
g holds fields 12 g .. 12 g + 11 in the order
    U0 Y0 V0 | Y1 U1 Y2 | V1 Y3 U2 | Y4 V2 Y5
so luma sample i of the line is field 12 (i // 6) + (1, 3, 5, 7, 9, 11)[i % 6],
U sample j is field 12 (j // 3) + (0, 4, 8)[j % 3] and V sample j is field
12 (j // 3) + (2, 6, 10)[j % 3], whatever W is: the tails of W % 6 in {2, 4}
are the same layout cut short, and nothing past the last pixel's fields is read.

uyvy422: bytes U Y0 V Y1 per pixel pair.

Both take buf [h, linesize] uint8, the line's pixel count W and an optional
crop (x, y, w, h) (x even, w may be odd: chroma width (w + 1) // 2) and
return (Y, U, V) of the window.
"""
import numpy as np

_Y_FIELD = (1, 3, 5, 7, 9, 11)
_U_FIELD = (0, 4, 8)
_V_FIELD = (2, 6, 10)


def _window(W, H, crop):
    x, y, w, h = (0, 0, W, H) if crop is None else crop
    assert W % 2 == 0 and x % 2 == 0 and 0 <= x and x + w <= W and 0 <= y and y + h <= H and w >= 1 and h >= 1
    return x, y, w, h


def unpack_v210(buf, W, crop=None):
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    H, ls = buf.shape
    assert ls % 4 == 0 and ls >= (W + 5) // 6 * 16
    x, y, w, h = _window(W, H, crop)
    words = buf.view("<u4").astype(np.uint32)  # [H, ls // 4]

    def field(f):
        f = np.asarray(f)
        return ((words[y:y + h][:, f // 3] >> (10 * (f % 3)).astype(np.uint32)) & 1023).astype(np.uint16)

    i = np.arange(x, x + w)
    j = np.arange(x // 2, x // 2 + (w + 1) // 2)
    Y = field(12 * (i // 6) + np.take(_Y_FIELD, i % 6))
    U = field(12 * (j // 3) + np.take(_U_FIELD, j % 3))
    V = field(12 * (j // 3) + np.take(_V_FIELD, j % 3))
    return Y, U, V


def unpack_uyvy(buf, W, crop=None):
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    H, ls = buf.shape
    assert ls >= 2 * W
    x, y, w, h = _window(W, H, crop)
    rows = buf[y:y + h]
    i = np.arange(x, x + w)
    j = np.arange(x // 2, x // 2 + (w + 1) // 2)
    return rows[:, 2 * i + 1].copy(), rows[:, 4 * j].copy(), rows[:, 4 * j + 2].copy()
