"""Host side of the frame checksums (spec PP-HASH-1), no GPU: the argument
checks of pp_frame_adler32, the framecrc listing (format, parse, compare), the
reference helper against hand-computed values, and the writer wrapper's host
path."""
import ctypes
import zlib
from fractions import Fraction

import numpy as np
import pytest

import framecrc_ref
from pixpath import _native, formats, framecrc


# ------------------------------------------------------------ argument checks
def _frames(data=(0x1000, 0x2000, 0x3000), ls=(256, 128, 128)):
    s = _native.pp_frames()
    for p in range(3):
        s.data[p] = data[p]
        s.linesize[p] = ls[p]
        s.frame_stride[p] = ls[p] * 64
    return s


def _call(ctx, fmt, w, h, src, n=1, out=0x4000):
    L = _native.lib()
    return L.pp_frame_adler32(ctx, fmt, w, h, None if src is None else ctypes.byref(src), n, 0,
                              ctypes.c_void_p(out), None)


def test_pp_frame_adler32_argument_checks_need_no_gpu():
    L = _native.lib()
    ctx = (ctypes.c_uint8 * 256)()  # never dereferenced: every call below is refused first
    P8, P10, U8, V = formats.YUV422P, formats.YUV422P10LE, formats.UYVY422, formats.V210
    src = _frames()
    assert _call(None, P8, 48, 8, src) == -1                       # NULL ctx
    assert b"null" in L.pp_last_error()
    assert _call(ctx, P8, 48, 8, None) == -1                       # NULL src
    assert _call(ctx, P8, 48, 8, src, out=None) == -1              # NULL out
    for bad in (-1, 8, 99):
        assert _call(ctx, bad, 48, 8, src) == -1                   # unknown format
        assert b"format" in L.pp_last_error()
    assert _call(ctx, P8, 0, 8, src) == -1 and b"0x8" in L.pp_last_error()
    assert _call(ctx, P8, 48, 0, src) == -1
    assert _call(ctx, P8, -3, 8, src) == -1
    assert _call(ctx, V, 47, 8, src) == -1                         # odd packed widths
    assert b"v210 needs an even width, not 47" in L.pp_last_error()
    assert _call(ctx, U8, 47, 8, src) == -1
    assert b"uyvy422 needs an even width" in L.pp_last_error()
    assert _call(ctx, P8, 48, 8, src, n=-1) == -1                  # negative nframes
    assert b"nframes" in L.pp_last_error()
    assert _call(ctx, P8, 300, 8, src) == -1                       # luma rows of 300 > 256
    assert b"linesize" in L.pp_last_error()
    assert _call(ctx, P8, 48, 8, _frames(ls=(256, 23, 128))) == -1  # chroma rows of 24 > 23
    assert b"plane 1" in L.pp_last_error()
    assert _call(ctx, P10, 48, 8, _frames(ls=(95, 128, 128))) == -1  # 96 bytes of 10-bit luma
    assert _call(ctx, U8, 48, 8, _frames(ls=(95, 0, 0))) == -1      # below 2 w
    assert _call(ctx, V, 50, 8, _frames(ls=(144, 0, 0))) == -1      # ceil(50/6)*16 unpacks, but the packet row is 256
    assert b"linesize" in L.pp_last_error()
    assert _call(ctx, P8, 48, 8, _frames(data=(0x1000, 0, 0x3000))) == -1  # a plane pointer missing
    assert b"null" in L.pp_last_error()
    # accepted geometry with nothing to do: OK without touching the context
    assert _call(ctx, P8, 47, 7, src, n=0) == 0
    assert _call(ctx, V, 50, 8, _frames(ls=(256, 0, 0)), n=0) == 0
    assert _call(ctx, U8, 48, 8, _frames(data=(0x1000, 0, 0), ls=(96, 0, 0)), n=0) == 0  # packed: plane 0 only


def test_frame_adler32_is_exported_without_an_abi_bump():
    assert "pp_frame_adler32" in _native.EXPORTS
    assert _native.lib().pp_abi_version() == 7


def test_geometry_constants_match_the_kernel():
    import os
    from pixpath import ops
    src = open(os.path.join(os.path.dirname(_native.__file__), "..", "csrc", "framecrc.hip")).read()
    assert "kCrcLaneBytes = %d;" % ops.CRC_LANE_BYTES in src and "kCrcLanes = %d;" % ops.CRC_LANES in src
    assert "kCrcWaveRows = %d;" % ops.CRC_WAVE_ROWS in src and "kCrcWaves = 4;" in src
    assert ops.CRC_BAND_ROWS == 4 * ops.CRC_WAVE_ROWS


# ------------------------------------------------------------------ the helper
def _adler_by_hand(data, init):
    a, b = init & 0xffff, init >> 16
    for d in data:
        a = (a + d) % 65521
        b = (b + a) % 65521
    return (b << 16) | a


def test_reference_helper_known_answers():
    planes = [np.array([[7]], np.uint8), np.array([[200]], np.uint8), np.array([[31]], np.uint8)]
    assert framecrc_ref.frame_string("yuv444p", 1, 1, planes) == bytes([7, 200, 31])
    # a = 7, 207, 238; b = 7, 214, 452
    assert framecrc_ref.adler32("yuv444p", 1, 1, planes, 0) == (452 << 16) | 238
    # from 1: a = 8, 208, 239; b = 8, 216, 455
    assert framecrc_ref.adler32("yuv444p", 1, 1, planes, 1) == (455 << 16) | 239 == zlib.adler32(bytes([7, 200, 31]))
    # the closed form of the spec: A = a0 + sum d, B = b0 + N a0 + sum (N - i) d_i
    assert 3 * 7 + 2 * 200 + 31 == 452
    for init in (0, 1, 0xFFF0FFF0, 0xFFFFFFFF, 0x1234ABCD):
        assert framecrc_ref.adler32("yuv444p", 1, 1, planes, init) == _adler_by_hand([7, 200, 31], init)


def test_reference_helper_strings():
    rng = np.random.default_rng(3)
    # 10-bit: two little-endian bytes a sample, nothing masked; padding columns and rows never count
    y = np.array([[0xFFFF, 0x0102, 0xAAAA], [3, 4, 0xBBBB], [0xCCCC] * 3], np.uint16)
    c = np.array([[0x0A0B, 0xDDDD], [0x0C0D, 0xDDDD]], np.uint16)
    s = framecrc_ref.frame_string("yuv422p10le", 2, 2, [y, c, c + 1])
    assert s == bytes([0xFF, 0xFF, 0x02, 0x01, 3, 0, 4, 0, 0x0B, 0x0A, 0x0D, 0x0C, 0x0C, 0x0A, 0x0E, 0x0C])
    # 4:2:0 of an odd size: chroma is rounded up
    pl = [rng.integers(0, 256, (5, 9)).astype(np.uint8) for _ in range(3)]
    assert framecrc_ref.frame_string("yuv420p", 5, 3, pl) == \
        pl[0][:3, :5].tobytes() + pl[1][:2, :3].tobytes() + pl[2][:2, :3].tobytes()
    pk = rng.integers(0, 256, (3, 300)).astype(np.uint8)
    assert framecrc_ref.frame_string("uyvy422", 6, 2, [pk]) == pk[:2, :12].tobytes()
    assert framecrc_ref.frame_string("v210", 50, 2, [pk]) == pk[:2, :256].tobytes()
    assert framecrc_ref.v210_linesize(50) == formats.v210_linesize(50) == 256
    assert framecrc_ref.v210_linesize(48) == 128 and framecrc_ref.v210_linesize(2) == 128


def test_chaining_identity():
    rng = np.random.default_rng(4)
    x, y = rng.integers(0, 256, 700).astype(np.uint8).tobytes(), rng.integers(0, 256, 9000).astype(np.uint8).tobytes()
    for s in (0, 1, 0xFFF0FFF0, 0x00010000):
        assert zlib.adler32(x + y, s) == zlib.adler32(y, zlib.adler32(x, s)) == _adler_by_hand(x + y, s)


# ------------------------------------------------------------------ the listing
FRAMES = [(4608, 0x05b789ef), (4608, 0), (4608, 0xffffffff), (12, 1)]


def test_format_lines_layout():
    text = framecrc.format_lines(FRAMES[:2], 64, 48, Fraction(30000, 1001))
    assert text.splitlines() == [
        "#tb 0: 1001/30000", "#media_type 0: video", "#codec_id 0: rawvideo", "#dimensions 0: 64x48", "#sar 0: 1/1",
        "0,          0,          0,        1,     4608, 0x05b789ef",
        "0,          1,          1,        1,     4608, 0x00000000"]
    assert text.endswith("\n")
    assert framecrc.format_lines([], 2, 2, 60).splitlines()[0] == "#tb 0: 1/60"


def test_format_parse_round_trip():
    assert framecrc.parse(framecrc.format_lines(FRAMES, 64, 48, 60)) == FRAMES
    assert framecrc.parse(framecrc.format_lines([], 64, 48, 60)) == []


def test_parse_accepts_other_headers_and_spacing():
    text = ("#format: frame checksums\n#version: 2\n#hash: Adler-32\n#software: Lavf60.16.100\n#tb 0: 1/25\n"
            "#media_type 0: video\n#codec_id 0: rawvideo\n#dimensions 0: 352x288\n#sar 0: 128/117\n"
            "0,0,0,1,152064,0x05B789EF\n"
            "\n"
            "  0 ,\t 1,   1 ,1,  152064 ,   0x0000abcd  \n"
            "0,          2,          2,        1,   152064, 0xdeadbeef, S=1,        8, 0x12345678\n"
            "# trailing comment\n")
    assert framecrc.parse(text) == [(152064, 0x05b789ef), (152064, 0xabcd), (152064, 0xdeadbeef)]
    with pytest.raises(ValueError, match="line 2"):
        framecrc.parse("#x\n0, 0, 0, 1, 12\n")


def test_compare():
    a = list(FRAMES)
    assert framecrc.compare(a, list(a)) is None
    assert framecrc.compare([], []) is None
    b = list(a)
    b[2] = (4608, 0xfffffffe)
    b[3] = (12, 2)
    assert framecrc.compare(a, b) == {"frame": 2, "a": (4608, 0xffffffff), "b": (4608, 0xfffffffe)}
    b = list(a)
    b[1] = (4607, 0)  # the size counts too
    assert framecrc.compare(a, b)["frame"] == 1
    assert framecrc.compare(a, a[:3]) == {"frames_a": 4, "frames_b": 3}
    assert framecrc.compare(a[:1], a) == {"frames_a": 1, "frames_b": 4}
    assert framecrc.compare(b, a[:1])  == {"frames_a": 4, "frames_b": 1}  # the common part is equal
    assert framecrc.report(4, None) == {"frames": 4, "equal": True}
    assert framecrc.report(4, framecrc.compare(a, a[:3])) == {"frames": 4, "equal": False, "frames_against": 3}
    b = list(a)
    b[0] = (4608, 1)
    assert framecrc.report(4, framecrc.compare(a, b)) == {
        "frames": 4, "equal": False, "frame": 0, "size": [4608, 4608], "crc": ["0x05b789ef", "0x00000001"]}


# ------------------------------------------------------- the writer's host path
class _Sink:
    def __init__(self):
        self.got, self.closed = [], False

    def write(self, frames):
        self.got.append(bytes(memoryview(frames).cast("B")))

    def close(self):
        self.closed = True


def test_writer_wrapper_host_path(tmp_path):
    rng = np.random.default_rng(6)
    fb = formats.frame_bytes("yuv420p", 6, 4)
    assert fb == 36
    frames = rng.integers(0, 256, (5, fb)).astype(np.uint8)
    sink = _Sink()
    path = tmp_path / "a.crc"
    wr = framecrc.FrameCrcWriter(sink, str(path), "yuv420p", 6, 4, 30)
    assert not hasattr(wr, "write_device")  # the sink takes host bytes only
    wr.write(frames[:3])
    wr.write(frames[3].tobytes())
    wr.write(frames[3])  # a repeat is listed twice
    wr.write(frames[4:])
    wr.close()
    assert sink.closed and b"".join(sink.got) == frames[[0, 1, 2, 3, 3, 4]].tobytes()
    text = path.read_text()
    assert text.startswith("#tb 0: 1/30\n") and "#dimensions 0: 6x4\n" in text
    assert framecrc.parse(text) == [(36, zlib.adler32(frames[k].tobytes(), 0)) for k in (0, 1, 2, 3, 3, 4)]


def test_hashed_format():
    class R:
        def __init__(self, name):
            self.fmt = formats.fmt(name)

    assert framecrc.hashed_format(R("v210")).name == "yuv422p10le"      # what v210dec outputs
    assert framecrc.hashed_format(R("v210"), packets=True).name == "v210"  # -c copy
    assert framecrc.hashed_format(R("uyvy422")).name == "uyvy422"        # rawvideo decoding is the identity
    assert framecrc.hashed_format(R("yuv420p10le"), packets=True).name == "yuv420p10le"


def test_cli_framecrc_options(monkeypatch, capsys, tmp_path):
    from pixpath import cli
    seen = {}

    def stub(path, **kw):
        seen.clear()
        seen.update(kw, path=path)
        return {"fmt": "yuv420p", "w": 6, "h": 4, "rate": Fraction(25), "frames": [(36, 0x11), (36, 0x22)]}

    monkeypatch.setattr(framecrc, "checksums_of_file", stub)
    assert cli.main(["framecrc", "x.avi"]) == 0
    assert seen == {"path": "x.avi", "batch": 32, "seed": 0, "packets": False}
    out = capsys.readouterr().out
    assert out == framecrc.format_lines([(36, 0x11), (36, 0x22)], 6, 4, 25)
    listing = tmp_path / "l.crc"
    assert cli.main(["framecrc", "x.avi", "--seed", "0x1", "--packets", "--batch", "7", "--out", str(listing)]) == 0
    assert seen == {"path": "x.avi", "batch": 7, "seed": 1, "packets": True}
    assert capsys.readouterr().out == "" and listing.read_text() == out
    import json
    assert cli.main(["framecrc", "x.avi", "--against", str(listing)]) == 0
    assert json.loads(capsys.readouterr().out) == {"frames": 2, "equal": True}
    listing.write_text(out.replace("0x00000022", "0x00000023"))
    assert cli.main(["framecrc", "x.avi", "--against", str(listing)]) == 1
    assert json.loads(capsys.readouterr().out) == {"frames": 2, "equal": False, "frame": 1, "size": [36, 36],
                                                   "crc": ["0x00000022", "0x00000023"]}
    listing.write_text(out + "0, 2, 2, 1, 36, 0x00000033\n")
    assert cli.main(["framecrc", "x.avi", "--against", str(listing)]) == 1
    assert json.loads(capsys.readouterr().out) == {"frames": 2, "equal": False, "frames_against": 3}
