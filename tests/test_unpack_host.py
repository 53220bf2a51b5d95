"""Host side of the unpackers (no GPU): the numpy restatement of the v210 /
uyvy422 layouts against the oracle's packer and a hand-written answer,
pp_unpack_execute's argument checks, the packed AVI reader, and the reader
routing of pixpath.metrics."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import pyoracle as po
import unpack_ref
from pixpath import _native, avi, clips, formats, io as pio, metrics


def _planes(rng, w, h, n=None, depth=10):
    mx = (1 << depth) - 1
    dt = np.uint16 if depth > 8 else np.uint8
    lead = () if n is None else (n,)
    return [rng.integers(4 if depth > 8 else 0, mx - 3 if depth > 8 else mx + 1, lead + (h, c)).astype(dt)
            for c in (w, w // 2, w // 2)]


def _uyvy_pack(planes):
    Y, U, V = planes
    out = np.zeros(Y.shape[:-1] + (2 * Y.shape[-1],), np.uint8)
    out[..., 0::4], out[..., 2::4] = U, V
    out[..., 1::2] = Y
    return out


# ------------------------------------------------------------- the restatement
@pytest.mark.parametrize("w", [2, 4, 6, 8, 10, 46, 48, 50, 94])
def test_unpack_v210_inverts_the_oracle_packer(w):
    planes = _planes(np.random.default_rng(w), w, 3)  # inside v210's [4, 1019] clip
    packed = po.v210_pack(planes)
    assert packed.shape == (3, po.v210_linesize(w))
    for got, want in zip(unpack_ref.unpack_v210(packed, w), planes):
        np.testing.assert_array_equal(got, want)


def test_unpack_v210_known_answer():
    Y, U, V = [101, 202, 303, 404, 505, 606], [11, 22, 33], [711, 822, 933]
    words = [U[0] | Y[0] << 10 | V[0] << 20, Y[1] | U[1] << 10 | Y[2] << 20,
             V[1] | Y[3] << 10 | U[2] << 20, Y[4] | V[2] << 10 | Y[5] << 20]
    buf = np.array(words, "<u4").view(np.uint8).reshape(1, 16)
    y, u, v = unpack_ref.unpack_v210(buf, 6)
    assert y.tolist() == [Y] and u.tolist() == [U] and v.tolist() == [V]
    # a window: pixels 2..4 -> Y2 Y3 Y4, chroma pairs 1 and 2
    y, u, v = unpack_ref.unpack_v210(buf, 6, (2, 0, 3, 1))
    assert y.tolist() == [Y[2:5]] and u.tolist() == [U[1:3]] and v.tolist() == [V[1:3]]


def test_unpack_v210_ignores_top_bits_tail_fields_and_padding():
    rng = np.random.default_rng(5)
    for w in (2, 4, 6, 8, 10, 50):
        planes = _planes(rng, w, 3)
        packed = po.v210_pack(planes)
        want = unpack_ref.unpack_v210(packed, w)
        top = packed.copy()
        top.view("<u4")[...] |= 0xC0000000
        noisy = top.copy()
        used_fields = 2 * w  # Y + U + V samples of a line; fields past them and the padding are garbage
        fw = noisy.view("<u4")
        for f in range(used_fields, fw.shape[1] * 3):
            fw[:, f // 3] ^= np.uint32(rng.integers(1, 1024) << (10 * (f % 3)))
        assert not np.array_equal(noisy, top)
        for a in (top, noisy):
            for got, ref in zip(unpack_ref.unpack_v210(a, w), want):
                np.testing.assert_array_equal(got, ref)


def test_unpack_uyvy_known_answer():
    buf = np.array([[10, 1, 20, 2, 11, 3, 21, 4, 12, 5, 22, 6]], np.uint8)
    y, u, v = unpack_ref.unpack_uyvy(buf, 6)
    assert y.tolist() == [[1, 2, 3, 4, 5, 6]] and u.tolist() == [[10, 11, 12]] and v.tolist() == [[20, 21, 22]]
    y, u, v = unpack_ref.unpack_uyvy(buf, 6, (2, 0, 3, 1))
    assert y.tolist() == [[3, 4, 5]] and u.tolist() == [[11, 12]] and v.tolist() == [[21, 22]]


# ------------------------------------------------------------ argument checks
def _frames(data=(0x1000, 0x2000, 0x3000), ls=(256, 128, 128), fs=None):
    s = _native.pp_frames()
    for p in range(3):
        s.data[p] = data[p]
        s.linesize[p] = ls[p]
        s.frame_stride[p] = (fs or [l * 64 for l in ls])[p]
    return s


def _call(ctx, fmt, W, H, src, win, dst, n=1):
    L = _native.lib()
    return L.pp_unpack_execute(ctx, fmt, W, H, None if src is None else ctypes.byref(src), win[0], win[1], win[2],
                               win[3], None if dst is None else ctypes.byref(dst), n, None)


def test_pp_unpack_argument_checks_need_no_gpu():
    L = _native.lib()
    ctx = (ctypes.c_uint8 * 256)()  # never dereferenced: every call below is refused first
    V, U8 = formats.V210, formats.UYVY422
    src, dst = _frames(), _frames()
    whole = (0, 0, 48, 8)
    assert _call(None, V, 48, 8, src, whole, dst) == -1
    assert _call(ctx, V, 47, 8, src, (0, 0, 46, 8), dst) == -1      # odd W
    assert b"v210 needs an even width, not 47" in L.pp_last_error()
    assert _call(ctx, U8, 47, 8, src, (0, 0, 46, 8), dst) == -1
    assert _call(ctx, V, 48, 8, src, (3, 0, 8, 8), dst) == -1       # odd x
    assert b"even" in L.pp_last_error()
    assert _call(ctx, V, 48, 8, src, (42, 0, 8, 8), dst) == -1      # past the canvas in x
    assert b"exceeds" in L.pp_last_error()
    assert _call(ctx, V, 48, 8, src, (0, 4, 48, 5), dst) == -1      # ... in y
    assert _call(ctx, V, 48, 8, src, (-2, 0, 8, 8), dst) == -1
    assert _call(ctx, V, 48, 8, src, (0, -1, 8, 8), dst) == -1
    assert _call(ctx, V, 48, 8, src, (0, 0, 0, 8), dst) == -1       # w = 0
    assert _call(ctx, V, 48, 8, src, (0, 0, 8, 0), dst) == -1
    for planar in (formats.YUV422P10LE, formats.YUV422P, formats.YUV420P, 99):
        assert _call(ctx, planar, 48, 8, src, whole, dst) == -1     # planar in_fmt
        assert b"packed" in L.pp_last_error()
    assert _call(ctx, V, 50, 8, _frames(ls=(128, 0, 0)), (0, 0, 48, 8), dst) == -1   # below ceil(50/6)*16 = 144
    assert b"linesize" in L.pp_last_error()
    assert _call(ctx, V, 50, 8, _frames(ls=(146, 0, 0)), (0, 0, 48, 8), dst) == -1   # not a multiple of 4
    assert _call(ctx, U8, 48, 8, _frames(ls=(95, 0, 0)), whole, dst) == -1           # below 2 W
    assert _call(ctx, V, 48, 8, None, whole, dst) == -1                              # null src
    assert b"null" in L.pp_last_error()
    assert _call(ctx, V, 48, 8, src, whole, None) == -1
    assert _call(ctx, V, 48, 8, _frames(data=(0, 0, 0)), whole, dst) == -1
    assert _call(ctx, V, 48, 8, src, whole, dst, n=-1) == -1                          # negative nframes
    assert b"nframes" in L.pp_last_error()
    for only in ((0x1000, 0x2000, 0), (0x1000, 0, 0x3000)):                          # one chroma pointer null
        assert _call(ctx, V, 48, 8, src, whole, _frames(data=only)) == -1
        assert b"chroma" in L.pp_last_error()
    assert _call(ctx, V, 48, 8, src, whole, _frames(ls=(94, 128, 128))) == -1         # short destination rows
    assert _call(ctx, V, 48, 8, src, whole, _frames(data=(0x1001, 0x2000, 0x3000))) == -1
    # accepted geometry with nothing to do: OK without touching the context
    assert _call(ctx, V, 50, 8, _frames(ls=(144, 0, 0)), (2, 1, 47, 7), dst, n=0) == 0
    assert _call(ctx, U8, 48, 8, _frames(ls=(96, 0, 0)), whole, _frames(data=(0x1000, 0, 0)), n=0) == 0


def test_unpack_is_exported_without_an_abi_bump():
    assert "pp_unpack_execute" in _native.EXPORTS
    assert _native.lib().pp_abi_version() == 7


def test_unpack_geometry_constants():
    from pixpath import ops
    assert ops.unpack_trip_px("v210") == ops.UNPACK_LANES * ops.UNPACK_UNROLL * 6
    assert ops.unpack_trip_px("uyvy422") == ops.UNPACK_LANES * ops.UNPACK_UNROLL * 8
    src = open(os.path.join(os.path.dirname(_native.__file__), "..", "csrc", "unpack_plan.hpp")).read()
    assert "kUnpackLanes = %d;" % ops.UNPACK_LANES in src and "kUnpackUnroll = %d;" % ops.UNPACK_UNROLL in src


# ------------------------------------------------------------ PackedAviReader
def _write_avi(path, fourcc, w, h, packets, rate=Fraction(30000, 1001)):
    wr = avi.AviWriter(str(path), w, h, rate, fourcc=fourcc)
    for p in packets:
        wr.write_packet(np.ascontiguousarray(p).reshape(-1))
    wr.close()
    return str(path)


def test_packed_avi_reader_v210(tmp_path):
    w, h, n = 50, 4, 3
    planes = _planes(np.random.default_rng(1), w, h, n)
    packed = [po.v210_pack([p[k] for p in planes]) for k in range(n)]
    path = _write_avi(tmp_path / "cpvs.avi", b"v210", w, h, packed)
    rd = pio.PackedAviReader(path)
    try:
        assert (rd.fmt.name, rd.w, rd.h, rd.rate) == ("v210", w, h, Fraction(30000, 1001))
        assert rd.linesize == 256 == formats.v210_linesize(w) and rd.frame_bytes == 256 * h
        buf = np.zeros((4, rd.frame_bytes), np.uint8)
        assert rd.read_into(buf, 2) == 2 and rd.read_into(buf[2:], 2) == 1 and rd.read_into(buf, 1) == 0
    finally:
        rd.close()
    for k in range(n):
        np.testing.assert_array_equal(buf[k].reshape(h, 256), packed[k])
        for got, want in zip(unpack_ref.unpack_v210(buf[k].reshape(h, 256), w), [p[k] for p in planes]):
            np.testing.assert_array_equal(got, want)


def test_packed_avi_reader_uyvy_and_fourcc_case(tmp_path):
    w, h, n = 18, 3, 2
    planes = _planes(np.random.default_rng(2), w, h, n, depth=8)
    packed = _uyvy_pack(planes)
    for fourcc in (b"UYVY", b"uyvy"):
        rd = pio.PackedAviReader(_write_avi(tmp_path / "u.avi", fourcc, w, h, packed, rate=60))
        try:
            assert (rd.fmt.name, rd.w, rd.h, rd.rate, rd.linesize, rd.frame_bytes) == ("uyvy422", w, h, 60, 36, 108)
            buf = np.zeros((n, rd.frame_bytes), np.uint8)
            assert rd.read_into(buf, n) == n
        finally:
            rd.close()
        np.testing.assert_array_equal(buf.reshape(n, h, 36), packed)
    rd = pio.PackedAviReader(_write_avi(tmp_path / "v.avi", b"V210", 6, 2, [np.zeros((2, 128), np.uint8)]))
    assert rd.fmt.name == "v210"
    rd.close()


def test_packed_avi_reader_accepts_the_minimal_v210_stride(tmp_path):
    w, h = 50, 4
    planes = _planes(np.random.default_rng(3), w, h)
    tight = po.v210_pack(planes)[:, :144]  # ceil(50 / 6) * 16
    rd = pio.PackedAviReader(_write_avi(tmp_path / "tight.avi", b"v210", w, h, [tight, tight]))
    try:
        assert rd.linesize == 144 and rd.frame_bytes == 144 * h
        buf = np.zeros((2, rd.frame_bytes), np.uint8)
        assert rd.read_into(buf, 2) == 2
    finally:
        rd.close()
    for got, want in zip(unpack_ref.unpack_v210(buf[1].reshape(h, 144), w), planes):
        np.testing.assert_array_equal(got, want)


def test_packed_avi_reader_refusals(tmp_path):
    frame = np.zeros((4, 256), np.uint8)
    with pytest.raises(ValueError, match="whole number"):  # 1026 bytes: not 4 equal lines
        pio.PackedAviReader(_write_avi(tmp_path / "a.avi", b"v210", 50, 4, [np.zeros(1026, np.uint8)]))
    with pytest.raises(ValueError, match="line size"):     # 4 x 128 < ceil(50/6)*16
        pio.PackedAviReader(_write_avi(tmp_path / "b.avi", b"v210", 50, 4, [frame[:, :128]]))
    with pytest.raises(ValueError, match="line size"):     # uyvy below 2 W
        pio.PackedAviReader(_write_avi(tmp_path / "c.avi", b"UYVY", 50, 4, [frame[:, :96]]))
    with pytest.raises(ValueError, match="FFV1"):
        pio.PackedAviReader(_write_avi(tmp_path / "d.avi", b"FFV1", 50, 4, [frame]))
    with pytest.raises(ValueError, match="same size"):     # second packet shorter
        pio.PackedAviReader(_write_avi(tmp_path / "e.avi", b"v210", 50, 4, [frame, frame[:3]]))


def test_open_reader_is_unchanged_for_avi(monkeypatch):
    seen = []
    monkeypatch.setattr(pio, "FFmpegReader", lambda *a, **k: seen.append(a) or "ffmpeg")
    assert pio.open_reader("/x/src.avi") == "ffmpeg" and seen[0][0] == "/x/src.avi"


# ------------------------------------------------------------ metrics routing
def test_metrics_open_routes_by_fourcc(tmp_path, monkeypatch):
    from pixpath import ffv1
    frame = np.zeros((4, 256), np.uint8)
    f_ffv1 = _write_avi(tmp_path / "avpvs.avi", b"FFV1", 50, 4, [frame])
    f_v210 = _write_avi(tmp_path / "cpvs.AVI", b"v210", 50, 4, [frame])
    f_uyvy = _write_avi(tmp_path / "cpvs8.avi", b"UYVY", 50, 4, [frame[:, :100]])
    monkeypatch.setattr(ffv1, "open_avpvs_reader", lambda path, batch=None: ("ffv1", path, batch))
    monkeypatch.setattr(pio, "PackedAviReader", lambda path: ("packed", path))
    monkeypatch.setattr(pio, "open_reader", lambda path, *a, **k: ("plain", path))
    assert clips.open_clip(f_ffv1, 7) == ("ffv1", f_ffv1, 7)
    assert clips.open_clip(f_v210, 7) == ("packed", f_v210)
    assert clips.open_clip(f_uyvy, 7) == ("packed", f_uyvy)
    assert clips.open_clip("/x/src.y4m", 7) == ("plain", "/x/src.y4m")


def test_crop_window_is_the_pads_offset():
    # pad_offset (csrc/pack_plan.hpp): (outer - inner) / 2 down to the padded format's chroma grid
    assert metrics.crop_window(64, 48, 64, 36) == (0, 6, 64, 36)
    assert metrics.crop_window(64, 50, 58, 36) == (2, 7, 58, 36)            # 4:2:2: x even, y as it is
    assert metrics.crop_window(64, 50, 58, 36, "yuv420p") == (2, 6, 58, 36)  # 4:2:0: y even too
    assert metrics.crop_window(64, 50, 58, 36, "yuv420p10le") == (2, 6, 58, 36)
    with pytest.raises(ValueError):
        metrics.crop_window(64, 48, 66, 36)


def test_cli_metrics_crop_options(monkeypatch, capsys):
    from pixpath import cli
    seen = {}

    def stub(ref, dist, **kw):
        seen.clear()
        seen.update(kw)
        return metrics.summarize(np.zeros((1, 3), np.int64), np.ones((1, 3)), "yuv422p", 16, 16)

    monkeypatch.setattr(metrics, "metrics_of_files", stub)
    assert cli.main(["metrics", "--ref", "a.y4m", "--input", "c.avi", "--crop", "64x36"]) == 0
    assert seen == {"batch": 32, "flags": "bicubic", "crop": (64, 36)}
    assert cli.main(["metrics", "--ref", "a.y4m", "--input", "c.avi", "--crop", "64x36", "--avpvs-pix-fmt",
                     "yuv420p"]) == 0
    assert seen == {"batch": 32, "flags": "bicubic", "crop": (64, 36), "crop_from": "yuv420p"}
    assert cli.main(["metrics", "--ref", "a.y4m", "--input", "c.avi"]) == 0
    assert seen == {"batch": 32, "flags": "bicubic"}
    capsys.readouterr()
