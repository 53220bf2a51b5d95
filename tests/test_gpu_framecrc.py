"""pp_frame_adler32 / ops.frame_adler32 on the GPU (spec PP-HASH-1) against
zlib.adler32 over the frame's byte string (framecrc_ref): every comparison is
==.  The shapes are the smallest at which the kernel can still be wrong: planes
shorter than a lane, the 16-B tail, the wave and band seams, unaligned and
padded layouts, packed row extents, many frames, start values, and the sizes
at which each accumulation level would overflow.  Then the two commands
through files."""
import ctypes
import json
import zlib
from fractions import Fraction

import numpy as np
import pytest

import framecrc_ref
import pyoracle as po
import synth

pytestmark = pytest.mark.gpu


def _make(gpu, fmt, w, h, n=2, seed=0, layout="std", fill=None):
    """A FrameBatch of n frames and its planes as numpy [n, rows, >= cols]
    views.  Layouts: std (pitch rounded up to 16 B), dense (pitch = row),
    view (a window of a wider, taller tensor, everything on the 16-B grid),
    view_odd (the same off the grid).  All padding holds random bytes."""
    import torch
    from pixpath import formats
    from pixpath.frames import FrameBatch
    f = formats.fmt(fmt)
    rng = np.random.default_rng(seed)
    es = 1 if f.packed else f.bytes_per_sample
    dt = np.uint16 if es == 2 else np.uint8
    tens, arrs = [], []
    for rows, cols in formats.plane_shapes(f, w, h):
        p16 = (cols * es + 15) // 16 * 16 // es
        R, C, x0, y0 = {"std": (rows, p16, 0, 0), "dense": (rows, cols, 0, 0),
                        "view": (rows + 5, p16 + 32 // es, 16 // es, 2),
                        "view_odd": (rows + 3, cols + 7, 3, 1)}[layout]
        big = rng.integers(0, 1 << (8 * es), (n, R, C)).astype(dt) if fill is None else np.full((n, R, C), fill, dt)
        t = torch.from_numpy(big).to(gpu)
        tens.append(t[:, y0:y0 + rows, x0:])
        arrs.append(big[:, y0:y0 + rows, x0:])
    return FrameBatch(f, w, h, n, planes=tens), arrs


def _want(fmt, w, h, arrs, init=0):
    return [framecrc_ref.adler32(fmt, w, h, [a[k] for a in arrs], init) for k in range(arrs[0].shape[0])]


def _check(gpu, fmt, w, h, init=0, **kw):
    from pixpath import ops
    b, arrs = _make(gpu, fmt, w, h, **kw)
    got = ops.frame_adler32(b, init).cpu().tolist()
    want = _want(fmt, w, h, arrs, init)
    print(fmt, w, h, kw, ["%08x" % v for v in got[:4]], ["%08x" % v for v in want[:4]])
    assert got == want
    return b, arrs, got


@pytest.mark.parametrize("fmt,w,h", [("yuv444p", 1, 1), ("yuv420p", 2, 2), ("yuv422p10le", 2, 1), ("yuv420p10le", 1, 1),
                                      ("yuv444p10le", 3, 2)])
def test_planes_shorter_than_a_lane(gpu, fmt, w, h):
    for layout in ("std", "dense", "view", "view_odd"):
        _check(gpu, fmt, w, h, layout=layout, seed=w)


@pytest.mark.parametrize("w", [15, 16, 17, 31, 33])
def test_the_16_byte_tail(gpu, w):
    _check(gpu, "yuv420p", w, 3, seed=w)
    _check(gpu, "yuv420p", w, 3, seed=w, layout="view")
    _check(gpu, "yuv444p10le", w, 3, seed=w)  # 2 w bytes: 30 .. 66


def test_the_wave_seam(gpu):
    from pixpath import ops
    span = ops.CRC_LANES * ops.CRC_LANE_BYTES  # bytes of a row one wave covers per trip
    assert span == 1024
    for rowbytes in (span - 1, span, span + 1, 2 * span - 1, 2 * span, 2 * span + 1):
        _check(gpu, "yuv444p", rowbytes, 2, seed=rowbytes)
    for rowbytes in (span - 2, span, span + 2):
        _check(gpu, "yuv444p10le", rowbytes // 2, 2, seed=rowbytes)


def test_the_band_and_wave_row_seams(gpu):
    from pixpath import ops
    band, rows = ops.CRC_BAND_ROWS, ops.CRC_WAVE_ROWS
    for h in (rows - 1, rows, rows + 1, band - 1, band, band + 1, 2 * band + 1):
        _check(gpu, "yuv444p", 20, h, seed=h)
    _check(gpu, "yuv420p", 20, 2 * band + 1, seed=1)  # chroma one row past a band


def test_unaligned_dense_rows_equal_the_aligned_path(gpu):
    from pixpath import ops
    from pixpath.frames import FrameBatch
    fmt, w, h = "yuv422p", 333, 97
    dense, arrs, got = _check(gpu, fmt, w, h, layout="dense", seed=5)
    assert dense.planes[0].stride(1) == 333 and dense.planes[1].stride(1) == 167
    aligned = FrameBatch.from_numpy(fmt, [a[:, :, :c] for a, (r, c) in zip(arrs, dense.shapes)], device=gpu)
    assert aligned.planes[0].stride(1) % 16 == 0
    assert ops.frame_adler32(aligned).cpu().tolist() == got
    _check(gpu, "yuv422p10le", 333, 97, layout="dense", seed=6)   # rows off the 16-B grid, 2-byte samples
    _check(gpu, "yuv420p", 1100, 3, layout="view_odd", seed=7)    # two trips on the byte path


def test_padding_is_never_hashed(gpu):
    from pixpath import ops
    fmt, w, h = "yuv422p10le", 70, 37
    b, arrs, got = _check(gpu, fmt, w, h, layout="view", seed=8, n=3)
    t = b.planes[0]
    assert t.stride(0) != t.shape[1] * t.stride(1) and t.stride(1) > w  # frame stride != rows x pitch
    assert (t.data_ptr() | t.stride(1) * 2 | t.stride(0) * 2) % 16 == 0  # the 16-B load path
    _, _, other = _check(gpu, fmt, w, h, layout="view_odd", seed=8, n=3)  # other pixels: seeded alike, laid out otherwise
    # new padding around the same pixels: the same checksums
    b2, arrs2 = _make(gpu, fmt, w, h, layout="view", seed=9, n=3)
    for p, (rows, cols) in enumerate(b.shapes):
        b2.planes[p][:, :rows, :cols].copy_(b.planes[p][:, :rows, :cols])
    assert ops.frame_adler32(b2).cpu().tolist() == got


@pytest.mark.parametrize("fmt,w", [("uyvy422", 2), ("uyvy422", 6), ("uyvy422", 50), ("v210", 2), ("v210", 6),
                                    ("v210", 46), ("v210", 48), ("v210", 50)])
def test_packed_row_extents(gpu, fmt, w):
    from pixpath import formats
    for layout in ("std", "view", "view_odd"):  # view*: a linesize larger than the row
        b, _, _ = _check(gpu, fmt, w, 3, layout=layout, seed=w)
        if fmt == "v210" and layout != "std":
            assert b.planes[0].stride(1) > formats.v210_linesize(w)
    if fmt == "v210":
        assert formats.v210_linesize(w) == (128 if w <= 48 else 256)


def test_600_frames(gpu):
    _, _, got = _check(gpu, "yuv420p", 8, 8, n=600, seed=11)
    assert len(set(got)) == 600


def test_start_values(gpu):
    from pixpath import ops
    from pixpath.frames import FrameBatch
    fmt, w, h = "yuv420p", 50, 21
    b, arrs = _make(gpu, fmt, w, h, n=4, seed=12)
    for init in (0, 1, 0xFFF0FFF0, 0xFFFFFFFF, int(np.random.default_rng(13).integers(0, 1 << 32))):
        assert ops.frame_adler32(b, init).cpu().tolist() == _want(fmt, w, h, arrs, init)
    # frame k seeded with the checksum of frames 0 .. k-1: zlib over the concatenation
    run, cat = 1, b""
    for k in range(4):
        one = FrameBatch(fmt, w, h, 1, planes=[t[k:k + 1] for t in b.planes])
        run = int(ops.frame_adler32(one, run).cpu()[0])
        cat += framecrc_ref.frame_string(fmt, w, h, [a[k] for a in arrs])
        assert run == zlib.adler32(cat) & 0xffffffff


@pytest.mark.parametrize("fmt,w,h,fill", [
    ("yuv422p", 1920, 1080, 0xFF),          # a 32-bit sum across rows fails here
    ("yuv422p10le", 3840, 2160, 0xFFFF),    # 33 MB, the largest product frame: a late mod fails here
    ("yuv422p", 1920, 1080, None),
    ("yuv422p10le", 3840, 2160, None),
])
def test_no_accumulation_level_overflows(gpu, fmt, w, h, fill):
    _check(gpu, fmt, w, h, n=1, fill=fill, seed=14)


def test_v210_1080p_packet_of_ff(gpu):
    _check(gpu, "v210", 1920, 1080, n=1, fill=0xFF)


def test_no_frames_and_a_stream_of_its_own(gpu):
    import torch
    from pixpath import _native, ops
    from pixpath.frames import FrameBatch
    fmt, w, h = "yuv422p", 40, 9
    b, arrs = _make(gpu, fmt, w, h, n=3, seed=15)
    out = torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
    s = b.frames_struct()
    L = _native.lib()
    assert L.pp_frame_adler32(ops.context(gpu).handle, b.fmt.id, w, h, ctypes.byref(s), 0, 0,
                              ctypes.c_void_p(out.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [0x5A5A5A5A] * 3  # nothing written
    empty = ops.frame_adler32(FrameBatch(fmt, w, h, 0, device=gpu))
    assert tuple(empty.shape) == (0,) and empty.dtype == torch.uint32
    st = torch.cuda.Stream(gpu)
    got = ops.frame_adler32(b, 1, stream=st)
    st.synchronize()
    assert got.dtype == torch.uint32 and got.device.type == "cuda"
    assert got.cpu().tolist() == _want(fmt, w, h, arrs, 1)
    got = ops.frame_adler32(b, 1, stream=st.cuda_stream)  # a raw hipStream_t
    st.synchronize()
    assert got.cpu().tolist() == _want(fmt, w, h, arrs, 1)


# ------------------------------------------------------------------ through files
def _write_y4m(path, fmt, frames, w, h, rate):
    from pixpath import io as pio
    wr = pio.Y4MWriter(str(path), fmt, w, h, rate)
    wr.write(pio.join_planes(synth.batch(frames)))
    wr.close()
    return str(path)


@pytest.fixture(scope="module")
def avpvs(gpu, tmp_path_factory):
    """A GPU-FFV1 AVPVS of 64x48 yuv422p10le at 60 fps from a dozen 48x36
    frames at 25 fps (frames repeat), written with --framecrc; the oracle's
    scaled frames in output order."""
    from pixpath import cli
    d = tmp_path_factory.mktemp("framecrc")
    src = [synth.smooth_frame(t, po.YUV420P, 48, 36) for t in range(12)]
    seg = _write_y4m(d / "seg.y4m", "yuv420p", src, 48, 36, 25)
    out, crc = str(d / "out.avi"), str(d / "a.crc")
    assert cli.main(["avpvs", "-y", "--input", seg, "--size", "64x48", "--pix-fmt", "yuv422p10le", "--fps", "60",
                     "--aopts=-an", "--gpu-ffv1", "--ffv1-slices", "2x2", "--batch", "5", "--framecrc", crc, out]) == 0
    m = po.fps_map(12, 25, 60)
    scaled = [po.scale(po.YUV420P, f, po.YUV422P10LE, 64, 48, po.SWS_BICUBIC) for f in src]
    assert len(m) > 12 and len(set(m.tolist())) == 12
    return {"dir": d, "avi": out, "crc": crc, "frames": [scaled[k] for k in m]}


def test_avpvs_listing_is_the_oracles_frames(avpvs):
    from pixpath import framecrc
    text = open(avpvs["crc"]).read()
    assert text.startswith("#tb 0: 1/60\n") and "#dimensions 0: 64x48\n" in text
    want = [(64 * 48 * 2 * 2, framecrc_ref.adler32("yuv422p10le", 64, 48, f)) for f in avpvs["frames"]]
    got = framecrc.parse(text)
    print(len(got), got[:3], want[:3])
    assert got == want


def test_round_trip_of_a_gpu_ffv1_avpvs(avpvs, capsys):
    from pixpath import cli, framecrc
    capsys.readouterr()
    assert cli.main(["framecrc", avpvs["avi"], "--against", avpvs["crc"], "--batch", "7"]) == 0
    assert json.loads(capsys.readouterr().out) == {"frames": len(avpvs["frames"]), "equal": True}
    assert cli.main(["framecrc", avpvs["avi"]]) == 0
    assert capsys.readouterr().out == open(avpvs["crc"]).read()  # the same listing, header included
    res = framecrc.checksums_of_file(avpvs["avi"], seed=1)
    assert (res["fmt"], res["w"], res["h"], res["rate"]) == ("yuv422p10le", 64, 48, Fraction(60))
    assert [c for _, c in res["frames"]] == [framecrc_ref.adler32("yuv422p10le", 64, 48, f, 1) for f in avpvs["frames"]]
    # one checksum flipped in a copy: exit 1, and the frame is named
    lines = open(avpvs["crc"]).read().splitlines()
    k = 7
    row = lines[5 + k]
    lines[5 + k] = row[:-1] + ("0" if row[-1] != "0" else "1")
    bad = str(avpvs["dir"] / "bad.crc")
    open(bad, "w").write("\n".join(lines) + "\n")
    assert cli.main(["framecrc", avpvs["avi"], "--against", bad]) == 1
    d = json.loads(capsys.readouterr().out)
    assert d["equal"] is False and d["frame"] == k and d["crc"][0] == row[-10:] and d["crc"][1] != row[-10:]


def test_host_writer_lists_the_same_frames(avpvs, gpu):
    """The same pass into a Y4M (host bytes, zlib on the writer's side)."""
    from pixpath import cli, framecrc
    d = avpvs["dir"]
    out, crc = str(d / "out.y4m"), str(d / "host.crc")
    assert cli.main(["avpvs", "-y", "--input", str(d / "seg.y4m"), "--size", "64x48", "--pix-fmt", "yuv422p10le",
                     "--fps", "60", "--batch", "5", "--framecrc", crc, out]) == 0
    assert open(crc).read() == open(avpvs["crc"]).read()
    assert framecrc.checksums_of_file(out)["frames"] == framecrc.parse(open(crc).read())


def test_v210_cpvs_packets_and_decoded(avpvs, gpu, capsys):
    from pixpath import avi, cli, framecrc
    d = avpvs["dir"]
    raw = str(d / "cpvs.raw")
    assert cli.main(["cpvs", "-y", "--input", avpvs["avi"], "--fps", "60", "--vcodec", "v210", "--pix-fmt",
                     "yuv422p10le", "--pad", "64x60", "--gpu-ffv1", raw]) == 0
    ls = po.v210_linesize(64)
    packets = np.fromfile(raw, np.uint8).reshape(-1, 60 * ls)
    assert packets.shape[0] == len(avpvs["frames"])
    path = str(d / "cpvs.avi")
    wr = avi.AviWriter(path, 64, 60, 60, fourcc=b"v210")
    for p in packets:
        wr.write_packet(np.ascontiguousarray(p))
    wr.close()
    padded = [po.pad(po.YUV422P10LE, f, 64, 60, 0, 6) for f in avpvs["frames"]]
    want_packets = [(60 * ls, zlib.adler32(po.v210_pack(f).tobytes(), 0) & 0xffffffff) for f in padded]
    res = framecrc.checksums_of_file(path, packets=True, batch=9)
    assert res["fmt"] == "v210" and res["frames"] == want_packets
    want_planes = [(64 * 60 * 2 * 2, framecrc_ref.adler32("yuv422p10le", 64, 60, f)) for f in padded]
    res = framecrc.checksums_of_file(path, batch=9)
    assert res["fmt"] == "yuv422p10le" and res["frames"] == want_planes
    capsys.readouterr()
    assert cli.main(["framecrc", path, "--packets"]) == 0
    assert framecrc.parse(capsys.readouterr().out) == want_packets


def test_uyvy_avi_is_hashed_as_its_packed_bytes(gpu, tmp_path):
    from pixpath import avi, framecrc
    rng = np.random.default_rng(21)
    packets = rng.integers(0, 256, (4, 10, 36)).astype(np.uint8)
    path = str(tmp_path / "u.avi")
    wr = avi.AviWriter(path, 18, 10, 30, fourcc=b"UYVY")
    for p in packets:
        wr.write_packet(np.ascontiguousarray(p).reshape(-1))
    wr.close()
    res = framecrc.checksums_of_file(path, batch=3)
    assert (res["fmt"], res["rate"]) == ("uyvy422", Fraction(30))
    assert res["frames"] == [(360, zlib.adler32(p.tobytes(), 0) & 0xffffffff) for p in packets]
