"""Plumbing the file-level GPU tests share: the writers of a Y4M clip, of a
packed (v210 / UYVY) AVI and of a CPVS canvas, the seeded SRC / PVS pair whose
luma error grows with the frame index, and the last printed JSON line."""
import json

import numpy as np

import pyoracle as po
import synth


def write_y4m(path, fmt, rate, planes):
    """The planes [N, rows, cols] of a planar clip as a Y4M file; returns the path."""
    from pixpath import io as pio
    wr = pio.Y4MWriter(str(path), fmt, planes[0].shape[2], planes[0].shape[1], rate)
    wr.write(np.ascontiguousarray(pio.join_planes(planes)))
    wr.close()
    return str(path)


def write_packed_avi(path, fourcc, w, h, rate, packets):
    """One packed frame per packet as an uncompressed AVI; returns the path."""
    from pixpath import avi
    wr = avi.AviWriter(str(path), w, h, rate, fourcc=fourcc)
    for p in packets:
        wr.write_packet(np.ascontiguousarray(p).reshape(-1))
    wr.close()
    return str(path)


def write_cpvs(path, gpu, fmt, planes, W, H, rate):
    """ops.cpvs of a planar clip onto the W x H canvas (v210 at 10 bit, UYVY at 8) as an AVI; returns the packed
    frames."""
    from pixpath import ops
    from pixpath.frames import FrameBatch
    packed = ops.cpvs(FrameBatch.from_numpy(fmt, planes, device=gpu), W, H)
    frames = packed.view(0).cpu().numpy()
    write_packed_avi(path, b"v210" if packed.fmt.name == "v210" else b"UYVY", W, H, rate, frames)
    return frames


def growing_error_pair(seed, fmt, w, h, n, error=lambda k: 3 * (k + 1)):
    """(src, pvs): n frames of seeded legal-range noise, and the same with a
    uniform error of up to +-error(k) on the luma of frame k (chroma as it is)."""
    rng = np.random.default_rng(seed)
    pf = po.FMT_BY_NAME[fmt]
    top = (1 << po.fmt_info(pf)[0]) - 1
    src = [synth.noise_frame(rng, pf, w, h) for _ in range(n)]
    pvs = []
    for k, f in enumerate(src):
        e = error(k)
        y = np.clip(f[0].astype(np.int64) + rng.integers(-e, e + 1, f[0].shape), 0, top).astype(f[0].dtype)
        pvs.append([y, f[1], f[2]])
    return src, pvs


def last_line(capsys):
    """The last line printed since capsys was last read, as JSON."""
    return json.loads(capsys.readouterr().out.strip().splitlines()[-1])
