"""Per-frame Adler-32 listings of a file (spec PP-HASH-1): what FFmpeg's
`-f framecrc` prints, from the chain's own readers and the MI355X.

A user with an FFmpeg runs `ffmpeg -i X.avi -f framecrc ref.crc` and
`cli framecrc X.avi --against ref.crc`, and two small text files say whether
FFmpeg decodes the chain's files to the frames the chain means
(INTEGRATION.md).  Inside the chain the same listing is the losslessness check
of a GPU-FFV1 AVPVS (`cli avpvs --gpu-ffv1 --framecrc a.crc`, then
`cli framecrc out.avi --against a.crc`) and a fingerprint to compare across
runs and ranks.  The checksums are computed on the device (pp_frame_adler32)
over the frames the readers put into HBM; 4 bytes a frame come back.

[EXT, unpinned] (no FFmpeg here): that framecrc starts each frame's Adler-32
from 0 (``seed``), and the listing layout below.
"""
from fractions import Fraction

from . import formats

LINE = "%d, %10d, %10d, %8d, %8d, 0x%08x"


def hashed_format(rd, packets=False):
    """The format a reader's frames are hashed in: what FFmpeg hands framecrc
    after decoding the file.  A v210 AVI is hashed as the yuv422p10le v210dec
    outputs, or with ``packets`` as its payload (the `-c copy` view); a
    uyvy422 AVI as its packed bytes (rawvideo decoding is the identity);
    everything else (FFV1, Y4M, raw) as its planar format."""
    if rd.fmt.id == formats.V210 and not packets:
        return formats.fmt("yuv422p10le")
    return rd.fmt


def _read_hashed(rd, n, device, window=None, packets=False):
    """Up to n frames of a reader as the device FrameBatch to hash, or None."""
    from . import clips
    if rd.fmt.packed and (packets or rd.fmt.id == formats.UYVY422):
        return clips.read_packets(rd, n, device)
    return clips.read_device(rd, n, device)


def checksums_of_file(path, batch=32, seed=0, packets=False):
    """PP-HASH-1 of every frame of ``path``, read with the chain's own readers
    (clips.open_clip: FFV1 AVIs decoded on the GPU, v210 / UYVY AVIs by
    io.PackedAviReader, anything else through io.open_reader), ``batch``
    frames at a time, hashed on the device from ``seed``.  Returns a dict:
    ``fmt`` (the name of the format hashed, see hashed_format), ``w``, ``h``,
    ``rate`` (a Fraction) and ``frames``: a list of (size_bytes, checksum),
    one per frame."""
    import functools

    import torch

    from . import clips, ops
    read = functools.partial(_read_hashed, packets=packets)
    with clips.clip_batches(path, max(1, int(batch)), read=read) as (rd, _, batches):
        f = hashed_format(rd, packets)
        size = formats.frame_bytes(f, rd.w, rd.h)
        outs = []
        for b in batches:
            outs.append(ops.frame_adler32(b, seed))
            # the reader may reuse its buffers on the next call
            torch.cuda.current_stream().synchronize()
        crcs = [c for o in outs for c in o.cpu().tolist()]
        return {"fmt": f.name, "w": int(rd.w), "h": int(rd.h), "rate": Fraction(rd.rate),
                "frames": [(size, int(c)) for c in crcs]}


def format_lines(frames, w, h, rate):
    """The listing of ``frames`` [(size_bytes, checksum)] as text: FFmpeg's
    framecrc layout as recalled ([EXT], unpinned) -- `#` header lines (time
    base = 1 / rate, media type, codec id, dimensions, sample aspect ratio),
    then one line per frame: stream index, dts, pts, duration, size, 0x +
    eight hex digits; frame k has dts = pts = k and duration 1."""
    r = Fraction(rate)
    out = ["#tb 0: %d/%d" % (r.denominator, r.numerator), "#media_type 0: video", "#codec_id 0: rawvideo",
           "#dimensions 0: %dx%d" % (w, h), "#sar 0: 1/1"]
    for k, (size, crc) in enumerate(frames):
        out.append(LINE % (0, k, k, 1, size, crc & 0xffffffff))
    return "\n".join(out) + "\n"


def parse(text):
    """[(size_bytes, checksum)] of a framecrc listing.  `#` lines and blank
    lines are ignored and any spacing is accepted, so FFmpeg's own listing
    (more header lines, side-data fields after the checksum) parses too."""
    frames = []
    for no, line in enumerate(text.splitlines(), 1):
        line = line.strip()
        if not line or line.startswith("#"):
            continue
        f = [v.strip() for v in line.split(",")]
        try:
            frames.append((int(f[4]), int(f[5], 16)))
        except (IndexError, ValueError):
            raise ValueError("framecrc line %d: %r" % (no, line))
    return frames


def compare(a, b):
    """The first difference of two listings [(size_bytes, checksum)], or None.
    A differing frame: {"frame": k, "a": (size, checksum), "b": (size,
    checksum)}; equal up to the shorter one's end: {"frames_a": n, "frames_b":
    m}.  Timestamps and headers play no part."""
    for k, (x, y) in enumerate(zip(a, b)):
        if tuple(x) != tuple(y):
            return {"frame": k, "a": tuple(x), "b": tuple(y)}
    if len(a) != len(b):
        return {"frames_a": len(a), "frames_b": len(b)}
    return None


def report(n, diff):
    """The JSON object `cli framecrc --against` prints."""
    if diff is None:
        return {"frames": n, "equal": True}
    out = {"frames": n, "equal": False}
    if "frame" in diff:
        out.update({"frame": diff["frame"], "size": [diff["a"][0], diff["b"][0]],
                    "crc": ["0x%08x" % diff["a"][1], "0x%08x" % diff["b"][1]]})
    else:
        out["frames_against"] = diff["frames_b"]
    return out


class FrameCrcWriter:
    """Writer wrapper (`cli avpvs --framecrc FILE`): records the checksum of
    every frame handed to the writer, in output order, repeats included, and
    writes the listing on close.  Device batches are hashed where they lie
    (ops.frame_adler32, read back once on close); host bytes with
    zlib.adler32, the same function.  The frames pass through untouched."""

    def __init__(self, inner, path, fmt, w, h, rate, seed=0):
        self.inner, self.path, self.seed = inner, path, int(seed)
        self.fmt, self.w, self.h, self.rate = formats.fmt(fmt), int(w), int(h), Fraction(rate)
        self.fb = formats.frame_bytes(self.fmt, self.w, self.h)
        self.items = []  # ints (host frames) and (device tensor, counts) in output order
        if hasattr(inner, "write_device"):
            self.write_device = self._write_device

    def write(self, frames):
        import zlib
        self.inner.write(frames)
        mv = memoryview(frames).cast("B")
        for i in range(len(mv) // self.fb):
            self.items.append(zlib.adler32(mv[i * self.fb:(i + 1) * self.fb], self.seed) & 0xffffffff)

    def _write_device(self, frames, stream=None, emit=None):
        from . import ops
        self.inner.write_device(frames, stream, emit)
        counts = [1] * frames.n if emit is None else [int(c) for c in emit]
        if any(counts):
            self.items.append((ops.frame_adler32(frames, self.seed, stream=stream), counts))

    def checksums(self):
        out, synced = [], False
        for it in self.items:
            if isinstance(it, tuple):
                if not synced:  # the checksums were enqueued on the writer's streams
                    import torch
                    torch.cuda.synchronize(it[0].device)
                    synced = True
                for c, k in zip(it[0].cpu().tolist(), it[1]):
                    out.extend([int(c)] * k)
            else:
                out.append(it)
        return out

    def close(self):
        self.inner.close()
        text = format_lines([(self.fb, c) for c in self.checksums()], self.w, self.h, self.rate)
        with open(self.path, "w") as f:
            f.write(text)
