"""clips.ReferenceWindow on CPU tensors: the resident reference frames that
`metrics_of_files` and `align_files` score against.  Every sample of every
plane of reference frame i is i, so the window can be read back against the
whole reference: after every ``extend(upto, behind)`` it shows frames first,
first + 1, ... count - 1 in that order, it has dropped nothing at or past
``behind``, ``count`` is what has been pulled and ``ended`` says that a pull
found the reference exhausted."""
import numpy as np
import pytest
import torch

from pixpath.clips import ReferenceWindow
from pixpath.frames import FrameBatch

W, H = 8, 4
SIZES = (3, 3, 2)  # the reference of 8 frames as its reader hands it over


def _batch(fmt, w, h, start, n):
    b = FrameBatch(fmt, w, h, n, device="cpu", zero=True)
    for p in range(3):
        b.view(p).copy_(torch.arange(start, start + n).reshape(n, 1, 1).to(b.planes[p].dtype).expand_as(b.view(p)))
    return b


class Source:
    """The reference's batches as an iterator that counts what it handed over."""

    def __init__(self, fmt="yuv420p", sizes=SIZES, w=W, h=H):
        self.fmt, self.w, self.h, self.sizes = fmt, w, h, list(sizes)
        self.pulled, self.batches, self.exhausted = 0, 0, False

    def __iter__(self):
        return self

    def __next__(self):
        if self.batches == len(self.sizes):
            self.exhausted = True
            raise StopIteration
        b = _batch(self.fmt, self.w, self.h, self.pulled, self.sizes[self.batches])
        self.pulled += b.n
        self.batches += 1
        return b


def _extend(win, src, upto, behind, fmt="yuv420p", w=W, h=H):
    """One call, then the four conditions; returns the batches the call pulled."""
    before = (src.batches, win.frames, win.first)
    win.extend(upto, behind)
    assert win.count == src.pulled and win.ended == src.exhausted
    if src.batches == before[0]:  # nothing appended: nothing dropped
        assert win.frames is before[1] and win.first == before[2]
    if win.frames is None:
        assert win.count == 0 and win.first == 0
        return src.batches - before[0]
    f = win.frames
    assert (f.fmt.name, f.w, f.h, f.n) == (fmt, w, h, win.count - win.first)
    assert win.first <= max(behind, before[2])  # every frame of [max(behind, first), count) is still there
    want = np.arange(win.first, win.count)
    for p in range(3):
        v = f.view(p).numpy()
        assert v.dtype == (np.uint16 if f.fmt.depth > 8 else np.uint8)
        assert v.shape == (f.n,) + tuple(f.shapes[p])
        assert (v == want.reshape(-1, 1, 1)).all(), (p, v[:, 0, 0], want)
    return src.batches - before[0]


def _window(src, scale=None, fmt=None, w=None, h=None):
    return ReferenceWindow(src, scale, fmt or src.fmt, w or src.w, h or src.h)


@pytest.mark.parametrize("step,pulls", [(1, [1, 0, 0, 1, 0, 0, 1, 0]), (2, [1, 1, 0, 1]), (5, [2])])
def test_monotone_walk(step, pulls):
    """Both arguments advance by ``step``: no pull, one pull, two pulls in one call."""
    src = Source()
    win = _window(src)
    got = []
    for upto in range(step, 8 + 1, step):
        got.append(_extend(win, src, upto, upto - step))
        assert win.count >= upto and not win.ended
    assert got == pulls


def test_behind_inside_at_the_end_and_past_the_resident_frames():
    src = Source()
    win = _window(src)
    assert _extend(win, src, 3, 0) == 1 and (win.first, win.count) == (0, 3)
    assert _extend(win, src, 4, 1) == 1 and (win.first, win.count) == (1, 6)   # inside: the tail 1, 2 is kept
    assert _extend(win, src, 7, 6) == 1 and (win.first, win.count) == (6, 8)   # at the end: replaced
    src = Source()
    win = _window(src)
    assert _extend(win, src, 3, 0) == 1
    assert _extend(win, src, 8, 7) == 2 and (win.first, win.count) == (6, 8)   # past the end: replaced, twice
    src = Source()
    win = _window(src)
    assert _extend(win, src, 8, 2) == 3 and (win.first, win.count) == (2, 8)   # trimmed once, then nothing to drop


def test_upto_past_the_clip():
    src = Source()
    win = _window(src)
    assert _extend(win, src, 20, 4) == 3
    assert win.ended and (win.first, win.count) == (4, 8)
    held = win.frames
    assert _extend(win, src, 30, 7) == 0  # the end is known: no pull, and so nothing dropped
    assert win.frames is held and win.ended and (win.first, win.count) == (4, 8)


def test_upto_at_the_clip_end_does_not_find_the_end():
    src = Source()
    win = _window(src)
    assert _extend(win, src, 8, 0) == 3 and not win.ended and win.count == 8
    assert _extend(win, src, 9, 0) == 0 and win.ended and (win.first, win.count) == (0, 8)


def test_empty_reference():
    src = Source(sizes=())
    win = _window(src)
    assert _extend(win, src, 1, 0) == 0
    assert win.frames is None and win.ended and win.count == 0
    assert _extend(win, src, 5, 3) == 0 and win.frames is None


def test_scale_callable_runs_once_per_batch():
    calls = []

    def scale(b):
        calls.append(b.n)
        first = int(b.view(0)[0, 0, 0])
        return _batch("yuv422p", 12, 6, first, b.n)
    src = Source()
    win = _window(src, scale, "yuv422p", 12, 6)
    for upto, behind in ((2, 0), (5, 1), (8, 4), (9, 4)):
        _extend(win, src, upto, behind, "yuv422p", 12, 6)
    assert calls == list(SIZES) and (win.first, win.count, win.ended) == (4, 8, True)


@pytest.mark.parametrize("fmt", ["yuv420p", "yuv422p10le"])
def test_depth(fmt):
    src = Source(fmt)
    win = _window(src)
    for upto, behind in ((1, 0), (4, 2), (8, 5), (9, 8)):
        _extend(win, src, upto, behind, fmt)
    assert (win.first, win.count, win.ended) == (5, 8, True)
    assert win.frames.planes[0].dtype == (torch.uint16 if fmt.endswith("10le") else torch.uint8)


@pytest.mark.parametrize("long_clip", [False, True], ids=["8_frames", "40_batches"])
def test_random_walk(long_clip):
    """200 non-decreasing pairs with behind <= upto: over the 8 frames in 3, 3, 2 (most calls pull nothing), and
    over 40 batches of 1 to 4 frames, where upto advances 0, 1 or 2 a call."""
    rng = np.random.default_rng(2024)
    sizes = [int(v) for v in rng.integers(1, 5, 40)] if long_clip else list(SIZES)
    src = Source(sizes=sizes)
    win = _window(src)
    upto = behind = 0
    for _ in range(200):
        upto += int(rng.integers(0, 3)) if long_clip else int(rng.random() < 0.06)
        behind = int(rng.integers(behind, upto + 1))
        _extend(win, src, upto, behind)
        assert win.ended or win.count >= upto
        assert win.first <= behind  # a non-decreasing ``behind``: all of [behind, count) is resident
    assert win.ended and win.count == sum(sizes)
