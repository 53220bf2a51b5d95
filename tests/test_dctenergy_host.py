"""PP-DCTE-1 on the CPU: the committed tables against the restatement and the
generator, their properties, the bounds the kernel's header comment states,
the restatement's fixed points, `pool`, the SRC-analysis hooks from precomputed
values and the command line's arguments.  No GPU."""
import contextlib
import io
import os
import re
import sys

import numpy as np
import pytest

import dctenergy_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "processing-chain_amd", "csrc", "dct32_tables.hpp")
ABSENT = (1 << 64) - 1


def _table(text, name):
    body = re.search(r"%s\[32\]\[32\] = \{(.*?)\n\};" % name, text, re.S).group(1)
    return np.array([int(v) for v in re.findall(r"-?\d+", body)], dtype=np.int64).reshape(32, 32)


@pytest.fixture(scope="module")
def tables():
    text = open(HEADER).read()
    return _table(text, "kDct32C"), _table(text, "kDct32W")


def _generator():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_dct32_tables as g
    finally:
        sys.path.pop(0)
    return g


def test_committed_tables_equal_the_restatement_and_the_generator(tables):
    C, W = tables
    assert np.array_equal(C, R.C) and np.array_equal(W, R.W)
    g = _generator()
    assert g.header_text() == open(HEADER).read()
    assert np.array_equal(np.array(g.coefficients()), C) and np.array_equal(np.array(g.weights()), W)


def test_table_properties(tables):
    C, W = tables
    assert np.abs(C).max() <= 4096 and (C[0] == 2896).all()
    sign = np.where(np.arange(32) % 2, -1, 1)[:, None]
    assert np.array_equal(C[:, ::-1], sign * C)              # C[k][31 - n] = (-1)^k C[k][n]
    assert np.array_equal(W, W.T) and W.max() == 696 and W.min() >= 256
    assert W[0, 0] == 696 and W[31, 31] == R.W[31, 31]
    # 2^14 times an orthonormal matrix: C C^T = 2^28 I within the rounding: an entry is off by at most 1/2, so a
    # product of two rows by at most 2 * 32 * 4096 / 2 + 32 / 4
    err = np.abs(C @ C.T - (1 << 28) * np.eye(32, dtype=np.int64))
    assert err.max() <= 32 * 4096 + 8, err.max()


def test_bounds_of_the_kernel_header(tables):
    """The numbers csrc/dctenergy.hip states under Exactness, from the committed table."""
    C, W = tables
    rows = np.abs(C).sum(axis=1)
    assert rows.max() == 92672 and rows.argmax() == 0
    t10 = (92672 * 1023 + (1 << 13)) >> 14
    t8 = (92672 * 255 + (1 << 11)) >> 12
    assert (t10, t8) == (5786, 5769) and 92672 * 1023 < 1 << 27
    assert 2 * 1023 < 1 << 11 and 2 * t10 == 11572 and 2 * t10 < 1 << 14   # the folded operands: 24 signed bits by far
    assert 92672 * t10 + (1 << 13) < 1 << 29
    y = (92672 * t10 + (1 << 13)) >> 14
    assert y == 32727
    assert 696 * y < 1 << 25 and 32 * 696 * y < 1 << 30 and 1024 * 696 * y < 1 << 35
    # and what the restatement meets on the probes that drive single coefficients as high as they go
    seen = {}
    for depth in (8, 10):
        top = (1 << depth) - 1
        for l, k in ((1, 1), (31, 31), (0, 31), (0, 0)):
            R.transform(np.where(np.outer(C[l], C[k]) > 0, top, 0), depth, seen)
    assert seen["racc"] <= 92672 * 1023 + (1 << 13) < 1 << 27 and seen["t"] <= t10 and seen["cacc"] < 1 << 29 and seen["y"] <= y


@pytest.mark.parametrize("depth", [8, 10])
def test_constant_plane(depth):
    """Energy exactly 0 (the rows of the committed C other than row 0 sum to 0
    exactly), and dc = nb * 128 * the value v on the 8-bit scale within the
    table's rounding: C[0][n] = 2896 is 4096 / sqrt 2 rounded, so a block's dc
    is 92672^2 v / 2^26 = 127.974 v, off 128 v by 0.0262 v, plus the two
    roundings' 92672 / 2^15 + 1 / 2 < 3.33.  Exact equality with 128 v cannot
    hold with the committed 2896: v = 1 gives 130, v = 255 gives 32631."""
    assert [int(r.sum()) for r in R.C[1:]] == [0] * 31
    for v8 in (0, 1, 16, 128, 235, 255):
        v = v8 << (depth - 8)
        a = np.full((2, 70, 100), v, np.uint16)
        rows = R.sums(a, depth, None, a[0])
        assert rows[0] == rows[1] and rows[0][0] == 0 and rows[0][2] == 0
        assert rows[0][1] % 6 == 0 and abs(rows[0][1] // 6 - 128 * v8) <= 0.0262 * v8 + 3.33
        E, T, L = R.pool(rows, 100, 70)
        assert E == [0.0, 0.0] and T == [0.0, 0.0] and L[0] == L[1] and abs(L[0] - v8) <= (0.0262 * v8 + 3.33) / 128
    assert R.sums(np.full((1, 32, 32), 16, np.uint8), 8)[0][1] == 128 * 16     # where the roundings cancel
    assert R.sums(np.full((1, 32, 32), 1, np.uint8), 8)[0][1] == 130 and R.sums(np.full((1, 32, 32), 1020, np.uint16), 10)[0][1] == 32631


def test_ten_bit_twin_gives_identical_outputs():
    rng = np.random.default_rng(5)
    a8 = rng.integers(0, 256, (3, 64, 96)).astype(np.uint16)
    a10 = a8 << 2
    assert R.sums(a8, 8, [0, 1, 1, 2], a8[2]) == R.sums(a10, 10, [0, 1, 1, 2], a10[2])
    assert R.blocks(a8, 8) == R.blocks(a10, 10)
    e, dc = R.frame(a8[0], 8)
    assert e.shape == (2, 3) and min(e.ravel()) > 0
    assert R.sums(a8, 8)[0][2] == ABSENT and R.sums(a8[:, :31], 8) == [[ABSENT] * 3] * 3
    big = rng.integers(0, 65536, (1, 32, 32))  # the clamp of the 16-bit container
    assert R.sums(big, 10) == R.sums(np.minimum(big, 1023), 10)


def test_pool():
    from pixpath import dctenergy as D
    w, h = 100, 70  # 3 x 2 blocks
    rows = [[6 << 20, 6 * 128 * 100, ABSENT], [3 << 20, 6 * 128 * 50, 9 << 19], [0, 0, 3 << 20]]
    E, T, L = D.pool(rows, w, h)
    assert E.tolist() == [1.0, 0.5, 0.0] and T.tolist() == [0.0, 0.75, 0.5] and L.tolist() == [100.0, 50.0, 0.0]
    assert (E.dtype, T.dtype, L.dtype) == (np.float64,) * 3
    rE, rT, rL = R.pool(rows, w, h)
    assert (E.tolist(), T.tolist(), L.tolist()) == (rE, rT, rL)
    a = np.array(rows, dtype=np.uint64)
    for arr in (a, a.view(np.int64)):
        got = D.pool(arr, w, h)
        assert [g.tolist() for g in got] == [E.tolist(), T.tolist(), L.tolist()]
    assert np.isnan(D.pool(rows, w, h, first=False)[1][0])
    none = D.pool([[ABSENT] * 3] * 2, 20, 20)        # no block: everything absent, h_0 included
    assert all(np.isnan(v).all() for v in none)
    assert [v.shape for v in D.pool(np.zeros((0, 3), np.uint64), w, h)] == [(0,)] * 3
    with pytest.raises(ValueError):
        D.pool(np.zeros((2, 3), np.float64), w, h)
    res = D.summarize(rows, w, h)
    assert res["mean"] == {"dct_energy_y": 0.5, "dct_temporal_y": (0.75 + 0.5) / 3, "brightness_y": 50.0}
    res.update({"frames": 3, "w": w, "h": h, "bitdepth": 8, "blocks": D.geometry(w, h)})
    rep = D.report(res, "/some/dir/clip.y4m", per_frame=True)
    assert rep["file"] == "clip.y4m" and rep["blocks"] == [3, 2] and "PP-DCTE-1" in rep["spec"]
    assert "VCA" in rep["spec"] and "unpinned" in rep["spec"]
    assert rep["dct_energy_y_frames"] == [1.0, 0.5, 0.0] and rep["brightness_y"] == 50.0
    assert not [k for k in D.report(res, "clip.y4m") if k.endswith("_frames")]


def _analyse(tmp_path, **kw):
    import yaml
    from pixpath import siti
    f = tmp_path / "SRC900.avi"
    f.write_bytes(b"not a video")
    with contextlib.redirect_stdout(io.StringIO()):
        yp = siti.analyse_src(str(f), 1, with_siti=False, src_info={"r_frame_rate": "60", "width": 64, "height": 64},
                              stream_sizes={"v": 11, "a": 0}, **kw)
    text = open(yp).read()
    return text, yaml.safe_load(text)


def test_analyse_src_key(tmp_path):
    from pixpath import dctenergy as D
    base_text, base = _analyse(tmp_path)
    assert "dct_energy" not in base                                   # off by default
    vals = {"dct_energy_y": np.array([1.5, 2.5]), "dct_temporal_y": np.array([0.0, 0.25]),
            "brightness_y": np.array([100.0, 101.0]), "bitdepth": 10}
    text, d = _analyse(tmp_path, with_dct_energy=True, dct_energy=vals)
    e = d.pop("dct_energy")
    assert d == base                                                  # the key is all that was added
    assert e == {"dct_energy_y": 2.0, "dct_temporal_y": 0.125, "brightness_y": 100.5,
                 "dct_energy_y_frames": [1.5, 2.5], "dct_temporal_y_frames": [0.0, 0.25],
                 "brightness_y_frames": [100.0, 101.0], "bitdepth": 10, "spec": D.SPEC}
    from pixpath import siti
    assert siti.dct_energy_from_yaml(str(tmp_path / "SRC900.avi")) == (2.0, 0.125, 100.5)
    _analyse(tmp_path)
    assert siti.dct_energy_from_yaml(str(tmp_path / "SRC900.avi")) is None
    assert siti.dct_energy_from_yaml(str(tmp_path / "absent.avi")) is None


def test_complexity_parse_args_defaults():
    from pixpath import siti
    a = siti.complexity_parse_args(["-i", "x.avi"], script_dir="/some/util")
    assert a.dct_energy == "none" and a.siti == "yaml"
    for v in ("none", "yaml", "gpu"):
        assert siti.complexity_parse_args(["-i", "x.avi", "--dct-energy", v], script_dir="/some/util").dct_energy == v
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        siti.complexity_parse_args(["-i", "x.avi", "--dct-energy", "cpu"], script_dir="/some/util")


def test_cli_arguments(monkeypatch):
    from pixpath import cli
    seen = []
    monkeypatch.setattr(cli, "cmd_complexity", lambda args: seen.append(args) or 0)
    assert cli.main(["complexity", "clip.y4m"]) == 0
    a = seen[-1]
    assert (a.input, a.per_frame, a.crop, a.avpvs_pix_fmt, a.batch) == ("clip.y4m", False, None, None, 32)
    assert cli.main(["complexity", "c.avi", "--per-frame", "--crop", "64x36", "--avpvs-pix-fmt", "yuv420p", "--batch", "5"]) == 0
    a = seen[-1]
    assert (a.input, a.per_frame, a.crop, a.avpvs_pix_fmt, a.batch) == ("c.avi", True, "64x36", "yuv420p", 5)
    assert cli._crop_settings(a) == {"crop": (64, 36), "crop_from": "yuv420p"}
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        cli.main(["complexity"])
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        cli.main(["complexity", "clip.y4m", "--window", "9"])
