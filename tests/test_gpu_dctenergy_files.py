"""PP-DCTE-1 end to end on small written clips: `dctenergy.dct_energy_of_file`
on a planar Y4M and on a v210 AVI made with the project's own writer, `cli
complexity` with and without --per-frame and with --crop, and
`complexity_main --dct-energy gpu`.  The sums are integers and the host
arithmetic is the same few float64 operations on both sides: every comparison
with the restatement (dctenergy_ref) on the decoded luma is exact."""
import json
import os

import numpy as np
import pytest

import dctenergy_ref as R
import pyoracle as po
import synth
from file_clips import write_packed_avi, write_y4m

pytestmark = pytest.mark.gpu
FMT, W, H, CW, CH, N = "yuv422p10le", 96, 70, 144, 80, 7


@pytest.fixture(scope="module")
def clip():
    rng = np.random.default_rng(71)
    frames = [synth.noise_frame(rng, po.YUV422P10LE, W, H) for _ in range(N)]
    frames[3] = [p.copy() for p in frames[2]]  # a repeated picture inside the clip
    for k in (4, 5):  # and smoother ones: less energy
        frames[k][0] = (synth.smooth_frame(k, po.YUV422P10LE, W, H)[0]).astype(np.uint16)
    luma = np.stack([f[0] for f in frames])
    rows = R.sums(luma, 10)
    return {"frames": frames, "luma": luma, "rows": rows, "pooled": R.pool(rows, W, H)}


def _v210(path, frames, w, h):
    write_packed_avi(path, b"v210", w, h, 60, [po.v210_pack(f) for f in frames])


def _same(res, pooled):
    E, T, L = pooled
    assert res["dct_energy_y"].tolist() == E and res["dct_temporal_y"].tolist() == T and res["brightness_y"].tolist() == L
    assert res["mean"] == {"dct_energy_y": float(np.mean(E)), "dct_temporal_y": float(np.mean(T)),
                           "brightness_y": float(np.mean(L))}


def test_planar_clip_across_batch_seams(gpu, clip, tmp_path):
    from pixpath import dctenergy, io as pio
    path = str(tmp_path / "src.y4m")
    write_y4m(path, FMT, 60, synth.batch(clip["frames"]))
    E, T, L = clip["pooled"]
    assert T[0] == 0.0 and T[3] == 0.0 and min(T[1:3] + T[4:]) > 0.0 and min(E) > 0.0  # frame 3 repeats frame 2
    for batch in (1, 3, 32):  # the carried prev across batch seams changes nothing
        res = dctenergy.dct_energy_of_file(path, batch=batch)
        assert (res["frames"], res["w"], res["h"], res["bitdepth"], res["blocks"]) == (N, W, H, 10, (3, 2))
        _same(res, clip["pooled"])
    rd = pio.open_reader(path)  # a full-frame reader: its luma plane is used
    _same(dctenergy.dct_energy_of_file(path, batch=4, reader=rd), clip["pooled"])
    with pytest.raises(ValueError):
        dctenergy.dct_energy_of_file(path, crop=(64, 32))  # crop is for a packed canvas


def test_v210_avi_and_cli(gpu, clip, tmp_path, capsys):
    from pixpath import cli, dctenergy
    src = str(tmp_path / "src.avi")
    _v210(src, clip["frames"], W, H)
    _same(dctenergy.dct_energy_of_file(src, batch=3), clip["pooled"])
    padded = [po.pad(po.YUV422P10LE, f, CW, CH, 24, 5) for f in clip["frames"]]  # where crop_window looks for it
    cpvs = str(tmp_path / "cpvs.avi")
    _v210(cpvs, padded, CW, CH)
    canvas = np.stack([f[0] for f in padded])
    got = dctenergy.dct_energy_of_file(cpvs, batch=4)
    assert (got["w"], got["h"], got["blocks"]) == (CW, CH, (4, 2))
    _same(got, R.pool(R.sums(canvas, 10), CW, CH))
    got = dctenergy.dct_energy_of_file(cpvs, batch=4, crop=(W, H))
    assert (got["w"], got["h"], got["frames"]) == (W, H, N)
    _same(got, clip["pooled"])
    E, T, L = clip["pooled"]
    capsys.readouterr()
    assert cli.main(["complexity", src]) == 0
    d = json.loads(capsys.readouterr().out)
    assert set(d) == {"file", "frames", "w", "h", "spec", "blocks", "dct_energy_y", "dct_temporal_y", "brightness_y"}
    assert d["dct_energy_y"] == float(np.mean(E)) and d["dct_temporal_y"] == float(np.mean(T))
    assert d["brightness_y"] == float(np.mean(L)) and d["blocks"] == [3, 2] and d["frames"] == N
    assert d["spec"] == dctenergy.SPEC and "PP-DCTE-1" in d["spec"]
    assert cli.main(["complexity", src, "--per-frame", "--batch", "2"]) == 0
    p = json.loads(capsys.readouterr().out)
    assert {k: v for k, v in p.items() if not k.endswith("_frames")} == d
    assert (p["dct_energy_y_frames"], p["dct_temporal_y_frames"], p["brightness_y_frames"]) == (E, T, L)
    assert cli.main(["complexity", cpvs, "--crop", "%dx%d" % (W, H)]) == 0
    c = json.loads(capsys.readouterr().out)
    assert {k: v for k, v in c.items() if k != "file"} == {k: v for k, v in d.items() if k != "file"}


def test_complexity_main_adds_three_columns(gpu, clip, tmp_path, monkeypatch):
    import pandas as pd
    import yaml
    from pixpath import siti
    tmp = tmp_path / "complexity"
    tmp.mkdir()
    srcs = []
    for name, frames in (("SRC801", clip["frames"][:3]), ("SRC802", clip["frames"][4:6])):
        path = str(tmp_path / (name + ".avi"))
        _v210(path, frames, W, H)
        (tmp / (name + "_crf23.avi")).write_bytes(b"encoded")  # present: nothing is encoded
        srcs.append(path)
    info = {"file_size": 500000, "video_duration": 2.0, "video_frame_rate": 60.0, "video_width": W, "video_height": H}
    monkeypatch.setattr(siti, "get_difficulty", lambda out: siti.difficulty_from_info(out, info))
    argv = ["-i"] + srcs + ["-t", str(tmp), "--siti", "none"]
    plain = open(siti.complexity_main(argv + ["-o", "plain.csv"])).read()
    lines = open(siti.complexity_main(argv + ["-o", "dct.csv", "--dct-energy", "gpu"])).read().splitlines()
    ref = plain.splitlines()
    assert lines[0] == ref[0] + ",dct_e,dct_h,dct_l"
    for a, b in zip(lines[1:], ref[1:]):
        assert a.startswith(b + ",")
    got = pd.read_csv(os.path.join(str(tmp), "dct.csv"), float_precision="round_trip").set_index("file")
    for name, sl in (("SRC801", slice(0, 3)), ("SRC802", slice(4, 6))):
        E, T, L = R.pool(R.sums(clip["luma"][sl], 10), W, H)
        row = got.loc[name + "_crf23.avi"]
        assert (row["dct_e"], row["dct_h"], row["dct_l"]) == (float(np.mean(E)), float(np.mean(T)), float(np.mean(L)))
    assert got.loc["SRC801_crf23.avi", "dct_e"] > got.loc["SRC802_crf23.avi", "dct_e"]  # noise against smooth
    # --dct-energy yaml: what analyse_src wrote, NaN where it wrote nothing; no GPU value is measured
    with open(srcs[0] + ".yaml", "w") as f:
        yaml.dump({"md5sum": "-", "dct_energy": {"dct_energy_y": 3.5, "dct_temporal_y": 0.25, "brightness_y": 90.0}}, f)
    y = pd.read_csv(siti.complexity_main(argv + ["-o", "y.csv", "--dct-energy", "yaml"]),
                    float_precision="round_trip").set_index("file")
    assert tuple(y.loc["SRC801_crf23.avi", ["dct_e", "dct_h", "dct_l"]]) == (3.5, 0.25, 90.0)
    assert np.isnan(y.loc["SRC802_crf23.avi", "dct_e"])
    assert open(siti.complexity_main(argv + ["-o", "again.csv"])).read() == plain  # the default: as before
