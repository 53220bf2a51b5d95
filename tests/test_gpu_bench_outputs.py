"""bench.py --dump-outputs and the plain / --full split, on a tiny batch.

One plain bench run (3 PVSes of 20 frames, 2 timed steps) dumps its outputs;
the dumped AVPVS sample must equal the oracle's scaler on the regenerated
seeded inputs bit for bit, the dumped SI/TI the numpy reference within 1e-4
relative (the tolerances of tests/test_gpu_scale.py and tests/test_gpu_siti.py),
and the line holds no figure that needs a run of its own.  Further tiny runs
show that --full brings the side measurements back and that the config4 and
ffv1 workloads dump their outputs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--pvs-total", "3", "--pool", "2", "--frames", "20"]
FULL_ONLY = ("pcie_pipeline", "siti_file", "e2e_avpvs")


def _bench(d, *args):
    """One bench.py run dumping into d: (result line, {name: array})."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PIXPATH_")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args) + ["--dump-outputs", d], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    return line, {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _check_arrays(arrays):
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert all(np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    return _bench(str(tmp_path_factory.mktemp("dump")), *ARGS)


def test_plain_line_is_lean(plain_run):
    line, _ = plain_run
    assert line["steps"] == 2 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert abs(line["value"] - 3 * 20 / (line["ms_per_step"] / 1000.0)) <= 0.01 * line["value"]
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "u16"
    assert line["cpu_baseline"] is None
    for k in FULL_ONLY:
        assert k not in line, k


def test_dump_is_float_and_small(plain_run):
    _, arrays = plain_run
    assert {"si", "ti"} <= set(arrays)
    _check_arrays(arrays)


def test_full_adds_the_side_measurements(tmp_path):
    """--full on the same tiny batch (the 600-frame e2e and the CPU baseline
    switched off by their own options): the PCIe pipeline line is back."""
    line, arrays = _bench(str(tmp_path), *(ARGS + ["--full", "--no-e2e", "--no-cpu-baseline", "--no-siti-file"]))
    assert line["pcie_pipeline"]["frames_per_s"] > 0
    assert "e2e_avpvs" not in line and "siti_file" not in line and line["cpu_baseline"] is None
    assert arrays["si"].shape == (3, 20)


def test_config4_plain_and_full(tmp_path):
    """config 4: the canvas chain is timed only with --full; both runs dump
    the same composed stall frames (the dump is taken before the chain runs)."""
    args = ["--workload", "config4", "--frames", "8", "--steps", "2", "--warmup", "1"]
    plain, pa = _bench(str(tmp_path / "plain"), *args)
    full, fa = _bench(str(tmp_path / "full"), *(args + ["--full"]))
    assert plain["canvas_chain"] is None and plain["steps"] == 2 and plain["ms_per_step"] > 0
    assert full["canvas_chain"]["avg_launch_ms"] > 0
    _check_arrays(pa)
    assert pa["stall_plane0"].shape == (8, 64, 1920) and pa["stall_plane1"].shape == (8, 64, 960)
    assert sorted(pa) == sorted(fa) and all(np.array_equal(pa[k], fa[k]) for k in pa)


def test_ffv1_plain_and_full(tmp_path):
    """ffv1: decode / concurrent / writer lanes only with --full; the dumped
    packets are the same in both runs and the sizes add up to the bytes."""
    args = ["--workload", "ffv1", "--frames", "8", "--steps", "1", "--warmup", "1", "--ffv1-concurrent", "2"]
    plain, pa = _bench(str(tmp_path / "plain"), *args)
    full, fa = _bench(str(tmp_path / "full"), *(args + ["--full", "--no-cpu-baseline"]))
    for k in ("decode", "concurrent", "writer_lanes"):
        assert k not in plain, k
    assert plain["ms_per_step"] > 0 and plain["value"] > 0
    assert full["decode"]["lossless"] is True and full["concurrent"]["lossless"] is True
    assert "writer_lanes" in full and full["config"] == plain["config"]
    _check_arrays(pa)
    assert pa["packet_sizes"].shape == (8,) and (pa["packet_sizes"] > 0).all()
    assert pa["packet_bytes"].size == min(int(pa["packet_sizes"].sum()), 4 << 20)
    assert sorted(pa) == sorted(fa) and all(np.array_equal(pa[k], fa[k]) for k in pa)


def test_dump_equals_the_oracle(plain_run, gpu, oracle):
    import siti_ref
    _, arrays = plain_run
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    po = oracle
    wl = bench.WORKLOADS["config2"]
    # bench.main: PVS i reads pool[i % 2], pool[j] seeded 910 + j; the two output
    # buffers hold the last PVS written to each: PVS002 (slot 0), PVS001 (slot 1)
    assert arrays["si"].shape == (3, 20) and arrays["ti"].shape == (3, 19)  # TI from the second frame on
    for pid, j in (("PVS002", 0), ("PVS001", 1)):
        src, luma = bench.make_inputs(wl, 20, 910 + j, gpu)
        planes = src.to_numpy()
        frames = arrays["avpvs_%s_frames" % pid].astype(int)
        assert frames[0] == 0 and frames[-1] == 19
        for k, f in enumerate(frames):
            ref = po.scale(po.YUV422P10LE, [p[f] for p in planes], po.YUV422P10LE, 1920, 1080, po.SWS_LANCZOS)
            for p in range(3):
                rows = arrays["avpvs_%s_rows%d" % (pid, p)].astype(int)
                got = arrays["avpvs_%s_plane%d" % (pid, p)][k]
                assert np.array_equal(got, ref[p][rows].astype(np.float32)), (pid, f, p)
        rsi, rti = siti_ref.siti(luma.cpu().numpy())
        i = int(pid[3:])
        np.testing.assert_allclose(arrays["si"][i], rsi, rtol=1e-4)
        np.testing.assert_allclose(arrays["ti"][i], rti[1:], rtol=1e-4)
