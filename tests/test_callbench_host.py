"""tools/callbench.py, the harness of the thirteen single-call timing tools
(tools/*_bench.py), and what the tools keep of their own on the CPU: their
command-line defaults, the output line, the throughput summary, that they
import without a GPU and without torch, and that the timer and the CPU
evaluations they once carried have not grown back."""
import ast
import importlib
import json
import os
import statistics
import subprocess
import sys

import pytest

TOOLS_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS_DIR not in sys.path:
    sys.path.insert(0, TOOLS_DIR)

import callbench  # noqa: E402

# --frames / --warmup / --iters of every tool, as they were before the tools shared a parser
DEFAULTS = {
    "metrics_bench": (600, 3, 20), "unpack_bench": (600, 3, 20), "framecrc_bench": (600, 3, 20),
    "stats_bench": (600, 3, 20), "align_bench": (600, 2, 10), "msssim_bench": (600, 3, 20),
    "vif_bench": (600, 3, 20), "adm_bench": (600, 3, 20), "motion_bench": (600, 3, 20),
    "banding_bench": (600, 2, 10), "dctenergy_bench": (600, 3, 10), "ciede_bench": (600, 2, 10),
    "psnrhvs_bench": (600, 2, 10),
}
TOOLS = sorted(DEFAULTS)


def test_the_table_names_every_tool():
    assert TOOLS == sorted(f[:-3] for f in os.listdir(TOOLS_DIR) if f.endswith("_bench.py")) and len(TOOLS) == 13


class _Stop(Exception):
    pass


def _parser_of(monkeypatch, tool, argv):
    """The parser `main` builds: main runs up to its GPU preamble, which is replaced by a stop."""
    made = []
    real = callbench.parser

    def parser(*args):
        made.append(real(*args))
        return made[-1]

    def stop(*args, **kw):
        raise _Stop

    monkeypatch.setattr(callbench, "parser", parser)
    monkeypatch.setattr(callbench, "require_gpu", stop)
    with pytest.raises(_Stop):
        importlib.import_module(tool).main(argv)
    return made[-1]


@pytest.mark.parametrize("tool", TOOLS)
def test_parser_defaults(monkeypatch, tool):
    a = _parser_of(monkeypatch, tool, []).parse_args([])
    assert (a.frames, a.warmup, a.iters) == DEFAULTS[tool] and a.out is None
    extra = {k: v for k, v in vars(a).items() if k not in ("frames", "warmup", "iters", "out")}
    want = {"stats_bench": {"contents": "noise,smooth,constant"}, "align_bench": {"batch": 32, "band": 96, "base_iters": 3}}
    assert extra == want.get(tool, {})


def test_stats_bench_refuses_19_iterations(monkeypatch, capsys):
    import stats_bench
    monkeypatch.setattr(callbench, "require_gpu", lambda *a, **k: pytest.fail("reached the GPU preamble"))
    with pytest.raises(SystemExit) as e:
        stats_bench.main(["--iters", "19"])
    assert e.value.code == 2 and "--iters must be at least 20" in capsys.readouterr().err
    _parser_of(monkeypatch, "stats_bench", ["--iters", "20"])  # 20 is accepted: main goes on to the preamble


def test_emit(tmp_path, capsys):
    res = {"tool": "t", "zeta": 1, "alpha": {"m": 2.5, "b": [1, 2]}, "beta": None}
    out = tmp_path / "not" / "there" / "yet.json"
    callbench.emit(res, str(out))
    printed = capsys.readouterr().out
    assert printed.count("\n") == 1 and out.read_text() == printed  # the printed line plus its newline
    assert printed.rstrip("\n") == json.dumps(res)
    back = json.loads(printed)
    assert list(back) == ["tool", "zeta", "alpha", "beta"] and list(back["alpha"]) == ["m", "b"]
    callbench.emit(res, None)
    assert capsys.readouterr().out == printed and os.listdir(str(tmp_path)) == ["not"]


def test_throughput_summary():
    ms = [1.23456, 1.5, 1.11111, 2.71828, 1.33333]
    nbytes = 9953280000
    avg = sum(ms) / len(ms)
    # metrics_bench.stats (also unpack_bench's), as it was spelt in the tool
    want = {"avg_launch_ms": round(avg, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "bytes": nbytes, "GBps": round(nbytes / avg / 1e6, 1), "frac": round(nbytes / (avg * 1e-3) / 8.0e12, 4)}
    got = callbench.throughput(ms, nbytes)
    assert got == want and list(got) == list(want)
    assert want["avg_launch_ms"] == 1.5795 and want["GBps"] == 6301.7 and want["frac"] == 0.7877
    # framecrc_bench.stats: the same with the median after the average
    want = {"avg_launch_ms": round(avg, 4), "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "bytes": nbytes, "GBps": round(nbytes / avg / 1e6, 1),
            "frac": round(nbytes / (avg * 1e-3) / 8.0e12, 4)}
    got = callbench.throughput(ms, nbytes, median=True)
    assert got == want and list(got) == list(want)
    # stats_bench.summary: TB/s to three digits
    want = {"avg_launch_ms": round(avg, 4), "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "bytes": nbytes, "TBps": round(nbytes / avg / 1e9, 3),
            "frac": round(nbytes / (avg * 1e-3) / 8.0e12, 4)}
    got = callbench.throughput(ms, nbytes, median=True, rate=("TBps", 1e9, 3))
    assert got == want and list(got) == list(want)
    assert want["TBps"] == 6.302 and want["median_ms"] == 1.3333


def test_header_keeps_each_tools_order(monkeypatch):
    import argparse
    import types
    fake = types.SimpleNamespace(cuda=types.SimpleNamespace(get_device_name=lambda i: "dev%d" % i))
    monkeypatch.setitem(sys.modules, "torch", fake)
    a = argparse.Namespace(frames=8, warmup=3, iters=20, out=None, batch=32, band=96)
    assert callbench.header("x_bench", a, timer="t", depths=[1]) == \
        {"tool": "x_bench", "device": "dev0", "w": 1920, "h": 1080, "frames": 8, "warmup": 3, "timer": "t", "depths": [1]}
    assert list(callbench.header("x_bench", a, timer="t", depths=[1])) == \
        ["tool", "device", "w", "h", "frames", "warmup", "timer", "depths"]
    assert list(callbench.header("m", a, ("fmt",) + callbench.HEAD + ("iters",), fmt="f", timer="t")) == \
        ["tool", "device", "fmt", "w", "h", "frames", "warmup", "iters", "timer"]
    got = callbench.header("al", a, ("w", "h", "frames", "batch", "band", "warmup"), timer="t")
    assert list(got) == ["tool", "device", "w", "h", "frames", "batch", "band", "warmup", "timer"] and got["band"] == 96


def test_tools_import_without_torch():
    """In a fresh interpreter: none of the thirteen, nor the harness, imports torch at module level."""
    code = ("import sys; sys.path.insert(0, %r); import importlib\n"
            "for t in %r + ['callbench']:\n"
            "    importlib.import_module(t)\n"
            "    assert 'torch' not in sys.modules, t\n" % (TOOLS_DIR, TOOLS))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("tool", TOOLS)
def test_no_gpu_message(tool):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(SystemExit) as e:
        importlib.import_module(tool).main([])
    assert e.value.code == "%s: no GPU visible (a timing needs the MI355X)" % tool


def test_no_tool_carries_a_timer_or_a_restatement():
    banned = {"timed", "timed_round_robin", "cpu_terms", "cpu_sad"}
    for tool in TOOLS:
        with open(os.path.join(TOOLS_DIR, tool + ".py")) as f:
            tree = ast.parse(f.read())
        defs = {n.name for n in ast.walk(tree) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}
        assigned = {t.id for n in ast.walk(tree) if isinstance(n, ast.Assign) for t in n.targets if isinstance(t, ast.Name)}
        assert not (defs | assigned) & banned, (tool, (defs | assigned) & banned)
