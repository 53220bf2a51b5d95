"""The event timer of tools/callbench.py on the GPU: it runs the callable
warmup + iters times, times the last `iters`, and takes several callables in turn."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import callbench  # noqa: E402

pytestmark = pytest.mark.gpu


def test_timed(gpu):
    import torch
    x = torch.zeros(1024, dtype=torch.int32, device=gpu)
    t = callbench.timed(lambda: x.add_(1), warmup=1, iters=3)
    assert list(t) == ["avg_ms", "min_ms", "max_ms", "launches"] and t["launches"] == 3
    assert 0 < t["min_ms"] <= t["avg_ms"] <= t["max_ms"]
    assert x.cpu().tolist() == [4] * 1024  # once to warm up, three times under the events
    assert list(callbench.timed(lambda: x.add_(1), 0, 2, count="passes")) == ["avg_ms", "min_ms", "max_ms", "passes"]


def test_timed_round_robin(gpu):
    import torch
    x, y = (torch.zeros(1024, dtype=torch.int32, device=gpu) for _ in range(2))
    order = []

    def one(name, t):
        def fn():
            order.append(name)
            t.add_(1)
        return fn

    ms = callbench.timed_round_robin({"x": one("x", x), "y": one("y", y)}, warmup=1, iters=3)
    assert list(ms) == ["x", "y"] and all(len(v) == 3 and min(v) > 0 for v in ms.values())
    assert order == ["x", "y"] * 4
    assert x.cpu().tolist() == [4] * 1024 and y.cpu().tolist() == [4] * 1024
