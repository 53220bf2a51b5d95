"""metrics.summarize and metrics.report against a recorded report with every
optional measurement in it (golden/metrics_report.json, written by
tools/gen_metrics_report_golden.py): the order of the keys, the place of every
null and every number.  The arithmetic is a few float64 operations in numpy;
1e-12 relative allows for another machine's libm in the last few units of
2.2e-16 and is far below what any change of a formula would move."""
import json
import os

import pytest

import metrics_report_case as case
from pixpath import metrics

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_report.json")
REL = 1e-12


def _same(got, want, where):
    if isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, "%s[%d]" % (where, i))
    elif want is None or isinstance(want, (str, bool, int)):
        assert type(got) is type(want) and got == want, where
    else:
        assert isinstance(got, float) and got == pytest.approx(want, rel=REL, abs=0.0), where


@pytest.mark.parametrize("name", ["plain", "matched"])
def test_report_is_the_recorded_one(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = json.loads(json.dumps(case.reports(metrics)[name]))  # as printed: what json makes of the values
    assert list(got) == list(want)
    for key in want:
        _same(got[key], want[key], "%s: %s" % (name, key))


def test_the_record_holds_every_measurement():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert set(want) == {"plain", "matched"}
    for key in ("ms_ssim_y", "vif_y", "adm2_y", "motion_y", "banding_added_y", "ciede2000"):
        for rep in want.values():
            assert key in rep and len(rep[key + "_frames"]) == case.N
    assert want["matched"]["psnr_y_frames"][2] is None and want["plain"]["psnr_y_frames"][2] is not None
    assert want["plain"]["motion_y_frames"][0] == 0.0 and want["plain"]["ciede2000_frames"][3] == 100.0
    assert want["plain"]["ssim_v_frames"][1] is None and want["plain"]["ms_ssim_y_frames"][1] is None
