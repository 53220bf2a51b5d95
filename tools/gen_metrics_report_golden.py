"""Rewrite tests/golden/metrics_report.json: the two `cli metrics --per-frame`
report objects (without and with ``matched``) that metrics.summarize and
metrics.report make of the synthetic terms of tests/metrics_report_case.py
(fixed seed; host only, no GPU).

    python tools/gen_metrics_report_golden.py

tests/test_metrics_report_golden.py then holds summarize and report to the
record: key order, every null, every number.  The record is the behaviour to
keep: regenerate it only when a change to the report is the point."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "processing-chain_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import metrics_report_case as case  # noqa: E402
from pixpath import metrics  # noqa: E402


def main():
    with open(os.path.join(ROOT, "tests", "golden", "metrics_report.json"), "w") as f:
        json.dump(case.reports(metrics), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
