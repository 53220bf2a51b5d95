"""Rewrite tests/pack_arms_table.py: the arms every case of tests/pack_arms.py
holds, as ops.pack_arms reports them now (host only, no GPU).

    python tools/gen_pack_arms.py

tests/test_pack_arms.py then checks the record against the library, against
each case's hand-written `arms`, and for coverage and uniqueness."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "processing-chain_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import pack_arms as pa  # noqa: E402


def main():
    lines = ['"""Arms held by every case of pack_arms.CASES (written by tools/gen_pack_arms.py)."""', "HELD = {"]
    for c in pa.CASES:
        if c.error:
            continue
        inst, arms = pa.query(c)
        lines.append("    %r: (%r, (" % (c.id, pa.instance(c, inst)))
        for a in sorted(arms):
            lines.append("        %r," % a)
        lines.append("    )),")
    lines.append("}")
    with open(os.path.join(ROOT, "tests", "pack_arms_table.py"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
