"""The V-pass skip changes no planning decision -- CPU only.

* every case of the kernel-instance table still plans to its recorded keys
  (family, source bytes, output bits, window width, V tap-pair bucket, direct,
  clamp, chunks); tests/test_scale_instances.py checks the same, this one names
  the case and the field that moved;
* a third of the headline plan's rows skip a tap pair (the count the recorded
  instruction cut is derived from).
"""
import pyoracle as po
import scale_instances as si
import strip_plan_ref as ref

from pixpath import ops


def test_every_table_case_keeps_its_instance_keys():
    moved = []
    for case, keys, gkeys in si.load():
        for generic, want in ((False, keys), (True, gkeys)):
            got = [tuple(k) for k in si.plan(case, generic=generic).instance_keys]
            want = [tuple(k) for k in want]
            if len(got) != len(want):
                moved.append("%s generic=%d: %d launches, recorded %d" % (case, generic, len(got), len(want)))
                continue
            for n, (g, w) in enumerate(zip(got, want)):
                for field, a, b in zip(ops.InstanceKey._fields, g, w):
                    if a != b:
                        moved.append("%s generic=%d launch %d: %s %r, recorded %r" % (case, generic, n, field, a, b))
    assert not moved, "\n".join(moved[:20])


def test_headline_plan_skips_a_third_of_its_rows():
    sc = ops.Scaler(po.YUV422P10LE, 1280, 720, po.YUV422P10LE, 1920, 1080, flags="lanczos", host_only=True)
    assert sc.kernel_path == 6
    for which in (2, 3):
        vtp, zero = ref.last_pair_zero(sc, which)
        assert vtp == 4 and int(zero.sum()) == 366 and len(zero) == 1080
