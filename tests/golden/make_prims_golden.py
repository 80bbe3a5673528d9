"""Writes tests/golden/prims_golden.npz: per family of tests/prims_cases.py the inputs `<family>.x`, and for the families held to a
bar the exact outputs as double-double pairs `<family>.hi`, `<family>.lo` and the sensitivity scale `<family>.S` (tests/prims_ref.py,
mpmath at 60 digits) -- the machine that runs the GPU tests does not need mpmath.  Prints, per family, the worst
|f64 restatement - exact| / (u S) and the bar that follows from it (4 x, rounded up to two digits): these go into
prims_cases.MEASURED by hand, so that a regenerated golden cannot move a bar unseen.

    python -m tests.golden.make_prims_golden
"""
import os

import numpy as np

from tests import prims_cases as pc
from tests import prims_ref as pr

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "prims_golden.npz")


def main():
    data, measured = {}, {}
    print(f"{'family':24s} {'op':22s} {'n':>4s}  {'f64 worst':>10s}  {'bar':>6s}")
    for name, (ops, x) in pc.families().items():
        data[name + ".x"] = x
        if pc.has_exact(ops[0]):
            hi, lo, S = pr.exact(ops[0], x)
            data[name + ".hi"], data[name + ".lo"], data[name + ".S"] = hi, lo, S
            if ops[0] == "pose_oplus":   # the other side of theta^2 = 1e-10, for the contracted build (prims_cases.pose_oplus_other_side)
                rows, y = pc.pose_oplus_other_side(x)
                if len(rows):
                    assert all(pr._f64_item("pose_oplus", a)[1][0] != pr._f64_item("pose_oplus", b)[1][0] for a, b in zip(x[rows], y))
                    h2, l2, S2 = pr.exact("pose_oplus", x[rows], branches_of=y)
                    data[name + ".alt_rows"], data[name + ".alt_hi"], data[name + ".alt_lo"], data[name + ".alt_S"] = rows, h2, l2, S2
                    print(f"{name:24s} {'(other side of 1e-10)':22s} {len(rows):4d}")
        for op in ops:
            if not pc.has_exact(op):
                print(f"{name:24s} {op:22s} {len(x):4d}  {'bits':>10s}")
                continue
            worst = float(pr.ratios(pr.f64(op, x), hi, lo, S).max())
            print(f"{name:24s} {op:22s} {len(x):4d}  {worst:10.4f}  {pc.round_up_2(4 * worst):6g}", flush=True)
            if op != "asd_rsqrt":   # (its bar is the header's claim: prims_cases.RSQRT_ULPS)
                measured[f"{op}@{name}"] = worst
    print("MEASURED = {")
    for k, v in measured.items():
        print(f'    "{k}": {float(f"{v:.4g}")!r},')
    print("}")
    np.savez_compressed(OUT, **data)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
