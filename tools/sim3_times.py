#!/usr/bin/env python3
"""Device time of asd_optimize_sim3 (hipEvents around k_sim3_opt) and wall time of the call, on TIMING_CASES of
tests/golden/make_sim3_golden.py (n = 100 and n = 2000, 10 % outliers): median and minimum of --reps calls after --warmup.
DESIGN.md section 4 quotes the output next to g2o's time on the same problems (`make_sim3_golden.py --times`)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402
from tests.golden.make_sim3_golden import TIMING_CASES, problem  # noqa: E402

ARGS = ("sim3", "P1c", "P2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "K1", "K2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    pkg = g.load_package()
    hip = pkg.AsdHip(n_features=2000, max_width=1241, max_height=376, max_patches=4096)
    try:
        for case in TIMING_CASES:
            pp = problem(case)
            dev, wall = [], []
            for k in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                S, keep, n_in = hip.optimize_sim3(*[pp[q] for q in ARGS], th2=10.0, fix_scale=False)
                t1 = time.perf_counter()
                if k >= a.warmup:
                    dev.append(hip.last_stage_ms("sim3"))
                    wall.append((t1 - t0) * 1e3)
            d = hip.debug_optimize_sim3()
            print(f"asd_optimize_sim3 n={case['n']}: device median {np.median(dev):.3f} ms min {min(dev):.3f} ms | call median {np.median(wall):.3f} ms | "
                  f"n_in {n_in} nBad {d['n_bad']} rounds {[(r['iterations'], r['trials']) for r in d['rounds']]}")
    finally:
        hip.close()


if __name__ == "__main__":
    main()
