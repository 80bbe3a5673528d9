#!/usr/bin/env python3
"""Times of asd_optimize_essential_graph on TIMING_CASES of tests/golden/make_essgraph_golden.py (128 and 1024 keyframes on a loop
with covisibility edges).  The flat problem is built here, without the reference: the edge list from edges_of() (the rules of
Optimizer.cc:808-939 restated, held to g2o's own edge lists by tests/test_essgraph_golden.py) and the measurements Sji = Sjw * Swi in
numpy.  Wall time of the call and device time between the call's events: median and minimum of --reps calls after --warmup.
DESIGN.md quotes the output (profiles/essgraph_times.json) next to g2o's time on the same problems
(`make_essgraph_golden.py --times`)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402
from tests.golden.make_essgraph_golden import TIMING_CASES, abi_problem, edges_of, problem  # noqa: E402


def q_rot(q, v):
    u = 2 * np.cross(q[:3], v)
    return v + q[3] * u + np.cross(q[:3], u)


def s_mul(a, b):
    o = np.zeros(8)
    o[3] = a[3] * b[3] - a[:3] @ b[:3]
    o[:3] = a[3] * b[:3] + b[3] * a[:3] + np.cross(a[:3], b[:3])
    o[4:7] = a[7] * q_rot(a[:4], b[4:7]) + a[4:7]
    o[7] = a[7] * b[7]
    return o


def s_inv(a):
    o = np.zeros(8)
    o[:3], o[3] = -a[:3], a[3]
    o[4:7] = q_rot(o[:4], -a[4:7] / a[7])
    o[7] = 1 / a[7]
    return o


def flat_problem(pp, synth):
    K = len(pp["mnId"])
    T = pp["Tcw"].reshape(K, 4, 4).astype(np.float64)
    plain = np.array([np.r_[synth.rot_to_quat(T[k, :3, :3]), T[k, :3, 3], 1.0] for k in range(K)])
    vScw = np.where(pp["corrected"][:, None] != 0, pp["corrected_sim3"], plain)
    non = np.where(pp["noncorrected"][:, None] != 0, pp["noncorrected_sim3"], vScw)
    edges, _ = edges_of(pp)
    meas = [s_mul(vScw[j], s_inv(vScw[i])) if kind == 0 else s_mul(non[j], s_inv(non[i])) for i, j, kind in edges]
    return abi_problem(pp, vScw, [e[0] for e in edges], [e[1] for e in edges], meas)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cases", default="", help="comma-separated subset of TIMING_CASES")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = g.load_package()
    out = dict(cases=[])
    ctx = pkg.AsdHip(n_features=500, max_width=640, max_height=240, max_patches=1024)
    try:
        for case in TIMING_CASES:
            if a.cases and case["name"] not in a.cases.split(","):
                continue
            pr = flat_problem(problem(case, pkg.synth), pkg.synth)
            wall, dev, r = [], [], None
            for k in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                r = ctx.optimize_essential_graph(pr)
                t1 = time.perf_counter()
                if k >= a.warmup:
                    wall.append((t1 - t0) * 1e3)
                    dev.append(float(ctx.last_stage_ms("essgraph")))
            rec = dict(name=case["name"], keyframes=len(pr["sim3"]), edges=len(pr["e_i"]), map_points=len(pr["mp_ref"]), reps=a.reps,
                       iterations=r["iterations"], trials=r["trials"], trials_per_iteration=ctx.essgraph_trials(), forms=ctx.essgraph_forms(),
                       chi2=r["chi2"], call_ms_median=float(np.median(wall)), call_ms_min=float(min(wall)),
                       device_ms_median=float(np.median(dev)), device_ms_min=float(min(dev)),
                       device_ms_per_trial=float(np.median(dev)) / max(r["trials"], 1))
            out["cases"].append(rec)
            print(json.dumps(rec), flush=True)
    finally:
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
