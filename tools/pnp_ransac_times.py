"""asd_pnp_ransac (PnPsolver::iterate on the device): device time of the call's two kernels (asd_last_stage_ms("pnp_ransac"), upload
included) and wall time of the call through the Python binding, per shape (n correspondences, iterations per problem, problems), with
the number of Refines the walk ran and whether a refined model came back.  Each shape is warmed up, then timed over --reps calls; the
device time is the median of the per-call values.  Prints one JSON line.

  python tools/pnp_ransac_times.py [--reps 50] [--warmup 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402
from tests import pnpsolver_cases as C  # noqa: E402
from tests import pnpsolver_ref as R  # noqa: E402

# Tracking::Relocalization: 5 candidates, SetRansacParameters(0.99, 10, 300, 4, 0.5) gives 35 iterations, a first iterate(5) runs them all
SHAPES = [(150, 35, 5, "returns"), (150, 35, 1, "returns"), (150, 35, 5, "no_pass"), (150, 35, 1, "no_pass"), (2000, 35, 1, "no_pass")]


def make_problem(n, n_iter, seed, mode):
    """30 % outliers, 0.5 px noise, seeded draws.  returns: the reference's min_inliers, the call ends at the first Refine that passes;
    no_pass: min_inliers = n, which no count reaches, so every iteration runs and no Refine does (the hypothesis kernel alone)"""
    rng = np.random.default_rng(seed)
    P = C._scene(rng, n, 0.30, 0.5)
    P["min_inliers"], _ = R.parameters(n, *C.RANSAC)
    if mode == "no_pass":
        P["min_inliers"] = n
    P.update(n_iter=n_iter, draws=C.draws_for(rng, n, n_iter), best_inliers=0)
    return P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    pkg = graft.load_package()
    hip = pkg.capi.AsdHip(n_features=500, max_width=640, max_height=480, max_patches=1024)
    out = {}
    try:
        for n, n_iter, n_prob, mode in SHAPES:
            probs = [make_problem(n, n_iter, 10 * n + j, mode) for j in range(n_prob)]
            for _ in range(a.warmup):
                res = hip.pnp_ransac(probs)
            refines = [hip.debug_pnp_ransac(j, 0)["n_refines"] for j in range(n_prob)]
            dev, wall = [], []
            for _ in range(a.reps):
                t = time.perf_counter()
                hip.pnp_ransac(probs)
                wall.append(1e3 * (time.perf_counter() - t))
                dev.append(hip.last_stage_ms("pnp_ransac"))
            out[f"n{n}_h{n_iter}_p{n_prob}_{mode}"] = dict(device_ms=round(float(np.median(dev)), 4), wall_ms=round(float(np.median(wall)), 4),
                                                            wall_ms_min=round(float(np.min(wall)), 4), reps=a.reps, refines=refines,
                                                            found=[r["found"] for r in res], iterations_done=[r["iterations_done"] for r in res])
    finally:
        hip.close()
    print(json.dumps(dict(pnp_ransac_times=out, note="wall time includes the ctypes packing of the binding")))


if __name__ == "__main__":
    main()
