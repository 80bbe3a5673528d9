"""asd_sim3_ransac (Sim3Solver::iterate on the device): device time of the call's two kernels (asd_last_stage_ms("sim3_ransac"), upload
included) and wall time of the call through the Python binding, per shape (n correspondences, hypotheses per problem, problems).  Each
shape is warmed up, then timed over --reps calls; the device time is the median of the per-call values.  Prints one JSON line.

  python tools/sim3_ransac_times.py [--reps 50] [--warmup 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402
from tests import sim3solver_ref as R  # noqa: E402

SHAPES = [(50, 5, 1), (50, 5, 4), (200, 300, 1), (2000, 300, 1)]


def make_problem(n, n_iter, seed):
    """60 % of n correspondences on one Sim3, random draws; min_inliers = n so that every hypothesis runs and none returns early"""
    rng = np.random.default_rng(seed)
    X1c, X2c, _planted, _ = R._planted(rng, n, 1.1, 0.6, 0.2, R.K_KITTI, R.K_KITTI)
    draws = np.array([[int(rng.integers(0, n - i)) for i in range(3)] for _ in range(n_iter)], np.int32)
    e = np.full(n, 9.210, np.float32)
    return dict(n=n, X1c=X1c, X2c=X2c, max_err1=e, max_err2=e, K1=R.K_KITTI, K2=R.K_KITTI, fix_scale=0, min_inliers=n, n_iter=n_iter, draws=draws,
                best_inliers=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    pkg = graft.load_package()
    hip = pkg.capi.AsdHip(n_features=500, max_width=640, max_height=480, max_patches=1024)
    out = {}
    try:
        for n, n_iter, n_prob in SHAPES:
            probs = [make_problem(n, n_iter, 10 * n + j) for j in range(n_prob)]
            for _ in range(a.warmup):
                res = hip.sim3_ransac(probs)
            assert all(r["iterations_done"] == n_iter for r in res)
            dev, wall = [], []
            for _ in range(a.reps):
                t = time.perf_counter()
                hip.sim3_ransac(probs)
                wall.append(1e3 * (time.perf_counter() - t))
                dev.append(hip.last_stage_ms("sim3_ransac"))
            out[f"n{n}_h{n_iter}_p{n_prob}"] = dict(device_ms=round(float(np.median(dev)), 4), wall_ms=round(float(np.median(wall)), 4),
                                                     wall_ms_min=round(float(np.min(wall)), 4), reps=a.reps)
    finally:
        hip.close()
    print(json.dumps(dict(sim3_ransac_times=out, note="wall time includes the ctypes packing of the binding")))


if __name__ == "__main__":
    main()
