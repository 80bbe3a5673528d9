"""asd_initialize (Initializer::Initialize on the device): device time of one call at 200 iterations for N = 100, 300 and 1000 matches,
per kernel -- asd_last_stage_ms("initializer_hyp") is the upload and k_init_hyp, "initializer" both kernels; k_init_reconstruct is the
difference -- and wall time of the call through the Python binding.  The scene is the general one of tests/initializer_cases.py with
10 % outliers and 0.1 px noise; every frame has twice as many keys as matches.  Each shape is warmed up, then timed over --reps calls;
the device times are medians of the per-call values.  Prints one JSON line.

  python tools/initializer_times.py [--reps 50] [--warmup 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402
from tests import initializer_cases as C  # noqa: E402
from tests import initializer_ref as R  # noqa: E402

SHAPES = [100, 300, 1000]


def make_problem(N, seed):
    rng = np.random.default_rng(seed)
    K = R.K_KITTI.astype(np.float64)
    Rm, t = C._rot([0.1, 1, 0.05], 0.03), np.array([0.8, 0.05, 0.3])
    X = np.stack([rng.uniform(-6, 6, N), rng.uniform(-2, 2, N), rng.uniform(6, 20, N)], axis=1)
    p1 = C._project(X, K) + rng.normal(0, 0.1, (N, 2))
    p2 = C._project(X @ Rm.T + t, K) + rng.normal(0, 0.1, (N, 2))
    out = rng.permutation(N)[:N // 10]
    p2[out] = np.stack([rng.uniform(0, C.W, len(out)), rng.uniform(0, C.H, len(out))], axis=1)
    n = 2 * N
    keys1 = np.stack([rng.uniform(0, C.W, n), rng.uniform(0, C.H, n)], axis=1)
    keys2 = keys1.copy()
    slot1, slot2 = np.sort(rng.permutation(n)[:N]), rng.permutation(n)[:N]
    keys1[slot1], keys2[slot2] = p1, p2
    m = np.full(n, -1, np.int32)
    m[slot1] = slot2
    return dict(keys1=keys1.astype(np.float32), keys2=keys2.astype(np.float32), matches12=m, K=R.K_KITTI.copy(), sigma=1.0, n_iter=200,
                draws=R.draws_from_raw(R.libc_rand(0, 1600), N, 200), min_parallax=1.0, min_triangulated=50)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    pkg = graft.load_package()
    hip = pkg.capi.AsdHip(n_features=500, max_width=640, max_height=480, max_patches=1024)
    out = {}
    try:
        for N in SHAPES:
            P = make_problem(N, 40 + N)
            for _ in range(a.warmup):
                res = hip.initialize([P])[0]
            both, hyp, wall = [], [], []
            for _ in range(a.reps):
                t = time.perf_counter()
                hip.initialize([P])
                wall.append(1e3 * (time.perf_counter() - t))
                both.append(hip.last_stage_ms("initializer"))
                hyp.append(hip.last_stage_ms("initializer_hyp"))
            med = lambda v: round(float(np.median(v)), 4)
            out[f"n{N}"] = dict(device_ms=med(both), k_init_hyp_ms=med(hyp), k_init_reconstruct_ms=round(med(both) - med(hyp), 4), wall_ms=med(wall),
                                wall_ms_min=round(float(np.min(wall)), 4), reps=a.reps, model=res["model"], ok=res["ok"])
    finally:
        hip.close()
    print(json.dumps(dict(initializer_times=out, note="k_init_hyp_ms includes the upload; wall time includes the ctypes packing of the binding")))


if __name__ == "__main__":
    main()
