"""Seeded synthetic problems for asd_pnp_ransac by name: KITTI intrinsics, at most 40 iterations each, draws made with the restated
RandomInt from a seeded stream of rand() values.  problem(case) -> dict with the fields of asd_pnp_ransac_problem (n, P3Dw, P2D, max_err,
K, min_inliers, n_iter, draws, best_inliers) plus planted (bool[n], the correspondences that follow the pose), R_true, t_true.  Cached: the
same arrays every time, never modified by a test."""
import numpy as np

from tests import pnpsolver_ref as R

CASES = ["clean64", "noisy150", "min15", "n_eq_min", "n_lt_min", "n63", "n64", "n65", "n257", "carry", "coplanar", "behind"]
BATCH = ["noisy150", "n_lt_min", "n65"]
RANSAC = (0.99, 10, 300, 4, 0.5)          # Tracking.cc:1141
TH2 = np.float32(5.991)
SIGMA2 = np.array([1.2 ** (2 * l) for l in range(8)]).astype(np.float32)
SEEDS = {"clean64": 2105}
# clean64: four-point EPnP reproduces the true inlier mask for about one all-inlier sample in 250 once the basis of the null space is free
# (pnpsolver_ref's module text), so no seed gives five such samples among 35 seeded draws (900 seeds tried: at most one).  These five
# samples of planted inliers do, under the restatement's own basis and eight seeded rotations of it (tests/test_pnpsolver_ref.py checks
# that); they replace the seeded draws at these iterations, every other iteration keeps its seeded draw.
CLEAN64_ROBUST = {4: [12, 4, 1, 3], 11: [15, 25, 16, 62], 18: [19, 42, 25, 27], 25: [61, 6, 49, 55], 32: [30, 54, 6, 19]}

_CACHE = {}


def _seed(case):
    return SEEDS.get(case, 3000 + CASES.index(case))


def project(Rm, t, Xw, K):
    Xc = np.asarray(Xw, np.float64) @ np.asarray(Rm, np.float64).T + np.asarray(t, np.float64)
    return np.stack([float(K[2]) + float(K[0]) * Xc[:, 0] / Xc[:, 2], float(K[3]) + float(K[1]) * Xc[:, 1] / Xc[:, 2]], axis=1), Xc[:, 2]


def _scene(rng, n, outlier_frac, noise_px, kind=""):
    K = R.K_KITTI
    if kind == "coplanar":      # the world plane z = 0.5: PW0's third column is exactly zero, CC is singular
        Rm = R._rot([0.45, 0.1, -0.05])
        t = np.array([0.3, -0.2, 16.0])
        Xw = np.stack([rng.uniform(-8, 8, n), rng.uniform(-5, 5, n), np.full(n, 0.5)], axis=1).astype(np.float32)
    else:
        Rm = R._rot(rng.normal(0, 0.3, 3))
        t = rng.normal(0, 1.0, 3)
        Xc = np.stack([rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), rng.uniform(6, 30, n)], axis=1)
        if kind == "behind":    # a quarter of the points at negative depth
            Xc[rng.permutation(n)[:n // 4], 2] *= -1.0
        Xw = ((Xc - t) @ Rm).astype(np.float32)
    uv, _ = project(Rm, t, Xw, K)
    uv = uv + rng.normal(0, noise_px, (n, 2)) if noise_px > 0 else uv
    planted = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    out = rng.permutation(n)[:n_out]
    planted[out] = False
    ang = rng.uniform(0, 2 * np.pi, n_out)
    uv[out] += rng.uniform(60, 200, n_out)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    max_err = (SIGMA2[rng.integers(0, 8, n)] * TH2).astype(np.float32)      # the product taken in f32 (:156)
    return dict(n=n, P3Dw=Xw, P2D=uv.astype(np.float32), max_err=max_err, K=K.copy(), planted=planted, R_true=Rm, t_true=t)


def draws_for(rng, n, n_iter):
    """n_iter x 4 draws of RandomInt(0, n - 1 - i) from a seeded stream of rand() values"""
    raw = rng.integers(0, 2 ** 31, (n_iter, 4))
    return np.array([[R.random_int(int(raw[k, i]), 0, n - 1 - i) for i in range(4)] for k in range(n_iter)], np.int32).reshape(n_iter, 4)


def problem(case):
    if case in _CACHE:
        return _CACHE[case]
    rng = np.random.default_rng(_seed(case))
    params = RANSAC
    n_iter = None
    best_in = 0
    if case == "clean64":
        P = _scene(rng, 64, 0.40, 0.0)
    elif case == "noisy150":
        P = _scene(rng, 150, 0.30, 0.5)
    elif case == "min15":
        P = _scene(rng, 15, 0.0, 0.2)
    elif case == "n_eq_min":
        P = _scene(rng, 10, 0.0, 0.0)
    elif case == "n_lt_min":
        P = _scene(rng, 8, 0.0, 0.0)
        n_iter = 5
    elif case[0] == "n" and case[1:].isdigit():
        P = _scene(rng, int(case[1:]), 0.0, 0.0)
        n_iter = 6
    elif case == "carry":
        P = _scene(rng, 100, 0.0, 0.0)
        best_in = 100                     # nothing beats it: iterations that pass :209 neither update nor refine
        n_iter = 8
    elif case == "coplanar":
        P = _scene(rng, 80, 0.25, 0.3, "coplanar")
        n_iter = 12
    elif case == "behind":
        P = _scene(rng, 96, 0.20, 0.3, "behind")
        n_iter = 12
    else:
        raise KeyError(case)
    n = P["n"]
    P["min_inliers"], max_its = R.parameters(n, *params)
    P["max_its"] = max_its
    P["n_iter"] = max_its if n_iter is None else n_iter      # the first iterate(5) of a solver runs max(5, mRansacMaxIts - 0) iterations
    assert P["n_iter"] <= 40
    P["draws"] = draws_for(rng, n, P["n_iter"]) if n >= 4 else np.zeros((P["n_iter"], 4), np.int32)
    if case == "clean64":
        P["draws"] = P["draws"].copy()
        for k, quad in CLEAN64_ROBUST.items():
            assert P["planted"][quad].all()
            P["draws"][k] = R.draws_of(quad, n)
    P["best_inliers"] = best_in
    for v in P.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[case] = P
    return P


def null_rotation(seed):
    """a seeded orthogonal 4x4 (another basis of a minimal set's null space)"""
    q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(4, 4)))
    return q * np.sign(np.diag(r))


_HYP = {}


def reference_hypotheses(case):
    """per iteration of the case, under the restatement alone: dict(idx, c64, cld (compute_pose in float64 / longdouble), mask, count)"""
    if case not in _HYP:
        P = problem(case)
        out = []
        for d in P["draws"][:P["n_iter"]] if P["n"] >= P["min_inliers"] else []:
            idx = R.sample(d, P["n"])
            c64 = R.compute_pose(P["P3Dw"][idx], P["P2D"][idx], P["K"], np.float64)
            cld = R.chain(c64["cws"], c64["v"], P["P3Dw"][idx], P["P2D"][idx], P["K"], R.LD)
            m = R.check_inliers(c64["R"], c64["t"], P["P3Dw"], P["P2D"], P["K"], P["max_err"])
            out.append(dict(idx=idx, c64=c64, cld=cld, mask=m, count=int(m.sum())))
        _HYP[case] = out
    return _HYP[case]


_REFINE = {}


def refine(case, mask, dtype=np.float64):
    """Refine (:260-305) on the correspondences of `mask` under the restatement -> dict(c (compute_pose), cld, mask, count)"""
    key = (case, np.asarray(mask, bool).tobytes(), np.dtype(dtype).name)
    if key not in _REFINE:
        P = problem(case)
        sel = np.nonzero(mask)[0]
        c = R.compute_pose(P["P3Dw"][sel], P["P2D"][sel], P["K"], dtype)
        cld = R.chain(c["cws"], c["v"], P["P3Dw"][sel], P["P2D"][sel], P["K"], R.LD)
        m = R.check_inliers(np.asarray(c["R"], np.float64), np.asarray(c["t"], np.float64), P["P3Dw"], P["P2D"], P["K"], P["max_err"])
        _REFINE[key] = dict(c=c, cld=cld, mask=m, count=int(m.sum()))
    return _REFINE[key]
