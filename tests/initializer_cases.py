"""Seeded synthetic problems for asd_initialize by name: KITTI-00 intrinsics, draws made with the restated RandomInt from libc's rand()
after srand(0), as Initializer::Initialize makes them.  problem(case) -> dict with the fields of asd_initializer_problem (keys1, keys2,
matches12, K, sigma, n_iter, draws, min_parallax, min_triangulated) plus planted (bool per match).  Cached: the same arrays every time,
never modified by a test.

All scenes: R = 0.03 rad about (0.1, 1, 0.05), t = (0.8, 0.05, 0.3), points in x +-6, y +-2, z 6-20, outliers uniform in the image.
The outcomes beside the named scenes are those of tests/initializer_ref.py (tests/test_initializer_ref.py holds them)."""
import numpy as np

from tests import initializer_ref as R

W, H = 1241.0, 376.0
#            N, pixel noise, outliers, kind, seed
SCENES = {
    "general64": (64, 0.05, 2, "general", 1),
    "general120": (120, 0.1, 12, "general", 2),
    "noisy120": (120, 0.3, 12, "general", 3),
    "planar120": (120, 0.3, 12, "planar", 23),      # the plane z = 10 + 0.3 x + 0.2 y (seeds 4, 16-22 are refused: see EXPECTED)
    "rotation120": (120, 0.3, 12, "rotation", 5),   # t = 0
    "small40": (40, 0.3, 2, "general", 6),
    # shapes: the wave and word borders, eight matches
    "n8": (8, 0.05, 0, "general", 7),
    "n63": (63, 0.1, 3, "general", 8),
    "n64": (64, 0.1, 3, "general", 9),
    "n65": (65, 0.1, 3, "general", 10),
    "n257": (257, 0.1, 20, "general", 11),
    "unmatched": (90, 0.1, 6, "general", 12),       # n1 = 150, n2 = 131: keys without a match in both frames
    "keys2000": (300, 0.1, 30, "general", 13),      # 2000 keys per frame, 300 matches
    "ties": (70, 0.1, 4, "general", 14),            # iterations 12-23 repeat 0-11: equal scores, the first is kept
    "degenerate": (80, 0.1, 4, "general", 15),      # minimal sets of repeated points: rank-deficient A, singular models
}
# the named scenes' outcomes under tests/initializer_ref.py: case -> (model: 0 H / 1 F, ok, nGood of the motion hypotheses in the order of
# the header's sign convention)
EXPECTED = {
    "general64": (1, 1, [62, 0, 0, 0]),                    # F path, RH 0.150, 62 good
    "general120": (1, 1, [0, 0, 108, 0]),                  # F path, RH 0.132, 108 good
    "noisy120": (1, 0, [0, 0, 0, 11]),                     # F path, refused: 97 of 108 inliers fail the 4 sigma^2 gate of CheckRT in image 1
    # H path, RH 0.488, ok: the two solutions of the plane tie at 108 good points, the first met is kept (:717 is strict) and its parallax,
    # 1.12 degrees, passes; the other one's 4.30 degrees is never looked at.  Under the same convention the scene's other seeds are refused:
    # seed 4 and 17 meet the tied hypothesis of 0.79 degrees first, seeds 16 and 18-22 have 108 against 106 or 107 (the 0.75 rule)
    "planar120": (0, 1, [108, 108, 0, 29, 1, 0, 0, 1]),
    "rotation120": (0, 0, [108, 108, 108, 108, 1, 0, 0, 1]),   # H path, RH 0.490, refused: four tie, parallax 0.2 degrees at most
    "small40": (1, 0, [0, 38, 0, 0]),                      # refused through nMinGood = 50
}
CASES = list(SCENES)
NAMED = CASES[:6]
BATCH = ["general64", "unmatched", "n65"]
N_ITER = {c: 200 for c in NAMED}

_CACHE = {}


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def _project(X, K):
    return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], axis=1)


def problem(case):
    if case in _CACHE:
        return _CACHE[case]
    N, noise, n_out, kind, seed = SCENES[case]
    rng = np.random.default_rng(7100 + seed)
    K = R.K_KITTI.astype(np.float64)
    Rm = _rot([0.1, 1, 0.05], 0.03)
    t = np.zeros(3) if kind == "rotation" else np.array([0.8, 0.05, 0.3])
    X = np.stack([rng.uniform(-6, 6, N), rng.uniform(-2, 2, N), rng.uniform(6, 20, N)], axis=1)
    if kind == "planar":
        X[:, 2] = 10 + 0.3 * X[:, 0] + 0.2 * X[:, 1]
    p1 = _project(X, K) + rng.normal(0, noise, (N, 2))
    p2 = _project(X @ Rm.T + t, K) + rng.normal(0, noise, (N, 2))
    planted = np.ones(N, bool)
    out = rng.permutation(N)[:n_out]
    planted[out] = False
    p2[out] = np.stack([rng.uniform(0, W, n_out), rng.uniform(0, H, n_out)], axis=1)
    extra1, extra2 = {"unmatched": (60, 41), "keys2000": (1700, 1700)}.get(case, (0, 0))
    n1, n2 = N + extra1, N + extra2
    keys1 = np.stack([rng.uniform(0, W, n1), rng.uniform(0, H, n1)], axis=1)
    keys2 = np.stack([rng.uniform(0, W, n2), rng.uniform(0, H, n2)], axis=1)
    slot1 = np.sort(rng.permutation(n1)[:N])          # the keypoints of frame 1 that have a match, ascending: match k is keypoint slot1[k]
    slot2 = rng.permutation(n2)[:N]
    keys1[slot1], keys2[slot2] = p1, p2
    matches12 = np.full(n1, -1, np.int32)
    matches12[slot1] = slot2
    if case == "degenerate":                          # matches 0-11 see one point of frame 2, matches 12-23 one point in both frames
        keys2[slot2[:12]] = keys2[slot2[0]]
        keys1[slot1[12:24]] = keys1[slot1[12]]
        keys2[slot2[12:24]] = keys2[slot2[12]]
    n_iter = N_ITER.get(case, 24)
    draws = R.draws_from_raw(R.libc_rand(0, 8 * n_iter), N, n_iter)
    if case == "ties":
        draws[12:] = draws[:12]                       # every minimal set twice: the walk meets its best score again
    if case == "degenerate":                          # the identity draws 0 .. 7 sample matches 0 .. 7; 12 .. 19 sample matches 12 .. 19
        draws[2] = [0, 1, 2, 3, 4, 5, 6, 7]
        draws[4] = [12, 13, 14, 15, 16, 17, 18, 19]
        draws[7] = [0, 1, 2, 3, 12, 13, 14, 15]
    P = dict(keys1=keys1.astype(np.float32), keys2=keys2.astype(np.float32), matches12=matches12, K=R.K_KITTI.copy(), sigma=1.0,
             n_iter=n_iter, draws=draws, min_parallax=1.0, min_triangulated=50, planted=planted, N=N)
    for v in P.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[case] = P
    return P
