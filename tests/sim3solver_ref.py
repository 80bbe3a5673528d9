"""Plain NumPy restatement of Sim3Solver (reference src/vslam/src/Sim3Solver.cc), written from its source text: what asd_sim3_ransac
(asd-slam_amd/csrc/sim3_ransac.hip) is held to by tests/test_sim3_solver.py, and what tests/test_sim3_solver_ref.py checks on its own.

The model (ComputeSim3, :226-337) has a mathematical answer -- the top eigenvector of Horn's 4x4 matrix N -- so `horn` evaluates the
formula in np.longdouble with a Jacobi of its own (the truth) and, independently, in float64 with np.linalg.eigh; the distance between the
two in units of tau = eps64 * cond, cond = |N|_2 / (lambda1 - lambda2), is what an honest f64 evaluation achieves.  The inlier test
(CheckInliers / Project, :340-403) is f32 arithmetic in a fixed operation order and is restated bit for bit.
"""
import math

import numpy as np

EPS64 = float(np.finfo(np.float64).eps)
F32 = np.float32
K_KITTI = np.array([718.856, 718.856, 607.1928, 185.2157], np.float32)
K_OTHER = np.array([707.0912, 707.0912, 601.8873, 183.1104], np.float32)
MODEL_MARGIN = 32.0      # the device's bar in units of tau
EIGH_MARGIN = 8.0        # what the float64 eigh evaluation must stay below over the case list
COND_GATE = 1e4


# ---------------------------------------------------------------------------------------------------------------- model (:226-337)
def _jacobi_top(N):
    """top eigenpair of the symmetric 4x4 N in N's dtype by cyclic Jacobi -> (eigenvalues descending, top eigenvector)"""
    dt = N.dtype.type
    a = N.copy()
    v = np.eye(4, dtype=N.dtype)
    for _sweep in range(60):   # (callers run this under np.errstate: theta * theta may overflow to inf, which gives t = 0)
        off = sum(abs(a[p, r]) for p in range(3) for r in range(p + 1, 4))
        if off == 0:
            break
        for p in range(3):
            for r in range(p + 1, 4):
                if a[p, r] == 0:
                    continue
                theta = (a[r, r] - a[p, p]) / (dt(2) * a[p, r])
                t = (dt(1) if theta >= 0 else dt(-1)) / (abs(theta) + np.sqrt(theta * theta + dt(1)))
                c = dt(1) / np.sqrt(t * t + dt(1))
                s = t * c
                J = np.eye(4, dtype=N.dtype)
                J[p, p] = c; J[r, r] = c; J[p, r] = s; J[r, p] = -s
                a = J.T @ a @ J
                a[p, r] = a[r, p] = dt(0)
                v = v @ J
    lam = np.array([a[i, i] for i in range(4)], dtype=N.dtype)
    order = np.argsort(-lam, kind="stable")
    return lam[order], v[:, order[0]]


def _rot_of_quat(q):
    """rotation of the unit quaternion (w, x, y, z): what atan2 / angle-axis / cv::Rodrigues (:274-284) give for q and -q alike"""
    w, x, y, z = q
    two = q.dtype.type(2)
    one = q.dtype.type(1)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=q.dtype)


def horn(P1, P2, fix_scale, dtype=np.longdouble, use_eigh=False):
    """ComputeSim3 (:226-337) on the 3x3 point sets P1, P2 ([point][xyz], float32 values) evaluated in `dtype`.  use_eigh: the
    eigenvector from np.linalg.eigh (float64 only) instead of the Jacobi above.  Returns a dict: q (w x y z, unit), R, s, t, T12, T21
    (4x4), O1, O2, cond = |N|_2 / (lambda1 - lambda2)."""
    dt = np.dtype(dtype).type
    P1 = np.asarray(P1, dtype=dtype)
    P2 = np.asarray(P2, dtype=dtype)
    O1 = P1.sum(axis=0) / dt(3)
    O2 = P2.sum(axis=0) / dt(3)
    Pr1 = (P1 - O1).T      # 3 x 3, one point per column like the reference
    Pr2 = (P2 - O2).T
    M = Pr2 @ Pr1.T        # :243
    N11 = M[0, 0] + M[1, 1] + M[2, 2]
    N12 = M[1, 2] - M[2, 1]
    N13 = M[2, 0] - M[0, 2]
    N14 = M[0, 1] - M[1, 0]
    N22 = M[0, 0] - M[1, 1] - M[2, 2]
    N23 = M[0, 1] + M[1, 0]
    N24 = M[2, 0] + M[0, 2]
    N33 = -M[0, 0] + M[1, 1] - M[2, 2]
    N34 = M[1, 2] + M[2, 1]
    N44 = -M[0, 0] - M[1, 1] + M[2, 2]
    N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]], dtype=dtype)
    if use_eigh:
        assert np.dtype(dtype) == np.float64
        lam, vec = np.linalg.eigh(N)
        lam = lam[::-1]
        q = vec[:, 3].copy()
    else:
        with np.errstate(all="ignore"):
            lam, q = _jacobi_top(N)
    with np.errstate(all="ignore"):
        q = q / np.sqrt((q * q).sum())
        gap = lam[0] - lam[1]
        cond = float(max(abs(lam[0]), abs(lam[3])) / gap) if gap > 0 else float("inf")
        R = _rot_of_quat(q)
        if fix_scale:
            s = dt(1)
        else:
            P3 = R @ Pr2
            s = (Pr1 * P3).sum() / (P3 * P3).sum()
        sR = s * R
        t = O1 - sR @ O2
        sRinv = (dt(1) / s) * R.T
        tinv = -(sRinv @ t)
    T12 = np.eye(4, dtype=dtype)
    T12[:3, :3] = sR
    T12[:3, 3] = t
    T21 = np.eye(4, dtype=dtype)
    T21[:3, :3] = sRinv
    T21[:3, 3] = tinv
    return dict(q=q, R=R, s=s, t=t, T12=T12, T21=T21, O1=O1, O2=O2, cond=cond)


def ulp32(x):
    """spacing of float32 at |x| (as float)"""
    return float(np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)))


def model_bounds(truth):
    """the model layer's bar per output, as arrays shaped like the outputs: 0.5 ulp32(truth) + 32 tau * scale (tau = eps64 * cond)"""
    tau = EPS64 * truth["cond"]
    s = abs(float(truth["s"]))
    o1 = float(np.abs(truth["O1"]).sum())
    o2 = float(np.abs(truth["O2"]).sum())
    half = lambda a: 0.5 * np.vectorize(ulp32)(np.asarray(a, dtype=np.float64))
    scale12 = np.empty((3, 4))
    scale12[:, :3] = s                       # T12's block is s R: a rotation entry times s
    scale12[:, 3] = o1 + s * o2
    scale21 = np.empty((3, 4))
    scale21[:, :3] = 1.0 / s
    scale21[:, 3] = o2 + o1 / s
    return dict(R=half(truth["R"]) + MODEL_MARGIN * tau, s=half(truth["s"]) + MODEL_MARGIN * tau * s,
                t=half(truth["t"]) + MODEL_MARGIN * tau * (o1 + s * o2),
                T12=half(truth["T12"][:3]) + MODEL_MARGIN * tau * scale12, T21=half(truth["T21"][:3]) + MODEL_MARGIN * tau * scale21,
                q=MODEL_MARGIN * tau, tau=tau)


def model_units(got, truth):
    """largest distance of an f64 evaluation `got` from `truth` in the bar's own units (tau * scale), over q (up to sign), R, s, t, T21"""
    b = model_bounds(truth)
    tau = b["tau"]
    s = abs(float(truth["s"]))
    o1 = float(np.abs(truth["O1"]).sum())
    o2 = float(np.abs(truth["O2"]).sum())
    f = lambda a: np.asarray(a, dtype=np.longdouble)
    dq = min(np.abs(f(got["q"]) - f(truth["q"])).max(), np.abs(f(got["q"]) + f(truth["q"])).max())
    u = [float(dq) / tau, float(np.abs(f(got["R"]) - f(truth["R"])).max()) / tau, float(abs(f(got["s"]) - f(truth["s"]))) / (tau * s),
         float(np.abs(f(got["t"]) - f(truth["t"])).max()) / (tau * (o1 + s * o2)),
         float(np.abs(f(got["T21"][:3, :3]) - f(truth["T21"][:3, :3])).max()) / (tau / s),
         float(np.abs(f(got["T21"][:3, 3]) - f(truth["T21"][:3, 3])).max()) / (tau * (o2 + o1 / s))]
    return max(u)


# ------------------------------------------------------------------------------------------------ inlier test (:340-423), f32 bit for bit
def _project_f32(T, K, X):
    """Project (:382-403): T rows 0-2 (f32), K = fx fy cx cy, X [n][3] -> (u, v), every intermediate rounded to f32"""
    T = np.asarray(T, F32)
    X = np.asarray(X, F32)
    with np.errstate(all="ignore"):
        c = []
        for r in range(3):
            a = F32(T[r, 0] * X[:, 0])
            b = F32(T[r, 1] * X[:, 1])
            d = F32(T[r, 2] * X[:, 2])
            c.append(F32(F32(F32(a + b) + d) + T[r, 3]))
        invz = F32(F32(1) / c[2])
        x = F32(c[0] * invz)
        y = F32(c[1] * invz)
        u = F32(F32(K[0] * x) + K[2])
        v = F32(F32(K[1] * y) + K[3])
    return u, v


def from_camera_to_image(X, K):
    """FromCameraToImage (:405-423)"""
    X = np.asarray(X, F32)
    with np.errstate(all="ignore"):
        invz = F32(F32(1) / X[:, 2])
        x = F32(X[:, 0] * invz)
        y = F32(X[:, 1] * invz)
        return F32(F32(K[0] * x) + K[2]), F32(F32(K[1] * y) + K[3])


def reproj_errors_f32(T12, T21, X1c, X2c, K1, K2):
    K1 = np.asarray(K1, F32)
    K2 = np.asarray(K2, F32)
    u1, v1 = from_camera_to_image(X1c, K1)
    u2, v2 = from_camera_to_image(X2c, K2)
    pu, pv = _project_f32(T12, K1, X2c)       # vP2im1
    qu, qv = _project_f32(T21, K2, X1c)       # vP1im2
    with np.errstate(all="ignore"):
        du, dv = F32(u1 - pu), F32(v1 - pv)   # dist1 = mvP1im1 - vP2im1
        err1 = F32(F32(du * du) + F32(dv * dv))
        du, dv = F32(qu - u2), F32(qv - v2)   # dist2 = vP1im2 - mvP2im2
        err2 = F32(F32(du * du) + F32(dv * dv))
    return err1, err2


def check_inliers_f32(T12, T21, X1c, X2c, K1, K2, max_err1, max_err2):
    """CheckInliers (:340-364) -> bool[n]; NaN compares false"""
    err1, err2 = reproj_errors_f32(T12, T21, X1c, X2c, K1, K2)
    with np.errstate(all="ignore"):
        return (err1 < np.asarray(max_err1, F32)) & (err2 < np.asarray(max_err2, F32))


# ---------------------------------------------------------------------------------------------------- the sequential parts, literally
def sample(draws, n):
    """:163-177 for one iteration: draws[i] = RandomInt(0, size - 1) of draw i -> the three correspondence indices"""
    avail = list(range(n))
    idx = []
    for i in range(3):
        randi = int(draws[i])
        assert 0 <= randi <= len(avail) - 1
        idx.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return idx


def select(counts, best_in, min_inliers):
    """:183-200 over the counts of the supplied iterations -> dict(best_inliers, best_updated, best_hyp, found, iterations_done, n_inliers)"""
    best, best_h, found = int(best_in), -1, -1
    done = len(counts)
    for k, c in enumerate(counts):
        c = int(c)
        if c >= best:
            best, best_h = c, k
            if c > min_inliers:
                found, done = k, k + 1
                break
    return dict(best_inliers=best, best_updated=int(best_h >= 0), best_hyp=best_h, found=int(found >= 0), found_hyp=found,
                iterations_done=done, n_inliers=best if found >= 0 else 0)


INT_MIN = -2 ** 31


def _c_log(x):
    """C's log() with libm's own rounding (math.log) and C's special cases instead of Python's exceptions"""
    if x > 0:
        return math.log(x)
    return float("-inf") if x == 0 else float("nan")


def max_iterations(n, probability, min_inliers, max_its):
    """SetRansacParameters (:114-138): the value left in mRansacMaxIts"""
    with np.errstate(all="ignore"):
        epsilon = np.float32(min_inliers) / np.float32(n)      # float epsilon = (float)mRansacMinInliers / N
    if min_inliers == n:
        its = 1
    else:
        e3 = math.pow(float(epsilon), 3)                       # pow(epsilon, 3): the float promoted to double
        with np.errstate(all="ignore"):
            v = np.float64(_c_log(1 - probability)) / np.float64(_c_log(1 - e3))      # IEEE division: x / 0, 0 / 0 as in C
        v = float(v)
        v = math.ceil(v) if math.isfinite(v) else v
        its = int(v) if (math.isfinite(v) and -2147483649.0 < v < 2147483648.0) else INT_MIN   # x86-64's conversion of what does not fit
    return max(1, min(its, max_its))


def random_int(raw, lo, hi, rand_max=2147483647):
    """DUtils::Random::RandomInt (src/dbow2/DUtils/Random.cpp:47-50) of the raw rand() value"""
    d = hi - lo + 1
    return int((float(raw) / (float(rand_max) + 1.0)) * d) + lo


# ------------------------------------------------------------------------------------------------------------------------- problems
def _rot(rv):
    rv = np.asarray(rv, np.float64)
    th = np.linalg.norm(rv)
    if th == 0:
        return np.eye(3)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def _planted(rng, n, scale, inlier_frac, noise_px, K1, K2):
    """n correspondences: points in front of camera 2, mapped to camera 1 by one Sim3; a fraction keeps it (image noise of noise_px),
    the rest are gross outliers.  Returns X1c, X2c (f32), the inlier flags, (s, R, t)"""
    R = _rot(rng.normal(0, 0.25, 3))
    t = rng.normal(0, 1.0, 3)
    X2 = np.stack([rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), rng.uniform(8, 30, n)], axis=1)
    X1 = scale * (X2 @ R.T) + t
    for i in range(n):   # keep every point well in front of camera 1 too
        while X1[i, 2] < 4:
            X2[i] = [rng.uniform(-8, 8), rng.uniform(-3, 3), rng.uniform(8, 30)]
            X1[i] = scale * (R @ X2[i]) + t
    n_in = int(round(inlier_frac * n))
    planted = np.zeros(n, bool)
    planted[rng.permutation(n)[:n_in]] = True
    # image noise as a displacement of the 3-D point at its depth (both cameras)
    X1 = X1 + np.stack([rng.normal(0, noise_px, n) * X1[:, 2] / float(K1[0]), rng.normal(0, noise_px, n) * X1[:, 2] / float(K1[1]), np.zeros(n)], axis=1)
    out = ~planted
    k = int(out.sum())
    sign = rng.choice([-1.0, 1.0], (k, 2))
    X1[out, :2] += sign * rng.uniform(40, 120, (k, 2)) * X1[out, 2:3] / float(K1[0])     # 40-120 px off in image 1
    return X1.astype(np.float32), X2.astype(np.float32), planted, (scale, R, t)


def _draws_for(rng, n, triple):
    """draws that make `sample` return `triple`: found by replaying the swap-with-back bookkeeping"""
    avail = list(range(n))
    d = []
    for idx in triple:
        r = avail.index(int(idx))
        d.append(r)
        avail[r] = avail[-1]
        avail.pop()
    return d


def _well_conditioned_draws(rng, n, X1c, X2c, fix_scale, count, pool=None, must_include=None):
    """`count` draw triples whose Horn problem has cond <= COND_GATE / 4 (margin to the gate), chosen among seeded random draws"""
    out = []
    while len(out) < count:
        if pool is None:
            d = [int(rng.integers(0, n - i)) for i in range(3)]
        else:
            tri = list(rng.choice(pool, 3, replace=False))
            if must_include is not None:
                tri[int(rng.integers(0, 3))] = int(rng.choice(must_include))
                if len(set(tri)) < 3:
                    continue
            d = _draws_for(rng, n, tri)
        idx = sample(d, n)
        if horn(X1c[idx], X2c[idx], fix_scale, np.float64, use_eigh=True)["cond"] <= COND_GATE / 4:
            out.append(d)
    return np.array(out, np.int32)


def _widest(rng, X, pool):
    """the widest triangle among 200 seeded triples of `pool`"""
    best, best_a = None, -1.0
    for _ in range(200):
        tri = rng.choice(pool, 3, replace=False)
        a = np.linalg.norm(np.cross(X[tri[1]] - X[tri[0]], X[tri[2]] - X[tri[0]]).astype(np.float64))
        if a > best_a:
            best, best_a = tri, a
    return [int(i) for i in best]


CASES = ["n3_one",
         "n63", "n64", "n65", "n255", "n256", "n257", "n63_fix", "n64_fix", "n65_fix", "n255_fix", "n256_fix", "n257_fix",
         "find_300_k0", "find_300_k4", "find_300_k299",
         "no_return", "best_in_high", "deg_identical3", "deg_identical2", "deg_z0", "no_more"]


def _case_seed(case):
    return 1000 + CASES.index(case)


_CACHE = {}


def problem(case):
    """A seeded synthetic problem by name -> dict with the fields of asd_sim3_ransac_problem (n, X1c, X2c, max_err1, max_err2, K1, K2,
    fix_scale, min_inliers, n_iter, draws, best_inliers) plus: degenerate (bool per hypothesis: held to the decision layer only),
    planted (bool[n]) / k_found for the planted scenarios.  Cached: the same arrays every time, never modified by a test."""
    if case in _CACHE:
        return _CACHE[case]
    rng = np.random.default_rng(_case_seed(case))
    K1, K2 = K_KITTI, K_KITTI
    sig = np.array([1.2 ** (2 * l) for l in range(8)])
    P = None
    if case == "n3_one":
        X1c, X2c, planted, _ = _planted(rng, 3, 1.3, 1.0, 0.2, K1, K2)
        P = dict(n=3, X1c=X1c, X2c=X2c, fix_scale=0, min_inliers=2, n_iter=1, draws=np.array([[2, 0, 0]], np.int32), best_inliers=0)
    elif case.startswith("n") and case[1:].split("_")[0].isdigit():
        n = int(case[1:].split("_")[0])
        fix = case.endswith("_fix")
        K2 = K_OTHER
        X1c, X2c, planted, _ = _planted(rng, n, 1.0 if fix else 0.8, 0.6, 0.2, K1, K2)
        draws = _well_conditioned_draws(rng, n, X1c, X2c, fix, 5)
        draws[0] = [n - 1, n - 2, n - 3]        # the last position at every size of the vector
        draws[1] = [0, 0, 0]                    # position 0 three times: the second and third read a moved element
        draws[4] = _draws_for(rng, n, _widest(rng, X2c, np.nonzero(planted)[0]))   # three planted inliers: a mask with many bits set
        P = dict(n=n, X1c=X1c, X2c=X2c, fix_scale=int(fix), min_inliers=n, n_iter=5, draws=draws, best_inliers=0, planted=planted)
    elif case.startswith("find_300"):
        k = int(case.split("_k")[1])
        n = 120
        X1c, X2c, planted, _ = _planted(rng, n, 1.15, 0.6, 0.2, K1, K2)
        inl, outl = np.nonzero(planted)[0], np.nonzero(~planted)[0]
        bad = _well_conditioned_draws(rng, n, X1c, X2c, False, 300, pool=np.arange(n), must_include=outl)
        # hypothesis k: three planted inliers, spread out (the widest triangle among a few seeded choices)
        draws = bad.copy()
        # hypothesis k: among 60 seeded triples of planted inliers the one whose model leaves the planted set the widest margin
        best, best_e = None, np.inf
        for _ in range(60):
            tri = [int(i) for i in rng.choice(inl, 3, replace=False)]
            hm = horn(X1c[tri], X2c[tri], False, np.float64, use_eigh=True)
            e1, e2 = reproj_errors_f32(hm["T12"].astype(np.float32), hm["T21"].astype(np.float32), X1c, X2c, K1, K2)
            e = float(max(e1[planted].max(), e2[planted].max()))
            if e < best_e:
                best, best_e = tri, e
        draws[k] = _draws_for(rng, n, best)
        P = dict(n=n, X1c=X1c, X2c=X2c, fix_scale=0, min_inliers=20, n_iter=300, draws=draws, best_inliers=0, planted=planted, k_found=k)
    elif case in ("no_return", "best_in_high"):
        n = 100
        X1c, X2c, planted, _ = _planted(rng, n, 0.9, 0.6, 0.2, K1, K2)
        draws = _well_conditioned_draws(rng, n, X1c, X2c, False, 8)
        draws[5] = draws[2]                      # the same triple again: the same count, and the later one must take over (>=)
        P = dict(n=n, X1c=X1c, X2c=X2c, fix_scale=0, min_inliers=n, n_iter=8, draws=draws, best_inliers=0 if case == "no_return" else 10 ** 6)
    elif case.startswith("deg_"):
        n = 40
        X1c, X2c, planted, _ = _planted(rng, n, 1.1, 0.6, 0.2, K1, K2)
        draws = _well_conditioned_draws(rng, n, X1c, X2c, False, 3)
        deg = np.zeros(3, bool)
        if case == "deg_identical3":
            for j in (1, 2):
                X1c[j], X2c[j] = X1c[0], X2c[0]
            draws[1] = _draws_for(rng, n, [0, 1, 2])
            deg[1] = True
        elif case == "deg_identical2":
            X1c[1], X2c[1] = X1c[0], X2c[0]
            draws[1] = _draws_for(rng, n, [0, 1, 7])
            deg[1] = True
        else:
            used = {i for j in range(3) for i in sample(draws[j], n)}
            free = [i for i in range(n) if i not in used]
            X1c[free[0], 2] = 0.0            # Z = 0 in camera 1: FromCameraToImage divides by it
            X2c[free[1], 2] = 0.0
            P_z0 = free[:2]
        P = dict(n=n, X1c=X1c, X2c=X2c, fix_scale=0, min_inliers=n, n_iter=3, draws=draws, best_inliers=0, degenerate=deg)
        if case == "deg_z0":
            P["z0_rows"] = P_z0
    elif case == "no_more":
        X1c, X2c, planted, _ = _planted(rng, 12, 1.0, 1.0, 0.2, K1, K2)
        P = dict(n=12, X1c=X1c, X2c=X2c, fix_scale=0, min_inliers=20, n_iter=5, draws=_well_conditioned_draws(rng, 12, X1c, X2c, False, 5), best_inliers=7)
    else:
        raise KeyError(case)
    n = P["n"]
    P.setdefault("degenerate", np.zeros(P["n_iter"], bool))
    P["K1"], P["K2"] = K1.copy(), K2.copy()
    P["max_err1"] = (9.210 * sig[rng.integers(0, 8, n)]).astype(np.float32)      # (float)(9.210 * sigma2)
    P["max_err2"] = (9.210 * sig[rng.integers(0, 8, n)]).astype(np.float32)
    if case.startswith("find_300"):
        P["max_err1"][:] = np.float32(9.210)     # level 0 everywhere: the margins asserted by the CPU test are margins to one threshold
        P["max_err2"][:] = np.float32(9.210)
    for v in P.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[case] = P
    return P


def reference_hypotheses(P):
    """per hypothesis of P: dict(idx, truth = horn in 80-bit, f64 = horn in float64 with eigh)"""
    out = []
    for d in P["draws"][:P["n_iter"]]:
        idx = sample(d, P["n"])
        with np.errstate(all="ignore"):
            truth = horn(P["X1c"][idx], P["X2c"][idx], P["fix_scale"])
            f64 = horn(P["X1c"][idx], P["X2c"][idx], P["fix_scale"], np.float64, use_eigh=True)
        out.append(dict(idx=idx, truth=truth, f64=f64))
    return out


def reference_counts(P):
    """inlier counts of every hypothesis under the reference alone: the 80-bit model rounded to f32, then check_inliers_f32"""
    counts, masks = [], []
    for h in reference_hypotheses(P):
        T12 = np.asarray(h["truth"]["T12"], np.float64).astype(np.float32)
        T21 = np.asarray(h["truth"]["T21"], np.float64).astype(np.float32)
        m = check_inliers_f32(T12, T21, P["X1c"], P["X2c"], P["K1"], P["K2"], P["max_err1"], P["max_err2"])
        counts.append(int(m.sum()))
        masks.append(m)
    return counts, masks
