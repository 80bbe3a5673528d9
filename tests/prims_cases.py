"""The inputs of the primitive tests, family by family, and the bars they are held to (tests/test_prims.py,
tests/test_prims_ref.py; stored with the exact outputs in tests/golden/prims_golden.npz by tests/golden/make_prims_golden.py).

A family is (op, inputs [n, width in]).  Families are kept apart so that an ill-conditioned one cannot loosen a well-conditioned one.
Needs numpy only; deterministic (seeded).
"""
import math

import numpy as np

from tests import prims_ref as pr

# ---- bars ------------------------------------------------------------------------------------------------------------------------------
# MEASURED["op@family"] = worst |f64 restatement - exact| / (u S) over the family, on the CPU (make_prims_golden.py prints them);
# BAR["op@family"] = 4 x that, rounded up to two digits: the device's sin / cos / acos / exp / log may take about 2 ulp where glibc
# takes under 1, and contraction and asd_rsqrt change the rounding, not its magnitude.  No device figure enters here.
MEASURED = {
    "quat_normalize@quat_normalize": 1.188,
    "rot_to_quat_eigen@rot_to_quat": 0.8897,
    "pose_oplus@pose_oplus_theta.t0": 1.245,
    "pose_oplus@pose_oplus_theta.t1": 1.522,
    "pose_oplus@pose_oplus_theta.t2": 9.161,
    "pose_oplus@pose_oplus_theta.t3": 3.439,
    "pose_oplus@pose_oplus_flip.t0": 1.501,
    "pose_oplus@pose_oplus_flip.t1": 1.425,
    "pose_oplus@pose_oplus_flip.t2": 11.4,
    "pose_oplus@pose_oplus_flip.t3": 1.502,
    "s3_exp@s3_exp.s0t0": 1.034,
    "s3_exp_eigen@s3_exp.s0t0": 1.034,
    "s3_exp@s3_exp.s0t1": 99160.0,
    "s3_exp_eigen@s3_exp.s0t1": 99160.0,
    "s3_exp@s3_exp.s0t2": 63.64,
    "s3_exp_eigen@s3_exp.s0t2": 63.64,
    "s3_exp@s3_exp.s0t3": 1.083,
    "s3_exp_eigen@s3_exp.s0t3": 1.083,
    "s3_exp@s3_exp.s1t0": 43690.0,
    "s3_exp_eigen@s3_exp.s1t0": 43690.0,
    "s3_exp@s3_exp.s1t1": 4434000.0,
    "s3_exp_eigen@s3_exp.s1t1": 4434000.0,
    "s3_exp@s3_exp.s1t2": 146900.0,
    "s3_exp_eigen@s3_exp.s1t2": 146900.0,
    "s3_exp@s3_exp.s1t3": 63820.0,
    "s3_exp_eigen@s3_exp.s1t3": 63820.0,
    "s3_exp@s3_exp.s2t0": 475.4,
    "s3_exp_eigen@s3_exp.s2t0": 475.4,
    "s3_exp@s3_exp.s2t1": 17510.0,
    "s3_exp_eigen@s3_exp.s2t1": 17510.0,
    "s3_exp@s3_exp.s2t2": 880.6,
    "s3_exp_eigen@s3_exp.s2t2": 880.6,
    "s3_exp@s3_exp.s2t3": 193.3,
    "s3_exp_eigen@s3_exp.s2t3": 193.3,
    "s3_exp@s3_exp.s3t0": 2.048,
    "s3_exp_eigen@s3_exp.s3t0": 2.048,
    "s3_exp@s3_exp.s3t1": 2.51,
    "s3_exp_eigen@s3_exp.s3t1": 2.51,
    "s3_exp@s3_exp.s3t2": 1.304,
    "s3_exp_eigen@s3_exp.s3t2": 1.304,
    "s3_exp@s3_exp.s3t3": 3.431,
    "s3_exp_eigen@s3_exp.s3t3": 3.431,
    "s3_log@s3_log.near_pi": 0.5825,
    "s3_log@s3_log.s0t0": 0.9446,
    "s3_log@s3_log.s0t2": 621.5,
    "s3_log@s3_log.s0t3": 116.5,
    "s3_log@s3_log.s1t0": 3613000000.0,
    "s3_log@s3_log.s1t2": 621.5,
    "s3_log@s3_log.s1t3": 116.5,
    "s3_log@s3_log.s2t0": 1072.0,
    "s3_log@s3_log.s2t2": 621.5,
    "s3_log@s3_log.s2t3": 116.5,
    "s3_log@s3_log.s3t0": 1.048,
    "s3_log@s3_log.s3t2": 621.5,
    "s3_log@s3_log.s3t3": 116.5,
    "s3_oplus@s3_oplus.s0t0": 1.167,
    "s3_oplus_eigen@s3_oplus.s0t0": 1.036,
    "s3_oplus@s3_oplus.s0t1": 15110.0,
    "s3_oplus_eigen@s3_oplus.s0t1": 15110.0,
    "s3_oplus@s3_oplus.s0t2": 29.55,
    "s3_oplus_eigen@s3_oplus.s0t2": 29.55,
    "s3_oplus@s3_oplus.s0t3": 1.196,
    "s3_oplus_eigen@s3_oplus.s0t3": 1.196,
    "s3_oplus@s3_oplus.s1t0": 43690.0,
    "s3_oplus_eigen@s3_oplus.s1t0": 43690.0,
    "s3_oplus@s3_oplus.s1t1": 43690.0,
    "s3_oplus_eigen@s3_oplus.s1t1": 43690.0,
    "s3_oplus@s3_oplus.s1t2": 2208.0,
    "s3_oplus_eigen@s3_oplus.s1t2": 2208.0,
    "s3_oplus@s3_oplus.s1t3": 43690.0,
    "s3_oplus_eigen@s3_oplus.s1t3": 43690.0,
    "s3_oplus@s3_oplus.s2t0": 180.5,
    "s3_oplus_eigen@s3_oplus.s2t0": 180.5,
    "s3_oplus@s3_oplus.s2t1": 468.0,
    "s3_oplus_eigen@s3_oplus.s2t1": 468.0,
    "s3_oplus@s3_oplus.s2t3": 180.4,
    "s3_oplus_eigen@s3_oplus.s2t3": 180.4,
    "s3_oplus@s3_oplus.s3t0": 1.376,
    "s3_oplus_eigen@s3_oplus.s3t0": 1.376,
    "s3_oplus@s3_oplus.s3t1": 1.488,
    "s3_oplus_eigen@s3_oplus.s3t1": 1.488,
    "s3_oplus@s3_oplus.s3t2": 0.6262,
    "s3_oplus_eigen@s3_oplus.s3t2": 0.6262,
    "s3_oplus@s3_oplus.s3t3": 1.181,
    "s3_oplus_eigen@s3_oplus.s3t3": 1.181,
    "s3_edge_error@s3_edge_error": 22.2,
    "quat_rotate@quat_rotate": 0.6497,
    "pose_map@pose_map": 0.6294,
    "jac_pose@jac_pose": 0.7226,
    "huber@huber": 1.0,
}


def round_up_2(v):
    """v rounded up to two significant digits"""
    if v <= 0:
        return 0.0
    e = math.floor(math.log10(v)) - 1
    return math.ceil(v / 10 ** e - 1e-9) * 10 ** e


BAR = {k: round_up_2(4 * v) for k, v in MEASURED.items()}
RSQRT_ULPS = 2   # asd_rsqrt: the header's own claim, at most 2 ulp of the correctly rounded 1 / sqrt(x)

# the families held to a bar (transcendentals or the device rsqrt); the others are compared bit for bit
TOLERANCE_OPS = ("quat_normalize", "pose_oplus", "rot_to_quat_eigen", "s3_exp", "s3_exp_eigen", "s3_log", "s3_oplus", "s3_oplus_eigen",
                 "s3_edge_error")


def _up(v, k=1):
    v = np.float64(v)
    for _ in range(k):
        v = np.nextafter(v, np.inf)
    return v


def _dn(v, k=1):
    v = np.float64(v)
    for _ in range(k):
        v = np.nextafter(v, -np.inf)
    return v


def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _quat_axis_angle(axis, theta):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([axis * math.sin(theta / 2), [math.cos(theta / 2)]])


def _rot(q):
    return pr.f64("s3_rot_of_quat", np.concatenate([q, [0, 0, 0, 1]]))[0]


def _theta2_hit(target, split=0.64):
    """(wx, wy) with fl(fl(wx wx) + fl(wy wy)) == target exactly: the f64 theta^2 of pose_oplus for omega = (wx, wy, 0)"""
    target = np.float64(target)
    wx = np.float64(math.sqrt(target * split))
    wy0 = np.float64(math.sqrt(target - wx * wx))
    wy = wy0 + np.arange(-20000, 20001) * np.spacing(wy0)
    hit = np.nonzero(wx * wx + wy * wy + np.float64(0) == target)[0]   # (elementwise numpy: one rounding per operation)
    if not len(hit):
        raise RuntimeError(f"no omega hits theta^2 = {target!r}")
    return wx, wy[hit[len(hit) // 2]]


def _poses(rng, n, tmag=1.0):
    return np.concatenate([_unit(rng, n, 4), tmag * rng.standard_normal((n, 3))], axis=1)


def _sim3s(rng, n, max_angle=math.pi, smin=0.1, smax=10.0, tmag=1.0):
    q = np.array([_quat_axis_angle(a, t) for a, t in zip(_unit(rng, n, 3), rng.uniform(-max_angle, max_angle, n))])
    s = np.exp(rng.uniform(math.log(smin), math.log(smax), n))
    return np.concatenate([q, tmag * rng.standard_normal((n, 3)), s[:, None]], axis=1)


# the angles of the pose_oplus families; the threshold values are the f64 theta^2 the code compares
POSE_OPLUS_THETA2_EXACT = [np.float64(0), _dn(1e-10), np.float64(1e-10), _dn(0.01), np.float64(0.01)]
POSE_OPLUS_THETAS = [1e-8, 1e-4, 1e-2, 0.1, 1.0, 3.0, math.pi - 1e-3, 2 * math.pi - 1e-3, 2 * math.pi + 1e-3, 10.0]


def _omegas(rng):
    """rotation vectors: every listed angle along the three coordinate axes and two random ones, and every listed f64 theta^2
    hit exactly, in the (x, y), (y, z) and (z, x) planes"""
    axes = np.concatenate([np.eye(3), _unit(rng, 2, 3)])
    out = [np.zeros(3)]
    for th in POSE_OPLUS_THETAS:
        out += [a * th for a in axes]
    for t2 in POSE_OPLUS_THETA2_EXACT[1:]:
        for split in (0.64, 0.8):
            wx, wy = _theta2_hit(t2, split)
            out += [np.array([wx, wy, 0.0]), np.array([0.0, wx, wy]), np.array([-wy, 0.0, wx])]
    return np.array(out)


def _rot_cases(rng):
    """3x3 inputs of the matrix -> quaternion conversions: every branch, the ties, and matrices that are not quite rotations (the
    functions take what they are given: s3_exp feeds I + W + W^2)"""
    R = []
    for q in _unit(rng, 24, 4):                       # mostly trace > 0 and a few below
        R.append(_rot(q))
    perm = np.array([0, 0, 1, 1, 0, 0, 0, 1, 0], np.float64)   # 120 degrees about (1,1,1): trace exactly 0, a three-way tie -> i = 0
    R.append(perm)
    for k in range(9):                                 # the same with one entry moved: the branches' formulas no longer agree
        P = perm.copy()
        if k % 4 != 0:
            P[k] += 1e-3
        R.append(P)
    R.append(perm.reshape(3, 3).T.ravel().copy())
    for ax in range(3):                                # trace < 0 with each diagonal entry the largest: near pi about each axis, and tilted
        for th in (math.pi, math.pi - 1e-3, 3.0, 2.5):
            a = np.zeros(3)
            a[ax] = 1.0
            R.append(_rot(_quat_axis_angle(a, th)))
            R.append(_rot(_quat_axis_angle(a + 0.2 * rng.standard_normal(3), th)))
    # ties on the diagonal with trace <= 0: R[4] == R[0] > R[8] must take i = 0, R[8] == R[4] > R[0] must take i = 1
    for d0, d1, d2 in ((0.25, 0.25, -0.75), (-0.75, 0.25, 0.25), (0.25, -0.75, 0.25), (-0.2, -0.2, -0.2), (0.0, 0.0, -0.5)):
        M = 0.3 * rng.standard_normal(9)
        M[0], M[4], M[8] = d0, d1, d2
        R.append(M)
    for _ in range(12):                                # trace a rounding away from 0 on either side
        M = 0.5 * rng.standard_normal(9)
        M[8] = -(M[0] + M[4])
        R.append(M.copy())
        M[8] = _up(M[8], 2)
        R.append(M.copy())
        M[8] = _dn(M[8], 4)
        R.append(M.copy())
    return np.array(R)


def _exp_updates(rng):
    eps = np.float64(1e-5)
    thetas = [0.0, 1e-8, _dn(eps), eps, _up(eps), 9.5e-6, 1e-4, 1e-2, 0.5, 1.0, 2.0, 3.0]
    sigmas = [0.0, 1e-9, _dn(eps), eps, _up(eps), -_dn(eps), -eps, -_up(eps), 1e-3, -1e-3, 0.3, -0.7, 2.0, -2.0]
    axes = np.concatenate([np.eye(3), _unit(rng, 1, 3)])
    out = []
    for th in thetas:
        for sg in sigmas:
            for a in (axes if th in (_dn(eps), eps, _up(eps)) else axes[[0, 3]]):
                out.append(np.concatenate([a * th, rng.standard_normal(3), [sg]]))
    return np.array(out)


def _d_of(S):
    R = pr.f64("s3_rot_of_quat", S)[0]
    return np.float64(0.5) * (R[0] + R[4] + R[8] - np.float64(1))


def _log_threshold_quats():
    """quaternions whose f64 d = (trace - 1) / 2 is one ulp either side of 1 - eps.  (1 - eps itself is no value d takes: the trace is
    summed near 3, where floats are 2^-51 apart, so d moves in steps of 2^-52, and 1 - eps is an odd multiple of 2^-53.)"""
    T = np.float64(1) - np.float64(0.00001)
    th = math.acos(float(T)) + np.arange(-4000, 4001) * 5e-16      # one ulp of d is about 50 of these steps
    out = []
    for t in (_dn(T), _up(T)):
        for axis in ((1, 1, 1), (1, 2, 3), (0, 0, 1), (3, -1, 2)):   # (about one axis alone d moves in steps of two ulps)
            a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
            x, y, z, w = a[0] * np.sin(th / 2), a[1] * np.sin(th / 2), a[2] * np.sin(th / 2), np.cos(th / 2)
            txx, tyy, tzz = (2 * x) * x, (2 * y) * y, (2 * z) * z     # the diagonal of s3_rot_of_quat, elementwise
            d = 0.5 * ((1 - (tyy + tzz)) + (1 - (txx + tzz)) + (1 - (txx + tyy)) - 1)
            hit = np.nonzero(d == t)[0]
            if len(hit):
                k = hit[len(hit) // 2]
                out.append(np.array([x[k], y[k], z[k], w[k]]))
                break
        else:
            raise RuntimeError(f"no quaternion hits d = {t!r}")
        assert _d_of(np.concatenate([out[-1], [0, 0, 0, 1.0]])) == t
    return out


def _log_inputs(rng, near_pi):
    out = []
    if near_pi:
        for th in (3.0001, 3.05, 3.1, 3.14, math.pi - 1e-3, math.pi - 1e-5):
            for a in np.concatenate([np.eye(3), _unit(rng, 2, 3)]):
                for s in (1.0, 1.3):
                    out.append(np.concatenate([_quat_axis_angle(a, th), rng.standard_normal(3), [s]]))
        return np.array(out)
    scales = [1.0, _up(1.0), _dn(1.0), math.exp(1e-5), _up(math.exp(1e-5), 3), _dn(math.exp(1e-5), 3), math.exp(-1e-5), _dn(math.exp(-1e-5), 3),
              1.001, 0.999, 0.1, 0.5, 2.0, 7.389, 10.0]
    for q in _log_threshold_quats():
        for s in scales:
            out.append(np.concatenate([q, rng.standard_normal(3), [s]]))
    for th in (0.0, 1e-8, 1e-4, 4e-3, 5e-3, 1e-2, 0.5, 1.0, 2.0, 3.0):
        for a in np.concatenate([np.eye(3)[:1], _unit(rng, 1, 3)]):
            for s in scales[::2]:
                out.append(np.concatenate([_quat_axis_angle(a, th), rng.standard_normal(3), [s]]))
    for k in range(40):   # off unit norm by up to 1e-6: the struct is not renormalised
        q = _quat_axis_angle(_unit(rng, 1, 3)[0], rng.uniform(0, 3.0)) * (1 + rng.uniform(-1e-6, 1e-6))
        out.append(np.concatenate([q, rng.standard_normal(3), [scales[k % len(scales)]]]))
    return np.array(out)


def _lu_cases(rng):
    out = []
    seen = {}
    while min([seen.get(k, 0) for k in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1))]) < 6:   # (first pivot row, second swap)
        x = rng.standard_normal(12)
        rec = pr._f64_item("s3_lu_solve3", x)[1]
        key = (2 if rec[1] else 1 if rec[0] else 0, int(rec[2]))
        if seen.get(key, 0) < 6:
            seen[key] = seen.get(key, 0) + 1
            out.append(x)
    for k in range(12):   # ties: first column (rows 0-1, 0-2, 1-2, all three), second column after elimination
        x = rng.standard_normal(12)
        v = abs(x[0]) + 1.0
        sg = -1.0 if k % 2 else 1.0
        if k % 4 == 0: x[0], x[3] = v, sg * v
        if k % 4 == 1: x[0], x[6] = v, -sg * v
        if k % 4 == 2: x[3], x[6] = v, sg * v
        if k % 4 == 3: x[0], x[3], x[6] = v, -v, v
        out.append(x)
    for k in range(6):    # second column tie: rows 1 and 2 equal up to sign below a dominant first row
        x = rng.standard_normal(12)
        x[0], x[3], x[6] = 4.0, 0.0, 0.0
        x[7] = x[4] if k % 2 else -x[4]
        out.append(x)
    for k in range(6):    # a 1e-12 leading entry
        x = rng.standard_normal(12)
        x[0] = 1e-12 if k % 2 else -1e-12
        out.append(x)
    out.append(np.array([1, 2, 3, 2, 4, 6, 1, 0, 1, 1, 2, 3], np.float64))     # exactly singular: rank 2
    out.append(np.array([1, 2, 3, 2, 4, 6, 3, 6, 9, 1, 1, 1], np.float64))     # rank 1
    out.append(np.zeros(12))                                                   # rank 0
    return np.array(out)


def _solve7_cases(rng):
    out = []

    def spd():
        M = rng.standard_normal((7, 7))
        return M @ M.T + 0.5 * np.eye(7)

    for k in range(12):
        out.append(np.concatenate([spd().ravel(), [0.0 if k % 2 else 10.0 ** rng.uniform(-5, 2)], rng.standard_normal(7)]))
    for j in range(7):   # a non-positive pivot at j (the pivots in front of it stay those of the SPD matrix), and the lambda that cures it
        H = spd()
        h = H[j, j]
        H[j, j] = -h
        b = rng.standard_normal(7)
        out.append(np.concatenate([H.ravel(), [0.0], b]))
        out.append(np.concatenate([H.ravel(), [1e-5 * h], b]))
        out.append(np.concatenate([H.ravel(), [2.5 * h], b]))
    Z = spd()
    Z[0, :] = 0
    Z[:, 0] = 0
    out.append(np.concatenate([Z.ravel(), [0.0], rng.standard_normal(7)]))   # a pivot of exactly 0
    out.append(np.concatenate([Z.ravel(), [1.0], rng.standard_normal(7)]))
    return np.array(out)


def _huber_cases(rng):
    out = []
    # delta < 0 is no robust kernel, but it is what makes the comparison observable at the kink: for delta > 0 both sides give the
    # same bits at e2 == delta^2 (sqrt(fl(d d)) == d in binary IEEE arithmetic, so 2 s d - d^2 == e2 and d / s == 1)
    for delta in (math.sqrt(5.991), math.sqrt(7.815), 1.0, 0.1, 3.0, 1e-3, -math.sqrt(5.991), -1.0, -0.37):
        d2 = np.float64(delta) * np.float64(delta)
        for e2 in (d2, _dn(d2), _up(d2), 0.0, 0.5 * d2, 2 * d2, 100 * d2, 5.991, 7.815):
            out.append([e2, delta])
    return np.array(out, np.float64)


def families():
    """name -> (ops, inputs): every op of `ops` runs on the inputs; the first one is the one whose exact outputs are stored"""
    rng = np.random.default_rng(20261020)
    F = {}
    F["asd_rsqrt"] = ("asd_rsqrt", np.concatenate([1 + 3 * (np.arange(256) + rng.uniform(0, 1, 256)) / 256, 10.0 ** np.arange(-200, 201, 5)])[:, None])
    q = _unit(rng, 48, 4) * (10.0 ** rng.uniform(-3, 3, 48))[:, None]
    q[:24, 3] = -np.abs(q[:24, 3])
    q[40:44, 3] = [0.0, -0.0, 5e-324, -5e-324]
    F["quat_normalize"] = ("quat_normalize", q)
    Rc = _rot_cases(rng)
    F["rot_to_quat"] = ("rot_to_quat_eigen", Rc)

    # pose_oplus by theta: each rotation vector with translations of magnitude 0, 1e-3 and 10 on a random pose
    om = _omegas(rng)
    rows = []
    for w in om:
        for tm in (0.0, 1e-3, 10.0):
            rows.append(np.concatenate([_poses(rng, 1)[0], w, tm * _unit(rng, 1, 3)[0]]))
    F["pose_oplus_theta"] = ("pose_oplus", np.array(rows))
    # pose_oplus whose product comes out with qw < 0 (the flip of the last quat_normalize), and poses at pi rotations
    rows = []
    for w in om[::5]:
        th = float(np.linalg.norm(w))
        e = _quat_axis_angle(w if th > 0 else [1, 0, 0], th)
        for k in range(3):
            a = _unit(rng, 1, 3)[0]
            qT = _quat_axis_angle(a, math.pi if k == 0 else rng.uniform(2.0, 3.1))
            prod_w = e[3] * qT[3] - e[:3] @ qT[:3]
            if prod_w > 0 and k > 0:
                qT = np.concatenate([-qT[:3], [qT[3]]]) if (e[3] * qT[3] + e[:3] @ qT[:3]) < 0 else -qT   # -q is the same rotation
            rows.append(np.concatenate([qT, rng.standard_normal(3), w, rng.standard_normal(3)]))
    F["pose_oplus_flip"] = ("pose_oplus", np.array(rows))

    U = _exp_updates(rng)
    F["s3_exp"] = ("s3_exp", U)
    F["s3_log"] = ("s3_log", np.concatenate([_log_inputs(rng, False), _log_inputs(rng, True)]))   # (theta > 3: a class of its own)
    est = _sim3s(rng, len(U), max_angle=1.0)
    O = np.concatenate([est, U, (np.arange(len(U)) % 2)[:, None].astype(np.float64)], axis=1)[::3]
    F["s3_oplus"] = ("s3_oplus", O)
    n = 64
    Cm, Si = _sim3s(rng, n, 1.0), _sim3s(rng, n, 1.0)
    # Sj = (C Si) moved by a moderate update, so that the error's angle stays below 3 (above it: s3_log_near_pi)
    upd = np.concatenate([_unit(rng, n, 3) * rng.uniform(0, 2.5, n)[:, None], rng.standard_normal((n, 3)), rng.uniform(-1, 1, n)[:, None]], 1)
    upd[:8, :3] *= 1e-7
    upd[:4, 6] = 0
    CS = pr.f64("s3_mul_eigen", np.concatenate([Cm, Si], 1))
    Sj = pr.f64("s3_oplus_eigen", np.concatenate([CS, upd, np.zeros((n, 1))], 1))
    F["s3_edge_error"] = ("s3_edge_error", np.concatenate([Cm, Si, Sj], 1))

    n = 48
    F["quat_rotate"] = ("quat_rotate", np.concatenate([_unit(rng, n, 4), rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 2, (n, 1))], 1))
    F["pose_map"] = ("pose_map", np.concatenate([_poses(rng, n), rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 2, (n, 1))], 1))
    z = np.concatenate([[1e-3, -1e-3, 1e-3], 10.0 ** rng.uniform(-3, 2, n - 3)])
    F["jac_pose"] = ("jac_pose", np.concatenate([rng.standard_normal((n, 2)) * z[:, None], z[:, None], rng.uniform(300, 800, (n, 2))], 1))
    A, Bm = _sim3s(rng, n), _sim3s(rng, n)
    F["s3_mul"] = ("s3_mul", np.concatenate([A, Bm], 1))
    F["s3_inverse"] = ("s3_inverse", A)
    F["s3_rot_of_quat"] = ("s3_rot_of_quat", A * np.concatenate([1 + rng.uniform(-1e-6, 1e-6, (n, 1))] * 4 + [np.ones((n, 4))], 1))
    X = rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-3, 2, (n, 1))
    F["s3_map"] = ("s3_map", np.concatenate([A, X], 1))
    # projections: points in front of the camera with depths from 1e-3 up
    S0 = _sim3s(rng, n, max_angle=0.3, tmag=0.0)
    Xc = np.concatenate([rng.standard_normal((n, 2)), np.ones((n, 1))], 1) * z[:, None]
    K = np.concatenate([rng.uniform(300, 800, (n, 2)), rng.uniform(200, 600, (n, 2))], 1)
    F["s3_project_error"] = ("s3_project_error", np.concatenate([S0, Xc, rng.uniform(0, 1000, (n, 2)), K], 1))
    F["s3_chi2"] = ("s3_chi2", np.concatenate([rng.standard_normal((n, 2)) * 10.0 ** rng.uniform(-3, 2, (n, 1)), 1.2 ** -rng.integers(0, 16, (n, 1))], 1))
    F["s3_lu_solve3"] = ("s3_lu_solve3", _lu_cases(rng))
    F["s3_solve7"] = ("s3_solve7", _solve7_cases(rng))
    F["huber"] = ("huber", _huber_cases(rng))
    out = {}
    for k, (op, x) in F.items():
        x = np.ascontiguousarray(x, np.float64)
        ops = SAME_INPUTS.get(op, (op,))
        if op not in _SPLIT_OPS:
            out[k] = (ops, x)
            continue
        cls = np.array([condition_class(op, row) for row in x])
        for c in sorted(set(cls)):
            out[f"{k}.{c}"] = (ops, np.ascontiguousarray(x[cls == c]))
    return out


# ops that take the same inputs run on one family (the exact value does not depend on the association, so it is stored once)
SAME_INPUTS = {"s3_exp": ("s3_exp", "s3_exp_eigen"), "s3_oplus": ("s3_oplus", "s3_oplus_eigen"), "s3_mul": ("s3_mul", "s3_mul_eigen"),
               "rot_to_quat_eigen": ("rot_to_quat_eigen", "s3_quat_of_rot", "s3_quat_of_rot_eigen")}


# g2o's formulas cancel next to their own thresholds: (s - 1) / sigma and ((sigma - 1) s + 1) / sigma^2 lose u / sigma and u / sigma^2
# just above |sigma| = 1e-5, (1 - cos theta) / theta^2 and (theta - sin theta) / theta^3 lose u / theta^2 and u / theta^3 just above
# theta = 1e-5 (pose_oplus: above theta = 0.1, where its series ends).  That noise belongs to the formula, so the header and its f64
# restatement both carry it; the families of these ops are split by where sigma and theta lie, so that the cases which have it
# cannot loosen the bar of those which do not.  `s` by |sigma|: s0 < 1e-5 <= s1 < 1e-4 <= s2 < 0.1 <= s3; `t` by theta:
# t0 < 1e-5 <= t1 < 1e-3 <= t2 < 0.05 <= t3 (pose_oplus, by its own branches: t0 theta^2 < 1e-10 <= t1 < 0.01 <= t2, theta < 0.5 <= t3).
_SPLIT_OPS = ("pose_oplus", "s3_exp", "s3_log", "s3_oplus")


def _sclass(sigma):
    a = abs(np.float64(sigma))
    return "s0" if a < _EPS else "s1" if a < 1e-4 else "s2" if a < 0.1 else "s3"


def _tclass(theta):
    return "t0" if theta < _EPS else "t1" if theta < 1e-3 else "t2" if theta < 0.05 else "t3"


_EPS = np.float64(0.00001)


def condition_class(op, row):
    """where the case lies among the formulas' thresholds, from the f64 quantities the code itself compares"""
    row = np.asarray(row, np.float64)
    if op == "pose_oplus":
        w = row[7:10]
        t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
        return "t0" if t2 < 1e-10 else "t1" if t2 < 0.01 else "t2" if t2 < 0.25 else "t3"
    if op == "s3_log":
        sigma = np.float64(math.log(row[7]))
        d = _d_of(row)
        if d > np.float64(1) - _EPS:
            return _sclass(sigma) + "t0"
        theta = math.acos(d)
        return "near_pi" if theta > 3 else _sclass(sigma) + max(_tclass(theta), "t1")
    u = row[8:15] if op.startswith("s3_oplus") else row
    sigma = 0.0 if op.startswith("s3_oplus") and row[15] != 0 else u[6]
    return _sclass(sigma) + _tclass(np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]))


# the se3.h ops that are algebraic but also exist in the contracted build: there the device fuses multiply-adds, so they are held to
# a bar against exact like the others (their contract-off instantiation is compared bit for bit)
FUSED_BOUND_OPS = ("quat_rotate", "pose_map", "huber", "jac_pose")


def pose_oplus_other_side(x):
    """(rows, inputs) -- the rows of pose_oplus inputs whose f64 theta^2 lies within 4 ulp of 1e-10, and the same inputs with omega
    nudged across that threshold.  Contraction rounds theta^2 itself differently (fma(wx, wx, fma(wy, wy, wz wz))), so in the
    contracted build such a row may take the branch of the other side, and g2o's formula jumps there: V = I + W + W^2 below,
    I + W / 2 + W^2 / 6 above, 0.5 |omega x upsilon| apart.  For these rows that build is held to the exact value of either side."""
    x = np.asarray(x, np.float64)
    w = x[:, 7:10]
    t2 = w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]
    rows = np.nonzero(np.abs(t2 - 1e-10) <= 4 * np.spacing(np.float64(1e-10)))[0]
    y = x[rows].copy()
    y[:, 7:10] *= np.where(t2[rows] < 1e-10, 1 + 1e-12, 1 - 1e-12)[:, None]
    return rows, y


def has_exact(op):
    return op in TOLERANCE_OPS or op in FUSED_BOUND_OPS or op == "asd_rsqrt"
