"""Plain restatements of the fp64 primitives of csrc/se3.h and csrc/sim3_math.h -- the yardstick of tests/test_prims.py and
tests/test_prims_ref.py.  Owned by this project: no g2o, no oracle.

Each op is written ONCE, operation for operation in the header's association, over an arithmetic `B`:

  * F64   -- numpy float64 scalars: one IEEE rounding per operation, no FMA, glibc's libm for the transcendentals.  `f64(op, x)`.
             The bit reference of the algebraic ops (+ - * / sqrt only) and the noise yardstick of the others.
  * EXACT -- mpmath at 60 digits: the same formula without rounding.  `exact(op, x)`.  Every comparison of the header (the eps
             branches, pivot choices, sign flips) is taken from the F64 run of the same input and replayed, so the branch is the one
             the code takes on the f64 input, also at a threshold.  Two places depart from the formula, where the header departs
             from g2o for accuracy: the series branch of pose_oplus is the TRUE exponential map and V matrix there, and asd_rsqrt
             is the true 1/sqrt(x).

`exact` also returns the sensitivity scale of every output, S_i = |f_i| + sum_j |df_i/dx_j| |x_j| (central differences in mpmath,
with the branches held): the error measure of the tests is |got_i - exact_i| / (u S_i), u = 2^-53 -- rounding of the inputs alone
moves f_i by about u S_i, so a figure of a few units is a well-behaved evaluation whatever the conditioning of the case.

`mut` seeds one deliberate mistake (tests/test_prims_ref.py proves that the checks fail on each of them).
"""
import math

import numpy as np

try:
    import mpmath
    mpmath.mp.dps = 60
except ImportError:   # the GPU tests read the stored golden and do not need it
    mpmath = None

U = 2.0 ** -53

# op -> (doubles in, doubles out); the order of asd_debug_prim's enum
OPS = [("asd_rsqrt", 1, 1), ("quat_normalize", 4, 4), ("quat_rotate", 7, 3), ("pose_map", 10, 3), ("pose_oplus", 13, 7),
       ("rot_to_quat_eigen", 9, 4), ("huber", 2, 2), ("jac_pose", 5, 12), ("s3_exp", 7, 8), ("s3_exp_eigen", 7, 8), ("s3_log", 8, 7),
       ("s3_mul", 16, 8), ("s3_mul_eigen", 16, 8), ("s3_inverse", 8, 8), ("s3_map", 11, 3), ("s3_oplus", 16, 8),
       ("s3_oplus_eigen", 16, 8), ("s3_quat_of_rot", 9, 4), ("s3_quat_of_rot_eigen", 9, 4), ("s3_rot_of_quat", 8, 9),
       ("s3_lu_solve3", 12, 3), ("s3_edge_error", 24, 7), ("s3_project_error", 17, 2), ("s3_chi2", 3, 1), ("s3_solve7", 57, 8)]
WIDTH = {name: (wi, wo) for name, wi, wo in OPS}
# + - * / sqrt only: IEEE arithmetic without contraction fixes every bit
ALGEBRAIC = ("quat_rotate", "pose_map", "huber", "jac_pose", "s3_mul", "s3_mul_eigen", "s3_inverse", "s3_map", "s3_quat_of_rot",
             "s3_quat_of_rot_eigen", "s3_rot_of_quat", "s3_lu_solve3", "s3_project_error", "s3_chi2", "s3_solve7")

MUTANTS = ("drop_720", "closed_below_eps", "trace_ge", "lu_no_pivot", "lu_last_wins", "lu_one_by_one", "plain_quat_product", "huber_lt")


class F64:
    exact = False
    c = staticmethod(np.float64)
    sqrt = staticmethod(lambda x: np.float64(np.sqrt(x)))
    sin = staticmethod(lambda x: np.float64(math.sin(x)))
    cos = staticmethod(lambda x: np.float64(math.cos(x)))
    acos = staticmethod(lambda x: np.float64(math.acos(x)))
    exp = staticmethod(lambda x: np.float64(math.exp(x)))
    log = staticmethod(lambda x: np.float64(math.log(x)))


class EXACT:
    exact = True
    c = staticmethod(lambda v: mpmath.mpf(float(v)) if not isinstance(v, mpmath.mpf) else v)
    sqrt = staticmethod(lambda x: mpmath.sqrt(x))
    sin = staticmethod(lambda x: mpmath.sin(x))
    cos = staticmethod(lambda x: mpmath.cos(x))
    acos = staticmethod(lambda x: mpmath.acos(x))
    exp = staticmethod(lambda x: mpmath.exp(x))
    log = staticmethod(lambda x: mpmath.log(x))


class Branches:
    """the comparisons of one evaluation: recorded in the F64 run, replayed (in the same order) in the EXACT runs"""

    def __init__(self, rec=None):
        self.replay = rec is not None
        self.rec = [] if rec is None else rec
        self.i = 0

    def __call__(self, cond):
        if self.replay:
            v = self.rec[self.i]
            self.i += 1
            return v
        self.rec.append(bool(cond))
        return self.rec[-1]


# ---------------------------------------------------------------------------------------------------------------- se3.h
def asd_rsqrt(B, br, x, mut=None):
    return B.c(1) / B.sqrt(x)   # the host's expression; EXACT: the true value


def quat_normalize(B, br, x, y, z, w, mut=None):
    if br(w < 0):
        x, y, z, w = -x, -y, -z, -w
    inv = asd_rsqrt(B, br, x * x + y * y + z * z + w * w)
    return x * inv, y * inv, z * inv, w * inv


def rot_of_quat(B, qx, qy, qz, qw):   # quat_to_rot and s3_rot_of_quat: Eigen's toRotationMatrix
    one = B.c(1)
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz, tyy, tyz, tzz = tx * qx, ty * qx, tz * qx, ty * qy, tz * qy, tz * qz
    return [one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx, one - (txx + tyy)]


def quat_rotate(B, qx, qy, qz, qw, v):
    ux, uy, uz = qy * v[2] - qz * v[1], qz * v[0] - qx * v[2], qx * v[1] - qy * v[0]
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return [v[0] + qw * ux + (qy * uz - qz * uy), v[1] + qw * uy + (qz * ux - qx * uz), v[2] + qw * uz + (qx * uy - qy * ux)]


def pose_map(B, br, T, X, mut=None):
    o = quat_rotate(B, T[0], T[1], T[2], T[3], X)
    return [o[0] + T[4], o[1] + T[5], o[2] + T[6]]


def _largest_diagonal(br, R):
    i = 0
    if br(R[4] > R[0]):
        i = 1
    if br(R[8] > (R[0] if i == 0 else R[4])):
        i = 2
    return i


def rot_to_quat_eigen(B, br, R, mut=None):
    half, one = B.c(0.5), B.c(1)
    tr = R[0] + R[4] + R[8]
    if br(tr >= 0 if mut == "trace_ge" else tr > 0):
        rs = asd_rsqrt(B, br, tr + one)
        ew = half * ((tr + one) * rs)
        s = half * rs
        return (R[7] - R[5]) * s, (R[2] - R[6]) * s, (R[3] - R[1]) * s, ew
    i = _largest_diagonal(br, R)
    if i == 0:
        s = B.sqrt(R[0] - R[4] - R[8] + one)
        ex, s = half * s, half / s
        return ex, (R[3] + R[1]) * s, (R[6] + R[2]) * s, (R[7] - R[5]) * s
    if i == 1:
        s = B.sqrt(R[4] - R[8] - R[0] + one)
        ey, s = half * s, half / s
        return (R[1] + R[3]) * s, ey, (R[7] + R[5]) * s, (R[2] - R[6]) * s
    s = B.sqrt(R[8] - R[0] - R[4] + one)
    ez, s = half * s, half / s
    return (R[2] + R[6]) * s, (R[5] + R[7]) * s, ez, (R[3] - R[1]) * s


def _skew(B, wx, wy, wz):
    z = B.c(0)
    O = [z, -wz, wy, wz, z, -wx, -wy, wx, z]
    O2 = [O[i * 3] * O[j] + O[i * 3 + 1] * O[3 + j] + O[i * 3 + 2] * O[6 + j] for i in range(3) for j in range(3)]
    return O, O2


def _horner(B, q, coef):   # c0 + q (c1 + q (c2 + ...)): the constants are f64 quotients, as the compiler folds them
    acc = coef[-1]
    for c in coef[-2::-1]:
        acc = c + q * acc
    return acc


def _series_coef(B, mut):
    c, o = B.c, B.c(1)
    b = [c(0.5), -o / 24, o / 720, -o / 40320, o / 3628800, -o / 479001600, o / c(87178291200.0)]
    if mut == "drop_720":
        b[2] = c(0)
    cc = [o / 6, -o / 120, o / 5040, -o / 362880, o / 39916800, -o / c(6227020800.0), o / c(1307674368000.0)]
    sh = [c(0.5), -o / 48, o / 3840, -o / 645120, o / 185794560, -o / c(81749606400.0), o / c(51011754393600.0)]
    ch = [o, -o / 8, o / 384, -o / 46080, o / 10321920, -o / c(3715891200.0), o / c(1961990553600.0)]
    return b, cc, sh, ch


def pose_oplus(B, br, T, u, mut=None):
    one, zero = B.c(1), B.c(0)
    wx, wy, wz = u[0], u[1], u[2]
    theta2 = wx * wx + wy * wy + wz * wz
    O, O2 = _skew(B, wx, wy, wz)
    eye = [one if i % 4 == 0 else zero for i in range(9)]
    small = br(theta2 < 1e-10)
    if small and mut != "closed_below_eps":   # R = I + W + W^2, V = R
        R = [eye[i] + O[i] + O2[i] for i in range(9)]
        V = list(R)
        ex, ey, ez, ew = quat_normalize(B, br, *rot_to_quat_eigen(B, br, R))
    elif not small and br(theta2 < 0.01):
        if B.exact:   # the true functions: the header's series is an accuracy departure from g2o, not a formula to restate
            th = B.sqrt(theta2)
            b, c = (one - B.cos(th)) / theta2, (th - B.sin(th)) / (theta2 * th)
            sh, ch = B.sin(th / 2) / th, B.cos(th / 2)
        else:
            b, c, sh, ch = (_horner(B, theta2, k) for k in _series_coef(B, mut))
        V = [eye[i] + b * O[i] + c * O2[i] for i in range(9)]
        ex, ey, ez, ew = wx * sh, wy * sh, wz * sh, ch
    else:
        itheta = asd_rsqrt(B, br, theta2)
        theta = theta2 * itheta
        sn, cs = B.sin(theta), B.cos(theta)
        it2 = itheta * itheta
        a, b = sn * itheta, (one - cs) * it2
        c = (theta - sn) * it2 * itheta
        R = [eye[i] + a * O[i] + b * O2[i] for i in range(9)]
        V = [eye[i] + b * O[i] + c * O2[i] for i in range(9)]
        ex, ey, ez, ew = quat_normalize(B, br, *rot_to_quat_eigen(B, br, R))
    et = [V[0] * u[3] + V[1] * u[4] + V[2] * u[5], V[3] * u[3] + V[4] * u[4] + V[5] * u[5], V[6] * u[3] + V[7] * u[4] + V[8] * u[5]]
    rt = quat_rotate(B, ex, ey, ez, ew, [T[4], T[5], T[6]])
    qx = ew * T[0] + ex * T[3] + ey * T[2] - ez * T[1]
    qy = ew * T[1] + ey * T[3] + ez * T[0] - ex * T[2]
    qz = ew * T[2] + ez * T[3] + ex * T[1] - ey * T[0]
    qw = ew * T[3] - ex * T[0] - ey * T[1] - ez * T[2]
    return list(quat_normalize(B, br, qx, qy, qz, qw)) + [et[0] + rt[0], et[1] + rt[1], et[2] + rt[2]]


def huber(B, br, e2, delta, mut=None):
    dsqr = delta * delta
    if br(e2 < dsqr if mut == "huber_lt" else e2 <= dsqr):
        return [e2, B.c(1)]
    s = B.sqrt(e2)
    return [2 * s * delta - dsqr, delta / s]


def jac_pose(B, br, x, y, z, fx, fy, mut=None):
    one, zero = B.c(1), B.c(0)
    iz = one / z
    iz2 = iz * iz
    return [x * y * iz2 * fx, -(one + (x * x * iz2)) * fx, y * iz * fx, -iz * fx, zero, x * iz2 * fx,
            (one + y * y * iz2) * fy, -x * y * iz2 * fy, -x * iz * fy, zero, -iz * fy, y * iz2 * fy]


# ---------------------------------------------------------------------------------------------------------- sim3_math.h
def s3_quat_of_rot(B, br, R, eigen=False, mut=None):   # -> x y z w
    half, one = B.c(0.5), B.c(1)
    t = R[0] + (R[4] + R[8]) if eigen else R[0] + R[4] + R[8]
    if br(t >= 0 if mut == "trace_ge" else t > 0):
        t = B.sqrt(t + one)
        w = half * t
        t = half / t
        return [(R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t, w]
    i = _largest_diagonal(br, R)
    if i == 0:
        t = B.sqrt(R[0] - R[4] - R[8] + one)
        x, t = half * t, half / t
        return [x, (R[3] + R[1]) * t, (R[6] + R[2]) * t, (R[7] - R[5]) * t]
    if i == 1:
        t = B.sqrt(R[4] - R[8] - R[0] + one)
        y, t = half * t, half / t
        return [(R[1] + R[3]) * t, y, (R[7] + R[5]) * t, (R[2] - R[6]) * t]
    t = B.sqrt(R[8] - R[0] - R[4] + one)
    z, t = half * t, half / t
    return [(R[2] + R[6]) * t, (R[5] + R[7]) * t, z, (R[3] - R[1]) * t]


_EPS = np.float64(0.00001)


def _abc(B, b_sig, b_small, s, sigma, theta):
    """A, B, C of Sim3(update) and Sim3::log -- the four eps branches as written (sim3.h:94-131, :170-221)"""
    half, one = B.c(0.5), B.c(1)
    if b_sig:
        Cc = one
        if b_small:
            return one / 2, one / 6, Cc
        theta2 = theta * theta
        return (one - B.cos(theta)) / theta2, (theta - B.sin(theta)) / (theta2 * theta), Cc
    Cc = (s - one) / sigma
    if b_small:
        sigma2 = sigma * sigma
        return ((sigma - one) * s + one) / sigma2, ((half * sigma2 - sigma + one) * s) / (sigma2 * sigma), Cc
    a, b = s * B.sin(theta), s * B.cos(theta)
    theta2, sigma2 = theta * theta, sigma * sigma
    c = theta2 + sigma2
    return (a * sigma + (one - b) * theta) / (theta * c), (Cc - ((b - one) * sigma + a * theta) / c) * one / theta2, Cc


def s3_exp(B, br, u, eigen=False, mut=None):   # -> Sim3d
    one, zero = B.c(1), B.c(0)
    wx, wy, wz, sigma = u[0], u[1], u[2], u[6]
    theta = B.sqrt(wx * wx + (wy * wy + wz * wz)) if eigen else B.sqrt(wx * wx + wy * wy + wz * wz)
    O, O2 = _skew(B, wx, wy, wz)
    s = B.exp(sigma)
    b_sig = br(abs(sigma) < _EPS)
    b_small = br(theta < _EPS) and mut != "closed_below_eps"
    A, Bc, Cc = _abc(B, b_sig, b_small, s, sigma, theta)
    if b_small:
        ra = rb = one
    else:
        ra, rb = B.sin(theta) / theta, (one - B.cos(theta)) / (theta * theta)
    eye = [one if i % 4 == 0 else zero for i in range(9)]
    R = [(eye[i] + O[i]) + O2[i] if b_small else (eye[i] + ra * O[i]) + rb * O2[i] for i in range(9)]
    W = [(A * O[i] + Bc * O2[i]) + Cc * eye[i] for i in range(9)]
    q = s3_quat_of_rot(B, br, R, eigen)
    t = [W[0] * u[3] + W[1] * u[4] + W[2] * u[5], W[3] * u[3] + W[4] * u[4] + W[5] * u[5], W[6] * u[3] + W[7] * u[4] + W[8] * u[5]]
    return q + t + [s]


def s3_mul(B, br, a, b, eigen=False, mut=None):
    ax, ay, az, aw = a[:4]
    bx, by, bz, bw = b[:4]
    if eigen and mut != "plain_quat_product":
        q = [(aw * bx + ay * bz) - (az * by - ax * bw), (aw * by + ay * bw) + (az * bx - ax * bz),
             (aw * bz - ay * bx) + (az * bw + ax * by), (aw * bw - ay * by) - (az * bz + ax * bx)]
    else:
        qw = aw * bw - ax * bx - ay * by - az * bz
        q = [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx, qw]
    r = quat_rotate(B, ax, ay, az, aw, b[4:7])
    return q + [a[7] * r[0] + a[4], a[7] * r[1] + a[5], a[7] * r[2] + a[6], a[7] * b[7]]


def s3_inverse(B, br, a, mut=None):
    one = B.c(1)
    k = -one / a[7]
    r = quat_rotate(B, -a[0], -a[1], -a[2], a[3], [k * a[4], k * a[5], k * a[6]])
    return [-a[0], -a[1], -a[2], a[3]] + r + [one / a[7]]


def s3_map(B, br, S, v, mut=None):
    r = quat_rotate(B, S[0], S[1], S[2], S[3], v)
    return [S[7] * r[0] + S[4], S[7] * r[1] + S[5], S[7] * r[2] + S[6]]


def s3_rot_of_quat(B, br, S, mut=None):
    return rot_of_quat(B, S[0], S[1], S[2], S[3])


def s3_lu_solve3(B, br, W, t, mut=None):
    a = [[W[0], W[1], W[2]], [W[3], W[4], W[5]], [W[6], W[7], W[8]]]
    b = list(t)
    gt = (lambda p, q: p >= q) if mut == "lu_last_wins" else (lambda p, q: p > q)

    def swap(p, q):
        a[p], a[q] = a[q], a[p]
        b[p], b[q] = b[q], b[p]

    if mut != "lu_no_pivot":
        piv, big = 0, abs(a[0][0])
        if br(gt(abs(a[1][0]), big)):
            big, piv = abs(a[1][0]), 1
        if br(gt(abs(a[2][0]), big)):
            piv = 2
        if piv:
            swap(0, piv)
    a[1][0] = a[1][0] / a[0][0]
    a[2][0] = a[2][0] / a[0][0]
    a[1][1] = a[1][1] - a[1][0] * a[0][1]
    a[1][2] = a[1][2] - a[1][0] * a[0][2]
    a[2][1] = a[2][1] - a[2][0] * a[0][1]
    a[2][2] = a[2][2] - a[2][0] * a[0][2]
    if mut != "lu_no_pivot" and br(gt(abs(a[2][1]), abs(a[1][1]))):
        swap(1, 2)
    a[2][1] = a[2][1] / a[1][1]
    a[2][2] = a[2][2] - a[2][1] * a[1][2]
    y0 = b[0]
    y1 = b[1] - a[1][0] * y0
    if mut == "lu_one_by_one":
        y2 = b[2] - a[2][0] * y0 - a[2][1] * y1
    else:
        y2 = b[2] - (a[2][0] * y0 + a[2][1] * y1)
    x2 = y2 / a[2][2]
    x1 = (y1 - a[1][2] * x2) / a[1][1]
    if mut == "lu_one_by_one":
        x0 = (y0 - a[0][1] * x1 - a[0][2] * x2) / a[0][0]
    else:
        x0 = (y0 - (a[0][1] * x1 + a[0][2] * x2)) / a[0][0]
    return [x0, x1, x2]


def s3_log(B, br, S, mut=None):
    half, one, zero = B.c(0.5), B.c(1), B.c(0)
    sigma = B.log(S[7])
    R = rot_of_quat(B, S[0], S[1], S[2], S[3])
    d = half * (R[0] + R[4] + R[8] - one)
    dR = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    b_sig = br(abs(sigma) < _EPS)
    b_small = br(d > np.float64(1) - _EPS)
    if b_small:
        k, theta = half, zero
    else:
        theta = B.acos(d)
        k = theta / (2 * B.sqrt(one - d * d))
    A, Bc, Cc = _abc(B, b_sig, b_small, S[7], sigma, theta)
    wx, wy, wz = k * dR[0], k * dR[1], k * dR[2]
    O = [zero, -wz, wy, wz, zero, -wx, -wy, wx, zero]
    W = []
    for i in range(3):
        for j in range(3):
            bo2 = (Bc * O[i * 3]) * O[j] + (Bc * O[i * 3 + 1]) * O[3 + j] + (Bc * O[i * 3 + 2]) * O[6 + j]
            W.append((A * O[i * 3 + j] + bo2) + Cc * (one if i == j else zero))
    ups = s3_lu_solve3(B, br, W, [S[4], S[5], S[6]])
    return [wx, wy, wz] + ups + [sigma]


def s3_edge_error(B, br, Cm, Si, Sj, mut=None):
    return s3_log(B, br, s3_mul(B, br, s3_mul(B, br, Cm, Si, True), s3_inverse(B, br, Sj), True))


def s3_oplus(B, br, est, u, fix_scale, eigen=False, mut=None):
    v = list(u)
    if fix_scale:
        v[6] = B.c(0)
    return s3_mul(B, br, s3_exp(B, br, v, eigen, mut), est, eigen)


def s3_project_error(B, br, S, X, ob, K, mut=None):
    r = quat_rotate(B, S[0], S[1], S[2], S[3], X)
    x, y, z = S[7] * r[0] + S[4], S[7] * r[1] + S[5], S[7] * r[2] + S[6]
    return [ob[0] - ((x / z) * K[0] + K[2]), ob[1] - ((y / z) * K[1] + K[3])]


def s3_chi2(B, br, e0, e1, isg, mut=None):
    return [e0 * (isg * e0) + e1 * (isg * e1)]


def s3_solve7(B, br, H, lam, b, mut=None):   # -> ok, x[7]
    L = {}
    ok = True
    for j in range(7):
        d = H[j * 7 + j] + lam
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        if br(not (d > 0)):
            ok = False
        ljj = B.sqrt(d)
        L[j, j] = ljj
        for i in range(j + 1, 7):
            v = H[j * 7 + i]
            for k in range(j):
                v = v - L[i, k] * L[j, k]
            L[i, j] = v / ljj
    y, x = [None] * 7, [None] * 7
    for i in range(7):
        v = b[i]
        for k in range(i):
            v = v - L[i, k] * y[k]
        y[i] = v / L[i, i]
    for i in range(6, -1, -1):
        v = y[i]
        for k in range(i + 1, 7):
            v = v - L[k, i] * x[k]
        x[i] = v / L[i, i]
    return [B.c(1) if ok else B.c(0)] + x


def _run(B, br, op, x, mut):
    """op by name on one item's inputs (a list of B's numbers) -> list of outputs"""
    if op == "asd_rsqrt": return [asd_rsqrt(B, br, x[0])]
    if op == "quat_normalize": return list(quat_normalize(B, br, *x))
    if op == "quat_rotate": return quat_rotate(B, x[0], x[1], x[2], x[3], x[4:7])
    if op == "pose_map": return pose_map(B, br, x[:7], x[7:10])
    if op == "pose_oplus": return pose_oplus(B, br, x[:7], x[7:13], mut)
    if op == "rot_to_quat_eigen": return list(rot_to_quat_eigen(B, br, x, mut))
    if op == "huber": return huber(B, br, x[0], x[1], mut)
    if op == "jac_pose": return jac_pose(B, br, *x)
    if op in ("s3_exp", "s3_exp_eigen"): return s3_exp(B, br, x, op.endswith("eigen"), mut)
    if op == "s3_log": return s3_log(B, br, x)
    if op in ("s3_mul", "s3_mul_eigen"): return s3_mul(B, br, x[:8], x[8:16], op.endswith("eigen"), mut)
    if op == "s3_inverse": return s3_inverse(B, br, x)
    if op == "s3_map": return s3_map(B, br, x[:8], x[8:11])
    if op in ("s3_oplus", "s3_oplus_eigen"): return s3_oplus(B, br, x[:8], x[8:15], float(x[15]) != 0, op.endswith("eigen"), mut)
    if op in ("s3_quat_of_rot", "s3_quat_of_rot_eigen"): return s3_quat_of_rot(B, br, x, op.endswith("eigen"), mut)
    if op == "s3_rot_of_quat": return s3_rot_of_quat(B, br, x)
    if op == "s3_lu_solve3": return s3_lu_solve3(B, br, x[:9], x[9:12], mut)
    if op == "s3_edge_error": return s3_edge_error(B, br, x[:8], x[8:16], x[16:24])
    if op == "s3_project_error": return s3_project_error(B, br, x[:8], x[8:11], x[11:13], x[13:17])
    if op == "s3_chi2": return s3_chi2(B, br, *x)
    if op == "s3_solve7": return s3_solve7(B, br, x[:49], x[49], x[50:57])
    raise KeyError(op)


def _f64_item(op, row, mut=None):
    br = Branches()
    with np.errstate(all="ignore"):
        y = _run(F64, br, op, [np.float64(v) for v in row], mut)
    return np.array([np.float64(v) for v in y]), br.rec


def f64(op, x, mut=None):
    """the literal float64 restatement on every row of x [n, width in] -> [n, width out]"""
    x = np.asarray(x, np.float64).reshape(-1, WIDTH[op][0])
    return np.array([_f64_item(op, row, mut)[0] for row in x]).reshape(len(x), WIDTH[op][1])


def exact(op, x, sensitivity=True, branches_of=None):
    """the high-precision restatement on every row of x -> (hi, lo, S): the value as a double-double pair, and the sensitivity
    scale S_i = |f_i| + sum_j |df_i/dx_j| |x_j| as float64 (None where not asked for).  branches_of: inputs whose f64 run supplies
    the comparisons instead of x's own (the formula of the other side of a threshold, evaluated at x)"""
    mp = mpmath.mpf
    x = np.asarray(x, np.float64).reshape(-1, WIDTH[op][0])
    bx = x if branches_of is None else np.asarray(branches_of, np.float64).reshape(x.shape)
    wo = WIDTH[op][1]
    hi, lo, S = np.empty((len(x), wo)), np.empty((len(x), wo)), np.empty((len(x), wo)) if sensitivity else None
    for n, row in enumerate(x):
        rec = _f64_item(op, bx[n])[1]
        xs = [mp(float(v)) for v in row]
        y = _run(EXACT, Branches(rec), op, xs, None)
        for i, v in enumerate(y):
            hi[n, i] = float(v)
            lo[n, i] = float(v - mp(hi[n, i]))
        if not sensitivity:
            continue
        s = [abs(v) for v in y]
        for j, xj in enumerate(xs):
            if xj == 0:
                continue
            h = abs(xj) * mp("1e-18")
            xp, xm = list(xs), list(xs)
            xp[j], xm[j] = xj + h, xj - h
            yp, ym = _run(EXACT, Branches(rec), op, xp, None), _run(EXACT, Branches(rec), op, xm, None)
            for i in range(wo):
                s[i] += abs((yp[i] - ym[i]) / (2 * h)) * abs(xj)
        S[n] = [float(v) for v in s]
    return hi, lo, S


def ratios(got, hi, lo, S):
    """|got - exact| / (u S) per component, formed in long double from the double-double pair; 0 where S = 0 and got is exact"""
    ld = np.longdouble
    err = np.abs((np.asarray(got, ld) - np.asarray(hi, ld)) - np.asarray(lo, ld))
    den = ld(U) * np.asarray(S, ld)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(den > 0, err / den, np.where(err == 0, 0, np.inf))
    return np.asarray(r, np.float64)


def same_bits(a, b):
    """elementwise: equal as bit patterns, any two NaNs counting as equal"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
