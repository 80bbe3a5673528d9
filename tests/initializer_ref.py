"""A plain restatement of the reference's Initializer (src/vslam/src/Initializer.cc) and the checks tests/test_initializer*.py hold
asd_initialize to.

f32 where the reference is f32: numpy float32, one operation at a time (vectorised over the matches: every element goes through the
same operations in the same order; the score is a sequential f32 sum, numpy's cumsum).  numpy.longdouble for what include/asd_slam.h
defines in f64: matrix products, inv(), determinant, norm, the null vector of A and the 3 x 3 decompositions (a one-sided Jacobi started
from LAPACK's float64 factors and polished in longdouble).  The signs of singular vectors are the solver's: every function that needs a
decomposition takes one as an argument, so the device's own factors can be fed through the same chain.

Triangulate's 4 x 4 SVD is OpenCV 3.2.0's JacobiSVDImpl_ in f32; it is not restated here a third time: `svd4` arguments take a callable
A [n][4][4] f32 -> vt.row(3) [n][4] f32 (the oracle's orc_svd4_vt on the CPU, asd_svd4_null on the device; tests/test_mapping*.py pin
them against each other).

Mutants (the `mut` set of initialize(), for tests/test_initializer_ref.py): see MUTANTS."""
import ctypes

import numpy as np

from tests.sim3solver_ref import EPS64, K_KITTI, random_int   # noqa: F401  (re-exported)

F32, F64, LD = np.float32, np.float64, np.longdouble
NAN32 = F32(np.nan)
MUTANTS = ("th_fundamental_5.991", "th_score_3.841", "chi_ge_H", "chi_ge_F", "score_test2_first", "normalize_matched_only",
           "walk_ge", "similar_0.8", "similar_ge", "min_good_0.8", "max_lt_le", "parallax_ge_F", "second_0.9", "second_le",
           "parallax_gt_H", "best_ge_min", "best_0.8", "index_40", "th2_ge", "depth_lt")


# ---------------------------------------------------------------------------------------------------------------- sampling (:84-100)
def libc_rand(seed, count):
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(ctypes.c_uint(seed))
    libc.rand.restype = ctypes.c_int
    return [libc.rand() for _ in range(count)]


def draws_from_raw(raw, N, n_iter):
    """draws[k][j] = RandomInt(0, N - 1 - j) fed with the raw rand() values in order (:86-100)"""
    it = iter(raw)
    return np.array([[random_int(int(next(it)), 0, N - 1 - j) for j in range(8)] for _ in range(n_iter)], np.int32).reshape(n_iter, 8)


def sample(draws, N):
    avail = list(range(N))
    idx = []
    for j in range(8):
        randi = int(draws[j])
        assert 0 <= randi <= len(avail) - 1
        idx.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return idx


def matches_of(matches12):
    """mvMatches12 (:55-64) -> (first [N], second [N])"""
    m = np.asarray(matches12, np.int32)
    first = np.nonzero(m >= 0)[0].astype(np.int32)
    return first, m[first]


# ---------------------------------------------------------------------------------------------------------------- Normalize (:791-837)
def seq_sum32(x):
    s = F32(0)
    for v in np.asarray(x, F32):
        s = F32(s + v)
    return s


def normalize(keys):
    k = np.asarray(keys, F32).reshape(-1, 2)
    N = len(k)
    with np.errstate(all="ignore"):
        meanX, meanY = F32(seq_sum32(k[:, 0]) / F32(N)), F32(seq_sum32(k[:, 1]) / F32(N))
        px, py = (k[:, 0] - meanX).astype(F32), (k[:, 1] - meanY).astype(F32)
        devX, devY = F32(seq_sum32(np.abs(px)) / F32(N)), F32(seq_sum32(np.abs(py)) / F32(N))
        sX, sY = F32(F64(1.0) / F64(devX)), F32(F64(1.0) / F64(devY))
        pts = np.stack([px * sX, py * sY], axis=1).astype(F32)
        T = np.array([[sX, 0, F32(-meanX) * sX], [0, sY, F32(-meanY) * sY], [0, 0, 1]], F32)
    return pts, T


# ---------------------------------------------------------------------------------------------------------------- matrix rules
def mul(A, B, dt=LD, detail=False):
    """the header's product rule: dt on the widened elements, terms in index order, one rounding.  detail: (f32, dt value, S)"""
    A, B = np.asarray(A, F32).astype(dt), np.asarray(B, F32).astype(dt)
    if B.ndim == 1:
        B = B[:, None]
    C = np.zeros((A.shape[0], B.shape[1]), dt)
    S = np.zeros_like(C)
    with np.errstate(all="ignore"):
        for k in range(A.shape[1]):
            p = A[:, k:k + 1] * B[k:k + 1, :]
            C = p if k == 0 else C + p
            S = S + np.abs(p)
    out = C.astype(F32)
    return (out, C, S) if detail else out


def det33(M, dt=LD):
    a, b, c, d, e, f, g, h, i = [dt(x) for x in np.asarray(M, F32).reshape(9)]
    return a * (e * i - f * h) + b * (f * g - d * i) + c * (d * h - e * g)


def inv33(M, dt=LD, detail=False):
    """adjugate over determinant; zero matrix for a zero determinant.  detail: (f32, dt value, S) with S the first-order error weight of
    the quotient: S_cof / |det| + |cof| S_det / det^2 + |q| (S_cof, S_det = the sums of the absolute products behind cofactor and determinant)"""
    m = np.asarray(M, F32).astype(dt).reshape(3, 3)
    cof = np.zeros((3, 3), dt)
    scof = np.zeros((3, 3), dt)
    for i in range(3):
        for j in range(3):
            r = [x for x in range(3) if x != i]
            c = [x for x in range(3) if x != j]
            p, q = m[r[0], c[0]] * m[r[1], c[1]], m[r[0], c[1]] * m[r[1], c[0]]
            sgn = 1 if (i + j) % 2 == 0 else -1
            cof[i, j] = sgn * (p - q)
            scof[i, j] = abs(p) + abs(q)
    det = m[0, 0] * cof[0, 0] + m[0, 1] * cof[0, 1] + m[0, 2] * cof[0, 2]
    sdet = sum(abs(m[0, j]) * scof[0, j] for j in range(3))
    if det == 0:
        z = np.zeros((3, 3), F32)
        return (z, z.astype(dt), np.zeros((3, 3), dt)) if detail else z
    with np.errstate(all="ignore"):
        q = cof.T / det
        S = scof.T / abs(det) + np.abs(cof.T) * sdet / (det * det) + np.abs(q)
    out = q.astype(F32)
    return (out, q, S) if detail else out


def jacobi_svd(A, dt=LD, sweeps=60):
    """one-sided Jacobi of A [m][n] in dt, started from LAPACK's float64 right vectors -> (sig [n], V [n][n]) unsorted"""
    A = np.asarray(A).astype(dt)
    m, n = A.shape
    eps = np.finfo(dt).eps
    V = np.eye(n, dtype=dt)
    if np.isfinite(A).all():
        V = np.linalg.svd(A.astype(F64), full_matrices=True)[2].T.astype(dt)
    W = A @ V
    floor2 = (8 * eps) ** 2 * (A * A).sum()
    for _ in range(sweeps):
        rotated = False
        G = W.T @ W                   # a filter only: a pair that passes is evaluated afresh
        dg = np.sqrt(np.abs(np.diag(G)))
        todo = np.argwhere(np.triu((np.abs(G) > eps * 0.5 * dg[:, None] * dg[None, :]) & (dg[:, None] ** 2 > floor2) & (dg[None, :] ** 2 > floor2), 1))
        for p, q in todo:
                alpha, beta, gamma = W[:, p] @ W[:, p], W[:, q] @ W[:, q], W[:, p] @ W[:, q]
                if min(alpha, beta) <= floor2 or not abs(gamma) > eps * np.sqrt(alpha * beta):
                    continue          # (a column at rounding level is a null column: nothing to orthogonalise)
                rotated = True
                zeta = (beta - alpha) / (2 * gamma)
                t = (1 if zeta >= 0 else -1) / (abs(zeta) + np.sqrt(zeta * zeta + 1))
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                W[:, p], W[:, q] = c * W[:, p] - s * W[:, q], s * W[:, p] + c * W[:, q]
                V[:, p], V[:, q] = c * V[:, p] - s * V[:, q], s * V[:, p] + c * V[:, q]
        if not rotated:
            break
    return np.sqrt((W * W).sum(axis=0)), V, W


def null_vector(A, dt=LD):
    """-> (unit null vector, singular values descending) of the f32 matrix A widened"""
    sig, V, _ = jacobi_svd(np.asarray(A, F32), dt)
    j = int(np.argmin(sig))
    v = V[:, j]
    if v[int(np.argmax(np.abs(v)))] < 0:      # the sign convention: the component of largest magnitude (the first of equal ones) is positive
        v = -v
    return v / np.sqrt(v @ v), np.sort(sig)[::-1]


def svd3(M, dt=LD):
    """the header's 3 x 3 rule -> (U, w descending, Vt) in dt"""
    sig, V, W = jacobi_svd(np.asarray(M, F32).reshape(3, 3), dt)
    order = np.argsort(-sig, kind="stable")
    thr = 2 * EPS64 * sig.sum()
    U = np.zeros((3, 3), dt)
    for j, o in enumerate(order):
        if sig[o] > thr:
            U[:, j] = W[:, o] / sig[o]
    w = sig[order]
    Vt = V[:, order].T.copy()
    for j in range(3):              # the sign convention: the component of v_j of largest magnitude (the first of equal ones) is positive
        if Vt[j, int(np.argmax(np.abs(Vt[j])))] < 0:
            Vt[j], U[:, j] = -Vt[j], -U[:, j]
    for j in range(3):
        if not w[j] > thr:
            U[:, j] = np.cross(U[:, (j + 1) % 3], U[:, (j + 2) % 3])
    return U, w, Vt


# ---------------------------------------------------------------------------------------------------------------- models
def build_A(pn1, pn2, model):
    """ComputeH21 :229-258 (16 x 9) / ComputeF21 :279-297 (8 x 9): every entry the f32 product"""
    rows = []
    for (u1, v1), (u2, v2) in zip(np.asarray(pn1, F32), np.asarray(pn2, F32)):
        if model == 0:
            rows.append([0, 0, 0, -u1, -v1, -1, F32(v2 * u1), F32(v2 * v1), v2])
            rows.append([u1, v1, 1, 0, 0, 0, F32(-u2 * u1), F32(-u2 * v1), -u2])
        else:
            rows.append([F32(u2 * u1), F32(u2 * v1), u2, F32(v2 * u1), F32(v2 * v1), v2, u1, v1, 1])
    return np.array(rows, F32)


def h_model(nullv, T1, T2inv, dt=LD, detail=False):
    """H21i = T2inv * Hn * T1 (:159), H12i = H21i.inv() (:160) from a null vector"""
    Hn = np.asarray(nullv).astype(F32).reshape(3, 3)
    a = mul(T2inv, Hn, dt)
    H21 = mul(a, T1, dt, detail)
    H12 = inv33(H21[0] if detail else H21, dt, detail)
    return H21, H12


def f_model(nullv, T1, T2, dt=LD, svd=None, detail=False):
    """the rank-2 step (:305-309) and F21i = T2t * Fn * T1 (:211); svd = (U, w, Vt) of Fpre to use instead of this module's"""
    Fpre = np.asarray(nullv).astype(F32).reshape(3, 3)
    U, w, Vt = svd if svd is not None else svd3(Fpre, dt)
    Uf, Vtf = np.asarray(U).astype(F32), np.asarray(Vt).astype(F32)
    D = np.diag(np.array([w[0], w[1], 0]).astype(F32))
    Fn = mul(mul(Uf, D, dt), Vtf, dt)
    T2t = np.ascontiguousarray(np.asarray(T2, F32).T)
    return mul(mul(T2t, Fn, dt), T1, dt, detail)


def _inv_sigma2(sigma):
    s = F32(sigma)
    return F32(F64(1.0) / F64(F32(s * s)))


def _recip(x):
    with np.errstate(all="ignore"):
        return (F64(1.0) / x.astype(F64)).astype(F32)


def _score(t1, t2, mut):
    inter = np.stack([t2, t1] if "score_test2_first" in mut else [t1, t2], axis=1).reshape(-1).astype(F32)
    return F32(np.cumsum(inter, dtype=F32)[-1]) if len(inter) else F32(0)


def check_homography(H21, H12, k1, k2, sigma, mut=()):
    """CheckHomography (:312-395) over the matched keys k1, k2 [N][2] -> (score f32, mask bool[N], chi [N][2])"""
    h, hi = np.asarray(H21, F32).reshape(9), np.asarray(H12, F32).reshape(9)
    u1, v1, u2, v2 = k1[:, 0], k1[:, 1], k2[:, 0], k2[:, 1]
    th, inv = F32(5.991), _inv_sigma2(sigma)
    with np.errstate(all="ignore"):
        w = _recip(hi[6] * u2 + hi[7] * v2 + hi[8])
        a, b = (hi[0] * u2 + hi[1] * v2 + hi[2]) * w, (hi[3] * u2 + hi[4] * v2 + hi[5]) * w
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv
        w = _recip(h[6] * u1 + h[7] * v1 + h[8])
        a, b = (h[0] * u1 + h[1] * v1 + h[2]) * w, (h[3] * u1 + h[4] * v1 + h[5]) * w
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv
        out1, out2 = (chi1 >= th, chi2 >= th) if "chi_ge_H" in mut else (chi1 > th, chi2 > th)
        t1, t2 = np.where(out1, F32(0), th - chi1).astype(F32), np.where(out2, F32(0), th - chi2).astype(F32)
    return _score(t1, t2, mut), ~(out1 | out2), np.stack([chi1, chi2], axis=1)


def check_fundamental(F21, k1, k2, sigma, mut=()):
    """CheckFundamental (:397-480) -> (score f32, mask bool[N], chi [N][2])"""
    f = np.asarray(F21, F32).reshape(9)
    u1, v1, u2, v2 = k1[:, 0], k1[:, 1], k2[:, 0], k2[:, 1]
    th = F32(5.991) if "th_fundamental_5.991" in mut else F32(3.841)
    ths = F32(3.841) if "th_score_3.841" in mut else F32(5.991)
    inv = _inv_sigma2(sigma)
    with np.errstate(all="ignore"):
        a2, b2, c2 = f[0] * u1 + f[1] * v1 + f[2], f[3] * u1 + f[4] * v1 + f[5], f[6] * u1 + f[7] * v1 + f[8]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv
        a1, b1, c1 = f[0] * u2 + f[3] * v2 + f[6], f[1] * u2 + f[4] * v2 + f[7], f[2] * u2 + f[5] * v2 + f[8]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv
        out1, out2 = (chi1 >= th, chi2 >= th) if "chi_ge_F" in mut else (chi1 > th, chi2 > th)
        t1, t2 = np.where(out1, F32(0), ths - chi1).astype(F32), np.where(out2, F32(0), ths - chi2).astype(F32)
    return _score(t1, t2, mut), ~(out1 | out2), np.stack([chi1, chi2], axis=1)


def walk(scores, mut=()):
    """:164-169 / :215-220: strict > from 0.0f -> (best iteration or -1, score)"""
    best, score = -1, F32(0)
    for k, s in enumerate(scores):
        if (F32(s) >= score and "walk_ge" in mut) or F32(s) > score:
            best, score = k, F32(s)
    return best, score


def choose_model(SH, SF, mut=()):
    with np.errstate(all="ignore"):
        RH = F32(F32(SH) / F32(F32(SH) + F32(SF)))     # :113
    return (0 if F64(RH) > 0.40 else 1), RH


# ---------------------------------------------------------------------------------------------------------------- motion hypotheses
def kmat(K):
    fx, fy, cx, cy = [F32(x) for x in K]
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F32)


def _unit(v, dt):
    v = np.asarray(v, F32).astype(dt).reshape(3)
    with np.errstate(all="ignore"):
        q = v / np.sqrt((v * v).sum())
    return q.astype(F32), q


def decomposition_H(H21, K, dt=LD):
    """A = invK * H21 * K (:595-596) -> the f32 matrix the SVD of :599 sees"""
    Km = kmat(K)
    return mul(mul(inv33(Km, dt), H21, dt), Km, dt)


def decomposition_F(F21, K, dt=LD):
    """E21 = K.t() * F21 * K (:491)"""
    Km = kmat(K)
    return mul(mul(np.ascontiguousarray(Km.T), F21, dt), Km, dt)


def hypotheses_H(svd, dt=LD):
    """:602-697 from (U, w, Vt) of A -> list of (R f32, t f32, R dt, S_R, t dt) (empty at the return of :607-611)"""
    U, w, Vt = [np.asarray(x).astype(F32) for x in svd]
    s = F32(det33(U, dt) * det33(Vt, dt))
    d1, d2, d3 = w
    with np.errstate(all="ignore"):
        if F64(F32(d1 / d2)) < 1.0000001 or F64(F32(d2 / d3)) < 1.0000001:
            return []
        den = F32(F32(d1 * d1) - F32(d3 * d3))
        a12, a23 = F32(F32(d1 * d1) - F32(d2 * d2)), F32(F32(d2 * d2) - F32(d3 * d3))
        aux1, aux3 = np.sqrt(F32(a12 / den)), np.sqrt(F32(a23 / den))
        root = np.sqrt(F32(a12 * a23))
        aux_st = F32(root / F32(F32(d1 + d3) * d2))
        ct = F32(F32(F32(d2 * d2) + F32(d1 * d3)) / F32(F32(d1 + d3) * d2))
        aux_sp = F32(root / F32(F32(d1 - d3) * d2))
        cp = F32(F32(F32(d1 * d3) - F32(d2 * d2)) / F32(F32(d1 - d3) * d2))
        sU = (F32(s) * U).astype(F32)
        out = []
        for h in range(8):
            i = h & 3
            x1 = aux1 if i < 2 else F32(-aux1)
            x3 = F32(-aux3) if i & 1 else aux3
            sg = F32(1) if i in (0, 3) else F32(-1)
            if h < 4:
                st = F32(sg * aux_st)
                Rp = np.array([[ct, 0, -st], [0, 1, 0], [st, 0, ct]], F32)
                k = F32(d1 - d3)
                tp = np.array([x1 * k, F32(0) * k, F32(-x3) * k], F32)
            else:
                sp = F32(sg * aux_sp)
                Rp = np.array([[cp, 0, sp], [0, -1, 0], [sp, 0, -cp]], F32)
                k = F32(d1 + d3)
                tp = np.array([x1 * k, F32(0) * k, x3 * k], F32)
            R, Rv, RS = mul(mul(sU, Rp, dt), Vt, dt, True)
            t, tv = _unit(mul(U, tp, dt).reshape(3), dt)
            out.append((R, t, Rv, RS, tv))
    return out


def hypotheses_F(svd, dt=LD):
    """DecomposeE (:951-971) and the four pairs of :506-509 from (U, w, Vt) of E21"""
    U, _, Vt = [np.asarray(x).astype(F32) for x in svd]
    t, tv = _unit(U[:, 2], dt)
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F32)
    Rs = []
    for Wm in (W, np.ascontiguousarray(W.T)):
        R, Rv, RS = mul(mul(U, Wm, dt), Vt, dt, True)
        if det33(R, dt) < 0:
            R, Rv = (-R).astype(F32), -Rv
        Rs.append((R, Rv, RS))
    return [(Rs[0][0], t, Rs[0][1], Rs[0][2], tv), (Rs[1][0], t, Rs[1][1], Rs[1][2], tv),
            (Rs[0][0], (-t).astype(F32), Rs[0][1], Rs[0][2], -tv), (Rs[1][0], (-t).astype(F32), Rs[1][1], Rs[1][2], -tv)]


# ---------------------------------------------------------------------------------------------------------------- CheckRT (:840-949)
def scaled_minus(alpha, a, b):
    """alpha * a - b as cv::Mat evaluates it (asd_triangulate_pairs' rule): plain f32 subtraction when alpha == 1"""
    alpha, a, b = np.asarray(alpha, F32), np.asarray(a, F32), np.asarray(b, F32)
    with np.errstate(all="ignore"):
        gen = (a.astype(F64) * alpha.astype(F64) + b.astype(F64) * -1.0 + 0.0).astype(F32)
        return np.where(alpha == F32(1), (a - b).astype(F32), gen)


def projection2(R, t, K, dt=LD):
    """P2 = K * [R | t] (:863-866), O2 = -R.t() * t (:868)"""
    Rt = np.concatenate([np.asarray(R, F32), np.asarray(t, F32).reshape(3, 1)], axis=1)
    P2 = mul(kmat(K), Rt, dt)
    O2 = (-mul(np.ascontiguousarray(np.asarray(R, F32).T), np.asarray(t, F32), dt).reshape(3)).astype(F32)
    return P2, O2


def triangulation_rows(K, P2, k1, k2):
    """the 4 x 4 matrices of Triangulate (:778-781) [n][4][4] f32"""
    Km = kmat(K)
    P1 = np.concatenate([Km, np.zeros((3, 1), F32)], axis=1)
    x1, y1, x2, y2 = [c[:, None] for c in (k1[:, 0], k1[:, 1], k2[:, 0], k2[:, 1])]
    return np.stack([scaled_minus(x1, P1[2][None], P1[0][None]), scaled_minus(y1, P1[2][None], P1[1][None]),
                     scaled_minus(x2, P2[2][None], P2[0][None]), scaled_minus(y2, P2[2][None], P2[1][None])], axis=1).astype(F32)


def points_from_null(v):
    """x3D = vt.row(3)[0..2] / vt.row(3)[3] (:785-786) as cv::Mat evaluates it"""
    v = np.asarray(v, F32)
    with np.errstate(all="ignore"):
        inv = (F64(1.0) / v[:, 3].astype(F64)).astype(F32)
        return (v[:, :3] * inv[:, None] + F32(0)).astype(F32)


def cos_key(c):
    """order-preserving keys of the cosines: -0 = +0, NaN after every number"""
    c = np.asarray(c, F32) + F32(0)
    u = c.view(np.uint32).astype(np.uint64)
    k = np.where(u & 0x80000000, (~u) & 0xffffffff, u | 0x80000000)
    return np.where(np.isnan(c), 0xfffffffe, k)


def check_rt_rows(R, t, K, k1, k2, X, th2, dt=LD, mut=()):
    """the loop body of :883-935 for the points X [n][3] f32 (one per inlier match) -> (flags [n]: bit 0 counted in nGood, bit 1 vbGood;
    cos [n] f32; exit [n]: 0 non-finite, 1 depth 1, 2 depth 2, 3 error 1, 4 error 2, 5 good with parallax, 6 good without)"""
    R, t = np.asarray(R, F32), np.asarray(t, F32).reshape(3)
    fx, fy, cx, cy = [F32(x) for x in K]
    _, O2 = projection2(R, t, K, dt)
    n = len(X)
    flags, exits = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    with np.errstate(all="ignore"):
        fin = np.isfinite(X).all(axis=1)
        Xd = X.astype(F64)
        n2 = (X - O2[None]).astype(F32)
        n2d = n2.astype(F64)                                               # norm and dot: f64 accumulations in index order
        dist2 = np.sqrt(n2d[:, 0] * n2d[:, 0] + n2d[:, 1] * n2d[:, 1] + n2d[:, 2] * n2d[:, 2]).astype(F32)
        dist1 = np.sqrt(Xd[:, 0] * Xd[:, 0] + Xd[:, 1] * Xd[:, 1] + Xd[:, 2] * Xd[:, 2]).astype(F32)
        dot = Xd[:, 0] * n2d[:, 0] + Xd[:, 1] * n2d[:, 1] + Xd[:, 2] * n2d[:, 2]
        cos = (dot / (dist1 * dist2).astype(F32).astype(F64)).astype(F32)
        low = cos.astype(F64) < 0.99998
        Rd, td = R.astype(dt), t.astype(dt)
        Xl = X.astype(dt)
        p2 = np.stack([((Rd[i, 0] * Xl[:, 0] + Rd[i, 1] * Xl[:, 1]) + Rd[i, 2] * Xl[:, 2]) + td[i] for i in range(3)], axis=1).astype(F32)
        neg1 = (X[:, 2] < 0) if "depth_lt" in mut else (X[:, 2] <= 0)
        neg2 = (p2[:, 2] < 0) if "depth_lt" in mut else (p2[:, 2] <= 0)
        invZ1 = _recip(X[:, 2])
        im1x, im1y = fx * X[:, 0] * invZ1 + cx, fy * X[:, 1] * invZ1 + cy
        e1 = (im1x - k1[:, 0]) * (im1x - k1[:, 0]) + (im1y - k1[:, 1]) * (im1y - k1[:, 1])
        invZ2 = _recip(p2[:, 2])
        im2x, im2y = fx * p2[:, 0] * invZ2 + cx, fy * p2[:, 1] * invZ2 + cy
        e2 = (im2x - k2[:, 0]) * (im2x - k2[:, 0]) + (im2y - k2[:, 1]) * (im2y - k2[:, 1])
        bad1, bad2 = (e1 >= th2, e2 >= th2) if "th2_ge" in mut else (e1 > th2, e2 > th2)
    for i in range(n):
        if not fin[i]:
            exits[i] = 0
        elif neg1[i] and low[i]:
            exits[i] = 1
        elif neg2[i] and low[i]:
            exits[i] = 2
        elif bad1[i]:
            exits[i] = 3
        elif bad2[i]:
            exits[i] = 4
        else:
            exits[i] = 5 if low[i] else 6
            flags[i] = 3 if low[i] else 1
    return flags, cos, exits


def select_cos(cos, flags, mut=()):
    """:938-946 -> (nGood, selected cosine f32 (NaN when nGood = 0), parallax in longdouble)"""
    good = cos[(flags & 1) != 0]
    if len(good) == 0:
        return 0, NAN32, LD(0)
    order = np.argsort(cos_key(good), kind="stable")
    c = good[order][min(40 if "index_40" in mut else 50, len(good) - 1)]
    with np.errstate(all="ignore"):
        return len(good), c, np.arccos(LD(c)) * 180 / LD(np.pi) if not np.isnan(c) else LD(np.nan)


def th2_of(sigma):
    s = F32(sigma)
    return F32(F64(4.0) * F64(F32(s * s)))


def check_rt(R, t, K, k1, k2, mask, sigma, svd4, dt=LD, mut=()):
    """CheckRT for one hypothesis -> dict(points [N][3] (NaN outside the mask), flags [N], cos [N], exits [N] (-1 outside the mask), n_good,
    cos_sel, parallax (longdouble), parallax32)"""
    N = len(k1)
    sel = np.nonzero(mask)[0]
    P2, _ = projection2(R, t, K, dt)
    pts = np.full((N, 3), np.nan, F32)
    flags, cos, exits = np.zeros(N, np.uint8), np.zeros(N, F32), np.full(N, -1, np.int32)
    if len(sel):
        X = points_from_null(svd4(triangulation_rows(K, P2, k1[sel], k2[sel])))
        pts[sel] = X
        flags[sel], cos[sel], exits[sel] = check_rt_rows(R, t, K, k1[sel], k2[sel], X, th2_of(sigma), dt, mut)
    n_good, c, par = select_cos(cos, flags, mut)
    return dict(points=pts, flags=flags, cos=cos, exits=exits, n_good=n_good, cos_sel=c, parallax=par, parallax32=F32(par))


def accept_F(n_good, parallax, n_inl, min_parallax, min_tri, mut=()):
    """:510-580 -> winner or -1"""
    g = [int(x) for x in n_good[:4]]
    maxGood = max(g)
    nMinGood = max(int((0.8 if "min_good_0.8" in mut else 0.9) * n_inl), int(min_tri))
    f = 0.8 if "similar_0.8" in mut else 0.7
    nsimilar = sum(1 for x in g if (x >= f * maxGood if "similar_ge" in mut else x > f * maxGood))
    if (maxGood <= nMinGood if "max_lt_le" in mut else maxGood < nMinGood) or nsimilar > 1:
        return -1
    c = g.index(maxGood)
    p, m = F32(parallax[c]), F32(min_parallax)
    return c if (p >= m if "parallax_ge_F" in mut else p > m) else -1


def accept_H(n_good, parallax, n_inl, min_parallax, min_tri, mut=()):
    """:700-748 -> (winner or -1, bestGood, secondBestGood)"""
    best, second, idx, bp = 0, 0, -1, F32(-1)
    for h in range(8):
        g = int(n_good[h])
        if g > best:
            second, best, idx, bp = best, g, h, F32(parallax[h])
        elif g > second and (g <= best if "second_le" in mut else g < best):
            second = g
    m = F32(min_parallax)
    ok = (second < (0.9 if "second_0.9" in mut else 0.75) * best and (bp > m if "parallax_gt_H" in mut else bp >= m)
          and (best >= min_tri if "best_ge_min" in mut else best > min_tri) and best > (0.8 if "best_0.8" in mut else 0.9) * n_inl)
    return (idx if ok else -1), best, second


# ---------------------------------------------------------------------------------------------------------------- Initialize (:43-120)
def matched_keys(P):
    first, second = matches_of(P["matches12"])
    k1, k2 = np.asarray(P["keys1"], F32).reshape(-1, 2), np.asarray(P["keys2"], F32).reshape(-1, 2)
    return first, second, k1[first], k2[second]


_MODELS = {}


def initialize(P, svd4, dt=LD, mut=()):
    """the whole of Initialize on one problem dict (tests/initializer_cases.py) -> outcome dict.  The singular vectors are this module's."""
    mut = set(mut)
    first, second, k1, k2 = matched_keys(P)
    N, n1 = len(first), len(np.asarray(P["keys1"]).reshape(-1, 2))
    if "normalize_matched_only" in mut:
        a, T1 = normalize(k1)
        b, T2 = normalize(k2)
        pn1, pn2 = np.zeros((n1, 2), F32), np.zeros((len(np.asarray(P["keys2"]).reshape(-1, 2)), 2), F32)
        pn1[first], pn2[second] = a, b
    else:
        pn1, T1 = normalize(P["keys1"])
        pn2, T2 = normalize(P["keys2"])
    T2inv = inv33(T2, dt)
    key = (id(P), "normalize_matched_only" in mut, dt)
    if key not in _MODELS:      # the models do not depend on the other mutants
        models = []
        for k in range(int(P["n_iter"])):
            idx = sample(P["draws"][k], N)
            a, b = pn1[first[idx]], pn2[second[idx]]
            H21, H12 = h_model(null_vector(build_A(a, b, 0), dt)[0], T1, T2inv, dt)
            models.append((H21, H12, f_model(null_vector(build_A(a, b, 1), dt)[0], T1, T2, dt)))
        _MODELS[key] = (P, models)
    sH, sF, mH, mF, Hs, Fs = [], [], [], [], [], []
    for H21, H12, F21 in _MODELS[key][1]:
        s, m, _ = check_homography(H21, H12, k1, k2, P["sigma"], mut)
        sH.append(s); mH.append(m); Hs.append(H21)
        s, m, _ = check_fundamental(F21, k1, k2, P["sigma"], mut)
        sF.append(s); mF.append(m); Fs.append(F21)
    bH, SH = walk(sH, mut)
    bF, SF = walk(sF, mut)
    model, RH = choose_model(SH, SF, mut)
    out = dict(N=N, SH=SH, SF=SF, RH=RH, model=model, best_H=bH, best_F=bF, ok=0, winner=-1, n_good=[], parallax=[], n_inliers=0,
               inliers_H=mH[bH] if bH >= 0 else np.zeros(N, bool), inliers_F=mF[bF] if bF >= 0 else np.zeros(N, bool),
               P3D=np.zeros((n1, 3), F32), triangulated=np.zeros(n1, np.uint8), exits=np.zeros(7, np.int64))
    best = bH if model == 0 else bF
    if best < 0:
        return out
    mask = (mH if model == 0 else mF)[best]
    out["n_inliers"] = int(mask.sum())
    if model == 0:
        hyps = hypotheses_H(svd3(decomposition_H(Hs[best], P["K"], dt), dt), dt)
    else:
        hyps = hypotheses_F(svd3(decomposition_F(Fs[best], P["K"], dt), dt), dt)
    rts = [check_rt(h[0], h[1], P["K"], k1, k2, mask, P["sigma"], svd4, dt, mut) for h in hyps]
    out["n_good"] = [r["n_good"] for r in rts]
    out["parallax"] = [r["parallax32"] for r in rts]
    for r in rts:
        out["exits"] += np.bincount(r["exits"][r["exits"] >= 0], minlength=7)
    if not hyps:
        return out
    if model == 0:
        w, _, out["second"] = accept_H(out["n_good"], out["parallax"], out["n_inliers"], P["min_parallax"], P["min_triangulated"], mut)
    else:
        w = accept_F(out["n_good"], out["parallax"], out["n_inliers"], P["min_parallax"], P["min_triangulated"], mut)
    out["winner"] = w
    if w >= 0:
        out["ok"] = 1
        out["R21"], out["t21"] = hyps[w][0], hyps[w][1]
        out["P3D"], out["triangulated"] = scatter(rts[w], first, n1)
    return out


def scatter(rt, first, n1):
    """vP3D / vbTriangulated by keypoint of frame 1 (:850-851, :931-935)"""
    P3D, tri = np.zeros((n1, 3), F32), np.zeros(n1, np.uint8)
    g = (rt["flags"] & 1) != 0
    P3D[first[g]] = rt["points"][g]
    tri[first[g]] = (rt["flags"][g] >> 1) & 1
    return P3D, tri


def outcome_signature(o):
    """what a mutant must change in some case"""
    return (o["model"], o["ok"], o["winner"], tuple(o["n_good"]), o["best_H"], o["best_F"], F32(o["SH"]).tobytes(), F32(o["SF"]).tobytes(),
            o["inliers_H"].tobytes(), o["inliers_F"].tobytes(), o["triangulated"].tobytes(),
            tuple(F32(p).tobytes() for p in o["parallax"]))


def ulp32(x):
    x = abs(F32(x))
    return float(np.spacing(x)) if np.isfinite(x) else float("inf")
