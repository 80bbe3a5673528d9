"""The yardstick of tests/test_dense_solve.py: the textbook backward-error bounds of a Cholesky solve, evaluated in 80-bit floats.

Factor (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 10.3): the computed factor of an n x n matrix has
    |A - L L^T| <= gamma(n + 1) |L| |L^T|                      componentwise,
solution (Theorem 10.4): the x computed from it by the two substitutions has
    |b - A x| <= gamma(3 n + 1) (|L| |L^T| |x|)                componentwise,
gamma(k) = k u / (1 - k u), u = 2^-53.  Both hold for any order of the sums and with fused multiply-adds, so they hold for every
kernel form, tile shape and MFMA accumulation order alike; what a form may use up is only the constant c in front (factor_ratio /
solution_ratio return the worst left side over the c = 1 right side, a test compares that with its c):
    forms 2, 3, 4  c = 2   IEEE sqrt and division; 2 is the slack for the theorems' first-order constants
    form 1         c = 4   its reciprocal square roots are good to about one ulp, not half, and L is not returned (the bound is
                           then taken with the 80-bit factor of A, which differs from the kernel's in the last places)
    form 0         block elimination with explicit pivot inverses has no such bound with constants one can write down: its algorithm is
                   restated here in plain NumPy f64 (block_elimination_f64), that restatement's worst solution ratio over the form-0
                   cases is FORM0_RESTATED = 0.38, and the kernel gets FORM0_C = max(4, 8 x that) = 4.  8 covers the cofactor order of the
                   kernel's 6 x 6 inverse, which a restatement on numpy.linalg.inv does not reproduce.
tests/test_dense_solve_ref.py proves the checker on the CPU: NumPy's own f64 Cholesky passes on every case, planted errors fail.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "the reference needs 80-bit long doubles"

U = 2.0 ** -53
C_CHOL = 2.0          # forms 2, 3, 4
C_CHOL_LDS = 4.0      # form 1
FORM0_RESTATED = 0.38  # block_elimination_f64's worst solution ratio over form_cases(0), rounded up (test_dense_solve_ref.py measures it: 0.373)
FORM0_C = max(4.0, 8.0 * FORM0_RESTATED)

TILE = 96
FAMILIES = ("plain", "scaled", "near", "band")
TILED_SIZES = (1, 6, 7, 95, 96, 97, 98, 111, 112, 113, 144, 145, 191, 192, 193, 198, 289, 581)
FORM_BLOCKS = {0: (1, 2, 15, 29, 30), 1: (1, 16, 31, 32), 2: (1, 33, 39, 64)}


def gamma(k):
    return LD(k) * LD(U) / (LD(1) - LD(k) * LD(U))


def tiled_cases():
    """(family, n) of forms 3 and 4"""
    out = []
    for n in TILED_SIZES:
        out.append(("plain", n))
        if n != 581:
            out.append(("scaled", n))
        if n in (97, 193, 289):
            out += [("near", n), ("band", n)]
    return out


def form_cases(form):
    """(family, n) of the one-workgroup forms: `near` only where L comes back (form 2)"""
    fams = ("plain", "scaled", "band") if form < 2 else FAMILIES
    return [(f, 6 * nb) for nb in FORM_BLOCKS[form] for f in fams]


def mirror(A):
    """the symmetric matrix whose lower triangle is A's"""
    Lo = np.tril(A)
    return Lo + np.tril(A, -1).T


def make(family, n, seed=None):
    """A (n x n f64, exactly symmetric, positive definite) and b of a family; the seed follows from (family, n)"""
    rng = np.random.default_rng(10007 * FAMILIES.index(family) + n if seed is None else seed)
    if family == "near":
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        A = (Q * np.logspace(0, -12, n)) @ Q.T
    else:
        G = rng.standard_normal((n, n + 8))
        A = G @ G.T
        if family == "scaled":
            d = 10.0 ** rng.uniform(-3, 3, n)
            A = d[:, None] * A * d[None, :]
        elif family == "band":
            blk = np.arange(n) // 6
            A = np.where(np.abs(blk[:, None] - blk[None, :]) > 3, 0.0, A)
            A = mirror(A)
            A[np.diag_indices(n)] += np.abs(A).sum(1)
    return mirror(A), rng.standard_normal(n)


def cholesky_ld(A):
    """the 80-bit Cholesky factor of the lower triangle of A, by plain row operations"""
    A = np.asarray(A, LD)
    n = len(A)
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        assert d > 0, "not positive definite"
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _worst(num, den):
    if not (np.all(np.isfinite(num)) and np.all(np.isfinite(den))):
        return float("inf")
    zero = den == 0
    if np.any(num[zero] != 0):
        return float("inf")
    r = num[~zero] / den[~zero]
    return float(r.max()) if r.size else 0.0


def factor_ratio(A, Lh):
    """max over the lower triangle of |A - L L^T| / (gamma(n + 1) |L| |L^T|); Lh: the matrix a kernel left (its upper triangle is ignored)"""
    n = len(A)
    L = np.tril(np.asarray(Lh, LD))
    if not np.all(np.isfinite(L)):
        return float("inf")
    il = np.tril_indices(n)
    num = np.abs(np.asarray(A, LD) - L @ L.T)[il]
    den = (gamma(n + 1) * (np.abs(L) @ np.abs(L).T))[il]
    return _worst(num, den)


def solution_ratio(A, b, x, L):
    """max over the rows of |b - A x| / (gamma(3 n + 1) |L| |L^T| |x|); A: its lower triangle is the matrix; L: a factor of it"""
    n = len(A)
    x = np.asarray(x, LD)
    L = np.tril(np.asarray(L, LD))
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(L))):
        return float("inf")
    As = mirror(np.asarray(A, LD))
    num = np.abs(np.asarray(b, LD) - As @ x)
    den = gamma(3 * n + 1) * (np.abs(L) @ (np.abs(L).T @ np.abs(x)))
    return _worst(num, den)


def forward_f64(L, b):
    """L y = b by rows in f64"""
    y = np.array(b, np.float64)
    for i in range(len(y)):
        y[i] = (y[i] - L[i, :i] @ y[:i]) / L[i, i]
    return y


def backward_f64(L, y, skip=None):
    """L^T x = y by rows in f64; skip = (r, c): the contribution of x[r] to row c is left out (a planted error)"""
    x = np.array(y, np.float64)
    for i in range(len(x) - 1, -1, -1):
        col = L[i + 1:, i].copy()
        if skip is not None and skip[1] == i and skip[0] > i:
            col[skip[0] - i - 1] = 0.0
        x[i] = (x[i] - col @ x[i + 1:]) / L[i, i]
    return x


def block_elimination_f64(A, b):
    """k_ba_solve_lds's algorithm in NumPy f64, 6 x 6 blocks:
         for j: W = A_jj^-1; T_I = A_Ij W (I > j); A_IK -= T_I A_Kj^T (I >= K > j); b_I -= T_I b_j
         then y_j = W_j b_j and x_j = y_j - sum_{I > j} T_Ij^T x_I"""
    A = mirror(np.array(A, np.float64))
    z = np.array(b, np.float64)
    n = len(A)
    nb = n // 6
    assert n == 6 * nb
    B = lambda I, J: (slice(6 * I, 6 * I + 6), slice(6 * J, 6 * J + 6))
    W, T = [None] * nb, {}
    for j in range(nb):
        W[j] = np.linalg.inv(A[B(j, j)])
        col = {I: A[B(I, j)].copy() for I in range(j + 1, nb)}
        for I in range(j + 1, nb):
            T[I, j] = col[I] @ W[j]
        for I in range(j + 1, nb):
            for K in range(j + 1, I + 1):
                A[B(I, K)] -= T[I, j] @ col[K].T
            A[B(I, I)] = mirror(A[B(I, I)])   # (the kernel's inverse reads the lower half of a pivot block)
            z[6 * I:6 * I + 6] -= T[I, j] @ z[6 * j:6 * j + 6]
    x = np.zeros(n)
    for j in range(nb):
        x[6 * j:6 * j + 6] = W[j] @ z[6 * j:6 * j + 6]
    for j in range(nb - 1, 0, -1):
        for K in range(j):
            x[6 * K:6 * K + 6] -= T[j, K].T @ x[6 * j:6 * j + 6]
    return x


def one_bad_pivot(A, j, kind):
    """A with row and column j cut loose and its diagonal entry replaced: exactly pivot j is not positive, in every elimination order.
    kind: 'neg' (-1), 'zero' (an exact 0) or 'nan'"""
    A = np.array(A, np.float64)
    A[j, :] = 0.0
    A[:, j] = 0.0
    A[j, j] = {"neg": -1.0, "zero": 0.0, "nan": np.nan}[kind]
    return A
