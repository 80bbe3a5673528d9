"""tests/dense_solve_ref.py proved on the CPU: NumPy's f64 Cholesky and substitutions pass its bounds on every case the GPU tests
run, and a solver that is wrong the way a tiled kernel goes wrong fails them.

The planted errors run on a NumPy f64 restatement of gba.hip's schedule (tiles of 96 rows, right-looking, the trailing update by
16 x 16 blocks): one k-term dropped from one 16 x 16 block of one trailing tile, the last row of the clipped tile left without its
update, one contribution missing from the backward substitution, and the last element of x off by 1e-9 relative.

Headroom measured here (printed by the tests): numpy.linalg.cholesky reaches at most 0.83 of the c = 1 factor bound (at n = 1) and
0.26 of the solution bound over all cases; form 0's restatement reaches 0.373 of the solution bound (FORM0_RESTATED = 0.38; 8 x that is
3.04, so the kernel's bar is the floor, FORM0_C = 4)."""
import numpy as np
import pytest

from tests import dense_solve_ref as R

ALL_CASES = sorted(set(R.tiled_cases() + [c for f in (0, 1, 2) for c in R.form_cases(f)]), key=lambda c: (c[1], c[0]))
TS = R.TILE


def tiled_f64(A, b, drop=None, stale_last_row=False, skip_back=None, nudge_x=False):
    """gba.hip's schedule in NumPy f64.  drop = (k, i, j, rb, cb, kk): tile column k's update of trailing tile (i, j) loses the term of
    column kk in its 16 x 16 block (rb, cb)"""
    A = np.array(A, np.float64)
    n = len(A)
    nt = (n + TS - 1) // TS
    sl = lambda t: slice(t * TS, min((t + 1) * TS, n))
    for k in range(nt):
        A[sl(k), sl(k)] = np.linalg.cholesky(R.mirror(A[sl(k), sl(k)]))
        Lkk = A[sl(k), sl(k)]
        for i in range(k + 1, nt):
            X = A[sl(i), sl(k)]   # X Lkk^T = A(i, k) by columns (substitution: numpy.linalg.solve would pivot)
            for c in range(X.shape[1]):
                X[:, c] = (X[:, c] - X[:, :c] @ Lkk[c, :c]) / Lkk[c, c]
        for i in range(k + 1, nt):
            for j in range(k + 1, i + 1):
                upd = A[sl(i), sl(k)] @ A[sl(j), sl(k)].T
                if drop is not None and drop[:3] == (k, i, j):
                    rb, cb, kk = drop[3:]
                    r0, c0 = sl(i).start + 16 * rb, sl(j).start + 16 * cb
                    rr, cc = slice(16 * rb, 16 * rb + 16), slice(16 * cb, 16 * cb + 16)
                    upd[rr, cc] -= np.outer(A[r0:r0 + 16, k * TS + kk], A[c0:c0 + 16, k * TS + kk])[:upd[rr, cc].shape[0], :upd[rr, cc].shape[1]]
                if stale_last_row and i == nt - 1:
                    upd[-1, :] = 0.0
                A[sl(i), sl(j)] -= upd
    L = np.tril(A)
    x = R.backward_f64(L, R.forward_f64(L, b), skip=skip_back)
    if nudge_x:
        x[-1] *= 1.0 + 1e-9
    return L, x


def ratios(A, b, L, x):
    return R.factor_ratio(A, L), R.solution_ratio(A, b, x, L)


@pytest.fixture(scope="module")
def worst():
    w = {"factor": 0.0, "solution": 0.0}
    yield w
    print(f"\nnumpy f64 Cholesky: worst factor ratio {w['factor']:.3f}, worst solution ratio {w['solution']:.3f} (c = 1 bounds)")


def test_gamma_and_precision():
    assert np.finfo(np.longdouble).eps < 2e-19
    assert float(R.gamma(1)) == pytest.approx(2.0 ** -53, rel=1e-15)
    assert R.FORM0_C == max(4.0, 8.0 * R.FORM0_RESTATED)


def test_families_are_symmetric_and_seeded():
    for fam in R.FAMILIES:
        A, b = R.make(fam, 97)
        A2, b2 = R.make(fam, 97)
        assert np.array_equal(A, A.T) and np.array_equal(A, A2) and np.array_equal(b, b2)
        assert np.all(np.linalg.eigvalsh(A) > 0)
    A, _ = R.make("band", 97)
    blk = np.arange(97) // 6
    assert np.all(A[np.abs(blk[:, None] - blk[None, :]) > 3] == 0.0)
    assert np.linalg.cond(R.make("near", 97)[0]) > 1e11 and np.linalg.cond(R.make("scaled", 97)[0]) > 1e6


def test_longdouble_cholesky_is_a_cholesky():
    A, _ = R.make("scaled", 98)
    L = R.cholesky_ld(A)
    assert L.dtype == np.longdouble and np.all(np.triu(L, 1) == 0)
    assert R.factor_ratio(A, L) < 1e-2   # eps(80 bit) / eps(f64) = 2^-11


@pytest.mark.parametrize("family,n", ALL_CASES, ids=[f"{f}-{n}" for f, n in ALL_CASES])
def test_numpy_cholesky_passes(family, n, worst):
    A, b = R.make(family, n)
    L = np.linalg.cholesky(A)
    x = R.backward_f64(L, R.forward_f64(L, b))
    rf, rs = ratios(A, b, L, x)
    worst["factor"], worst["solution"] = max(worst["factor"], rf), max(worst["solution"], rs)
    print(f"{family} n={n}: factor {rf:.3f} solution {rs:.3f}")
    assert rf <= 1.0 and rs <= 1.0            # the theorems themselves, c = 1
    # ... and with the 80-bit factor in the bound, as forms 0 and 1 are judged
    assert R.solution_ratio(A, b, x, R.cholesky_ld(A)) <= 1.0


def test_tiled_restatement_passes_unplanted():
    for fam in R.FAMILIES:
        for n in (97, 193, 289):
            A, b = R.make(fam, n)
            rf, rs = ratios(A, b, *tiled_f64(A, b))
            assert rf <= R.C_CHOL and rs <= R.C_CHOL, (fam, n, rf, rs)


PLANT_SIZES = (193, 289)   # 193: a clipped tile of one row; 289: off-diagonal trailing tiles, clipped ti and full tj


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("n", PLANT_SIZES)
def test_dropped_k_term_fails_the_factor_check(family, n):
    A, b = R.make(family, n)
    nt = (n + TS - 1) // TS
    # a diagonal trailing tile, the clipped diagonal tile (both beside the diagonal, where `band` has entries too), an off-diagonal one
    drops = [(0, 1, 1, 0, 0, 95), (nt - 2, nt - 1, nt - 1, 0, 0, 95)] + ([(0, nt - 1, 1, 0, 3, 40)] if family != "band" else [])
    for drop in drops:
        try:
            L, x = tiled_f64(A, b, drop=drop)
        except np.linalg.LinAlgError:
            print(f"{family} n={n} drop={drop}: no longer positive definite (a kernel reports chol_ok = 0)")
            continue
        rf, rs = ratios(A, b, L, x)
        print(f"{family} n={n} drop={drop}: factor {rf:.3g} solution {rs:.3g}")
        assert rf > (1 if family == "near" else 100) * R.C_CHOL, (drop, rf)   # (`near`: the lost term itself is tiny)
        if family != "near":
            assert R.solution_ratio(A, b, x, R.cholesky_ld(A)) > 100 * R.FORM0_C, drop   # the check of the forms that return no L


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("n", PLANT_SIZES)
def test_stale_last_row_of_the_clipped_tile_fails(family, n):
    A, b = R.make(family, n)
    L, x = tiled_f64(A, b, stale_last_row=True)
    rf, rs = ratios(A, b, L, x)
    print(f"{family} n={n}: factor {rf:.3g} solution {rs:.3g}")
    assert rf > 100 * R.C_CHOL


@pytest.mark.parametrize("family", ("plain", "scaled", "band"))
@pytest.mark.parametrize("n", PLANT_SIZES)
def test_missing_back_substitution_term_fails(family, n):
    A, b = R.make(family, n)
    for skip in ((n - 1, n - 2), (100, 3), (n - 1, 0)) if family != "band" else ((n - 1, n - 2), (100, 97)):
        L, x = tiled_f64(A, b, skip_back=skip)
        rf, rs = ratios(A, b, L, x)
        print(f"{family} n={n} skip={skip}: factor {rf:.3g} solution {rs:.3g}")
        assert rf <= R.C_CHOL and rs > 100 * R.C_CHOL, skip


@pytest.mark.parametrize("family", ("plain", "scaled", "band"))
@pytest.mark.parametrize("n", PLANT_SIZES)
def test_last_element_off_by_1e_9_fails(family, n):
    A, b = R.make(family, n)
    L, x = tiled_f64(A, b, nudge_x=True)
    rf, rs = ratios(A, b, L, x)
    print(f"{family} n={n}: solution {rs:.3g}")
    assert rf <= R.C_CHOL and rs > R.C_CHOL
    assert R.solution_ratio(A, b, x, R.cholesky_ld(A)) > R.C_CHOL_LDS


def test_non_finite_results_fail():
    A, b = R.make("plain", 7)
    L = np.linalg.cholesky(A)
    x = R.backward_f64(L, R.forward_f64(L, b))
    Ln, xn = L.copy(), x.copy()
    Ln[3, 1], xn[2] = np.nan, np.inf
    assert R.factor_ratio(A, Ln) == float("inf") and R.solution_ratio(A, b, xn, L) == float("inf")
    # the strict upper triangle of what a kernel hands back is not part of L
    Lu = L.copy()
    Lu[np.triu_indices(7, 1)] = np.nan
    assert R.factor_ratio(A, Lu) == R.factor_ratio(A, L)


def test_form0_restatement_figure():
    """block_elimination_f64's worst solution ratio over the form-0 cases: the figure form 0's bar is made from"""
    w = 0.0
    for fam, n in R.form_cases(0):
        A, b = R.make(fam, n)
        r = R.solution_ratio(A, b, R.block_elimination_f64(A, b), R.cholesky_ld(A))
        print(f"{fam} n={n}: {r:.3f}")
        w = max(w, r)
    print(f"form 0 restated: worst solution ratio {w:.3f}; FORM0_RESTATED = {R.FORM0_RESTATED}, bar {R.FORM0_C}")
    assert w <= R.FORM0_RESTATED
    # and it solves: against the Cholesky solution, far inside what the conditioning allows
    A, b = R.make("plain", 180)
    L = np.linalg.cholesky(A)
    assert np.allclose(R.block_elimination_f64(A, b), R.backward_f64(L, R.forward_f64(L, b)), rtol=1e-8, atol=0)


def test_one_bad_pivot():
    A, _ = R.make("plain", 24)
    for kind in ("neg", "zero", "nan"):
        B = R.one_bad_pivot(A, 13, kind)
        keep = np.arange(24) != 13
        assert np.all(np.linalg.eigvalsh(B[np.ix_(keep, keep)]) > 0) and np.all(B[13, keep] == 0) and not B[13, 13] > 0
