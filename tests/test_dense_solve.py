"""The five dense SPD solves every optimiser ends in, each as ONE solve through asd_debug_dense_solve, against the backward-error
bounds of tests/dense_solve_ref.py (80-bit; proved on the CPU by tests/test_dense_solve_ref.py).

  form 0  k_ba_solve_lds   block elimination, explicit 6 x 6 pivot inverses      1, 2, 15, 29, 30 pose blocks
  form 1  k_ba_chol_lds    block Cholesky in LDS, Newton reciprocal square roots  1, 16, 31, 32
  form 2  k_ba_chol        one-workgroup Cholesky out of global memory            1, 33, 39, 64
  form 3  gba_solve_enqueue, trailing update on v_mfma_f64_16x16x4_f64            n = 1 .. 581 (dense_solve_ref.TILED_SIZES)
  form 4  the same on plain FMA

Bars (the worst left side over the c = 1 right side must stay at or below c): forms 2, 3, 4: c = 2 on the factor and on the solution;
form 1: c = 4 on the solution, with the 80-bit factor of A in the bound (the kernel keeps L in LDS); form 0: c = FORM0_C = 4 -- its
algorithm restated in NumPy f64 reaches 0.373 of the solution bound over these cases, 8 x that is 3.04, below the floor of 4.
Measured on an MI355X (worst over each form's cases; printed when the module finishes, recorded in DESIGN.md):
  form 0: solution 0.173 (plain, n = 6)   form 1: solution 0.116 (band, n = 6)   form 2: factor 0.331 (plain, n = 6), solution 0.098
  forms 3 and 4 alike: factor 0.828, solution 0.258 (plain, n = 1: one sqrt and two divisions, what numpy's f64 gives too); beyond
  n = 6 no form exceeds 0.19 of the factor bound or 0.06 of the solution bound.
"""
import ctypes as C

import numpy as np
import pytest

from tests import dense_solve_ref as R

pytestmark = pytest.mark.gpu

FORMS = (0, 1, 2, 3, 4)
BAR = {0: R.FORM0_C, 1: R.C_CHOL_LDS, 2: R.C_CHOL, 3: R.C_CHOL, 4: R.C_CHOL}
CASES = [(f, fam, n) for f in (0, 1, 2) for fam, n in R.form_cases(f)] + [(f, fam, n) for f in (3, 4) for fam, n in R.tiled_cases()]
FAIL_N = {0: 90, 1: 186, 2: 234, 3: 289, 4: 289}   # 15 / 31 / 39 pose blocks; three full tiles and a clipped one of one row
ASD_ERR_INVALID = -1


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def same_result(a, b):
    """x, the flag and (where it comes back) the lower triangle of L, bit for bit"""
    if a["chol_ok"] != b["chol_ok"] or not same_bits(a["x"], b["x"]):
        return False
    return a["L"] is None or same_bits(np.tril(a["L"]), np.tril(b["L"]))


def new_ctx(pkg):
    return pkg.AsdHip(n_features=500, max_width=640, max_height=240, max_patches=1024)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = new_ctx(pkg)
    yield c
    c.close()


@pytest.fixture(scope="module")
def solved(ctx):
    """(form, family, n) -> (A, b, result) of the first solve of that input on the module's context"""
    memo = {}

    def get(form, family, n):
        if (form, family, n) not in memo:
            A, b = R.make(family, n)
            memo[form, family, n] = (A, b, ctx.dense_solve(A, b, form))
        return memo[form, family, n]
    return get


@pytest.fixture(scope="module")
def factor_ld():
    memo = {}

    def get(family, n):
        if (family, n) not in memo:
            memo[family, n] = R.cholesky_ld(R.make(family, n)[0])
        return memo[family, n]
    return get


@pytest.fixture(scope="module")
def worst():
    w = {f: {"factor": (0.0, None), "solution": (0.0, None)} for f in FORMS}
    yield w
    print()
    for f in FORMS:
        print(f"dense solve form {f}: worst factor ratio {w[f]['factor'][0]:.3f} {w[f]['factor'][1]}, "
              f"worst solution ratio {w[f]['solution'][0]:.3f} {w[f]['solution'][1]} (bar {BAR[f]:g})")


@pytest.mark.parametrize("form,family,n", CASES, ids=[f"form{f}-{fam}-{n}" for f, fam, n in CASES])
def test_backward_error_bounds(form, family, n, solved, factor_ld, worst):
    A, b, r = solved(form, family, n)
    assert r["chol_ok"] == 1
    if form >= 2:
        rf = R.factor_ratio(A, r["L"])
        rs = R.solution_ratio(A, b, r["x"], r["L"])
        if rf > worst[form]["factor"][0]:
            worst[form]["factor"] = (rf, (family, n))
    else:
        assert r["L"] is None
        rf = None
        rs = R.solution_ratio(A, b, r["x"], factor_ld(family, n))
    if rs > worst[form]["solution"][0]:
        worst[form]["solution"] = (rs, (family, n))
    print(f"form {form} {family} n={n}: factor {rf if rf is None else round(rf, 4)} solution {rs:.4f} (bar {BAR[form]:g})")
    if rf is not None:
        assert rf <= BAR[form]
    assert rs <= BAR[form]


@pytest.mark.parametrize("form", FORMS)
def test_two_runs_give_the_same_bits(form, ctx, solved):
    cases = R.tiled_cases() if form >= 3 else R.form_cases(form)
    for family, n in [c for c in cases if c[1] in (1, 6, 90, 186, 192, 234, 145, 289)]:
        A, b, first = solved(form, family, n)
        assert same_result(ctx.dense_solve(A, b, form), first), (family, n)


@pytest.mark.parametrize("form", (3, 4))
@pytest.mark.parametrize("n", (7, 97, 145, 193, 289))
def test_upper_triangle_is_never_read(form, n, ctx, solved):
    """the strict upper triangle full of NaN: L, x and the flag are those of the mirrored matrix, bit for bit; and outside the
    diagonal tiles the upper triangle comes back as it went in (gba.h) -- in both runs"""
    A, b, ref = solved(form, "scaled" if n != 193 else "band", n)
    An = A.copy()
    An[np.triu_indices(n, 1)] = np.nan
    got = ctx.dense_solve(An, b, form)
    assert got["chol_ok"] == 1 and same_result(got, ref)
    tile = np.arange(n) // R.TILE
    outside = (tile[:, None] < tile[None, :])
    assert same_bits(got["L"][outside], An[outside]) and same_bits(ref["L"][outside], A[outside])
    # inside the diagonal tiles nothing that was read came from above the diagonal either: the NaNs are still NaNs there
    assert np.all(np.isnan(got["L"][np.triu_indices(n, 1)]))
    # (gba.h promises nothing inside them: the MFMA form stores the diagonal 16 x 16 blocks of a trailing diagonal tile whole)
    inside = np.triu(np.ones((n, n), bool), 1) & ~outside
    print(f"form {form} n={n}: {int((bits(ref['L'][inside]) != bits(A[inside])).sum())} of {int(inside.sum())} upper entries inside the diagonal tiles rewritten")


def bad_rows(form):
    """a row of the first block / tile, of a middle one, and the last row (the last, clipped, tile of forms 3 and 4)"""
    n = FAIL_N[form]
    return (3, 96 + 50, n - 1) if form >= 3 else (3, 6 * (n // 12) + 2, n - 1)


@pytest.mark.parametrize("kind", ("neg", "zero", "nan"))
@pytest.mark.parametrize("form", FORMS)
def test_one_pivot_not_positive(form, kind, ctx):
    """flag 0 and ASD_OK, wherever the pivot sits.  Forms 3 and 4 with the pivot in tile 0: the good tiles behind it leave the flag at 0
    (k_gba_potrf's k > 0 branch)"""
    n = FAIL_N[form]
    A, b = R.make("plain", n)
    for j in bad_rows(form):
        r = ctx.dense_solve(R.one_bad_pivot(A, j, kind), b, form)   # (an error status would raise)
        assert r["chol_ok"] == 0, (j, kind)


@pytest.mark.parametrize("form", FORMS)
def test_flag_is_set_again_by_a_good_solve(form, ctx, solved):
    n = FAIL_N[form]
    A, b, ref = solved(form, "plain", n)
    assert same_result(ctx.dense_solve(A, b, form, chol_ok_in=0), ref) and ref["chol_ok"] == 1


def test_good_solve_after_a_failed_one_has_fresh_context_bits(pkg, ctx):
    fresh = new_ctx(pkg)
    try:
        want = {}
        for form in FORMS:
            A, b = R.make("scaled", FAIL_N[form])
            want[form] = fresh.dense_solve(A, b, form)
    finally:
        fresh.close()
    for form in FORMS:
        A, b = R.make("scaled", FAIL_N[form])
        assert ctx.dense_solve(R.one_bad_pivot(A, bad_rows(form)[1], "neg"), b, form)["chol_ok"] == 0
        got = ctx.dense_solve(A, b, form)
        assert got["chol_ok"] == 1 and same_result(got, want[form]), form


@pytest.mark.parametrize("form", FORMS)
def test_done_writes_nothing(form, ctx):
    n = FAIL_N[form]
    A, b = R.make("plain", n)
    A[np.triu_indices(n, 1)] = -7.25   # (not a mirror: the matrix must come back as given, not as some symmetric copy)
    sentinel = np.arange(n) * 0.5 - 1234.0
    for flag in (0, 1):
        r = ctx.dense_solve(A, b, form, done=1, chol_ok_in=flag, x0=sentinel)
        assert same_bits(r["x"], sentinel) and r["chol_ok"] == flag
        if form >= 2:
            assert same_bits(r["L"], A)


def raw_call(ctx, form, n):
    """the C entry point with a size its buffers do not have: a refusal must come before anything is read"""
    buf = np.zeros(8)
    ok = C.c_int32(-1)
    ctx.lib.asd_debug_dense_solve.restype = C.c_int32
    p = buf.ctypes.data_as(C.c_void_p)
    return int(ctx.lib.asd_debug_dense_solve(ctx.ctx, C.c_int32(form), C.c_int32(n), p, p, C.c_int32(0), C.c_int32(1), None, p, C.byref(ok)))


def test_refusals(pkg, synth, ctx):
    for form in FORMS:
        for n in (0, -6):
            assert raw_call(ctx, form, n) == ASD_ERR_INVALID, (form, n)
    for form, n in ((0, 7), (1, 7), (2, 7), (0, 6 * 31), (1, 6 * 33), (2, 6 * 2049), (3, 7 * 2048 + 1), (4, 7 * 2048 + 1), (5, 6), (-1, 6)):
        assert raw_call(ctx, form, n) == ASD_ERR_INVALID, (form, n)
        assert "asd_debug_dense_solve" in ctx.last_error()
    A, b = R.make("plain", 7)
    for form in (0, 1, 2):
        with pytest.raises(pkg.AsdError) as e:
            ctx.dense_solve(A, b, form)
        assert e.value.code == ASD_ERR_INVALID
    # the sizes just inside are taken (form 2's and the tiled forms' limits are too large for a test)
    for form, n in ((0, 180), (1, 192)):
        A, b = R.make("plain", n)
        assert ctx.dense_solve(A, b, form)["chol_ok"] == 1
    # ... and nothing runs while a LocalBA lane run is outstanding
    A, b = R.make("plain", 12)
    ctx.local_ba_submit(synth.ba_problem(n_free=4, n_fixed=2, n_points=200, seed=7))
    try:
        for form in FORMS:
            with pytest.raises(pkg.AsdError) as e:
                ctx.dense_solve(A, b, form)
            assert e.value.code == ASD_ERR_INVALID and "asd_local_ba_wait" in str(e.value)
    finally:
        ctx.local_ba_wait()
    assert ctx.dense_solve(A, b, 0)["chol_ok"] == 1
