"""tests/pnpsolver_ref.py and tests/pnpsolver_cases.py on their own (no GPU): the restatement recovers planted poses, its float64 and
longdouble chains agree inside the chain layer's exclusion cap, the walk asd_pnp_ransac applies equals the literal state machine of
PnPsolver.cc:182-257, the tracked sampling equals the vector swap, and asd_pnp_ransac_parameters (host only, through ctypes) equals the
restated SetRansacParameters."""
import numpy as np
import pytest

from tests import pnpsolver_cases as C
from tests import pnpsolver_ref as R


def test_case_list_covers_the_issue():
    assert set(C.CASES) >= {"clean64", "noisy150", "min15", "n_eq_min", "n_lt_min", "n63", "n64", "n65", "n257", "carry", "coplanar", "behind"}
    assert len(C.BATCH) == 3 and set(C.BATCH) <= set(C.CASES)
    for case in C.CASES:
        P = C.problem(case)
        assert P["n_iter"] <= 40 and P["draws"].shape == (P["n_iter"], 4)
        if P["n"] >= 4:
            assert all(0 <= P["draws"][k, i] <= P["n"] - 1 - i for k in range(P["n_iter"]) for i in range(4))
    assert C.problem("min15")["n_iter"] == 14 and C.problem("n_eq_min")["n_iter"] == 1
    assert C.problem("n_lt_min")["n"] < C.problem("n_lt_min")["min_inliers"]
    P = C.problem("coplanar")
    assert np.unique(P["P3Dw"][:, 2]).size == 1
    P = C.problem("behind")
    depth = (P["P3Dw"].astype(np.float64) @ P["R_true"].T + P["t_true"])[:, 2]
    assert int((depth < 0).sum()) == P["n"] // 4


@pytest.mark.parametrize("case", ["clean64", "noisy150"])
def test_refine_on_the_true_inlier_set_recovers_the_pose(case):
    """The bound is what the input perturbation implies, without credit for averaging.  An image perturbation of delta pixels turns a ray
    by delta / f, so |dR| <= 4 delta / f (4: an entry of R moves by at most the angle, and the least-squares fit of EPnP is allowed a
    factor over the single-ray figure); a rotation error of that angle moves a point at depth Z sideways by Z times it, and depth is
    observed through the lateral extent of the scene (8 m half width at up to 30 m), so |dt| <= 4 delta / f * 30 * (30 / 8).
    clean64: delta = the f32 rounding of the image point (half an ulp at 1241 px: 6.1e-5) plus that of the world point seen at 6 m
    (30 * 2^-24 / 6 * f = 2.1e-4 px): 2.8e-4 px.  noisy150: delta = the 0.5 px noise (the sigma itself: 105 points average it down)."""
    P = C.problem(case)
    f = float(P["K"][0])
    delta = 2.8e-4 if case == "clean64" else 0.5
    r = C.refine(case, P["planted"], R.LD)
    dR = float(np.abs(np.asarray(r["c"]["R"], np.float64) - P["R_true"]).max())
    dt = float(np.abs(np.asarray(r["c"]["t"], np.float64) - P["t_true"]).max())
    print(f"{case}: |dR| {dR:.3g} (bound {4 * delta / f:.3g}), |dt| {dt:.3g} (bound {4 * delta / f * 30 * 30 / 8:.3g})")
    assert dR <= 4 * delta / f and dt <= 4 * delta / f * 30 * 30 / 8
    assert np.array_equal(r["mask"], P["planted"])


@pytest.mark.parametrize("case", C.CASES)
def test_f64_and_longdouble_chains_agree_inside_the_exclusion_cap(case):
    P = C.problem(case)
    H = C.reference_hypotheses(case)
    left_out = sum(R.excluded(h["c64"], h["cld"]) for h in H)
    assert left_out <= R.MAX_EXCLUDED * max(len(H), 1), (case, left_out, len(H))
    for h in H:
        if h["count"] >= P["min_inliers"]:
            r = C.refine(case, h["mask"])
            assert not R.excluded(r["c"], r["cld"]), (case, "a Refine is never left out", R.chain_distance(r["c"], r["cld"]))


def test_basis_residual_constant():
    """JACOBI_RESIDUAL_UNITS is the worst residual of this file's float64 Jacobi over every hypothesis and Refine of the case list"""
    worst = 0.0
    for case in C.CASES:
        P = C.problem(case)
        items = []
        for h in C.reference_hypotheses(case):
            items.append((h["idx"], h["c64"]))
            if h["count"] >= P["min_inliers"]:
                items.append((list(np.nonzero(h["mask"])[0]), C.refine(case, h["mask"])["c"]))
        for sel, c in items:
            b = R.basis_check(c["cws"], c["v"], c["eig"], P["P3Dw"][sel], P["P2D"][sel], P["K"])
            cc = R.control_check(c["cws"], P["P3Dw"][sel])
            worst = max(worst, b["residual"])
            assert b["unit"] <= 1e-14 and b["orth"] <= 1e-13 and b["ascending"], (case, b)
            assert b["below_rest"] <= R.JACOBI_RESIDUAL_UNITS and b["eig_err"] <= R.JACOBI_RESIDUAL_UNITS, (case, b)
            assert cc["centroid"] <= 1 and cc["descending"] and cc["residual"] <= 64 + len(sel) and cc["lam_err"] <= 64 + len(sel), (case, cc)
    print(f"worst float64 Jacobi residual over the case list: {worst:.4g} eps64 |MtM|_2 (constant {R.JACOBI_RESIDUAL_UNITS})")
    assert 0.5 * R.JACOBI_RESIDUAL_UNITS <= worst <= R.JACOBI_RESIDUAL_UNITS


def test_clean64_has_five_samples_that_do_not_depend_on_the_null_basis():
    P = C.problem("clean64")
    rots = [None] + [C.null_rotation(100 + i) for i in range(8)]
    good = 0
    for k, d in enumerate(P["draws"]):
        idx = R.sample(d, P["n"])
        if not P["planted"][idx].all():
            continue
        ok = True
        for q in rots:
            c = R.compute_pose(P["P3Dw"][idx], P["P2D"][idx], P["K"], np.float64, rotate_null=q)
            ok = ok and np.array_equal(R.check_inliers(c["R"], c["t"], P["P3Dw"], P["P2D"], P["K"], P["max_err"]), P["planted"])
            if not ok:
                break
        good += ok
    assert good >= 5, good


def test_sampling_equals_the_vector_swap():
    rng = np.random.default_rng(5)
    for n in (4, 5, 6, 7, 64, 150):
        for _ in range(300):
            d = [int(rng.integers(0, n - i)) for i in range(4)]
            idx = R.sample(d, n)
            assert idx == R.sample_tracked(d, n) and len(set(idx)) == 4
            assert R.draws_of(idx, n) == d
    assert R.sample([3, 0, 0, 0], 4) == [3, 0, 2, 1]
    assert R.sample([0, 0, 0, 0], 6) == [0, 5, 4, 3] == R.sample_tracked([0, 0, 0, 0], 6)


def _literal_against_walk(counts, masks, refine_count_of_mask, best_in, best_mask_in, min_inliers):
    ref_calls = []
    def rc(k):
        ref_calls.append(k)
        return refine_count_of_mask(masks[k])
    w = R.walk(counts, rc, best_in, min_inliers)
    lit, calls = R.walk_literal(counts, refine_count_of_mask, masks, best_in, best_mask_in, min_inliers)
    for f in lit:
        assert w[f] == lit[f], (f, w, lit, counts, best_in, min_inliers)
    assert ref_calls == w["refines"] and len(ref_calls) <= calls
    return w


def test_walk_equals_the_literal_state_machine_on_random_counts():
    rng = np.random.default_rng(11)
    found = carried = 0
    for _ in range(3000):
        n_it = int(rng.integers(1, 12))
        min_inl = int(rng.integers(4, 12))
        counts = [int(c) for c in rng.integers(0, 20, n_it)]
        masks = [("m", k) for k in range(n_it)]
        rcount = {m: int(rng.integers(0, 20)) for m in masks}
        best_in, best_mask_in = 0, None
        if rng.random() < 0.5:          # a best model carried in from an earlier call: its Refine failed there (or the call had returned)
            best_in = int(rng.integers(min_inl, 20))
            best_mask_in = ("m", "carried")
            rcount[best_mask_in] = int(rng.integers(0, min_inl + 1))
            carried += 1
        w = _literal_against_walk(counts, masks, lambda m: rcount[m], best_in, best_mask_in, min_inl)
        found += w["found"]
    assert found > 300 and carried > 1000


@pytest.mark.parametrize("case", [c for c in C.CASES if c != "n_lt_min"])
def test_walk_equals_the_literal_state_machine_on_the_cases(case):
    P = C.problem(case)
    H = C.reference_hypotheses(case)
    masks = [h["mask"] for h in H]
    count_of = lambda m: C.refine(case, m)["count"]
    carried = None
    if P["best_inliers"] > 0:
        carried = np.zeros(P["n"], bool)     # a carried best model whose Refine failed: any mask whose Refine stays at or under min_inliers
        carried[:4] = True
        assert count_of(carried) <= P["min_inliers"]
    _literal_against_walk([h["count"] for h in H], masks, count_of, P["best_inliers"], carried, P["min_inliers"])


def test_parameters_entry_point_restates_set_ransac_parameters(pkg):
    from_lib = pkg.capi.pnp_ransac_parameters
    assert R.parameters(15, 0.99, 10, 300, 4, 0.5) == (10, 14)
    assert R.parameters(64, 0.99, 10, 300, 4, 0.5) == (32, 35)
    assert R.parameters(10, 0.99, 10, 300, 4, 0.5) == (10, 1)            # min == n
    assert R.parameters(1000, 0.99, 10, 300, 4, 0.05)[1] == 300          # the cap
    assert R.parameters(20, 0.99, 15, 300, 4, 0.4)[0] == 15              # epsilon raised by min / n
    table = [(n, prob, mi, mx, ms, eps) for n in (0, 3, 4, 8, 10, 15, 64, 150, 1000, 8192) for prob in (0.5, 0.99, 1.0)
             for mi in (0, 4, 10, 64) for mx in (1, 35, 300) for ms in (4,) for eps in (0.0, 0.05, 0.4, 0.5, 1.0, 1.5)]
    table += [(3, 0.99, 2, 300, 3, 0.5), (50, 0.99, 10, 300, 6, 0.1), (2 ** 31 - 1, 0.99, 10, 300, 4, 8.0)]
    for row in table:
        assert from_lib(*row) == R.parameters(*row), row
    assert R.n_iter_rule(5, 35, 0) == 35 and R.n_iter_rule(5, 35, 33) == 5 and R.n_iter_rule(5, 35, 40) == 5
