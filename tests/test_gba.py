"""asd_bundle_adjustment (ba.hip: gba_impl; gba.hip: the tiled Cholesky) -- Optimizer::BundleAdjustment, Optimizer.cc:51-237.

Pinning: tests/golden/gba_golden.npz holds what the REFERENCE's own vendored g2o returns with the reference's solver
(BlockSolverX + LinearSolverEigen, -O2) on the cases of tests/golden/make_gba_golden.py.  Iterations and the trials of every
iteration must equal g2o's; quaternions, translations, points, chi2 (relative) and the edges' chi2 (relative to max(chi2, 1)) must
be within 4 x S of it, S = the largest distance between three reference runs (the same solver built with -mfma -ffp-contract=fast,
and BlockSolver_6_3 + LinearSolverDense), per component, as the generator measured and stored it.  Every case runs in the form the
size picks and in both forced forms (ASD_GBA_SOLVE=tiled|single, read when the context is made).
"""
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.golden.make_gba_golden import CASES, T, problem, trials_of
from tests.test_optimizer import POINT_ATOL, POSE_ATOL

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in CASES]
FORMS = ("default", "tiled", "single")
TILED_FROM = 40   # ASD_GBA_TILED_FROM


@pytest.fixture(scope="module")
def golden():
    G = np.load(os.path.join(GOLDEN, "gba_golden.npz"))
    assert json.loads(str(G["cases"])) == json.loads(json.dumps(CASES)), "the fixture was made from another case list"
    return G


@pytest.fixture(scope="module")
def probs(synth):
    return {c["name"]: problem(c, synth) for c in CASES}


@pytest.fixture(scope="module")
def ctxs(pkg):
    """one context per form; ASD_GBA_SOLVE is read at asd_ctx_create"""
    made = {}
    old = os.environ.pop("ASD_GBA_SOLVE", None)
    try:
        for form in FORMS:
            if form != "default":
                os.environ["ASD_GBA_SOLVE"] = form
            made[form] = pkg.AsdHip(n_features=500, max_width=640, max_height=240, max_patches=1024)
            os.environ.pop("ASD_GBA_SOLVE", None)
        yield made
    finally:
        os.environ.pop("ASD_GBA_SOLVE", None)
        if old is not None:
            os.environ["ASD_GBA_SOLVE"] = old
        for c in made.values():
            c.close()


def run(ctx, pp, **kw):
    return ctx.bundle_adjustment(pp, n_iterations=int(pp["n_iterations"]), robust=int(pp["robust"]), **kw)


def figures(got, exp_poses, exp_points, exp_chi2, exp_edge):
    """[quaternion, translation, points, chi2 relative, edge chi2 relative to max(chi2, 1)], as make_gba_golden.distances"""
    qa, qb = got["poses"][:, :4], exp_poses[:, :4]
    sgn = np.where((qa * qb).sum(1, keepdims=True) < 0, -1.0, 1.0)
    dq = float(np.abs(qa * sgn - qb).max()) if len(qa) else 0.0
    dt = float(np.abs(got["poses"][:, 4:] - exp_poses[:, 4:]).max()) if len(qa) else 0.0
    dp = float(np.abs(got["points"] - exp_points).max()) if len(exp_points) else 0.0
    dc = abs(got["chi2"] - exp_chi2) / abs(exp_chi2) if exp_chi2 != 0 else abs(got["chi2"])
    de = float((np.abs(got["edge_chi2"] - exp_edge) / np.maximum(np.abs(exp_edge), 1.0)).max()) if len(exp_edge) else 0.0
    return np.array([dq, dt, dp, dc, de])


def expected_form(form, nPf, Ea):
    if Ea == 0:
        return -1, 0
    tiled = form == "tiled" or (form == "default" and nPf >= TILED_FROM)
    if tiled:
        return 3, (nPf + T - 1) // T
    return (0 if nPf <= 30 else 1 if nPf <= 32 else 2), 0


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_gba_matches_g2o(name, form, golden, probs, ctxs):
    i, pp, ctx = NAMES.index(name), probs[name], ctxs[form]
    got = run(ctx, pp)
    forms, per_it = ctx.gba_forms(), ctx.gba_trials()
    exp_trials = trials_of(dict(trials=golden[f"c{i}_trials"]))
    fig = figures(got, golden[f"c{i}_poses"], golden[f"c{i}_points"], float(golden[f"c{i}_chi2"]), golden[f"c{i}_edge_chi2"])
    tol = 4 * golden["S"]
    print(f"{name} [{form}] forms {forms} iterations {got['iterations']} trials {per_it} | figures " + " ".join(f"{v:.2e}" for v in fig) +
          " | 4S " + " ".join(f"{v:.2e}" for v in tol))
    assert got["iterations"] == int(golden[f"c{i}_info"][0])
    assert per_it == exp_trials and got["trials"] == sum(exp_trials)
    free_with_edges = len(set(pp["e_pose"][pp["fixed"][pp["e_pose"]] == 0].tolist()))
    assert (forms[0], forms[4]) == expected_form(form, free_with_edges, len(pp["e_point"])), forms
    assert forms[1] == free_with_edges and forms[3] == len(pp["e_point"]) and forms[2] == len(set(pp["e_point"].tolist()))
    for k, what in enumerate(("quaternion", "translation", "points", "chi2", "edge chi2")):
        assert fig[k] <= tol[k], f"{name} [{form}]: {what} {fig[k]:.3e} > 4 S = {tol[k]:.3e}"


@pytest.mark.parametrize("n_free", [T - 1, T, T + 1, 2 * T + 1, 3 * T + 5])
def test_gba_tile_counts(n_free, probs, ctxs):
    run(ctxs["tiled"], probs[f"band_{n_free}"])
    forms = ctxs["tiled"].gba_forms()
    assert forms[0] == 3 and forms[1] == n_free and forms[4] == {T - 1: 1, T: 1, T + 1: 2, 2 * T + 1: 3, 3 * T + 5: 4}[n_free]
    run(ctxs["single"], probs[f"band_{n_free}"])
    assert ctxs["single"].gba_forms()[0] == (0 if n_free <= 30 else 2) and ctxs["single"].gba_forms()[4] == 0


@pytest.mark.parametrize("form", FORMS)
def test_gba_untouched_vertices(form, probs, ctxs):
    """a point without an edge, a free pose without an edge and the fixed pose come back as given: the points bit for bit, the poses
    as a call with n_iterations = 0 returns them (the quaternion normalised, as SE3Quat's constructor does)"""
    ctx = ctxs[form]
    pp = probs["point_no_edges"]
    lone = len(pp["points"]) // 2
    assert not (pp["e_point"] == lone).any()
    got, asis = run(ctx, pp), ctx.bundle_adjustment(pp, n_iterations=0)
    assert np.array_equal(got["points"][lone], pp["points"][lone])
    assert np.array_equal(got["poses"][0], asis["poses"][0]) and np.array_equal(got["poses"][0, 4:], pp["poses"][0, 4:])
    assert not np.array_equal(got["points"][lone + 1], pp["points"][lone + 1])
    pp = probs["pose_no_edges"]
    assert not (pp["e_pose"] == 2).any() and not pp["fixed"][2]
    got, asis = run(ctx, pp), ctx.bundle_adjustment(pp, n_iterations=0)
    for p in (0, 2):
        assert np.array_equal(got["poses"][p], asis["poses"][p]) and np.array_equal(got["poses"][p, 4:], pp["poses"][p, 4:])
        assert np.abs(got["poses"][p, :4] - pp["poses"][p, :4]).max() <= 4e-16
    assert not np.array_equal(got["poses"][1], asis["poses"][1])
    assert np.array_equal(asis["points"], pp["points"]) and asis["iterations"] == 0 and asis["trials"] == 0


@pytest.mark.parametrize("form", ("tiled", "single"))
@pytest.mark.parametrize("name", [f"band_{2 * T + 1}", "loop_20", "far_start"])
def test_gba_two_runs_equal_bits(name, form, probs, ctxs):
    a, b = run(ctxs[form], probs[name]), run(ctxs[form], probs[name])
    for k in ("poses", "points", "edge_chi2"):
        assert np.array_equal(a[k], b[k]), k
    assert (a["chi2"], a["iterations"], a["trials"]) == (b["chi2"], b["iterations"], b["trials"])


def test_gba_stop_on_entry(probs, ctxs):
    pp = probs["band_17"]
    stop = np.ones(1, np.int32)
    got = run(ctxs["default"], pp, stop=stop)
    asis = ctxs["default"].bundle_adjustment(pp, n_iterations=0, robust=int(pp["robust"]))
    assert got["iterations"] == 0 and got["trials"] == 0 and ctxs["default"].gba_trials() == []
    assert np.array_equal(got["points"], pp["points"]) and np.array_equal(got["poses"], asis["poses"])
    assert np.array_equal(got["poses"][:, 4:], pp["poses"][:, 4:]) and np.abs(got["poses"] - pp["poses"]).max() <= 4e-16
    assert got["chi2"] == asis["chi2"] and np.array_equal(got["edge_chi2"], asis["edge_chi2"])
    stop[0] = 0   # a flag that is present and clear changes nothing
    a, b = run(ctxs["default"], pp, stop=stop), run(ctxs["default"], pp)
    assert a["iterations"] == b["iterations"] > 0 and np.array_equal(a["poses"], b["poses"]) and np.array_equal(a["points"], b["points"])


def test_gba_capacity_and_refusals(pkg, probs, ctxs):
    ctx = ctxs["default"]
    P = 2048 + 2   # ASD_GBA_MAX_FREE_POSES + 1 free poses (+ the fixed one); no edges: nothing is allocated
    big = dict(poses=np.tile([0.0, 0, 0, 1, 0, 0, 0], (P, 1)), fixed=np.r_[np.uint8(1), np.zeros(P - 1, np.uint8)], points=np.zeros((1, 3)),
               e_point=np.zeros(0, np.int32), e_pose=np.zeros(0, np.int32), e_obs=np.zeros((0, 2)), e_info=np.zeros(0), K=probs["its0"]["K"])
    with pytest.raises(pkg.AsdError) as e:
        ctx.bundle_adjustment(big)
    assert e.value.code == -5 and "ASD_GBA_MAX_FREE_POSES" in str(e.value)
    # edges, but none of their keyframes free: the reference stops on an assertion, the call refuses
    pp = dict(probs["its0"])
    pp["fixed"] = np.ones_like(pp["fixed"])
    with pytest.raises(pkg.AsdError) as e:
        ctx.bundle_adjustment(pp)
    assert e.value.code == -1 and "no free pose" in str(e.value)
    pp = dict(probs["its0"])
    pp["e_pose"] = pp["e_pose"].copy()
    pp["e_pose"][3] = len(pp["poses"])
    with pytest.raises(pkg.AsdError) as e:
        ctx.bundle_adjustment(pp)
    assert e.value.code == -1


def test_gba_refused_while_lane_local_ba_is_outstanding(pkg, synth, probs, ctxs):
    ctx = ctxs["default"]
    lba = synth.ba_problem(n_free=4, n_fixed=2, n_points=200, seed=7)
    ctx.local_ba_submit(lba)
    try:
        with pytest.raises(pkg.AsdError) as e:
            run(ctx, probs["band_17"])
        assert e.value.code == -1 and "asd_local_ba_wait" in str(e.value)
    finally:
        ctx.local_ba_wait()
    assert run(ctx, probs["band_17"])["iterations"] > 0


def test_local_ba_bits_are_unchanged_by_gba(pkg, synth, probs, ctxs):
    """asd_local_ba before and after asd_bundle_adjustment on one context, in either form, returns what a context that never ran
    one returns"""
    lba = synth.ba_problem(n_free=6, n_fixed=3, n_points=400, seed=8)
    fresh = pkg.AsdHip(n_features=500, max_width=640, max_height=240, max_patches=1024)
    try:
        ref = fresh.local_ba(lba)
    finally:
        fresh.close()
    for form in ("tiled", "single"):
        ctx = ctxs[form]
        before = ctx.local_ba(lba)
        run(ctx, probs["band_33"])
        after = ctx.local_ba(lba)
        for res in (before, after):
            for k in ("poses", "points", "edge_chi2", "edge_depth_pos", "edge_outlier1"):
                assert np.array_equal(res[k], ref[k]), (form, k)
            assert (res["chi2_first"], res["chi2_second"], res["iters_first"], res["iters_second"]) == \
                (ref["chi2_first"], ref["chi2_second"], ref["iters_first"], ref["iters_second"])


@pytest.mark.parametrize("form", FORMS)
def test_gba_live_against_reference_local_ba(form, synth, oracle, oracle_mod, ctxs):
    """no fixture: a clean problem on which no chi2 comes near either Huber width, so LocalBA's first round alone
    (its_first = n, its_second = 0) is the same optimisation.  Against the reference's g2o where oracle/_ref is built (BlockSolver_6_3 +
    LinearSolverDense), else against the oracle's restatement of it."""
    n = 8
    pp = synth.gba_map(n_kf=T + 4, pts_per_kf=40, seed=71, pix_noise=0.3, pose_sigma=0.0005, point_sigma=0.002)
    ref = (oracle_mod.RefG2O() if oracle_mod.RefG2O.available(abi=2) else oracle).local_ba(pp, its_first=n, its_second=0)
    ctx = ctxs[form]
    start = ctx.bundle_adjustment(pp, n_iterations=0)
    got = ctx.bundle_adjustment(pp, n_iterations=n, robust=True)
    assert start["edge_chi2"].max() < 5.0 and got["edge_chi2"].max() < 5.0 and ref["edge_chi2"].max() < 5.0
    assert got["iterations"] == ref["iters_first"]
    if "trials_first" in ref:
        assert got["trials"] == ref["trials_first"]
    sgn = np.where((got["poses"][:, :4] * ref["poses"][:, :4]).sum(1, keepdims=True) < 0, -1.0, 1.0)
    print(f"[{form}] live: poses {np.abs(got['poses'] * np.c_[sgn, sgn, sgn, sgn, 1 + 0 * sgn, 1 + 0 * sgn, 1 + 0 * sgn] - ref['poses']).max():.2e} "
          f"points {np.abs(got['points'] - ref['points']).max():.2e}")
    np.testing.assert_allclose(got["poses"][:, :4] * sgn, ref["poses"][:, :4], atol=POSE_ATOL, rtol=0)
    np.testing.assert_allclose(got["poses"][:, 4:], ref["poses"][:, 4:], atol=POSE_ATOL, rtol=0)
    np.testing.assert_allclose(got["points"], ref["points"], atol=POINT_ATOL, rtol=0)
