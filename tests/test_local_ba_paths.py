"""LocalBundleAdjustment on every form asd_local_ba picks from the shape of the problem (ba.hip, local_ba_impl):
  - the dense solve of the reduced pose system by nPf, the free poses with active edges: k_ba_solve_lds (1-30),
    k_ba_chol_lds (31-32), k_ba_chol (33 and more);
  - the active structure: built on the device (k_ba_struct_*) when P <= 1024, at most 32 free poses and no duplicate
    (pose, landmark) edges, else on the host (and on the host everywhere with ASD_BA_STRUCT=host).

Pinning: tests/golden/ba_paths_golden.npz holds the outputs of the REFERENCE's own vendored g2o on these problems
(tests/golden/make_ba_paths_golden.py, which also makes the problems: synth.ba_problem plus explicit post-edits).  The bar is
tests/test_optimizer.py's: poses 1e-8, points 1e-6, outlier / depth flags and iteration counts identical, chi2 relative 1e-6.
asd_debug_local_ba_forms reports which forms ran, so a later change of a threshold cannot quietly stop a case covering its path.
"""
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.golden.make_ba_paths_golden import CASES, OUT_KEYS, problem
from tests.golden.make_live_golden import problem_digest
from tests.test_optimizer import POINT_ATOL, POSE_ATOL

NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: (i, c) for i, c in enumerate(CASES)}
SOLVE = {0: "solve_lds", 1: "chol_lds", 2: "chol"}
RESULT_KEYS = ("poses", "points", "edge_chi2", "edge_outlier1", "edge_depth_pos", "chi2_first", "chi2_second", "iters_first", "iters_second")


@pytest.fixture(scope="module")
def golden():
    G = np.load(os.path.join(GOLDEN, "ba_paths_golden.npz"))
    assert json.loads(str(G["cases"])) == json.loads(json.dumps(CASES)), "the fixture was made from another case list"
    return G


@pytest.fixture(scope="module")
def probs(synth):
    return {c["name"]: problem(c, synth) for c in CASES}


def stored(G, i):
    return {k: G[f"c{i}_out_{k}"] for k in OUT_KEYS}


def check_result(got, exp, what):
    """the bar of tests/test_optimizer.py::check_ba; exp["edge_chi2"] may be the fixture's float32 copy"""
    np.testing.assert_allclose(got["poses"], exp["poses"], atol=POSE_ATOL, rtol=0, err_msg=what)
    np.testing.assert_allclose(got["points"], exp["points"], atol=POINT_ATOL, rtol=0, err_msg=what)
    np.testing.assert_array_equal(got["edge_outlier1"], exp["edge_outlier1"], err_msg=what)
    np.testing.assert_array_equal(got["edge_depth_pos"], exp["edge_depth_pos"], err_msg=what)
    np.testing.assert_allclose(got["edge_chi2"], np.asarray(exp["edge_chi2"], np.float64), rtol=1e-6, atol=1e-7, err_msg=what)
    assert (int(got["iters_first"]), int(got["iters_second"])) == (int(exp["iters_first"]), int(exp["iters_second"])), what
    np.testing.assert_allclose(got["chi2_first"], float(exp["chi2_first"]), rtol=1e-6, err_msg=what)
    np.testing.assert_allclose(got["chi2_second"], float(exp["chi2_second"]), rtol=1e-6, err_msg=what)


def max_diffs(got, exp):
    return float(np.abs(got["poses"] - exp["poses"]).max()), float(np.abs(got["points"] - exp["points"]).max())


def masked_pose(prob):
    """the free pose whose observations make_ba_paths_golden.problem made gross outliers"""
    free = np.flatnonzero(prob["fixed"] == 0)
    return int(free[len(free) // 2])


# ------------------------------------------------------------------ the fixture and the oracle (CPU)
def test_paths_golden_inputs_match_generator(golden, probs):
    for i, c in enumerate(CASES):
        assert problem_digest(probs[c["name"]]) == str(golden[f"c{i}_in_sha256"]), f"{c['name']}: the generator no longer makes the stored problem"


def test_paths_cases_have_their_shapes(probs):
    """each case has the shape that selects its forms (what the device reports is checked on the GPU)"""
    for c in CASES:
        prob = probs[c["name"]]
        P, free = len(prob["poses"]), int((prob["fixed"] == 0).sum())
        solve, struct = c["forms"]
        assert solve == (0 if free <= 30 else 1 if free <= 32 else 2), c["name"]
        pairs = prob["e_pose"].astype(np.int64) * len(prob["points"]) + prob["e_point"]
        dup = len(np.unique(pairs)) < len(pairs)
        assert struct == int(P > 1024 or free > 32 or dup), c["name"]
        assert dup == (c["edit"] == "dup"), c["name"]
        if c["edit"] in ("interleave", "pad1092"):   # fixed ids are not a prefix
            assert (np.diff(prob["fixed"].astype(int)) > 0).any(), c["name"]
        assert set(np.unique(prob["e_pose"])) >= set(np.flatnonzero(prob["fixed"] == 0)), f"{c['name']}: a free pose without edges"


def test_paths_golden_is_not_on_a_knife_edge(golden, probs):
    """no edge's final chi2 lies within 1e-6 (relative) of the 5.991 gate: a last-bit difference cannot flip a flag"""
    for i, c in enumerate(CASES):
        chi2 = golden[f"c{i}_out_edge_chi2"].astype(np.float64)
        margin = np.abs(chi2 - 5.991) / 5.991
        assert margin.min() >= 1e-6, f"{c['name']}: edge {int(margin.argmin())} chi2 {chi2[margin.argmin()]}"
    # the masked-pose case: every observation of that pose is gated out after round 1 (round 2 has none of its edges)
    i, c = BY_NAME["masked_pose"]
    sel = probs["masked_pose"]["e_pose"] == masked_pose(probs["masked_pose"])
    assert sel.sum() > 20 and golden[f"c{i}_out_edge_outlier1"][sel].all()


def test_oracle_matches_paths_golden(oracle, oracle_mod, golden, probs):
    """the oracle against the stored g2o outputs and, where oracle/_ref is built, against the reference g2o itself"""
    live = oracle_mod.RefG2O() if oracle_mod.RefG2O.available() else None
    for i, c in enumerate(CASES):
        prob = probs[c["name"]]
        o = oracle.local_ba(prob)
        check_result(o, stored(golden, i), f"{c['name']} vs fixture")
        if live is not None:
            check_result(o, live.local_ba(prob), f"{c['name']} vs live g2o")


# ------------------------------------------------------------------ HIP (GPU)
def run_case(ctx, prob):
    got = ctx.local_ba(prob)
    return got, ctx.local_ba_forms()


def check_forms(forms, c, prob):
    """both rounds report the intended solve and structure; nPf / nLa / Ea are those of the round-0 structure (all edges active)"""
    solve, struct = c["forms"]
    pf = np.unique(prob["e_pose"])
    n_pf = int((prob["fixed"][pf] == 0).sum())
    expect = [solve, struct, n_pf, len(np.unique(prob["e_point"])), len(prob["e_point"])]
    for r in range(2):
        assert list(forms[r]) == expect, f"{c['name']} round {r}: {list(forms[r])} != {expect} ({SOLVE[solve]})"


@pytest.fixture(scope="module")
def big_ctx(pkg):
    """the P > 1024 case runs on a context of its own, closed afterwards"""
    ctx = pkg.AsdHip(n_features=500, max_width=640, max_height=240, max_patches=1024)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_local_ba_path_matches_g2o_and_oracle(name, request, golden, probs, oracle):
    i, c = BY_NAME[name]
    prob = probs[name]
    ctx = request.getfixturevalue("big_ctx" if len(prob["poses"]) > 1024 else "hip")
    got, forms = run_case(ctx, prob)
    check_forms(forms, c, prob)
    exp = oracle.local_ba(prob)
    check_result(got, stored(golden, i), f"{name} vs g2o fixture")
    check_result(got, exp, f"{name} vs oracle")
    dp, dl = max_diffs(got, exp)
    print(f"{name}: {SOLVE[c['forms'][0]]} / {'host' if c['forms'][1] else 'device'} structure, nPf {forms[0][2]}: "
          f"HIP vs oracle max |d| poses {dp:.1e} points {dl:.1e}")
    again, forms2 = run_case(ctx, prob)
    np.testing.assert_array_equal(forms2, forms)
    for k in RESULT_KEYS:
        np.testing.assert_array_equal(again[k], got[k], err_msg=f"{name}: second run differs in {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["free31", "free32", "interleaved31", "masked_pose"])
def test_hip_local_ba_path_host_structure_equals_device(name, pkg, probs, hip, monkeypatch):
    """ASD_BA_STRUCT=host (read when the context is made) builds the same tables on the host: every output bit-identical"""
    prob = probs[name]
    monkeypatch.setenv("ASD_BA_STRUCT", "host")
    host = pkg.AsdHip(n_features=500, max_width=640, max_height=240, max_patches=1024)
    monkeypatch.delenv("ASD_BA_STRUCT")
    try:
        a, fa = run_case(hip, prob)
        b, fb = run_case(host, prob)
    finally:
        host.close()
    assert fa[0][1] == 0 and fb[0][1] == 1, (fa, fb)
    np.testing.assert_array_equal(fa[:, [0, 2, 3, 4]], fb[:, [0, 2, 3, 4]])
    for k in RESULT_KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{name}: {k}")


@pytest.mark.gpu
def test_hip_local_ba_lane_equals_inline_at_chol(hip, probs):
    """k_ba_chol (33 free poses) on the lane (asd_local_ba_submit / _wait) equals the in-line run bit for bit, forms included"""
    prob = probs["free33"]
    inline, fi = run_case(hip, prob)
    hip.local_ba_submit(prob)
    got = hip.local_ba_wait()
    fl = hip.local_ba_forms()
    assert fl[0][0] == 2
    np.testing.assert_array_equal(fl, fi)
    for k in RESULT_KEYS:
        np.testing.assert_array_equal(got[k], inline[k], err_msg=k)
