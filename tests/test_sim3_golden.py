"""The fixture of asd_optimize_sim3 (tests/golden/sim3_golden.npz): what the REFERENCE's own g2o returns for Optimizer::OptimizeSim3
(Optimizer.cc:1002-1194) on the case list of tests/golden/make_sim3_golden.py, from two builds of it (-O2, and -O2 -mfma
-ffp-contract=fast).  These tests need no GPU: they check that the fixture belongs to this case list and these inputs, that its
admission rules hold, that g2o's own outputs show every path a case names, and that the Python binding has the new entry points.
tests/test_sim3_opt.py runs the device against it.

Why two builds: OptimizeSim3's edges have no analytic Jacobian, g2o differentiates them numerically with delta = 1e-9, and the second
round ends where that differencing noise decides the accept / reject tests.  Two roundings of the same program then differ by up to S
(stored in the fixture, about 1e-7; capped at 2.5e-7) per Sim3 component, so the device is held to 4 x S against the -O2 build: a
third rounding pattern (tree sums, device exp / sin / cos), and one pair of samples underestimates a noise range.

The stale-errors path (the re-classification reads chi2() without computeError(), so after a round that ended on a rejected trial
it reads the rejected trial's errors) is implemented by the kernel but NOT claimed by the fixture: a round ends on a rejected trial
only through ten rejections in a row, by then the damping has grown by 2^45, and in every run of g2o tried (this list and some six
hundred seeded variants) the rejected estimate was bit for bit the estimate it was popped back to.  The driver reports the flag
(info[4], info[7]); it is 0 everywhere.
"""
import json

import numpy as np
import pytest

from tests.golden.make_sim3_golden import (BUILDS, CASES, DROPPED, GATE_MARGIN, GOLDEN, PATHS, S_CAP, TH2, WORKGROUP, problem, problem_digest,
                                           rounds_of, sim3_distance)

BY_NAME = {c["name"]: (i, c) for i, c in enumerate(CASES)}


@pytest.fixture(scope="module")
def golden():
    G = np.load(GOLDEN)
    assert json.loads(str(G["cases"])) == json.loads(json.dumps(CASES)), "the fixture was made from another case list"
    return G


def out_of(G, i, tag):
    return dict(sim3=G[f"c{i}_{tag}_sim3"], keep=G[f"c{i}_{tag}_keep"], info=G[f"c{i}_{tag}_info"], trials=G[f"c{i}_{tag}_trials"],
                n_in=int(G[f"c{i}_{tag}_n_in"]), margin=float(G[f"c{i}_{tag}_margin"]))


def test_sim3_fixture_inputs_match_generator(golden):
    assert json.loads(str(golden["builds"])) == json.loads(json.dumps(BUILDS))
    assert json.loads(str(golden["dropped"])) == json.loads(json.dumps(DROPPED)) and len(DROPPED) <= 2
    for i, c in enumerate(CASES):
        pp = problem(c)
        assert problem_digest(pp) == str(golden[f"c{i}_in_sha256"]), f"{c['name']}: the generator no longer makes the stored problem"
        # what the entry point's comment promises of its inputs: points, observations, information values, calibration f32-representable
        for k in ("P1c", "P2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "K1", "K2"):
            assert np.array_equal(pp[k].astype(np.float32).astype(np.float64), pp[k]), (c["name"], k)
        assert float(pp["th2"]) == TH2


def test_sim3_case_list_covers_the_issue():
    n_of = {c["name"]: c["n"] for c in CASES}
    for n in (0, 9, 10, 11, 63, 64, 65, WORKGROUP - 1, WORKGROUP, WORKGROUP + 1, 600, 2000):
        assert any(c["n"] == n and not c["fix_scale"] for c in CASES), n
    assert max(n_of.values()) == 2000
    assert len({c["n"] for c in CASES if c["fix_scale"]}) >= 4, "fix_scale at several sizes"
    assert {"early", "no_drop"} <= set(BY_NAME["n9"][1]["paths"])
    assert "round2" in BY_NAME["n10"][1]["paths"] and "round2" in BY_NAME["n11"][1]["paths"]
    c = BY_NAME["drop_to_9"][1]
    assert c["n"] >= 10 and {"early", "drop"} <= set(c["paths"])
    assert {"early", "all_dropped"} <= set(BY_NAME["all_outliers"][1]["paths"])
    assert "rejected_r1" in BY_NAME["far_start"][1]["paths"] and BY_NAME["far_start"][1]["start_sigma"] >= 0.3
    assert sum("near_gate" in c["paths"] for c in CASES) >= 2
    assert any("cap5" in c["paths"] for c in CASES) and any("cap10" in c["paths"] for c in CASES) and any("its_gt5" in c["paths"] for c in CASES)
    pp = problem(BY_NAME["K1_ne_K2"][1])
    assert not np.array_equal(pp["K1"], pp["K2"])
    pp = problem(BY_NAME["n600"][1])
    assert len(np.unique(pp["inv_sigma2_1"])) == 8 and len(np.unique(pp["inv_sigma2_2"])) == 8


def test_sim3_behind_case_has_points_behind_camera_1():
    """the three edited points map to z < 0 (not 0) in camera 1 at the start estimate; the reference has no depth test here"""
    from tests.golden.make_sim3_golden import sim3_map
    pp = problem(BY_NAME["behind_100"][1])
    z = np.array([sim3_map(pp["sim3"], x)[2] for x in pp["P2c"][:5]])
    assert (z[:3] < -1.0).all() and (z[3:] > 1.0).all()


def test_sim3_fixture_admission_rules(golden):
    """no chi2 that a re-classification read lies within GATE_MARGIN of th2, in either build; the builds agree on every discrete output;
    S is the largest two-build distance and respects the cap"""
    S = np.zeros(8)
    for i, c in enumerate(CASES):
        a, b = out_of(golden, i, "a"), out_of(golden, i, "b")
        assert a["margin"] >= GATE_MARGIN and b["margin"] >= GATE_MARGIN, c["name"]
        assert np.array_equal(a["keep"], b["keep"]) and a["n_in"] == b["n_in"], c["name"]
        assert a["info"][0] == b["info"][0] and a["info"][1] == b["info"][1], c["name"]      # nBad, early return
        assert a["info"][2] == b["info"][2] and a["info"][5] == b["info"][5], c["name"]      # active edges per round
        S = np.maximum(S, sim3_distance(b["sim3"], a["sim3"]))
    assert float(golden["S"]) == S.max() and np.array_equal(golden["S_comp"], S)
    assert 0 < S.max() <= S_CAP
    assert 4 * S.max() <= 1e-6


def test_sim3_golden_takes_the_named_paths(golden):
    for i, c in enumerate(CASES):
        for tag in ("a", "b"):
            o = out_of(golden, i, tag)
            for path in c["paths"]:
                assert PATHS[path](o, c["n"]), f"{c['name']} ({tag}): g2o's run does not show {path}"
            rounds = rounds_of(o["info"], o["trials"])
            for r in rounds:   # optimize() returns its iteration count, -1 on the empty graph
                assert r["ret"] == (len(r["trials"]) if r["active"] else -1), c["name"]
                assert r["ends_rejected"] == 0, c["name"]   # see the module docstring
            assert rounds[0]["active"] == 2 * c["n"]
            if len(rounds) == 2:
                assert rounds[1]["active"] == 2 * (c["n"] - int(o["info"][0])) and rounds[1]["active"] >= 20
                assert o["n_in"] == int(o["keep"].sum())
            else:   # early return: keep carries round one's drops, the Sim3 is not written
                assert o["n_in"] == 0 and int(o["keep"].sum()) == c["n"] - int(o["info"][0]) < 10
                assert np.array_equal(o["sim3"], problem(c)["sim3"]), c["name"]


def test_sim3_golden_keeps_a_fixed_scale_bit_identical(golden):
    """g2o's oplusImpl zeroes update[6] under _fix_scale, exp(0) == 1 and s * 1 == s: the scale never changes by a bit"""
    for i, c in enumerate(CASES):
        if c["fix_scale"]:
            for tag in ("a", "b"):
                assert golden[f"c{i}_{tag}_sim3"][7] == problem(c)["sim3"][7], c["name"]


def test_capi_has_the_loop_closing_entry_points(pkg):
    for name in ("optimize_sim3", "debug_optimize_sim3", "match_bow_kf"):
        assert callable(getattr(pkg.AsdHip, name, None)), name
