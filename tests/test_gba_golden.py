"""tests/golden/gba_golden.npz -- what the REFERENCE's own vendored g2o returns for Optimizer::BundleAdjustment (Optimizer.cc:51-237)
on the problems of tests/golden/make_gba_golden.py -- is the fixture of the case list in this tree, its runs show the paths the
cases name, and the tolerance it carries (4 x S, S = the distance between three reference runs) is within the suite's loosest BA
tolerance.  No GPU: tests/test_gba.py holds the device to the fixture."""
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.golden.make_gba_golden import CASES, DELTA2, DROPPED, HUBER_MARGIN, PATHS, T, TOL_CAP, problem, problem_digest, trials_of


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "gba_golden.npz"))


def stored(G, i):
    return dict(poses=G[f"c{i}_poses"], points=G[f"c{i}_points"], edge_chi2=G[f"c{i}_edge_chi2"], info=G[f"c{i}_info"],
                trials=G[f"c{i}_trials"], chi2=float(G[f"c{i}_chi2"]))


def test_gba_golden_is_of_this_case_list(golden, synth):
    assert json.loads(str(golden["cases"])) == json.loads(json.dumps(CASES)), "the fixture was made from another case list"
    assert int(golden["tile_poses"]) == T
    for i, c in enumerate(CASES):
        assert problem_digest(problem(c, synth)) == str(golden[f"c{i}_in_sha256"]), f"{c['name']}: the generator no longer makes the stored problem"


def test_gba_golden_shows_the_named_paths(golden, synth):
    for i, c in enumerate(CASES):
        o, pp = stored(golden, i), problem(c, synth)
        for path in c["paths"]:
            assert PATHS[path](o, pp), f"{c['name']}: the stored run does not show {path}"
        assert int(o["info"][2]) == sum(trials_of(o))
    names = [c["name"] for c in CASES]
    for free in (T - 1, T, T + 1, 2 * T + 1, 3 * T + 5):
        pp = problem(CASES[names.index(f"band_{free}")], synth)
        assert int((pp["fixed"] == 0).sum()) == free
    o = stored(golden, names.index("outliers"))
    assert float(np.abs(o["edge_chi2"] / DELTA2 - 1).min()) >= HUBER_MARGIN


def test_gba_golden_tolerance(golden):
    S = golden["S"]
    assert S.shape == (5,) and (S > 0).all()
    assert 4 * S.max() <= TOL_CAP, S


def test_gba_golden_dropped(golden):
    assert len(DROPPED) <= 2
    assert json.loads(str(golden["dropped"])) == json.loads(json.dumps(DROPPED))
