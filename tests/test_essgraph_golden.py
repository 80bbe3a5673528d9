"""tests/golden/essgraph_golden.npz -- what the REFERENCE's own vendored g2o returns for Optimizer::OptimizeEssentialGraph
(Optimizer.cc:737-1000) on the problems of tests/golden/make_essgraph_golden.py -- is the fixture of the case list in this tree, its
runs show the paths the cases name, its edge lists are those the rules of :808-939 give, and S (the distance between three reference
runs) is within the cap.  No GPU: tests/test_essgraph.py holds the device to the fixture."""
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.golden.make_essgraph_golden import (CASES, DROPPED, FULL, PATHS, S_CAP, S_NAMES, STORED, TILE, edges_of, problem, problem_digest,
                                               trials_of)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "essgraph_golden.npz"))


def stored(G, i):
    o = {k: G[f"c{i}_{k}"] for k in STORED}
    o["chi2"] = float(G[f"c{i}_chi2"])
    return o


def test_essgraph_golden_is_of_this_case_list(golden, synth):
    assert json.loads(str(golden["cases"])) == json.loads(json.dumps(CASES)), "the fixture was made from another case list"
    assert int(golden["tile"]) == TILE and json.loads(str(golden["s_names"])) == list(S_NAMES)
    for i, c in enumerate(CASES):
        assert problem_digest(problem(c, synth)) == str(golden[f"c{i}_in_sha256"]), f"{c['name']}: the generator no longer makes the stored problem"


def test_essgraph_golden_shows_the_named_paths(golden, synth):
    for i, c in enumerate(CASES):
        o, pp = stored(golden, i), problem(c, synth)
        for path in c["paths"]:
            assert PATHS[path](o, pp), f"{c['name']}: the stored run does not show {path}"
        assert int(o["info"][2]) == sum(trials_of(o)) and int(o["info"][3]) == len(o["e_i"])
        assert [(a, b) for a, b, _ in edges_of(pp)[0]] == list(zip(o["e_i"].tolist(), o["e_j"].tolist())), c["name"]
    assert sum(c["its"] == FULL for c in CASES) >= 3
    names = {c["name"] for c in CASES}
    assert {"chain_3", "loop_8", "loop_8_fix_scale", "drift_far", "dup_pair", "lone_kf", "its0", "no_edges", "fixed_mid", "tile_13", "tile_14",
            "tile_28", "covis_40"} <= names | {d[0] for d in DROPPED}


def test_essgraph_golden_tolerance(golden):
    S = golden["S"]
    assert S.shape == (6,) and (S > 0).all()
    assert S.max() <= S_CAP and 4 * S.max() <= 1e-6, S


def test_essgraph_golden_dropped(golden):
    assert len(DROPPED) <= 2
    assert json.loads(str(golden["dropped"])) == json.loads(json.dumps(DROPPED))
