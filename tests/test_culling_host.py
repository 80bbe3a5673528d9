"""asd::LocalMapping::KeyFrameCulling and asd::LocalMapping::MapPointCulling (asd-slam_amd/host/asd_adapters.hpp) through
host/test_culling, against tests/culling_ref.py; and MapPointCulling's list rule alone (host/map_point_culling.hpp) through
host/test_map_point_culling, a program without device code that is also the one to build under AddressSanitizer / UBSan."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.culling_cases import problem_text, random_case
from tests.culling_ref import map_point_culling

HOST = os.path.join(ROOT, "asd-slam_amd", "host")
CSRC = os.path.join(ROOT, "asd-slam_amd", "csrc")


def _built(name):
    path = os.path.join(HOST, name)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", CSRC, f"../host/{name}"])
    return path


def _rule(records, observations, n_current):
    text = f"{len(records)}\n" + "".join(" ".join(str(int(x)) for x in (*r, o)) + "\n" for r, o in zip(records, observations))
    r = subprocess.run([_built("test_map_point_culling"), str(n_current)], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    return out["set_bad"], out["recent"]


# (row, mnFirstKFid, mnFound, mnVisible, isBad), Observations(); nCurrentKFid = 10
HAND = [((100, 9, 1, 1, 1), 9),      # isBad: leaves the list, no SetBadFlag
        ((101, 9, 24, 100, 0), 9),   # found ratio 0.24 < 0.25f: SetBadFlag
        ((102, 9, 1, 4, 0), 9),      # exactly 0.25 is not below: stays (one keyframe old)
        ((103, 8, 25, 100, 0), 2),   # exactly 0.25, two keyframes old, two observations: SetBadFlag
        ((104, 8, 1, 1, 0), 3),      # two keyframes old, three observations: stays
        ((105, 7, 1, 1, 0), 3),      # three keyframes old: leaves the list, no SetBadFlag
        ((106, 7, 1, 1, 0), 2),      # three keyframes old with two observations: the observation test comes first, SetBadFlag
        ((107, 10, 1, 1, 0), 0),     # added by this keyframe, no observation yet: stays
        ((108, 9, 0, 0, 0), 5)]      # never visible: 0 / 0 compares false, stays


def test_map_point_culling_rule_by_hand():
    records, obs = [r for r, _ in HAND], [o for _, o in HAND]
    assert map_point_culling(records, obs, 10) == ([1, 3, 6], [102, 104, 107, 108])
    assert _rule(records, obs, 10) == ([1, 3, 6], [102, 104, 107, 108])
    assert _rule([], [], 10) == ([], [])


def test_map_point_culling_rule_random():
    rng = np.random.default_rng(5)
    records = [(int(1000 + i), int(rng.integers(0, 12)), int(rng.integers(0, 9)), int(rng.integers(1, 33)), int(rng.uniform() < 0.1)) for i in range(400)]
    obs = [int(x) for x in rng.integers(0, 6, 400)]
    exp = map_point_culling(records, obs, 11)
    assert len(exp[0]) > 50 and len(exp[1]) > 20 and any(f * 4 == v for _, _, f, v, _ in records)
    assert _rule(records, obs, 11) == exp


@pytest.mark.gpu
def test_adapters_equal_the_restatement(tmp_path):
    m, cand = random_case(40, 48, 200, 1, 0.8)
    kfs = sorted(m.kf_points)
    rng = np.random.default_rng(6)
    calls = [(cand, [0] * len(cand), 0), (cand, [int(x) for x in rng.choice([0, 0, 1, 2], len(cand))], 0), (cand, [0] * len(cand), 1),
             (kfs, [0] * len(kfs), 1)]
    ref = m._copy()
    expected = [ref.keyframe_culling(c, f, a) for c, f, a in calls]
    assert len(expected[0]["bad_rows"]) > 0 and sum(d == 1 for d in expected[2]["decision"]) >= 2
    # the recent points: every branch of the rule over the map the culls left, Observations() from the table
    pts = list(range(0, 200))
    n_current = max(kfs) + 1
    records = []
    for i, p in enumerate(pts):
        found, visible = [(1, 4), (24, 100), (3, 4), (1, 1)][i % 4]
        records.append((p, n_current - (i // 4) % 4, found, visible, int(p in ref.pt_bad)))
    exp_points = map_point_culling(records, ref.observations(pts), n_current)
    by_rule = {i for i in exp_points[0] if records[i][2] * 4 >= records[i][3]}
    assert by_rule and len(by_rule) < len(exp_points[0]) and exp_points[1] and len(exp_points[0]) + len(exp_points[1]) < len(records)
    rows = pts + [250, 100000]
    path = tmp_path / "culling.txt"
    path.write_text(problem_text(m, calls, records, n_current, rows))
    r = subprocess.run([_built("test_culling"), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    for got, exp in zip(out["calls"], expected):
        assert got["rc"] == 0
        for k in ("decision", "n_mps", "n_redundant", "bad_rows"):
            assert got[k] == [int(x) for x in exp[k]], k
    assert out["points"]["rc"] == 0
    assert (out["points"]["set_bad"], out["points"]["recent"]) == exp_points
    assert out["observations"] == ref.observations(rows)
