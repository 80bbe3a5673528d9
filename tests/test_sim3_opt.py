"""asd_optimize_sim3 (csrc/sim3.hip) against the REFERENCE's own g2o: every case of tests/golden/make_sim3_golden.py is run on the
device and compared with the fixture's -O2 build.

The bar: every Sim3 component within 4 x S of g2o's (scale relative), where S is the largest distance between the two builds of
g2o over the case list, read from the fixture (tests/test_sim3_golden.py explains why the 1e-8 of the pose solvers cannot apply
here and checks S <= 2.5e-7); keep, n_in, nBad, the early return, the iteration cap chosen and the active edges of both rounds
identical.  Iteration counts are asserted for round one only, and only where the two builds of g2o agree with each other; round two
ends at the differencing noise floor (the builds themselves disagree there, e.g. clean_300), so its counts are printed, not asserted.

k_sim3_opt runs one workgroup of 256 threads (make_sim3_golden.WORKGROUP): n = 255 / 256 / 257 are the last partial pass, the full
pass and the first second pass of its edge loop, 63 / 64 / 65 the same for one wave.
"""
import json

import numpy as np
import pytest

from tests.golden.make_sim3_golden import CASES, GOLDEN, TH2, WORKGROUP, problem, rounds_of, sim3_distance

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: (i, c) for i, c in enumerate(CASES)}
ARGS = ("sim3", "P1c", "P2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "K1", "K2")


@pytest.fixture(scope="module")
def golden():
    G = np.load(GOLDEN)
    assert json.loads(str(G["cases"])) == json.loads(json.dumps(CASES)), "the fixture was made from another case list"
    return G


def run(hip, pp):
    S, keep, n_in = hip.optimize_sim3(*[pp[k] for k in ARGS], th2=float(pp["th2"]), fix_scale=int(pp["fix_scale"]))
    return S, keep, n_in, hip.debug_optimize_sim3()


@pytest.mark.parametrize("name", NAMES)
def test_hip_optimize_sim3_matches_g2o(hip, golden, name):
    i, c = BY_NAME[name]
    pp = problem(c)
    tol = 4 * float(golden["S"])
    assert tol <= 1e-6
    S, keep, n_in, dbg = run(hip, pp)
    ref = {k: golden[f"c{i}_a_{k}"] for k in ("sim3", "keep", "info", "trials")}
    info, info_b = ref["info"], golden[f"c{i}_b_info"]
    g_rounds, g_rounds_b = rounds_of(info, ref["trials"]), rounds_of(info_b, golden[f"c{i}_b_trials"])
    dist = sim3_distance(S, ref["sim3"])
    print(f"{name}: |device - g2o| {dist.max():.2e} (tol {tol:.2e}) n_in {n_in} nBad {dbg['n_bad']} cap {dbg['cap']} early {dbg['early']} | device rounds "
          f"{[(r['iterations'], r['trials'], r['ends_rejected']) for r in dbg['rounds']]} | g2o iterations {[r['ret'] for r in g_rounds]} / {[r['ret'] for r in g_rounds_b]} "
          f"trials {[r['trials'] for r in g_rounds]}")
    assert np.array_equal(keep, ref["keep"])
    assert n_in == int(golden[f"c{i}_a_n_in"])
    assert dbg["n"] == c["n"] and dbg["n_bad"] == int(info[0]) and dbg["early"] == int(info[1])
    assert dbg["cap"] == (10 if info[0] > 0 else 5)
    assert [r["active"] for r in dbg["rounds"]] == [r["active"] for r in g_rounds]
    if g_rounds[0]["ret"] == g_rounds_b[0]["ret"]:
        assert dbg["rounds"][0]["iterations"] == g_rounds[0]["ret"]
    if len(dbg["rounds"]) == 2:
        assert 1 <= dbg["rounds"][1]["iterations"] <= dbg["cap"]
    assert (dist <= tol).all(), dist
    if dbg["early"]:
        assert np.array_equal(S.view(np.uint64), pp["sim3"].view(np.uint64)), "the early return must not write the Sim3"
        assert n_in == 0
    if c["fix_scale"]:   # g2o keeps a fixed scale bit-identical (tests/test_sim3_golden.py), and so does the device
        assert S[7] == pp["sim3"][7]


def test_hip_optimize_sim3_is_one_bit_pattern(hip):
    """20 repeated calls: fixed reduction shapes, no atomics"""
    for name in ("n65", "n257_fix", "hard_40"):
        pp = problem(BY_NAME[name][1])
        seen = set()
        for _ in range(20):
            S, keep, n_in, dbg = run(hip, pp)
            seen.add((S.tobytes(), keep.tobytes(), n_in, json.dumps(dbg)))
        assert len(seen) == 1, name


def test_hip_optimize_sim3_empty_and_aid(hip):
    """n == 0: ASD_OK, n_in 0, the Sim3 untouched; the aid reports an empty first round and the early return"""
    pp = problem(BY_NAME["n0"][1])
    S, keep, n_in, dbg = run(hip, pp)
    assert n_in == 0 and len(keep) == 0 and np.array_equal(S.view(np.uint64), pp["sim3"].view(np.uint64))
    assert dbg == dict(rounds=[dict(active=0, iterations=-1, trials=0, ends_rejected=0)], n_bad=0, cap=5, early=1, n=0)
    assert TH2 == 10.0 and WORKGROUP == 256
