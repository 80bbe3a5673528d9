"""asd::Sim3Solver and the RANSAC rounds of asd::LoopClosing::ComputeSim3 (asd-slam_amd/host/asd_adapters.hpp) through
host/test_sim3_solver, against a Python loop over single sim3_ransac calls that consumes the same raw rand() values with the reference's
sequential semantics (LoopClosing.cc:322-377: candidate by candidate, 5 iterations each, rand() called as the iterations run)."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import sim3solver_ref as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

PROBE = os.path.join(ROOT, "asd-slam_amd", "host", "test_sim3_solver")
# raw streams (seeds of the test's own generator) chosen with the reference alone so that, with the first model rejected: 3 -- candidate 0
# returns in round one, is rejected, and candidate 1 iterates in the same round on the numbers handed back; 10 -- candidate 1 returns first,
# candidate 0 in the next round with candidate 1 drawn for behind it
RAW_SEEDS, N_RAW, N_REJECT = (3, 10), 600, 1


def candidates():
    """two candidates: 60 correspondences of which 45 % follow the planted Sim3, and 80 of which 60 % do; the keypoint index of
    correspondence i (mvnIndices1) is a seeded increasing map into twice as many keypoints"""
    out = []
    for ci, (n, frac, fix) in enumerate([(60, 0.45, 0), (80, 0.6, 0)]):
        rng = np.random.default_rng(500 + ci)
        X1c, X2c, planted, _ = R._planted(rng, n, 1.05, frac, 0.2, R.K_KITTI, R.K_KITTI)
        idx1 = np.sort(rng.permutation(2 * n)[:n])
        sig = np.array([1.2 ** (2 * l) for l in range(8)])
        e1 = np.floor(9.210 * sig[rng.integers(0, 8, n)]).astype(np.float32)      # what vector<size_t> mvnMaxError1 holds
        e2 = np.floor(9.210 * sig[rng.integers(0, 8, n)]).astype(np.float32)
        out.append(dict(N1=2 * n, n=n, fix_scale=fix, min_inliers=20, max_its_arg=300, K1=R.K_KITTI, K2=R.K_KITTI, idx1=idx1, X1c=X1c, X2c=X2c,
                        max_err1=e1, max_err2=e2, planted=planted))
    return out


def raw_values(seed):
    return [int(v) for v in np.random.default_rng(seed).integers(0, 2 ** 31, N_RAW)]


def write_problem_file(path, cands, raw, n_reject):
    hx = lambda a: " ".join(float(x).hex() for x in np.asarray(a, np.float32).reshape(-1))
    with open(path, "w") as f:
        f.write(f"{len(raw)}\n" + " ".join(map(str, raw)) + f"\n{n_reject} {len(cands)}\n")
        for c in cands:
            f.write(f"{c['N1']} {c['n']} {c['fix_scale']} {c['min_inliers']} {c['max_its_arg']}\n")
            f.write(" ".join(repr(float(k)) for k in list(c["K1"]) + list(c["K2"])) + "\n")
            f.write(" ".join(str(int(i)) for i in c["idx1"]) + "\n")
            for k in ("X1c", "X2c", "max_err1", "max_err2"):
                f.write(hx(c[k]) + "\n")


class Stream:
    def __init__(self, raw):
        self.raw, self.at = raw, 0


def iterate(solve, c, st, stream, n_iterations=5):
    """Sim3Solver::iterate(nIterations) of candidate c (state st) as one single-problem call: the draws are the next raw values, and
    only those of the iterations that ran are consumed"""
    if c["n"] < c["min_inliers"]:
        return dict(model=0, no_more=1, res=None, raw=[])
    n_iter = max(0, min(n_iterations, st["max_its"] - st["iterations"]))
    raw = stream.raw[stream.at:stream.at + 3 * n_iter]
    assert len(raw) == 3 * n_iter, "the raw stream of the test is too short"
    draws = np.array([R.random_int(r, 0, c["n"] - 1 - (k % 3)) for k, r in enumerate(raw)], np.int32).reshape(n_iter, 3)
    res = solve(dict(c, n_iter=n_iter, draws=draws, best_inliers=st["best"]))
    used = 3 * res["iterations_done"]
    stream.at += used
    st["iterations"] += res["iterations_done"]
    st["best"] = res["best_inliers"]
    if res["best_updated"]:
        st["model"] = (res["R12"].copy(), res["t12"].copy(), np.float32(res["s12"]))
    no_more = int(not res["found"] and st["iterations"] >= st["max_its"])
    return dict(model=res["found"], no_more=no_more, res=res, raw=raw[:used])


def new_state(c):
    return dict(iterations=0, best=0, model=None, max_its=R.max_iterations(c["n"], 0.99, c["min_inliers"], c["max_its_arg"]))


def run_single(solve, c, raw):
    stream, st, calls = Stream(raw), new_state(c), []
    while True:
        r = iterate(solve, c, st, stream)
        calls.append((r, dict(st)))
        if r["model"] or r["no_more"]:
            return calls


def run_multi(solve, cands, raw, n_reject):
    stream = Stream(raw)
    states = [new_state(c) for c in cands]
    discarded = [False] * len(cands)
    hits, accepted, rounds = [], -1, 0
    while not all(discarded) and accepted < 0:
        rounds += 1
        for i, c in enumerate(cands):
            if discarded[i]:
                continue
            r = iterate(solve, c, states[i], stream)
            if r["no_more"]:
                discarded[i] = True
            if r["model"]:
                hits.append((i, rounds, r, dict(states[i])))
                if len(hits) > n_reject:
                    accepted = i
                    break
    return dict(hits=hits, accepted=accepted, rounds=rounds, states=states, discarded=discarded, at=stream.at)


def same_call(js, r, st, c):
    """one printed call of the probe against one iterate() of the Python loop"""
    assert js["model"] == r["model"] and js["no_more"] == r["no_more"]
    assert js["iterations"] == st["iterations"] and js["best_inliers"] == st["best"]
    assert js["raw"] == r["raw"]
    res = r["res"]
    exp_inl = [int(c["idx1"][i]) for i in np.nonzero(res["inliers"])[0]] if res["found"] else []
    assert js["inliers"] == exp_inl and js["n_inliers"] == (res["n_inliers"] if res["found"] else 0)
    if st["model"] is not None:
        Rm, t, s = st["model"]
        assert [float.fromhex(x) for x in js["R"]] == [float(x) for x in Rm.reshape(-1)]
        assert [float.fromhex(x) for x in js["t"]] == [float(x) for x in t] and float.fromhex(js["s"]) == float(s)


@pytest.fixture(scope="module", params=RAW_SEEDS)
def probe_output(request, tmp_path_factory):
    if not os.path.exists(PROBE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "asd-slam_amd", "csrc"), "../host/test_sim3_solver"])
    path = tmp_path_factory.mktemp("sim3") / "problem.txt"
    write_problem_file(path, candidates(), raw_values(request.param), N_REJECT)
    r = subprocess.run([PROBE, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return request.param, json.loads(r.stdout)


def test_single_solver_iterates_like_single_calls(hip, probe_output):
    solve = lambda p: hip.sim3_ransac([p])[0]
    seed, out = probe_output
    for ci, c in enumerate(candidates()):
        js = out["single"][ci]
        calls = run_single(solve, c, raw_values(seed))
        assert js["max_its"] == calls[0][1]["max_its"] and js["ran_out"] == 0
        assert len(js["calls"]) == len(calls)
        for a, (r, st) in zip(js["calls"], calls):
            same_call(a, r, st, c)
        assert calls[-1][0]["model"] == 1, "both candidates have a model to find"


def test_multi_candidate_rounds_are_the_sequential_loop(hip, probe_output):
    solve = lambda p: hip.sim3_ransac([p])[0]
    cands = candidates()
    seed, out = probe_output
    exp = run_multi(solve, cands, raw_values(seed), N_REJECT)
    js = out["multi"]
    assert js["ran_out"] == 0
    assert js["accepted"] == exp["accepted"] >= 0 and js["rounds"] == exp["rounds"]
    assert len(js["hits"]) == len(exp["hits"]) == N_REJECT + 1
    for a, (i, rnd, r, st) in zip(js["hits"], exp["hits"]):
        assert a["candidate"] == i and a["round"] == rnd
        same_call(a["call"], r, st, cands[i])
    assert js["iterations"] == [s["iterations"] for s in exp["states"]]
    assert js["best_inliers"] == [s["best"] for s in exp["states"]]
    assert js["discarded"] == [int(d) for d in exp["discarded"]]
    assert js["source_at"] - js["pending"] == exp["at"], "the raw values consumed are exactly the reference's"
    # the scenario this test is about: candidate 0 returned a model in a round in which candidate 1 was live behind it, so the batched
    # round had drawn for candidate 1 and had to hand those numbers back and leave its state alone
    assert any(i == 0 and not exp["discarded"][1] for i, _rnd, _r, _st in exp["hits"])
    assert js["pending"] > 0
