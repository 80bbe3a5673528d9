#!/usr/bin/env python3
"""Generate tests/golden/ba_lm_golden.npz: what the REFERENCE's own vendored g2o (compiled in place by oracle/ref_g2o/Makefile,
output in oracle/_ref/, never committed) returns on LocalBA problems shaped to take the Levenberg control's exits
(optimization_algorithm_levenberg.cpp:61-147, sparse_optimizer.cpp:354-419) -- tests/test_local_ba_lm.py:
  - a round that ends on Raul's rule (three iterations in a row with a relative gain below 1e-3) before its iteration count,
    with the active structure built on the device (<= 32 free poses) and on the host (>= 33);
  - a second round with every edge gated out: optimize() finds no active vertex and returns -1 before its first iteration;
  - its_first / its_second other than 5 / 10: (1, 2), (0, 10), (5, 20) -- (5, 20) ends on Raul's rule after 3 iterations;
  - full rounds of 5 and 10 iterations.

Runs only in the build container.  Each problem is synth.ba_problem(**kw) followed by the explicit post-edit of problem() below,
which the tests share.  The fixture stores the case list, a digest of every problem's inputs, g2o's outputs, the trial counts and
the Levenberg trace of each round (oracle/ref_g2o/driver.cpp: per iteration the trials, lambda and activeRobustChi2; the chi2
after every computeActiveErrors), and the edge chi2 the gating between the rounds read (a second g2o run with its_second = 0:
optimize(0) computes no error, so they are the first round's last).  edge_chi2 and gate_chi2 are stored as float32, like
ba_paths_golden.npz: the tests compare them at rtol 1e-6 and use them for the distance from the 5.991 gate.

The generator asserts from g2o's own trace that each case takes its intended exit (replay() restates the control from the chi2
sequence).  It also runs two bounded, seeded searches and records what they found under "search":
  - for a first round that ends on Raul's rule (iters_first < 5): low-noise problems started at the ground truth;
  - for a rejected trial: free poses moved or turned, depths scaled, gross outliers, points pushed towards the cameras.
Neither search has found one: the first round's Huber-weighted iterations keep gaining more than 1e-3, and every LocalBA
trial's Gauss-Newton step with lambda = 1e-5 max(diag H) lowered the cost.  PoseOptimization's goldens (ba_golden.npz) do
reject trials; the rejection branch of the device control is shared with it only in its statement, so it stays unpinned here.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402
from tests.golden.make_live_golden import problem_digest  # noqa: E402

OUT_KEYS = ("poses", "points", "edge_outlier1", "edge_depth_pos", "edge_chi2", "chi2_first", "chi2_second", "iters_first",
            "iters_second", "trials_first", "trials_second")

NBAD = dict(n_free=5, n_fixed=3, n_points=300, seed=3, pose_sigma=0.002, point_sigma=0.002, pix_noise=0.3, outlier_frac=0.0)
# name, synth.ba_problem kwargs, post-edit, (its_first, its_second), intended exit per round:
#   "its" = the iteration count ran out, "nbad" = Raul's rule, "none" = no active vertex (-1), "zero" = no iteration asked for
CASES = [
    dict(name="nbad_r2", kw=NBAD, edit=None, its=(5, 10), exits=("its", "nbad")),
    dict(name="nbad_r2_truth", kw=dict(NBAD, seed=4, pose_sigma=0.0, point_sigma=0.0), edit=None, its=(5, 10), exits=("its", "nbad")),
    # 33 free poses: the host-built structure and k_ba_chol
    dict(name="nbad_r2_host", kw=dict(n_free=33, n_fixed=33, n_points=1000, obs_per_point=10, seed=3, pose_sigma=0.002,
                                      point_sigma=0.002, pix_noise=0.3, outlier_frac=0.0), edit=None, its=(5, 10), exits=("its", "nbad")),
    dict(name="full", kw=dict(n_free=5, n_fixed=3, n_points=300, seed=5), edit=None, its=(5, 10), exits=("its", "its")),
    # every point 20x closer to the origin: all observations gross outliers after round 1
    dict(name="gated_all", kw=dict(n_free=5, n_fixed=2, n_points=300, seed=11), edit="shrink", its=(5, 10), exits=("its", "none")),
    dict(name="gated_all_its0", kw=dict(n_free=5, n_fixed=2, n_points=300, seed=11), edit="shrink", its=(5, 0), exits=("its", "none")),
    dict(name="gated_all_sparse", kw=dict(n_free=3, n_fixed=1, n_points=60, obs_per_point=2, seed=9, pose_sigma=0.5, point_sigma=8.0),
         edit=None, its=(5, 10), exits=("its", "none")),
    dict(name="its_1_2", kw=NBAD, edit=None, its=(1, 2), exits=("its", "its")),
    dict(name="its_0_10", kw=NBAD, edit=None, its=(0, 10), exits=("zero", "its")),
    dict(name="its_5_20", kw=NBAD, edit=None, its=(5, 20), exits=("its", "nbad")),
]


def problem(case, synth):
    """synth.ba_problem(**kw) and the case's post-edit"""
    prob = synth.ba_problem(**case["kw"])
    if case["edit"] == "shrink":
        prob["points"] = prob["points"] * 0.05
    else:
        assert case["edit"] is None, case["edit"]
    return prob


def replay(iters, calls):
    """Levenberg control of one round (levenberg.cpp:95-147) restated from g2o's trace.  Returns per iteration (ini chi2, [chi2 of
    each trial], [accepted?], chi2 at its end, the exit it took or None).  A trial is accepted when it lowered the chi2 (rho > 0:
    the gain ratio's denominator x^T (lambda x + b) + 1e-3 is positive for the damped Gauss-Newton step)."""
    chis = list(calls[1:]) + ([float(iters[-1][2])] if len(iters) else [])
    out, j, nbad = [], 0, 0
    for n_tr, _lam, _chi in iters:
        n_tr = int(n_tr)
        ini = cur = chis[j]
        temps = chis[j + 1:j + 1 + n_tr]
        j += 1 + n_tr
        acc = []
        for t in temps:
            acc.append(t < cur)
            if t < cur:
                cur = t
        assert acc.count(True) <= 1 and (acc[-1] or n_tr == 10), "a trial after an accepted one"
        exit_ = None
        if n_tr == 10 and not acc[-1]:
            exit_ = "trials"
        else:
            nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
            if nbad >= 3:
                exit_ = "nbad"
        out.append(dict(ini=ini, temps=temps, acc=acc, cur=cur, exit=exit_))
    assert j == len(chis), (j, len(chis))
    return out


def round_exit(n_done, its, rep):
    if n_done == -1:
        return "none"
    if its == 0:
        return "zero"
    assert n_done == len(rep)
    if rep and rep[-1]["exit"] is not None:
        return rep[-1]["exit"]
    assert n_done == its, (n_done, its)
    return "its"


def run(ref, prob, its):
    res = ref.local_ba(prob, *its)
    gate = ref.local_ba(prob, its[0], 0)["edge_chi2"]   # the errors the gating read: optimize(0) computes none
    return res, gate


def search(ref, synth):
    """the two bounded searches; returns what they tried and found"""
    found_nbad, found_rej, tried_nbad, tried_rej = [], [], 0, 0
    for seed in range(300, 306):
        for pn in (0.02, 0.1, 0.3):
            kw = dict(n_free=4, n_fixed=2, n_points=200, seed=seed, pose_sigma=0.0, point_sigma=0.0, pix_noise=pn, outlier_frac=0.0)
            r = ref.local_ba(synth.ba_problem(**kw))
            tried_nbad += 1
            if r["iters_first"] < 5:
                found_nbad.append(kw)
    rng = np.random.default_rng(7)
    for seed in range(400, 412):
        for family in ("move", "turn", "depth", "outliers", "near"):
            prob = synth.ba_problem(n_free=5, n_fixed=3, n_points=300, seed=seed, outlier_frac=0.3 if family == "outliers" else 0.02)
            free = np.flatnonzero(prob["fixed"] == 0)
            p = int(free[rng.integers(len(free))])
            if family == "move":
                prob["poses"][p, 4:] += rng.uniform(-3, 3, 3)
            elif family == "turn":
                ang = rng.uniform(0.2, 0.5) * 0.5
                axis = rng.standard_normal(3)
                axis /= np.linalg.norm(axis)
                q = np.r_[axis * np.sin(ang), np.cos(ang)]   # small rotation composed on the left (x, y, z, w)
                a, b = q, prob["poses"][p, :4]
                prob["poses"][p, :4] = [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                                        a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0],
                                        a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3],
                                        a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]
            elif family == "depth":
                prob["points"] *= rng.uniform(0.3, 3.0, (len(prob["points"]), 1))
            elif family == "near":
                prob["points"][:, 2] *= rng.uniform(0.05, 0.3)
            r = ref.local_ba(prob)
            tried_rej += 1
            rep = [replay(t["iters"], t["calls"]) for t in r["lm_trace"] if len(t["iters"])]
            if any(not all(it["acc"]) for rr in rep for it in rr):
                found_rej.append(dict(seed=seed, family=family))
    return dict(round1_nbad=dict(tried=tried_nbad, found=found_nbad), rejected_trial=dict(tried=tried_rej, found=found_rej))


def main():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "oracle", "ref_g2o")])
    synth = g.load_package().synth
    ref = g.load_oracle().RefG2O()
    assert ref.abi >= 2, "oracle/_ref/libg2o_ref.so predates the traced driver: rebuild it (__graft_entry__.build())"
    out = {"cases": np.array(json.dumps(CASES))}
    for i, case in enumerate(CASES):
        prob = problem(case, synth)
        res, gate = run(ref, prob, case["its"])
        again, _ = run(ref, prob, case["its"])
        for k in OUT_KEYS:
            assert np.array_equal(np.asarray(res[k]), np.asarray(again[k])), f"{case['name']}: g2o is not deterministic in {k}"
        out[f"c{i}_in_sha256"] = np.array(problem_digest(prob))
        for k in OUT_KEYS:
            v = np.asarray(res[k])
            out[f"c{i}_out_{k}"] = v.astype(np.float32) if k == "edge_chi2" else v
        out[f"c{i}_gate_chi2"] = gate.astype(np.float32)
        exits = []
        for r in range(2):
            t = res["lm_trace"][r]
            out[f"c{i}_r{r}_iters"] = t["iters"]
            out[f"c{i}_r{r}_calls"] = t["calls"]
            n_done = int(res["iters_first" if r == 0 else "iters_second"])
            exits.append(round_exit(n_done, case["its"][r], replay(t["iters"], t["calls"])))
        assert tuple(exits) == tuple(case["exits"]), f"{case['name']}: g2o took {exits}, not {case['exits']}"
        print(case["name"], "P", len(prob["poses"]), "E", len(prob["e_point"]), "iters", res["iters_first"], res["iters_second"],
              "trials", res["trials_first"], res["trials_second"], "exits", exits, "outliers", int(res["edge_outlier1"].sum()))
    found = search(ref, synth)
    print("search:", json.dumps(found))
    out["search"] = np.array(json.dumps(found))
    path = os.path.join(ROOT, "tests", "golden", "ba_lm_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
