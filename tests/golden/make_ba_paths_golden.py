#!/usr/bin/env python3
"""Generate tests/golden/ba_paths_golden.npz: what the REFERENCE's own vendored g2o (compiled in place by oracle/ref_g2o/Makefile,
output in oracle/_ref/, never committed) returns on LocalBA problems shaped to take every form asd_local_ba picks from the
problem's shape (tests/test_local_ba_paths.py):
  - the dense solve of the reduced pose system: k_ba_solve_lds (<= 30 free poses with edges), k_ba_chol_lds (31-32), k_ba_chol (>= 33);
  - the active structure: built on the device (P <= 1024, <= 32 free poses, no duplicate (pose, point) edges) or on the host.

Runs only in the build container.  Each problem is synth.ba_problem(**kw) followed by the explicit post-edits of problem() below,
which the tests share.  The fixture stores the case list, a digest of every problem's inputs (a generator change cannot silently move
the goalposts) and g2o's outputs.  To stay small it stores edge_chi2 as float32: the tests compare it at rtol 1e-6 and use it for
the distance of every edge from the 5.991 gate, both far above float32's 6e-8 relative rounding.
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

OUT_KEYS = ("poses", "points", "edge_outlier1", "edge_depth_pos", "edge_chi2", "chi2_first", "chi2_second", "iters_first", "iters_second")

# name, synth.ba_problem kwargs, post-edit, intended (dense solve, structure) per round: solve 0 solve_lds / 1 chol_lds / 2 chol,
# structure 0 device / 1 host.  Round 1 runs over the structure of round 0 with its level-1 edges masked, so it repeats round 0's form.
CASES = [
    dict(name="free29", kw=dict(n_free=29, n_fixed=4, n_points=450, seed=101), edit=None, forms=(0, 0)),
    dict(name="free30", kw=dict(n_free=30, n_fixed=4, n_points=450, seed=102), edit=None, forms=(0, 0)),
    dict(name="free31", kw=dict(n_free=31, n_fixed=4, n_points=450, seed=103), edit=None, forms=(1, 0)),
    dict(name="free32", kw=dict(n_free=32, n_fixed=4, n_points=450, seed=104), edit=None, forms=(1, 0)),
    dict(name="free33", kw=dict(n_free=33, n_fixed=4, n_points=500, seed=105), edit=None, forms=(2, 1)),
    dict(name="free64", kw=dict(n_free=64, n_fixed=4, n_points=800, seed=106), edit=None, forms=(2, 1)),
    dict(name="free100", kw=dict(n_free=100, n_fixed=6, n_points=1200, seed=107), edit=None, forms=(2, 1)),
    # fixed keyframes interleave with the free ones by id, as the reference orders its vertices (ascending KF id)
    dict(name="interleaved", kw=dict(n_free=20, n_fixed=12, n_points=450, seed=108), edit="interleave", forms=(0, 0)),
    dict(name="interleaved31", kw=dict(n_free=31, n_fixed=9, n_points=450, seed=109), edit="interleave", forms=(1, 0)),
    # ~15 % of the edges observed twice by the same pose: the structure is built on the host
    dict(name="dup_edges", kw=dict(n_free=24, n_fixed=6, n_points=400, seed=110), edit="dup", forms=(0, 1)),
    # more than kStructMaxP = 1024 poses, 8 of them free and spread over the ids: the structure is built on the host
    # (a problem of 8 free + 8 fixed poses joined with one of 1092 fixed poses, ids shuffled together)
    dict(name="p1108", kw=dict(n_free=8, n_fixed=8, n_points=400, seed=111), edit="pad1092", forms=(0, 1)),
    # every observation of one free pose a gross outlier: round 1 masks all its edges; the pose keeps its (now empty) block
    dict(name="masked_pose", kw=dict(n_free=31, n_fixed=4, n_points=450, seed=113), edit="mask_pose", forms=(1, 0)),
]


def problem(case, synth):
    """synth.ba_problem(**kw) and the case's post-edit (deterministic: every draw comes from its own seeded stream)"""
    prob = synth.ba_problem(**case["kw"])
    edit = case["edit"]
    rng = np.random.default_rng(1000 + case["kw"]["seed"])
    if edit == "pad1092":
        # a second problem of 1092 fixed poses (its landmarks are seen by fixed poses only) joined behind the first
        pad = synth.ba_problem(n_free=0, n_fixed=1092, n_points=200, obs_per_point=2, seed=case["kw"]["seed"] + 1)
        P1, L1 = len(prob["poses"]), len(prob["points"])
        for k in ("poses", "fixed", "points", "e_obs", "e_info"):
            prob[k] = np.concatenate([prob[k], pad[k]])
        prob["e_point"] = np.concatenate([prob["e_point"], pad["e_point"] + L1]).astype(np.int32)
        prob["e_pose"] = np.concatenate([prob["e_pose"], pad["e_pose"] + P1]).astype(np.int32)
        edit = "interleave"
    if edit == "interleave":
        # new id of old pose i: a seeded permutation, so fixed and free ids interleave
        P = len(prob["poses"])
        new_id = rng.permutation(P).astype(np.int32)
        poses, fixed = np.empty_like(prob["poses"]), np.empty_like(prob["fixed"])
        poses[new_id], fixed[new_id] = prob["poses"], prob["fixed"]
        prob["poses"], prob["fixed"] = poses, fixed
        prob["e_pose"] = new_id[prob["e_pose"]]
    elif edit == "dup":
        # each chosen edge gets a second observation by the same pose (0.1 px apart), inserted right behind it
        E = len(prob["e_point"])
        dup = np.sort(rng.choice(E, int(0.15 * E), replace=False))
        order = np.sort(np.r_[np.arange(E), dup])
        second = np.r_[False, order[1:] == order[:-1]]
        for k in ("e_point", "e_pose", "e_obs", "e_info"):
            prob[k] = np.ascontiguousarray(prob[k][order])
        prob["e_obs"][second] += rng.choice([-0.1, 0.1], (int(second.sum()), 2))
    elif edit == "mask_pose":
        # the middle free pose: every observation moved by +-40 px in both coordinates
        fixed = prob["fixed"]
        p = int(np.flatnonzero(fixed == 0)[len(np.flatnonzero(fixed == 0)) // 2])
        sel = prob["e_pose"] == p
        prob["e_obs"][sel] += rng.choice([-40.0, 40.0], (int(sel.sum()), 2))
    else:
        assert edit is None, edit
    return prob


def main():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "oracle", "ref_g2o")])
    synth = g.load_package().synth
    ref = g.load_oracle().RefG2O()
    out = {"cases": np.array(json.dumps(CASES))}
    for i, case in enumerate(CASES):
        prob = problem(case, synth)
        res = ref.local_ba(prob)
        out[f"c{i}_in_sha256"] = np.array(problem_digest(prob))
        for k in OUT_KEYS:
            v = np.asarray(res[k])
            out[f"c{i}_out_{k}"] = v.astype(np.float32) if k == "edge_chi2" else v
        print(case["name"], "P", len(prob["poses"]), "L", len(prob["points"]), "E", len(prob["e_point"]), "iters", res["iters_first"],
              res["iters_second"], "outliers", int(res["edge_outlier1"].sum()))
    path = os.path.join(ROOT, "tests", "golden", "ba_paths_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
