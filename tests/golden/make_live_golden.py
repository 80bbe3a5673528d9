#!/usr/bin/env python3
"""Generate tests/golden/live_golden.npz: what the REFERENCE's own vendored g2o and DBoW2 classes (compiled in place by
oracle/ref_g2o/Makefile and oracle/ref_dbow2/Makefile, outputs in oracle/_ref/, never committed) return on the inputs of the two
"live" tests -- tests/test_optimizer.py::test_oracle_vs_live_reference_nominal (the SURVEY 8(d) nominal LocalBA problem,
E ~ 29k) and tests/test_bow.py::test_reference_dbow2_live_when_built -- so that those tests compare against the reference
wherever they run, with or without oracle/_ref.

Runs only in the build container.  The nominal problem comes from asd-slam_amd/synth.py (seeded); the fixture stores a digest
of its inputs (a generator change cannot silently move the goalposts) and the g2o outputs the test asserts on.  The DBoW2
inputs are small and stored as they are.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

BA_KEYS = ("poses", "points", "edge_outlier1", "iters_first", "iters_second")
BOW_SIZES = (0, 5, 1500)
BOW_KEYS = ("bow_id", "bow_val", "fv_node", "fv_start", "fv_idx")


def problem_digest(prob):
    return hashlib.sha256(b"".join(np.ascontiguousarray(prob[k]).tobytes() for k in sorted(prob))).hexdigest()


def bow_inputs():
    """(n, word, weight, node) for every size, drawn in the order the test draws them"""
    rng = np.random.default_rng(77)
    out = []
    for n in BOW_SIZES:
        word = rng.integers(0, 400, n).astype(np.int32)
        node = (word // 13).astype(np.int32)
        weight = np.where(rng.uniform(size=n) < 0.1, 0.0, rng.uniform(0.1, 5.0, n))
        out.append((n, word, weight, node))
    return out


def main():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "oracle", "ref_g2o")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "ref_dbow2")])
    po = g.load_oracle()
    prob = g.load_package().synth.ba_problem()
    res = po.RefG2O().local_ba(prob)
    out = {"nominal_in_sha256": np.array(problem_digest(prob))}
    for k in BA_KEYS:
        out["nominal_out_" + k] = np.asarray(res[k])
    print("nominal LocalBA: E", len(prob["e_point"]), "iters", res["iters_first"], res["iters_second"], "outliers", int(res["edge_outlier1"].sum()))
    ref = po.RefDBoW2()
    for n, word, weight, node in bow_inputs():
        out[f"bow_n{n}_in_word"], out[f"bow_n{n}_in_weight"], out[f"bow_n{n}_in_node"] = word, weight, node
        for weighting in range(4):
            for scoring in range(6):
                (bid, bval), fv = ref.assemble(word, weight, node, weighting, scoring)
                for key, v in zip(BOW_KEYS, (bid, bval) + fv):
                    out[f"bow_n{n}_w{weighting}_s{scoring}_{key}"] = v
    path = os.path.join(ROOT, "tests", "golden", "live_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
