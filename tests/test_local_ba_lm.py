"""LocalBundleAdjustment's Levenberg control (ba.hip, lm_begin_body / lm_control_body) and the host's batching of trials
(local_ba_impl, run_round), on problems that take the control's exits:
  - Raul's rule, nBad >= 3 (levenberg.cpp:138-146), ending a round before its iteration count, with the device-built and the
    host-built structure;
  - a second round with every edge gated out: g2o's optimize() finds no active vertex and returns -1 (sparse_optimizer.cpp:356);
  - its_first / its_second of (1, 2), (0, 10) and (5, 20).

Pinning: tests/golden/ba_lm_golden.npz holds the outputs, trial counts and Levenberg trace of the REFERENCE's own vendored g2o
(tests/golden/make_ba_lm_golden.py, which also makes the problems).  The bar is tests/test_optimizer.py's, and iteration and
trial counts must equal g2o's.  asd_debug_local_ba_lm reports the iterations, trials and trial blocks of each round, so the
batching can be checked: a round's first chunk of blocks is as long as the trials the same round of the context's previous
LocalBA took, further chunks are 2 blocks, and the blocks behind the round's end must change nothing.
"""
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.golden.make_ba_lm_golden import CASES, OUT_KEYS, problem, replay, round_exit
from tests.golden.make_live_golden import problem_digest
from tests.test_local_ba_paths import check_result, max_diffs

NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: (i, c) for i, c in enumerate(CASES)}
RESULT_KEYS = ("poses", "points", "edge_chi2", "edge_outlier1", "edge_depth_pos", "chi2_first", "chi2_second", "iters_first", "iters_second")


@pytest.fixture(scope="module")
def golden():
    G = np.load(os.path.join(GOLDEN, "ba_lm_golden.npz"))
    assert json.loads(str(G["cases"])) == json.loads(json.dumps(CASES)), "the fixture was made from another case list"
    return G


@pytest.fixture(scope="module")
def probs(synth):
    return {c["name"]: problem(c, synth) for c in CASES}


def stored(G, i):
    return {k: G[f"c{i}_out_{k}"] for k in OUT_KEYS}


def check_counts(got, exp, what):
    """iterations and trials of both rounds equal g2o's"""
    for k in ("iters_first", "iters_second", "trials_first", "trials_second"):
        assert int(got[k]) == int(exp[k]), f"{what}: {k} {int(got[k])} != {int(exp[k])}"


# ------------------------------------------------------------------ the fixture and the oracle (CPU)
def test_lm_golden_inputs_match_generator(golden, probs):
    for i, c in enumerate(CASES):
        assert problem_digest(probs[c["name"]]) == str(golden[f"c{i}_in_sha256"]), f"{c['name']}: the generator no longer makes the stored problem"


def test_lm_golden_takes_the_intended_exits(golden):
    """g2o's own trace, replayed, ends every round where the case says (and agrees with its iteration and trial counts)"""
    for i, c in enumerate(CASES):
        for r, key in enumerate(("first", "second")):
            iters, calls = golden[f"c{i}_r{r}_iters"], golden[f"c{i}_r{r}_calls"]
            n_done = int(golden[f"c{i}_out_iters_{key}"])
            assert round_exit(n_done, c["its"][r], replay(iters, calls)) == c["exits"][r], (c["name"], r)
            assert int(iters[:, 0].sum()) == int(golden[f"c{i}_out_trials_{key}"]), (c["name"], r)
            if c["exits"][r] == "nbad":
                assert 3 <= n_done < c["its"][r], (c["name"], r, n_done)
    search = json.loads(str(golden["search"]))
    assert search["round1_nbad"]["tried"] > 0 and search["rejected_trial"]["tried"] > 0


def test_lm_golden_is_not_on_a_knife_edge(golden):
    """a last-bit difference between g2o, the oracle and HIP cannot flip a decision:
      - every nBad decision is >= 1e-6 (relative) away from (iniChi - currentChi) * 1e3 == iniChi;
      - every accept / reject changes the chi2 by >= 1e-8 relative (the sign of rho is the sign of that change);
      - no edge chi2 the gating read, nor any final one, lies within 1e-6 (relative) of 5.991."""
    for i, c in enumerate(CASES):
        for r in range(2):
            for k, it in enumerate(replay(golden[f"c{i}_r{r}_iters"], golden[f"c{i}_r{r}_calls"])):
                where = f"{c['name']} round {r} iteration {k}"
                if it["exit"] != "trials":
                    margin = abs((it["ini"] - it["cur"]) * 1e3 - it["ini"]) / it["ini"]
                    assert margin >= 1e-6, f"{where}: nBad decision margin {margin:.2e}"
                ref = it["ini"]
                for t in it["temps"]:
                    assert abs(t - ref) >= 1e-8 * ref, f"{where}: trial chi2 {t} against {ref}"
                    ref = min(ref, t)
        for key in ("gate_chi2", "out_edge_chi2"):
            chi2 = golden[f"c{i}_{key}"].astype(np.float64)
            margin = np.abs(chi2 - 5.991) / 5.991
            assert margin.min() >= 1e-6, f"{c['name']} {key}: edge {int(margin.argmin())} chi2 {chi2[margin.argmin()]}"


def test_oracle_matches_lm_golden(oracle, oracle_mod, golden, probs):
    """the oracle against the stored g2o outputs (counts included) and, where oracle/_ref is built from this tree's driver
    (revision 2: trial counts, edge errors ahead of an its_first = 0 round), against the reference g2o itself"""
    live = oracle_mod.RefG2O() if oracle_mod.RefG2O.available(abi=2) else None
    for i, c in enumerate(CASES):
        prob = probs[c["name"]]
        o = oracle.local_ba(prob, *c["its"])
        exp = stored(golden, i)
        check_result(o, exp, f"{c['name']} vs fixture")
        check_counts(o, exp, f"{c['name']} vs fixture")
        if live is not None:
            ref = live.local_ba(prob, *c["its"])
            check_result(o, ref, f"{c['name']} vs live g2o")
            check_counts(o, ref, f"{c['name']} vs live g2o")


# ------------------------------------------------------------------ HIP (GPU)
def new_ctx(pkg):
    return pkg.AsdHip(n_features=500, max_width=640, max_height=240, max_patches=1024)


def check_lm(lm, exp, what):
    """the aid's iterations and trials per round equal g2o's"""
    for r, key in enumerate(("first", "second")):
        assert (int(lm[r][0]), int(lm[r][1])) == (int(exp[f"iters_{key}"]), int(exp[f"trials_{key}"])), f"{what} round {r}: {lm[r].tolist()}"


def assert_same(a, b, what):
    for k in RESULT_KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_local_ba_lm_matches_g2o_and_oracle(name, hip, golden, probs, oracle):
    i, c = BY_NAME[name]
    prob = probs[name]
    got = hip.local_ba(prob, *c["its"])
    lm = hip.local_ba_lm()
    exp = stored(golden, i)
    check_result(got, exp, f"{name} vs g2o fixture")
    check_lm(lm, exp, f"{name} vs g2o fixture")
    o = oracle.local_ba(prob, *c["its"])
    check_result(got, o, f"{name} vs oracle")
    for k in RESULT_KEYS:
        assert not np.isnan(np.asarray(got[k], np.float64)).any(), f"{name}: NaN in {k}"
    dp, dl = max_diffs(got, o)
    print(f"{name}: iterations {lm[:, 0].tolist()} trials {lm[:, 1].tolist()} blocks {lm[:, 2].tolist()}: "
          f"HIP vs oracle max |d| poses {dp:.1e} points {dl:.1e}")
    again = hip.local_ba(prob, *c["its"])
    np.testing.assert_array_equal(hip.local_ba_lm()[:, :2], lm[:, :2])
    assert_same(again, got, f"{name}: second run")


def run_abab(ctx, a, b, submit):
    out = []
    for prob in (a, b, a, b):
        if submit:
            ctx.local_ba_submit(prob)
            res = ctx.local_ba_wait()
        else:
            res = ctx.local_ba(prob)
        out.append((res, ctx.local_ba_lm()))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("submit", [False, True], ids=["inline", "lane"])
def test_hip_local_ba_lm_batching(submit, pkg, golden, probs):
    """A (second round ends on Raul's rule after 3 trials) and B (10 iterations) as A, B, A, B on one fresh context: call 2's second
    round is enqueued as 3 + 2 + 2 + 2 + 2 blocks, call 3's as 10 blocks for 3 trials (7 no-ops behind the end); every result is
    bit-identical to the same problem on a fresh context and matches g2o"""
    (ia, ca), (ib, cb) = BY_NAME["nbad_r2"], BY_NAME["full"]
    a, b = probs["nbad_r2"], probs["full"]
    fresh = {}
    for key, prob in (("a", a), ("b", b)):
        ctx = new_ctx(pkg)
        try:
            fresh[key] = ctx.local_ba(prob)
        finally:
            ctx.close()
    ctx = new_ctx(pkg)
    try:
        runs = run_abab(ctx, a, b, submit)
    finally:
        ctx.close()
    # rows: round; columns: iterations, trials, blocks enqueued, first chunk
    expect = [
        [[5, 5, 5, 5], [3, 3, 10, 10]],    # A on a fresh context: its_first / its_second blocks in one chunk each
        [[5, 5, 5, 5], [10, 10, 11, 3]],   # B: round 2 predicted from A's 3 trials, then chunks of 2
        [[5, 5, 5, 5], [3, 3, 10, 10]],    # A: round 2 predicted from B's 10 trials
        [[5, 5, 5, 5], [10, 10, 11, 3]],
    ]
    for k, ((res, lm), exp_lm, key) in enumerate(zip(runs, expect, "abab")):
        what = f"call {k + 1} ({key.upper()})"
        assert lm.tolist() == exp_lm, f"{what}: {lm.tolist()} != {exp_lm}"
        assert_same(res, fresh[key], f"{what} against a fresh context")
        check_result(res, stored(golden, ia if key == "a" else ib), f"{what} vs g2o fixture")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gated_all", "gated_all_sparse"])
def test_hip_local_ba_all_gated(name, hip, golden, probs):
    """every edge gated out after round 1: the second round reports g2o's -1, runs no trial and moves nothing -- poses and points
    bit-identical to an its_second = 0 run, no NaN, the stored per-edge chi2 and depth flags as g2o left them"""
    i, c = BY_NAME[name]
    prob = probs[name]
    got = hip.local_ba(prob, *c["its"])
    lm = hip.local_ba_lm()
    exp = stored(golden, i)
    assert int(got["iters_second"]) == int(exp["iters_second"]) == -1, got["iters_second"]
    assert lm[1].tolist()[:2] == [-1, 0], lm.tolist()
    assert got["edge_outlier1"].all()
    zero = hip.local_ba(prob, c["its"][0], 0)
    assert int(zero["iters_second"]) == -1
    for k in ("poses", "points", "edge_chi2", "edge_depth_pos", "edge_outlier1"):
        np.testing.assert_array_equal(got[k], zero[k], err_msg=f"{name}: {k} against its_second = 0")
    for k in RESULT_KEYS:
        assert not np.isnan(np.asarray(got[k], np.float64)).any(), f"{name}: NaN in {k}"
    np.testing.assert_allclose(got["edge_chi2"], exp["edge_chi2"].astype(np.float64), rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(got["edge_depth_pos"], exp["edge_depth_pos"])
    assert got["chi2_second"] == 0.0
