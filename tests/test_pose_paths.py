"""PoseOptimization (ba.hip, pose_opt_body): every edge-store form, pass geometry, round structure and Levenberg exit of
asd_pose_optimize against the REFERENCE's own vendored g2o.

Pinning: tests/golden/pose_paths_golden.npz holds g2o's pose, flags, inlier count and per-round trace (active edges, what
optimize(10) returned, trials per iteration, the robust chi2 after every computeActiveErrors, nBad, flags changed) for the case
list of tests/golden/make_pose_paths_golden.py, which also makes the problems and checks from g2o's trace that every case takes the
path it names.  asd_debug_pose_opt reports the store a call took and what each round did, so a changed threshold cannot quietly turn
a case into a run of another form, and the rounds the solver does not run (the `repeat` shortcut) are compared with the rounds g2o
really ran.

The bar is tests/test_optimizer.py's: pose within 1e-8 per component of g2o's, flags and inlier count identical.

What is compared of the counts, and why not more.  A PoseOptimization round nearly always ends at the rounding floor: its last
accept / reject decisions change the robust chi2 by less than 1e-8 relative (often by exactly 0), so whether a round takes 1 or 9
trials there is decided by the last bit of a sum, and the device sums in another order.  Counts are therefore compared over the
"decisive prefix" of each round: the iterations before the first one in which an accept / reject moved the chi2 by less than 1e-8
relative or the nBad test had a margin below 1e-6.  The aid reports totals per round, so a round that is decisive throughout must
equal g2o's iterations and trials; otherwise the device must have run at least the prefix and the iteration behind it.  Ten
rejections in a row multiply lambda by 2^45: the later trials move the pose by nothing and differ in rounding only, and a round
that ends on a rejected trial (the only way the re-classification's S.Teval differs from S.T) exists only at that floor.  Such
rounds are run for their results in many cases (the eight seeds of reject_*), and test_hip_meets_the_floor_paths counts from the aid in
how many of them the device itself ended a round on a rejected trial, and rejected a trial in the middle of a round (on an MI355X:
12 and 8 of the 45 cases; g2o ends a round on a rejected trial in 17).  For the same reason these tests cannot tell a
re-classification at S.Teval from one at S.T: where the two poses differ at all, they differ by a step taken with lambda x 2^36 or
more, which moves an edge's chi2 by far less than the 1e-6 the fixture keeps every edge away from the gate.  That hand mutation
passes every test here although the device does meet the situation; the other four of the issue's list (the `round <= 2` bound of
the repeat shortcut dropped, bare hardware reciprocal, wave early exit one wave too soon, lowered full-LDS limit) each fail
test_hip_pose_paths_match_g2o.

Not positive definite: no generator input was found on which g2o's dense LDLT fails (lambda = 1e-5 max diag H keeps the damped system
positive definite on every finite problem tried, the rank-deficient collinear and same-point cases included); no case fakes it.
The aid's count of such trials must be 0 everywhere.  Likewise the solver's phase 2 (a pass that re-evaluates the current pose after
an iteration that ended on a rejected trial without ending the round) needs a gain ratio that is neither < 0, == 0 nor accepted,
i.e. a non-finite one: no finite problem takes it, and the aid must report 0 such passes.
"""
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.golden.make_live_golden import problem_digest
from tests.golden.make_pose_paths_golden import (AXES, CASES, GATE_MARGIN, LDS_BYTES, NBAD_MARGIN, ORACLE_TOL, PATHS, TRIAL_MARGIN,
                                                 decisive_prefix, ends_rejected, expected_skips, problem, rejected_mid, replay,
                                                 store_of, unpack_trace)
from tests.test_optimizer import POSE_ATOL

NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: (i, c) for i, c in enumerate(CASES)}
FLOOR_SEEDS = ("reject_71", "reject_72", "reject_73", "reject_77", "reject_80", "reject_86", "reject_88", "reject_89")


@pytest.fixture(scope="module")
def golden():
    G = np.load(os.path.join(GOLDEN, "pose_paths_golden.npz"))
    assert json.loads(str(G["cases"])) == json.loads(json.dumps(CASES)), "the fixture was made from another case list"
    return G


@pytest.fixture(scope="module")
def probs(synth):
    return {c["name"]: problem(c, synth) for c in CASES}


def args_of(pp):
    return pp["pose"], pp["Xw"], pp["obs"], pp["info"], pp["K"]


def stored(G, i):
    return G[f"c{i}_out_pose"], G[f"c{i}_out_outlier"], int(G[f"c{i}_out_ninl"]), unpack_trace(G, i)


# ------------------------------------------------------------------ the fixture and the oracle (CPU)
def test_pose_paths_inputs_match_generator(golden, probs):
    for i, c in enumerate(CASES):
        assert problem_digest(probs[c["name"]]) == str(golden[f"c{i}_in_sha256"]), f"{c['name']}: the generator no longer makes the stored problem"


def test_pose_paths_cases_select_their_store(probs):
    """the host's rule restated: f32-exact observations, <= 16 distinct information bit patterns, 35 n + 16 resp. 50 n + 16 <= 150 KiB;
    both sides of every limit are in the list, and every store holds a size with n % 8 != 0 (flag packing)"""
    assert 35 * 4388 + 16 <= LDS_BYTES < 35 * 4389 + 16 and 50 * 3071 + 16 <= LDS_BYTES < 50 * 3072 + 16
    odd = set()
    for c in CASES:
        pp = probs[c["name"]]
        assert store_of(pp) == c["store"], c["name"]
        if len(pp["Xw"]) % 8:
            odd.add(c["store"])
    assert {0, 1, 2} <= odd
    assert {(BY_NAME[n][1]["store"]) for n in ("compact_4388", "compact_4389", "f64obs_3071", "f64obs_3072", "info17_1500", "info17_3500")} == {0, 1, 2}


def test_pose_paths_golden_takes_the_intended_paths(golden):
    """g2o's own trace shows every path its case names, and every axis of the exits is met by some case"""
    met = {a: [] for a in AXES}
    for i, c in enumerate(CASES):
        trace = unpack_trace(golden, i)
        for path in c["paths"]:
            assert PATHS[path](trace), f"{c['name']}: g2o's trace does not show {path}"
        for rnd in trace:
            assert len(rnd["calls"]) == len(rnd["trials"]) + sum(rnd["trials"]), c["name"]
            assert rnd["ret"] == (len(rnd["trials"]) if rnd["active"] else -1), c["name"]
        for r in range(1, len(trace)):
            assert trace[r]["active"] == len(golden[f"c{i}_out_outlier"]) - trace[r - 1]["n_bad"], c["name"]
        for a in AXES:
            if PATHS[a](trace):
                met[a].append(c["name"])
    for a in AXES:
        assert met[a], f"no case takes the path {a}"
    assert all(PATHS["ends_rejected"](unpack_trace(golden, BY_NAME[n][0])) for n in FLOOR_SEEDS)
    # the defining events of far_start lie inside the decisive prefix: 10 iterations in rounds 0 and 1, rejected trials in the middle of round 1
    tr = unpack_trace(golden, BY_NAME["far_start"][0])
    assert decisive_prefix(tr[0]) == 10 and decisive_prefix(tr[1]) == 10 and tr[1]["trials"] == [1, 4, 1, 1, 1, 1, 1, 6, 1, 1]


def test_pose_paths_golden_is_not_on_a_knife_edge(golden):
    """no edge chi2 that a re-classification read lies within 1e-6 (relative) of 5.991 (the driver takes the distance from the
    values the re-classification itself read, so a round that ended on a rejected trial is measured at the rejected pose); no
    admitted case has oracle and g2o further apart than 1e-9.  (At the gate an edge's error is about 2.4 px sigma; a pose component
    off by d moves a projection by up to about fx d = 720 d px, the chi2 by about 600 d relative: d <= 1e-9 cannot cross 1e-6.)"""
    for i, c in enumerate(CASES):
        for r, rnd in enumerate(unpack_trace(golden, i)):
            assert rnd["gate_margin"] >= GATE_MARGIN, f"{c['name']} round {r}: edge {rnd['gate_edge']} is {rnd['gate_margin']:.2e} from the gate"
        assert float(golden[f"c{i}_orc_dist"]) <= ORACLE_TOL, c["name"]
    assert len(json.loads(str(golden["dropped"]))) <= 2
    assert (GATE_MARGIN, ORACLE_TOL, TRIAL_MARGIN, NBAD_MARGIN) == (1e-6, 1e-9, 1e-8, 1e-6)


def check_trace(got, exp, what):
    """per round: active edges, nBad and flag changes identical; trials per iteration identical over the decisive prefix"""
    assert len(got) == len(exp), f"{what}: {len(got)} rounds, not {len(exp)}"
    for r, (a, b) in enumerate(zip(got, exp)):
        for k in ("active", "n_bad", "changed", "reinlier"):
            assert a[k] == b[k], f"{what} round {r}: {k} {a[k]} != {b[k]}"
        assert (a["ret"] == -1) == (b["ret"] == -1), f"{what} round {r}"
        pre = decisive_prefix(b)
        assert a["trials"][:pre] == b["trials"][:pre], f"{what} round {r}: trials {a['trials']} against {b['trials']} (decisive prefix {pre})"
        if pre == len(b["trials"]):
            assert a["trials"] == b["trials"], f"{what} round {r}"
        else:
            assert len(a["trials"]) > pre, f"{what} round {r}"


def test_oracle_matches_pose_paths_golden(oracle, oracle_mod, golden, probs):
    """the oracle against the stored g2o results and, where oracle/_ref is built from this tree's driver (revision 3), against the
    reference g2o itself: pose within 1e-9, flags and inlier count identical, the trace as check_trace says"""
    live = oracle_mod.RefG2O() if oracle_mod.RefG2O.available(abi=3) else None
    for i, c in enumerate(CASES):
        pp = probs[c["name"]]
        pose, flags, ninl = oracle.pose_optimize(*args_of(pp))
        trace = oracle.pose_optimize_trace()
        refs = [stored(golden, i) + ("fixture",)]
        if live is not None:
            refs.append(live.pose_optimize(*args_of(pp)) + (live.pose_optimize_trace(), "live g2o"))
        for rpose, rflags, rninl, rtrace, what in refs:
            np.testing.assert_allclose(pose, rpose, atol=ORACLE_TOL, rtol=0, err_msg=f"{c['name']} vs {what}")
            np.testing.assert_array_equal(flags, rflags, err_msg=f"{c['name']} vs {what}")
            assert ninl == rninl, f"{c['name']} vs {what}"
            check_trace(trace, rtrace, f"{c['name']} vs {what}")
        if live is not None:   # g2o itself reproduces its stored results bit for bit
            np.testing.assert_array_equal(refs[1][0], refs[0][0], err_msg=c["name"])
            np.testing.assert_array_equal(refs[1][1], refs[0][1], err_msg=c["name"])


# ------------------------------------------------------------------ HIP (GPU)
def run_hip(ctx, pp):
    pose, flags, ninl = ctx.pose_optimize(*args_of(pp))
    store, rounds = ctx.pose_opt_debug()
    return pose, flags, ninl, store, rounds


def check_hip(got, exp, c, pp, oracle):
    pose, flags, ninl, store, rounds = got
    epose, eflags, eninl, trace = exp
    name = c["name"]
    dist = float(np.abs(pose - epose).max())
    print(f"{name}: store {store} |pose - g2o| {dist:.1e} rounds {rounds[:, :5].tolist()}")
    if not np.array_equal(flags, eflags):   # a flip at a distance above 1e-9 is a conditioning finding, below it a logic error
        k = np.flatnonzero(flags != eflags)
        print(f"{name}: flags differ at {k.tolist()}, pose distance {dist:.2e}, nearest gate margins per round "
              f"{[(r['gate_edge'], r['gate_margin']) for r in trace]}")
    np.testing.assert_allclose(pose, epose, atol=POSE_ATOL, rtol=0, err_msg=name)
    np.testing.assert_array_equal(flags, eflags, err_msg=name)
    assert ninl == eninl, name
    # float32 write-back (Converter::toCvMat) agrees to 1 ulp
    np.testing.assert_allclose(oracle.pose7_to_tcw(pose), oracle.pose7_to_tcw(epose), rtol=2e-7, atol=1e-7, err_msg=name)
    assert store == c["store"], f"{name}: took store {store}, not {c['store']}"
    if len(pp["Xw"]) < 3:
        assert (rounds == -1).all(), name
        return
    skips = expected_skips(trace)
    for r in range(4):
        row = rounds[r]
        if r >= len(trace):
            assert (row == -1).all(), f"{name} round {r}: {row.tolist()}"
            continue
        g = trace[r]
        assert row[0] == (1 if r in skips else 0), f"{name} round {r}: state {row[0]}, g2o's flags changed {[t['changed'] for t in trace]}"
        # g2o really runs the round: a round the solver does not run must report what g2o's run of it produced
        assert row[1] == g["active"] and row[7] == g["n_bad"], f"{name} round {r}: active / nBad {row[1]} / {row[7]}, g2o {g['active']} / {g['n_bad']}"
        assert row[4] == 1 + row[3] + row[5], f"{name} round {r}: passes {row.tolist()}"
        assert row[5] == 0 and row[6] == 0, f"{name} round {r}: phase-2 passes / trials not positive definite {row.tolist()}"
        if g["ret"] == -1:
            assert row[2] == 0 and row[3] == 0, f"{name} round {r}: {row.tolist()}"
            continue
        pre, rep = decisive_prefix(g), replay(g)
        if pre == len(g["trials"]):
            assert (row[2], row[3]) == (len(g["trials"]), sum(g["trials"])), f"{name} round {r}: iterations / trials {row[2]} / {row[3]}, g2o {g['trials']}"
            assert row[8] == int(ends_rejected(g)) and row[9] == sum(1 for it in rep[:-1] if not all(it["acc"])), f"{name} round {r}: {row.tolist()}"
        else:
            assert row[2] > pre and row[3] >= sum(g["trials"][:pre]) + 1, f"{name} round {r}: iterations / trials {row[2]} / {row[3]}, g2o {g['trials']} prefix {pre}"
            assert row[9] >= sum(1 for it in rep[:pre] if not all(it["acc"])), f"{name} round {r}: {row.tolist()}"


@pytest.mark.gpu
def test_hip_pose_opt_debug_before_any_run(pkg):
    ctx = pkg.AsdHip(n_features=500, max_width=640, max_height=240, max_patches=1024)
    try:
        store, rounds = ctx.pose_opt_debug()
        assert store == -1 and (rounds == -1).all()
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_pose_paths_match_g2o(name, hip, golden, probs, oracle):
    i, c = BY_NAME[name]
    pp = probs[name]
    got = run_hip(hip, pp)
    check_hip(got, stored(golden, i), c, pp, oracle)
    again = run_hip(hip, pp)
    for a, b in zip(got, again):
        np.testing.assert_array_equal(a, b, err_msg=f"{name}: second run")


@pytest.mark.gpu
def test_hip_meets_the_floor_paths(hip, golden, probs):
    """Paths that exist only at the rounding floor cannot be promised per case; over the cases that g2o takes them in, the device
    must meet them too: a round that ends on a rejected trial (re-classification at S.Teval != S.T) and a trial rejected in the middle
    of a round.  The counts are printed."""
    ended, mid, g_ended = [], [], []
    for i, c in enumerate(CASES):
        if len(probs[c["name"]]["Xw"]) < 3:
            continue
        _, _, _, _, rounds = run_hip(hip, probs[c["name"]])
        trace = unpack_trace(golden, i)
        ran = rounds[rounds[:, 0] == 0]
        if (ran[:, 8] == 1).any():
            ended.append(c["name"])
        if (ran[:, 9] > 0).any():
            mid.append(c["name"])
        if any(ends_rejected(r) for r in trace):
            g_ended.append(c["name"])
    print(f"a round ended on a rejected trial: device {len(ended)} cases {ended}; g2o {len(g_ended)} cases {g_ended}")
    print(f"a trial rejected in the middle of a round: device {len(mid)} cases {mid}")
    assert ended, "the device never ended a round on a rejected trial: the re-classification at S.Teval is not exercised"
    assert "far_start" in mid and rejected_mid(unpack_trace(golden, BY_NAME["far_start"][0]), decisive_only=True) > 0


@pytest.mark.gpu
def test_hip_pose_paths_leave_no_state_behind(pkg, golden, probs):
    """one fresh context runs the whole list in order and then in reverse: nothing of a previous call (the staging buffer's
    information-index bytes, the flag scratch, the global store after an LDS case, the aid's block) may leak into the next -- the
    second sweep is bit-identical to the first, which matches g2o's flags"""
    ctx = pkg.AsdHip(n_features=500, max_width=640, max_height=240, max_patches=1024)
    try:
        first = {c["name"]: run_hip(ctx, probs[c["name"]]) for c in CASES}
        second = {c["name"]: run_hip(ctx, probs[c["name"]]) for c in reversed(CASES)}
    finally:
        ctx.close()
    for i, c in enumerate(CASES):
        for a, b in zip(first[c["name"]], second[c["name"]]):
            np.testing.assert_array_equal(a, b, err_msg=f"{c['name']}: reverse sweep")
        np.testing.assert_array_equal(first[c["name"]][1], golden[f"c{i}_out_outlier"], err_msg=c["name"])
        assert first[c["name"]][3] == c["store"], c["name"]
