"""Cases shared by the fuse-apply tests: hand-worked maps with the expected outcome of every call written out (tests/test_fuse_apply_ref.py
pins the restatement on them, tests/test_fuse_apply.py and tests/test_fuse_apply_host.py run the device and the flat host rule on them),
the random generator with what chance does not give planted, and the problem file of host/test_fuse_apply_rule."""
import numpy as np

from tests.culling_cases import RANDOM_SHAPES, mk, random_case
from tests.fuse_apply_ref import observations

KEYS = ("action", "other", "obs_cand", "obs_other", "n_moved", "n_dropped")
MODE_CODES = {0: (0, 1, 2, 3, 4, 7), 1: (0, 1, 3, 4, 7), 2: (0, 1, 3, 5, 6)}   # the outcomes a mode can produce


def _exp(action, other, obs_cand, obs_other, n_moved, n_dropped, n_fused):
    return dict(action=action, other=other, obs_cand=obs_cand, obs_other=obs_other, n_moved=n_moved, n_dropped=n_dropped, n_fused=n_fused)


def hand_cases():
    """-> [(name, map, calls, rows_after)]; calls = [(kf, mode, cand, best_idx, expected)], applied one after the other; rows_after = the
    whole table and the bad points after the last call.  Every expectation is worked by hand against ORBmatcher.cc:842-957, :986-1083,
    LoopClosing.cc:540-555, :619-627 and MapPoint.cc:206-244."""
    out = []
    # an empty entry takes the candidate; Observations() of the candidate is read in front of the step
    out.append(("add at an empty entry", mk({1: [100, -1], 2: [101]}),
                [(1, 0, [101], [1], _exp([1], [-1], [1], [0], [0], [0], 1))],
                ({1: [100, 101], 2: [101]}, set())))
    # 2 against 2: '>' is strict, so the keyframe's point is the one replaced; both its observations are re-seated
    out.append(("tie", mk({1: [100], 2: [100], 3: [101], 4: [101]}),
                [(1, 0, [101], [0], _exp([3], [100], [2], [2], [2], [0], 1))],
                ({1: [101], 2: [101], 3: [101], 4: [101]}, {100})))
    out.append(("3 in the keyframe against 2", mk({1: [100], 2: [100], 3: [100], 4: [101], 5: [101]}),
                [(1, 0, [101], [0], _exp([2], [100], [2], [3], [2], [0], 1))],
                ({1: [100], 2: [100], 3: [100], 4: [100], 5: [100]}, {101})))
    out.append(("2 in the keyframe against 3", mk({1: [100], 2: [100], 3: [101], 4: [101], 5: [101]}),
                [(1, 0, [101], [0], _exp([3], [100], [3], [2], [2], [0], 1))],
                ({1: [101], 2: [101], 3: [101], 4: [101], 5: [101]}, {100})))
    # the loser 101 is seen by 2 and 4, the winner 100 by 1, 2, 3: the observation in 2 is erased, the one in 4 moves
    out.append(("observers partly shared", mk({1: [100, -1], 2: [100, 101], 3: [100, -1], 4: [-1, 101]}),
                [(1, 0, [101], [0], _exp([2], [100], [2], [3], [1], [1], 1))],
                ({1: [100, -1], 2: [100, -1], 3: [100, -1], 4: [-1, 100]}, {101})))
    # 101 is added (1 -> 2 observations); 102 then meets it: 2 against 2, 101 goes and takes its fresh observation along
    out.append(("two candidates on one empty keypoint", mk({1: [-1], 2: [101], 3: [102], 4: [102]}),
                [(1, 0, [101, 102], [0, 0], _exp([1, 3], [-1, 101], [1, 2], [0, 2], [0, 2], [0, 0], 2))],
                ({1: [102], 2: [102], 3: [102], 4: [102]}, {101})))
    # mode 1: both candidates note 100; pass 2 replaces it by 101, then once more by 102 with nothing left to move
    out.append(("two candidates on one occupied keypoint, mode 1", mk({1: [100], 2: [100], 3: [101], 4: [102]}),
                [(1, 1, [101, 102], [0, 0], _exp([3, 3], [100, 100], [1, 1], [2, 0], [2, 0], [0, 0], 2))],
                ({1: [101], 2: [101], 3: [101], 4: [102]}, {100})))
    # mode 1: pass 1 puts 101 at the empty keypoint, 102 notes it, pass 2 replaces it
    out.append(("mode 1 replaces what pass 1 added", mk({1: [-1], 2: [101], 3: [102]}),
                [(1, 1, [101, 102], [0, 0], _exp([1, 3], [-1, 101], [1, 1], [0, 2], [0, 2], [0, 0], 2))],
                ({1: [102], 2: [102], 3: [102]}, {101})))
    # 101 (2) beats 100 (1) and has 3; 102 (4) beats 101 (3) and has 7; 103 (1) loses to 102 (7): every winner but the last loses later
    chain = {1: [100], 2: [101], 3: [101], 4: [102], 5: [102], 6: [102], 7: [102], 8: [103]}
    out.append(("a chain of depth 3", mk(chain),
                [(1, 0, [101, 102, 103], [0, 0, 0], _exp([3, 3, 2], [100, 101, 102], [2, 4, 1], [1, 3, 7], [1, 3, 1], [0, 0, 0], 3))],
                ({k: [102] for k in range(1, 9)}, {100, 101, 103})))
    out.append(("the entry's point is flagged bad", mk({1: [100], 2: [101]}, bad_points=[100]),
                [(1, 0, [101], [0], _exp([4], [100], [1], [1], [0], [0], 1)), (1, 1, [101], [0], _exp([4], [100], [1], [1], [0], [0], 1))],
                ({1: [100], 2: [101]}, {100})))
    # the first call replaces 101 by 100 (2 > 1); in the second 101 is bad at its turn
    out.append(("a candidate that turned bad in an earlier call", mk({1: [100, -1], 2: [100, -1], 3: [101, -1]}),
                [(1, 0, [101], [0], _exp([2], [100], [1], [2], [1], [0], 1)), (1, 0, [101], [1], _exp([7], [-1], [0], [0], [0], [0], 0))],
                ({1: [100, -1], 2: [100, -1], 3: [100, -1]}, {101})))
    out.append(("a candidate already in the keyframe", mk({1: [100, -1], 2: [100]}),
                [(1, 0, [100], [1], _exp([7], [-1], [0], [0], [0], [0], 0)), (1, 1, [100], [1], _exp([7], [-1], [0], [0], [0], [0], 0))],
                ({1: [100, -1], 2: [100]}, set())))
    out.append(("mode 2: the matched point is the keyframe's own", mk({1: [100], 2: [100]}),
                [(1, 2, [100], [0], _exp([5], [100], [2], [2], [0], [0], 1))],
                ({1: [100], 2: [100]}, set())))
    # mode 2 has no comparison: 100 (3 observations) goes for 101 (2); keyframe 2 already holds 101, so that observation is erased
    out.append(("mode 2: replace without a comparison", mk({1: [100, -1], 2: [100, 101], 3: [-1, 101], 4: [100, -1]}),
                [(1, 2, [101], [0], _exp([3], [100], [2], [3], [2], [1], 1))],
                ({1: [101, -1], 2: [-1, 101], 3: [-1, 101], 4: [101, -1]}, {100})))
    out.append(("mode 2: an empty entry and a candidate seen elsewhere in the keyframe", mk({1: [100, -1]}),
                [(1, 2, [-1, 100], [-1, 1], _exp([0, 6], [-1, -1], [0, 1], [0, 0], [0, 0], [0, 0], 0))],
                ({1: [100, -1]}, set())))
    out.append(("mode 2: an empty entry takes the point", mk({1: [-1, -1], 2: [100]}),
                [(1, 2, [-1, 100], [-1, 1], _exp([0, 1], [-1, -1], [0, 1], [0, 0], [0, 0], [0, 0], 1))],
                ({1: [-1, 100], 2: [100]}, set())))
    # rows no entry ever named: 500 is added with Observations() == 0; 501 (0) loses to 100 (1) and has nothing to move
    out.append(("candidates no entry ever named", mk({1: [-1, 100]}),
                [(1, 0, [500, 501], [0, 1], _exp([1, 2], [-1, 100], [0, 0], [0, 1], [0, 0], [0, 0], 2))],
                ({1: [500, 100]}, {501})))
    out.append(("n = 0", mk({1: [100]}), [(1, 0, [], [], _exp([], [], [], [], [], [], 0))], ({1: [100]}, set())))
    out.append(("nobody takes a step", mk({1: [100, -1]}), [(1, 0, [-1, 101, -1], [0, -1, -1], _exp([0] * 3, [-1] * 3, [0] * 3, [0] * 3, [0] * 3, [0] * 3, 0))],
                ({1: [100, -1]}, set())))
    return out


def assert_same(got, exp):
    for k in KEYS:
        assert [int(x) for x in got[k]] == [int(x) for x in exp[k]], k
    assert int(got["n_fused"]) == int(exp["n_fused"])


def random_fuse_case(shape, seed, mode):
    """-> (CullingMap, kf, cand, best_idx): culling_cases.random_case at `shape`, the middle keyframe as target.  Modes 0 and 1: the
    candidates are a permutation of up to 3 n_kp points that have observations plus 4 rows never named, best_idx uniform over the row with
    probability 0.6; in front of them a planted chain -- a fresh row for an empty keypoint, then the least and the most observed point
    outside the keyframe for the same keypoint (the second beats the first, the third the second when it has more observations).
    Mode 2: cand[i] for keypoint i of the first n_kp of that list with probability 0.6, and planted: two keypoints whose own point is
    the candidate (action 5) and an empty keypoint with a candidate the keyframe holds elsewhere (action 6)."""
    n_kf, n_kp, n_points, fill = shape
    m, _ = random_case(n_kf, n_kp, n_points, seed, fill)
    rng = np.random.default_rng(9000 + seed)
    kfs = sorted(m.kf_points)
    kf = kfs[len(kfs) // 2]
    row = m.kf_points[kf]
    named = sorted(p for p in m.obs if m.obs[p])
    fresh0 = max(max(named), max(m.pt_bad | {0})) + 1000
    n_cand = min(len(named), 3 * n_kp)
    cand = [int(x) for x in rng.permutation(named)[:n_cand]] + [fresh0 + i for i in range(4)]
    best = [int(rng.integers(0, n_kp)) if rng.uniform() < 0.6 else -1 for _ in cand]
    if mode == 2:
        cand = cand[:n_kp]
        cand += [-1] * (n_kp - len(cand))
        best = [i if cand[i] >= 0 and rng.uniform() < 0.6 else -1 for i in range(n_kp)]
        occupied = [i for i in range(n_kp) if row[i] >= 0]
        empty = [i for i in range(n_kp) if row[i] < 0]

        def plant(i, p):
            for k in range(n_kp):
                if cand[k] == p:
                    cand[k], best[k] = -1, -1
            cand[i], best[i] = p, i
        for i in occupied[-2:]:
            plant(i, row[i])
        if empty and len(occupied) > 2:
            plant(empty[-1], row[occupied[0]])
        return m, kf, cand, best
    outside = sorted((p for p in named if kf not in m.obs[p] and p not in m.pt_bad), key=lambda p: (observations(m, p), p))
    empty = [i for i in range(n_kp) if row[i] < 0]
    if empty and len(outside) >= 2:
        chain = [fresh0 + 4, outside[0], outside[-1]]
        keep = [(c, b) for c, b in zip(cand, best) if c not in chain]
        cand = chain + [c for c, _ in keep]
        best = [empty[0]] * 3 + [b for _, b in keep]
    return m, kf, cand, best


def random_cases(mode, seeds=(1, 2)):
    return [random_fuse_case(shape, seed, mode) for shape in RANDOM_SHAPES for seed in seeds]


def stats(cand, best, out):
    """what the non-degeneracy test counts for one call: the outcomes, collisions (a step at a keypoint an earlier step of the call
    used), steps with a dropped observation, chains (a Replace whose loser won an earlier Replace of the call)"""
    codes = {}
    for a in out["action"]:
        codes[int(a)] = codes.get(int(a), 0) + 1
    used, collisions, won, chains = set(), 0, set(), 0
    for c, b, a, o in zip(cand, best, out["action"], out["other"]):
        if a in (1, 2, 3):
            collisions += b in used
            used.add(b)
        if a in (2, 3):
            loser, winner = (c, o) if a == 2 else (o, c)
            chains += loser in won
            won.add(winner)
    return dict(codes=codes, collisions=collisions, drops=sum(1 for d in out["n_dropped"] if d > 0), chains=chains)


def problem_text(m, calls):
    """the problem file of host/test_fuse_apply_rule: the map (rows and bad points), then `calls` = [(kf, mode, cand, best_idx, apply)]"""
    out = [f"{len(m.kf_points)} {len(m.pt_bad)}"]
    for kf in sorted(m.kf_points):
        out.append(f"{kf} {len(m.kf_points[kf])}")
        out.append(" ".join(str(int(x)) for x in m.kf_points[kf]))
    out.append(" ".join(str(p) for p in sorted(m.pt_bad)))
    out.append(str(len(calls)))
    for kf, mode, cand, best, apply in calls:
        out.append(f"{kf} {mode} {len(cand)} {int(apply)}")
        out.append(" ".join(str(int(x)) for x in cand))
        out.append(" ".join(str(int(x)) for x in best))
    return "\n".join(out) + "\n"
