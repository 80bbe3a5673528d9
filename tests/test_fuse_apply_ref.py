"""tests/fuse_apply_ref.py, the yardstick of asd_fuse_apply, asd_map_get and asd_map_points, pinned on maps small enough to work by hand
(tests/fuse_apply_cases.hand_cases, each expectation worked against the reference lines the restatement cites), and the random cases
shown not to be degenerate."""
from tests import fuse_apply_ref as ref
from tests.fuse_apply_cases import MODE_CODES, assert_same, hand_cases, random_cases, stats


def test_hand_worked_maps():
    names = set()
    for name, m, calls, (rows_after, bad_after) in hand_cases():
        names.add(name)
        for kf, mode, cand, best, want in calls:
            before = (m._copy().kf_points, set(m.pt_bad))
            dry = ref.fuse_apply(m, kf, cand, best, mode, apply=False)
            assert (m.kf_points, m.pt_bad) == before, name        # apply = 0 leaves the map alone
            assert_same(dry, want)
            assert_same(ref.fuse_apply(m, kf, cand, best, mode, apply=True), want)
        assert m.kf_points == rows_after and m.pt_bad == bad_after, name
        for p in set(x for r in rows_after.values() for x in r if x >= 0):
            assert ref.observations(m, p) == sum(r.count(p) for r in rows_after.values()), name
    assert len(names) == len(hand_cases()) >= 14


def test_every_outcome_is_pinned_by_hand():
    seen = {0: set(), 1: set(), 2: set()}
    for _name, _m, calls, _after in hand_cases():
        for _kf, mode, _cand, _best, want in calls:
            seen[mode] |= set(want["action"])
    assert seen[0] >= {0, 1, 2, 3, 4, 7} and seen[1] >= {1, 3, 4, 7} and seen[2] >= {0, 1, 3, 5, 6}


def test_replace_is_literal():
    """MapPoint.cc:206-244 on its own: the self-replace, a winner that is flagged bad and has no observations (modes 1 and 2 have no test)"""
    name, m, calls, _ = [c for c in hand_cases() if c[0] == "observers partly shared"][0]
    assert ref.replace(m, 100, 100) is None and 100 not in m.pt_bad
    assert ref.replace(m, 101, 100) == (1, 1) and 101 in m.pt_bad and ref.observations(m, 101) == 0
    assert ref.replace(m, 100, 101) == (4, 0)                      # everything lands on the bad, empty 101
    assert m.kf_points == {1: [101, -1], 2: [101, -1], 3: [101, -1], 4: [-1, 101]} and m.pt_bad == {100, 101}
    ref.check_precondition(m)


def test_queries():
    name, m, calls, _ = [c for c in hand_cases() if c[0] == "observers partly shared"][0]
    m.pt_bad.add(101)
    assert ref.map_get(m, 2) == [100, 101]
    assert ref.map_points(m, [4, 2, 999, 1]) == [100] and ref.map_points(m, [4]) == [] and ref.map_points(m, []) == []
    assert ref.replaced_pairs([7, 8, 9], dict(action=[2, 1, 3], other=[5, -1, 6])) == [(7, 5), (6, 9)]


def test_random_cases_are_not_degenerate():
    """over the random cases of each mode: every outcome the mode can produce at least 5 times, at least 5 collisions on one keypoint and
    5 steps with a dropped observation (collisions: modes 0 and 1 -- mode 2 names every keypoint once), at least 3 chains in mode 0; the
    precondition holds after every call (asserted inside)"""
    for mode in (0, 1, 2):
        codes, collisions, drops, chains = {}, 0, 0, 0
        for m, kf, cand, best in random_cases(mode):
            out = ref.fuse_apply(m, kf, cand, best, mode, apply=True)
            s = stats(cand, best, out)
            for c, k in s["codes"].items():
                codes[c] = codes.get(c, 0) + k
            collisions += s["collisions"]; drops += s["drops"]; chains += s["chains"]
            again = ref.fuse_apply(m, kf, cand, best, mode, apply=True)   # the second call on the mutated map keeps the precondition too
            assert len(again["action"]) == len(cand)
        assert set(codes) == set(MODE_CODES[mode]), (mode, codes)
        assert all(codes[c] >= 5 for c in MODE_CODES[mode]), (mode, codes)
        assert drops >= 5, (mode, drops)
        if mode != 2:                                                 # (mode 2 is called with best_idx[i] = i: no keypoint is met twice)
            assert collisions >= 5, (mode, collisions)
        if mode == 0:
            assert chains >= 3, chains
