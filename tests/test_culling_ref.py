"""tests/culling_ref.py, the yardstick of asd_keyframe_culling and asd_map_observations, pinned on maps small enough to work by hand
against LocalMapping.cc:739-809, KeyFrame.cc:723-741 and MapPoint.cc:119-142, :180-197: the expected numbers are written out in
tests/culling_cases.hand_cases and, for the state a cull leaves, below."""
import pytest

from tests.culling_cases import RANDOM_SHAPES, hand_cases, mk, random_case, without_erasure
from tests.culling_ref import CullingMap

CASES = hand_cases()


@pytest.mark.parametrize("name,m,cand,flags,exp", CASES, ids=[c[0] for c in CASES])
def test_hand_worked_map(name, m, cand, flags, exp):
    before = (m._copy().kf_points, set(m.kf_bad), set(m.pt_bad))
    r = m.keyframe_culling(cand, flags, False)
    assert (r["decision"], r["n_mps"], r["n_redundant"], r["bad_rows"]) == exp
    assert (m.kf_points, m.kf_bad, m.pt_bad) == before                   # apply = 0 leaves the map as it was
    r = m.keyframe_culling(cand, flags, True)
    assert (r["decision"], r["n_mps"], r["n_redundant"], r["bad_rows"]) == exp
    for kf, d in zip(cand, r["decision"]):
        if d == 1:
            assert kf in m.kf_bad and all(p == -1 for p in m.kf_points[kf])
        else:
            assert kf not in m.kf_bad
    for p in r["bad_rows"]:
        assert p in m.pt_bad and not m.obs[p] and all(p not in row for row in m.kf_points.values())


def test_the_cases_cover_what_they_are_named_for():
    by = {c[0]: c[4] for c in CASES}
    assert by["octave L+1"][0] != by["octave L+2"][0] and by["octave 14 under 15"][0] != by["octave 13 under 15"][0]
    assert by["observations 3"][0] == [0] and by["observations 4"][0] == [1]
    assert by["order 6 7"][0] == by["order 7 6"][0] == [1, 0]           # the same pair in both orders: the first one goes
    assert by["not erase"][0] == [2, 1]
    assert by["cascade"][0] == [1, 1] and by["no cascade"][0] == [0]    # 11 is culled only behind 10


def test_state_after_the_cascade():
    name, m, cand, flags, _ = [c for c in CASES if c[0] == "cascade"][0]
    m.keyframe_culling(cand, flags, True)
    assert m.kf_bad == {10, 11} and m.pt_bad == {200}
    assert m.kf_points[12] == [-1] and m.kf_points[10] == [-1] * 11 and m.kf_points[11] == [-1] * 10
    assert m.kf_points[20] == list(range(300, 310)) + list(range(320, 329))
    assert m.observations([200, 300, 320, 999]) == [0, 4, 4, 0]
    assert m.octave[10] == [0] * 11                                      # a culled keyframe keeps its octaves
    again = m.keyframe_culling([10, 11, 12], [0, 0, 0], True)
    assert again["decision"] == [0, 0, 0] and again["n_mps"] == [0, 0, 0] and again["bad_rows"] == []


def test_mb_not_erase_erases_nothing():
    m = mk({5: [100], 6: [100], 7: [100], 8: [100]})
    m.keyframe_culling([6], [2], True)
    assert m.observations([100]) == [4] and not m.kf_bad and m.kf_points[6] == [100]


def test_bad_point_with_entries_keeps_them_elsewhere():
    name, m, cand, flags, _ = [c for c in CASES if c[0] == "bad and empty"][0]
    r = m.keyframe_culling(cand, flags, True)
    assert r["bad_rows"] == [] and m.kf_points[1] == [-1, -1, -1] and m.kf_points[2] == [100, 101]
    assert m.observations([100, 101]) == [3, 1]


def test_octave_lifetime():
    m = mk({1: [100, 101], 2: [100]})
    m.put_keyframe(1, [102, -1])                                        # the same n keeps the octaves
    assert m.octave[1] == [0, 0]
    m.put_keyframe(1, [102])
    assert 1 not in m.octave
    m.erase_keyframe(2)
    assert 2 not in m.octave and isinstance(m, CullingMap)


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_random_generator_is_not_degenerate(seed):
    """what tests/test_culling.py relies on: culls in every shape, cascaded bad points, and outcomes that depend on the in-loop erasure"""
    cascades = order_dependent = 0
    for n_kf, n_kp, n_points, fill in RANDOM_SHAPES:
        m, cand = random_case(n_kf, n_kp, n_points, seed, fill)
        r = m.keyframe_culling(cand, [0] * len(cand), False)
        assert sum(d == 1 for d in r["decision"]) >= 2
        cascades += len(r["bad_rows"]) > 0
        order_dependent += [int(d == 1) for d in r["decision"]] != without_erasure(m, cand)
    assert cascades >= 1 and order_dependent >= 1
