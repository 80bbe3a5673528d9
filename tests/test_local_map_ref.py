"""tests/local_map_ref.py, the yardstick of asd_update_local_map and asd_map_shared_counts, pinned on maps small enough to work by
hand against Tracking.cc:803-841, :871-1015 and KeyFrame.cc:533-637: every expected list below is written out."""
from tests.local_map_ref import RefMap


def _map(kfs):
    m = RefMap()
    for kf, pts in kfs.items():
        m.put_keyframe(kf, pts)
    return m


def test_parent_break_leaves_the_outer_loop():
    """keyframes 1 and 2 are voted; 1 takes its parent 10, and the break at :1004 ends the expansion: 2's covisible 20 is never added"""
    m = _map({1: [100, -1], 2: [-1, 100], 10: [101], 20: [102]})
    m.set_links(1, [], [], 10)
    m.set_links(2, [20], [], -1)
    r = m.update_local_map([100])
    assert r["local_kfs"] == [1, 2, 10] and r["ref_kf"] == 1
    assert r["local_rows"] == [100, 101] and r["search_rows"] == [101]
    # without a parent the same map takes 2's covisible
    m.set_links(1, [], [], -1)
    assert m.update_local_map([100])["local_kfs"] == [1, 2, 20]


def test_expansion_order_covisible_child_parent_and_bad_tests():
    """per keyframe: the first not-bad, not-included covisible (7 is bad, 8 is taken), then the first such child in ascending id (5 is
    included already, 6 is taken), then the parent WITHOUT a bad test (9 is bad and still taken)"""
    m = _map({1: [100], 5: [100, 103], 6: [104], 7: [105], 8: [106], 9: [107, 100]})
    m.kf_bad |= {7, 9}
    m.set_links(1, [7, 8, 6], [6, 5], 9)
    r = m.update_local_map([100])
    # votes: 1, 5 and 9 observe point 100; 9 is bad and skipped from the list, but comes back as 1's parent
    assert r["local_kfs"] == [1, 5, 8, 6, 9] and r["ref_kf"] == 1
    assert r["local_rows"] == [100, 103, 106, 104, 107]
    assert r["search_rows"] == [103, 106, 104, 107]


def test_more_than_80_stop():
    """80 voted keyframes: the first iteration still runs (80 is not > 80) and adds keyframe 0's covisible; then the list holds 81 and
    the pass stops.  81 voted keyframes: nothing is added at all"""
    for n, expected_tail in ((80, [1000]), (81, [])):
        m = _map({k: [5] for k in range(n)})     # one keypoint each, all observing point 5 ...
        for k in range(n):
            m.set_links(k, [1000 + k], [], -1)
        for k in range(n):
            m.put_keyframe(1000 + k, [6 + k])
        r = m.update_local_map([5])
        assert r["local_kfs"] == list(range(n)) + expected_tail
        assert r["ref_kf"] == 0
        assert r["local_rows"] == [5] + [6 + 0] * len(expected_tail)
    # the bound is a parameter: with max_kfs = 3 three voted keyframes take one neighbour and stop
    m = _map({1: [5], 2: [5], 3: [5], 11: [], 12: [], 13: []})
    for k in (1, 2, 3):
        m.set_links(k, [10 + k], [], -1)
    assert m.update_local_map([5], max_kfs=3)["local_kfs"] == [1, 2, 3, 11]
    assert m.update_local_map([5], max_kfs=2)["local_kfs"] == [1, 2, 3]


def test_lowest_id_maximum_and_bad_keyframes():
    """counts 3: 2, 5: 2, 9: 1 -> pKFmax = 3 (the first strictly larger in ascending id); a bad keyframe with the highest count is
    neither listed nor pKFmax"""
    m = _map({5: [100, 101], 3: [101, 100], 9: [-1, 100], 4: [100, 101, 102]})
    r = m.update_local_map([100, 101, -1])
    assert r["local_kfs"] == [3, 4, 5, 9] and r["ref_kf"] == 3
    r = m.update_local_map([100, 101, 102])
    assert r["ref_kf"] == 4
    m.kf_bad.add(4)
    r = m.update_local_map([100, 101, 102])
    assert r["local_kfs"] == [3, 5, 9] and r["ref_kf"] == 3
    assert r["local_rows"] == [101, 100]            # 4's point 102 is gone with it
    # every voted keyframe bad: the list is emptied (:943), no pKFmax
    m.kf_bad |= {3, 5, 9}
    r = m.update_local_map([100], prev_kfs=[3, 5])
    assert r["local_kfs"] == [] and r["ref_kf"] == -1 and r["local_rows"] == []


def test_no_vote_keeps_the_previous_list():
    """nobody votes (no points, or only bad ones): mvpLocalKeyFrames stays the caller's, bad keyframes in it still contribute their
    points (:885 has no bad test), ids the map does not hold contribute none"""
    m = _map({1: [100, 101], 2: [101, 102], 3: [103]})
    m.kf_bad.add(2)
    m.pt_bad.add(100)
    r = m.update_local_map([-1, 100, -1], seen_points=[102], prev_kfs=[2, 77, 1, 2])
    assert r["local_kfs"] == [2, 77, 1, 2] and r["ref_kf"] == -1
    assert r["local_rows"] == [101, 102]            # 100 is bad; 101 is taken at its first occurrence
    assert r["search_rows"] == [101]                # 102 carries mnLastFrameSeen


def test_a_point_held_twice_votes_twice():
    """the frame holds point 100 at two keypoints: keyframe 2 gets two votes and beats keyframe 1's one (a tie would have gone to 1)"""
    m = _map({1: [101], 2: [100]})
    r = m.update_local_map([100, 101, 100])
    assert r["local_kfs"] == [1, 2] and r["ref_kf"] == 2
    assert m.update_local_map([100, 101])["ref_kf"] == 1
    assert r["local_rows"] == [101, 100] and r["search_rows"] == []


def test_search_list_skips_frame_points_and_stage1_outliers():
    m = _map({1: [100, 101, 102, 103, 104]})
    m.pt_bad.add(104)
    r = m.update_local_map([101, -1], seen_points=[103])
    assert r["local_rows"] == [100, 101, 102, 103]
    assert r["search_rows"] == [100, 102]


def test_update_connections_tie_order_and_fallback():
    """weights 2: 16, 3: 16, 4: 20, 5: 3 with th = 15: sorted ascending by (weight, id) and reversed -> 4, then 3 before 2"""
    m = _map({1: list(range(55)), 2: list(range(0, 16)), 3: list(range(16, 32)), 4: list(range(32, 52)), 5: [52, 53, 54]})
    assert m.shared_counts(1) == [(2, 16), (3, 16), (4, 20), (5, 3)]
    assert m.update_connections(1) == ([4, 3, 2], [20, 16, 16])
    # a bad point does not count; the keyframe itself is excluded; bad keyframes are NOT excluded
    m.pt_bad.add(0)
    m.kf_bad.add(3)
    assert m.shared_counts(1) == [(2, 15), (3, 16), (4, 20), (5, 3)]
    assert m.update_connections(1) == ([4, 3, 2], [20, 16, 15])
    # nobody reaches th: the maximum alone, the first strictly larger in ascending id (3 and 4 tie at 5)
    f = _map({1: list(range(13)), 2: [0, 1, 2], 3: [3, 4, 5, 6, 7], 4: [8, 9, 10, 11, 12]})
    assert f.update_connections(1) == ([3], [5])
    # no shared point at all: nothing changes
    assert _map({1: [0], 2: [1]}).update_connections(1) == ([], [])
