"""Cases shared by the LocalBA graph tests: hand-worked maps with every expected list written out (tests/test_local_ba_graph_ref.py pins
the restatement on them, tests/test_local_ba_graph.py runs the device on them), and the helpers that compare a result with an expectation."""
from tests.culling_cases import mk

GRAPH_KEYS = ("local_kfs", "local_rows", "fixed_kfs", "pose_kfs", "pose_fixed", "point_rank", "e_point", "e_pose", "e_kf", "e_idx", "e_octave")
ERASE_KEYS = ("n_erased", "bad_rows", "new_ref")


def assert_graph(got, exp, what=""):
    for k in GRAPH_KEYS:
        assert [int(x) for x in got[k]] == [int(x) for x in exp[k]], f"{what}: {k}"


def assert_erase(got, exp, what=""):
    assert int(got["n_erased"]) == int(exp["n_erased"]), f"{what}: n_erased"
    for k in ("bad_rows", "new_ref"):
        assert [int(x) for x in got[k]] == [int(x) for x in exp[k]], f"{what}: {k}"


def _lists():
    """Keyframe 10 with the neighbours 8 (bad), 7, 99 (not in the table) and 12 (a row without a point).
    local rows: 10 gives 105, then -1, then 101, then 103 which is bad; 7 gives 101 again (taken once), 102, 104.
    fixed: 105 is seen by 8 (a neighbour: stamped local although bad), 10, 30 -> 30; 101 by 7, 10, 20, 40 -> 20, and 40 is bad;
    102 by 5, 7 -> 5; 104 by 7, 20.  So lFixedCameras = 30, 20, 5 and the pose order 5, 7, 10, 12, 20, 30, 99.
    rows sorted: 101, 102, 104, 105, so 105 has rank 3."""
    m = mk({10: [105, -1, 101, 103], 7: [101, 102, 104], 8: [105, 106], 12: [-1, -1], 30: [103, 105], 20: [104, 101], 5: [102], 40: [101]},
           {10: [1, 0, 2, 3], 7: [0, 1, 2], 8: [4, 5], 12: [0, 0], 30: [1, 1], 20: [2, 2], 5: [6], 40: [7]}, bad_points=[103])
    m.kf_bad |= {8, 40}
    exp = dict(local_kfs=[10, 7, 99, 12], local_rows=[105, 101, 102, 104], fixed_kfs=[30, 20, 5],
               pose_kfs=[5, 7, 10, 12, 20, 30, 99], pose_fixed=[1, 0, 0, 0, 1, 1, 0], point_rank=[3, 0, 1, 2],
               #        105 -------  101 ----------  102 ---  104 ---
               e_point=[3, 3,        0, 0, 0,        1, 1,    2, 2],
               e_kf=[10, 30,         7, 10, 20,      5, 7,    7, 20],
               e_pose=[2, 5,         1, 2, 4,        0, 1,    1, 4],
               e_idx=[0, 1,          0, 2, 1,        0, 1,    2, 0],
               e_octave=[1, 1,       0, 2, 2,        6, 1,    2, 2])
    return dict(name="lists", map=m, kf=10, neigh=[8, 7, 99, 12], graph=exp, observations={105: 3, 101: 4, 102: 2, 104: 2, 106: 1})


def _alone():
    """a keyframe without neighbours whose only point nobody else sees; and nothing at all in its row"""
    m = mk({3: [-1, 50], 4: [-1]}, {3: [0, 2], 4: [0]})
    one = dict(local_kfs=[3], local_rows=[50], fixed_kfs=[], pose_kfs=[3], pose_fixed=[0], point_rank=[0], e_point=[0], e_pose=[0], e_kf=[3],
               e_idx=[1], e_octave=[2])
    none = dict(local_kfs=[4], local_rows=[], fixed_kfs=[], pose_kfs=[4], pose_fixed=[0], point_rank=[], e_point=[], e_pose=[], e_kf=[],
                e_idx=[], e_octave=[])
    return [dict(name="alone", map=m, kf=3, neigh=[], graph=one, observations={50: 1}),
            dict(name="empty row", map=m, kf=4, neigh=[], graph=none, observations={})]


def graph_cases():
    return [_lists()] + _alone()


def _erase_map():
    """Keyframe 1 with the neighbour 2; 3, 4, 5 come out fixed; 6 is bad and sees 203.
    200: seen by 1 2 3 4      201, 202: by 1 2 3      203: by 1 2 3 and the bad 6      204: by 1 2 3 4 5"""
    pts = [200, 201, 202, 203, 204]
    m = mk({1: pts, 2: pts, 3: pts, 4: [200, 204], 5: [204], 6: [203]})
    m.kf_bad.add(6)
    g = dict(local_kfs=[1, 2], local_rows=pts, fixed_kfs=[3, 4, 5], pose_kfs=[1, 2, 3, 4, 5], pose_fixed=[0, 0, 1, 1, 1], point_rank=[0, 1, 2, 3, 4],
             #        200 ---------  201 ------  202 ------  203 ------  204 ------------
             e_point=[0, 0, 0, 0,    1, 1, 1,    2, 2, 2,    3, 3, 3,    4, 4, 4, 4, 4],
             e_kf=[1, 2, 3, 4,       1, 2, 3,    1, 2, 3,    1, 2, 3,    1, 2, 3, 4, 5],
             e_pose=[0, 1, 2, 3,     0, 1, 2,    0, 1, 2,    0, 1, 2,    0, 1, 2, 3, 4],
             e_idx=[0, 0, 0, 0,      1, 1, 1,    2, 2, 2,    3, 3, 3,    4, 4, 4, 1, 0],
             e_octave=[0] * 18)
    return m, g


def erase_cases():
    """-> [dict(name, map, kf, neigh, graph, flagged edges, ref_kf before, expected result, map after, ref_kf after)]
    edge 2 (200, kf 3): 4 observations, 3 left: stays, and its mpRefKF 1 was not erased;
    edge 5 (201, kf 2): 3 observations, 2 left: bad;
    edges 7 and 9 (202, kf 1 and kf 3): the first leaves 2, the point is bad on the spot and the second pair is a no-op: ONE erasure;
    edge 11 (203, kf 2): 4 observations with the bad keyframe's entry, 3 left: stays -- it would be bad were that entry not counted;
    edges 13 and 14 (204, kf 1 and kf 2): mpRefKF 1 goes, the seat moves to 2, 2 goes, the seat ends at 3; 3 left: stays."""
    m, g = _erase_map()
    flagged = [2, 5, 7, 9, 11, 13, 14]
    exp = dict(n_erased=6, bad_rows=[201, 202], new_ref=[1, -1, -1, 1, 3])
    after = {1: [200, -1, -1, 203, -1], 2: [200, -1, -1, -1, -1], 3: [-1, -1, -1, 203, 204], 4: [200, 204], 5: [204], 6: [203]}
    ref0 = {p: 1 for p in g["local_rows"]}
    ref1 = {200: 1, 203: 1, 204: 3}                            # (201 and 202 are bad: their seat is nobody's business)
    out = [dict(name="policy", map=m, kf=1, neigh=[2], graph=g, flagged=flagged, ref_kf=ref0, result=exp, after=after, bad_after=[201, 202],
                ref_after=ref1)]
    m2, g2 = _erase_map()
    out.append(dict(name="nothing flagged", map=m2, kf=1, neigh=[2], graph=g2, flagged=[], ref_kf=dict(ref0),
                    result=dict(n_erased=0, bad_rows=[], new_ref=[-1] * 5), after={k: list(v) for k, v in m2.kf_points.items()}, bad_after=[],
                    ref_after={200: 1, 203: 1, 204: 1}))
    return out


def flags_of(case):
    f = [0] * len(case["graph"]["e_kf"])
    for e in case["flagged"]:
        f[e] = 1
    return f
