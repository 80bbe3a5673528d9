"""Known answers for tests/loop_ref.py, the numpy restatement of ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, ...)
(ORBmatcher.cc:533-666): hand-built keyframes whose result can be read off the source, one per rule that separates this overload
from the KeyFrame-Frame one.  Distances come from the oracle's dist_matrix (DescriptorDistance: the squared distance, f32).
tests/test_match_bow_kf.py runs the same cases, and larger ones, on the device against the restatement.
"""
import numpy as np

from tests import loop_ref
from tests.conftest import load_package


def vec(**kv):
    """a 128-float descriptor, zero but for d<k> = value"""
    d = np.zeros(128, np.float32)
    for k, v in kv.items():
        d[int(k[1:])] = v
    return d


def keyframe(descs, angles=None):
    KP = load_package().capi.KP_DTYPE
    n = len(descs)
    kps = np.zeros(n, KP)
    kps["x"] = 100 + 10 * np.arange(n)
    kps["y"] = 100
    kps["size"] = 31
    kps["response"] = 50
    kps["angle"] = 0 if angles is None else np.asarray(angles, np.float32)
    return kps, np.stack(descs).astype(np.float32)


def pairs(m):
    """m keypoints per keyframe, keypoint k of one matching keypoint k of the other only (distance 0.0004; 2 and more to the others)"""
    return [vec(**{f"d{4 * k}": 1.0}) for k in range(m)], [vec(**{f"d{4 * k}": 1.0, f"d{4 * k + 1}": 0.02}) for k in range(m)]


def hand_cases():
    """name -> dict(kf1, kf2 = (kps, desc), nodes1, nodes2, has1, has2, nn_ratio, ori, expect = match12, n = return value)"""
    out = {}
    ones = lambda n: np.ones(n, np.uint8)
    # two idx1 prefer the same idx2: the first in visiting order takes it, the second takes its runner-up (:587, :613-614) ...
    d1 = [vec(d0=1.0), vec(d0=1.0, d1=0.1)]
    d2 = [vec(d0=1.0, d2=0.02), vec(d0=1.0, d3=0.3)]
    out["contested"] = dict(kf1=keyframe(d1), kf2=keyframe(d2), nodes1=[7, 7], nodes2=[7, 7], has1=ones(2), has2=ones(2), nn_ratio=0.85, ori=False,
                            expect=[0, 1], n=2)
    # ... or nothing, where the runner-up has no map point
    out["contested_nothing"] = dict(out["contested"], has2=np.array([1, 0], np.uint8), expect=[0, -1], n=1)
    # a duplicate descriptor in keyframe 2: the strict `dist < bestDist1` keeps the first; the copy becomes the second best, so the
    # pair survives only a ratio above 1
    dup = [vec(d0=1.0, d2=0.02), vec(d0=1.0, d2=0.02)]
    out["duplicate"] = dict(kf1=keyframe([vec(d0=1.0)]), kf2=keyframe(dup), nodes1=[3], nodes2=[3, 3], has1=ones(1), has2=ones(2), nn_ratio=1.2,
                            ori=False, expect=[0], n=1)
    out["duplicate_ratio"] = dict(out["duplicate"], nn_ratio=0.85, expect=[-1], n=0)
    # squared distance exactly 0.5 = TH_LOW: matches under `<=` (the KeyFrame-Frame overload, :231), must not match under `<` (:609)
    out["threshold"] = dict(kf1=keyframe([vec(d0=1.0)]), kf2=keyframe([vec(d0=0.5, d1=0.5)]), nodes1=[5], nodes2=[5], has1=ones(1), has2=ones(1),
                            nn_ratio=0.85, ori=False, expect=[-1], n=0)
    out["below_threshold"] = dict(out["threshold"], kf2=keyframe([vec(d0=0.5, d1=0.4375)]), expect=[0], n=1)
    # masks: a query without a map point is not visited; a candidate without one is passed over for the next best
    a, b = pairs(3)
    b2 = b + [vec(d0=1.0, d3=0.3)]          # a second, worse candidate for keypoint 0
    out["mask1"] = dict(kf1=keyframe(a), kf2=keyframe(b2), nodes1=[1, 1, 1], nodes2=[1, 1, 1, 1], has1=np.array([1, 0, 1], np.uint8), has2=ones(4),
                        nn_ratio=0.85, ori=False, expect=[0, -1, 2], n=2)
    out["mask2"] = dict(out["mask1"], has1=ones(3), has2=np.array([0, 1, 1, 1], np.uint8), expect=[3, 1, 2], n=3)
    # disjoint node sets, and a node of one keyframe between two shared ones (the lower_bound branches of the join)
    out["disjoint"] = dict(kf1=keyframe(a), kf2=keyframe(b), nodes1=[1, 1, 1], nodes2=[2, 2, 2], has1=ones(3), has2=ones(3), nn_ratio=0.85, ori=False,
                           expect=[-1, -1, -1], n=0)
    out["join_skips"] = dict(kf1=keyframe(a), kf2=keyframe(b), nodes1=[1, 4, 9], nodes2=[1, 6, 9], has1=ones(3), has2=ones(3), nn_ratio=0.85, ori=False,
                             expect=[0, -1, 2], n=2)
    out["unplaced"] = dict(out["join_skips"], nodes1=[1, -1, 9], nodes2=[1, 9, 9], expect=[0, -1, 2], n=2)
    # orientation: bins 0 / 3 / 6 / 9 / 12 hold 4 / 4 / 3 / 2 / 1 matches -> the two of bin 9 and the one of bin 12 go; rot < 0 wraps (+360)
    a, b = pairs(14)
    rot = [0] * 5 + [90] * 4 + [180] * 3 + [270] * 2
    ang2 = np.array([20.0] * 14, np.float32)
    ang1 = (ang2 + np.array(rot, np.float32)) % 360
    ang1[0], ang2[0] = 10.0, 12.0           # rot = -2 -> 358 -> bin 12
    nodes = [k % 3 for k in range(14)]
    exp_on = list(range(14))
    exp_on[0] = exp_on[12] = exp_on[13] = -1
    out["orientation_on"] = dict(kf1=keyframe(a, ang1), kf2=keyframe(b, ang2), nodes1=nodes, nodes2=nodes, has1=ones(14), has2=ones(14), nn_ratio=0.85,
                                 ori=True, expect=exp_on, n=11)
    out["orientation_off"] = dict(out["orientation_on"], ori=False, expect=list(range(14)), n=14)
    # the tenth rule (:1616): 11 matches in one bin, 1 in another -> 1 < 0.1f * 11: the second bin does not count
    a, b = pairs(12)
    ang1 = np.array([50.0] * 11 + [140.0], np.float32)
    out["orientation_tenth"] = dict(kf1=keyframe(a, ang1), kf2=keyframe(b, np.full(12, 50.0, np.float32)), nodes1=[0] * 12, nodes2=[0] * 12, has1=ones(12),
                                    has2=ones(12), nn_ratio=0.85, ori=True, expect=list(range(11)) + [-1], n=11)
    return out


def run_ref(oracle, c):
    (k1, d1), (k2, d2) = c["kf1"], c["kf2"]
    return loop_ref.search_by_bow_kf(oracle.dist_matrix(d1, d2), c["nodes1"], c["nodes2"], c["has1"], c["has2"], k1["angle"], k2["angle"],
                                     c["nn_ratio"], c["ori"])


def test_loop_ref_known_answers(oracle):
    for name, c in hand_cases().items():
        got, n = run_ref(oracle, c)
        assert got.tolist() == c["expect"] and n == c["n"], (name, got.tolist(), n)


def test_loop_ref_threshold_case_sits_exactly_on_th_low(oracle):
    c = hand_cases()["threshold"]
    assert oracle.dist_matrix(c["kf1"][1], c["kf2"][1])[0, 0] == loop_ref.TH_LOW == np.float32(0.5)
    c = hand_cases()["below_threshold"]
    assert oracle.dist_matrix(c["kf1"][1], c["kf2"][1])[0, 0] < loop_ref.TH_LOW


def test_loop_ref_bins_and_maxima():
    assert loop_ref.rot_bin(10.0, 12.0) == 12 and loop_ref.rot_bin(20.0, 20.0) == 0 and loop_ref.rot_bin(45.0, 0.0) == 2   # 1.5 rounds away from zero
    assert loop_ref.rot_bin(44.9, 0.0) == 1 and loop_ref.rot_bin(359.9, 0.0) == 12
    assert loop_ref.three_maxima([0, 5, 0, 4, 3, 2]) == (1, 3, 4)
    assert loop_ref.three_maxima([11, 1, 0]) == (0, -1, -1)
    assert loop_ref.three_maxima([20, 2, 1]) == (0, 1, -1)      # 2 >= 0.1f * 20, 1 < 0.1f * 20
    assert loop_ref.three_maxima([0, 0, 0]) == (-1, -1, -1)
    assert loop_ref.feature_vector([3, -1, 1, 3]) == [(1, [2]), (3, [0, 3])]
