"""asd_match_bow_kf (ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, ...), ORBmatcher.cc:533-666) on the device against the numpy
restatement tests/loop_ref.py: every match id and the count must be equal -- on the hand-built cases of tests/test_loop_ref.py (one
per rule that separates this overload from the KeyFrame-Frame one) and on two synthetic keyframes of 300 and 2000 keypoints over a
20-node and a 200-node feature vector, with map-point masks on both sides and keypoints the vocabulary did not place.
"""
import numpy as np
import pytest

from tests import loop_ref
from tests.test_loop_ref import hand_cases, run_ref
from tests.test_matcher import BOUNDS, _two_views

pytestmark = pytest.mark.gpu
HAND = hand_cases()


def run_hip(hip, c, slots=(6, 7)):
    (k1, d1), (k2, d2) = c["kf1"], c["kf2"]
    hip.frame_set(slots[0], k1, d1, BOUNDS)
    hip.frame_set(slots[1], k2, d2, BOUNDS)
    return hip.match_bow_kf(slots[0], slots[1], len(k1), np.asarray(c["nodes1"], np.int32), np.asarray(c["nodes2"], np.int32), c["has1"], c["has2"],
                            c["nn_ratio"], c["ori"])


@pytest.mark.parametrize("name", sorted(HAND))
def test_hip_match_bow_kf_hand_cases(hip, oracle, name):
    c = HAND[name]
    got, n = run_hip(hip, c)
    exp, ne = run_ref(oracle, c)
    assert exp.tolist() == c["expect"] and ne == c["n"]
    np.testing.assert_array_equal(got, exp)
    assert n == ne


def test_hip_match_bow_overloads_differ_at_the_threshold(hip):
    """squared distance exactly TH_LOW: the KeyFrame-Frame overload (<=, :231) matches, this one (<, :609) does not"""
    c = HAND["threshold"]
    got, n = run_hip(hip, c)
    assert n == 0 and got.tolist() == [-1]
    m, nm = hip.match_bow(6, 7, 1, np.asarray(c["nodes1"], np.int32), np.asarray(c["nodes2"], np.int32), c["has1"], c["nn_ratio"], c["ori"])
    assert nm == 1 and m.tolist() == [0]


@pytest.mark.parametrize("n,n_nodes,ori", [(300, 20, True), (2000, 200, True), (2000, 20, False)])
def test_hip_match_bow_kf_synthetic(hip, oracle, n, n_nodes, ori):
    k1, d1, k2, d2, perm, _ = _two_views(n, 900 + n + n_nodes)
    rng = np.random.default_rng(n + n_nodes)
    # nodes: true matches mostly share one (a tenth is moved elsewhere), some keypoints are not placed at all
    nodes1 = rng.integers(0, n_nodes, n).astype(np.int32)
    nodes2 = nodes1[perm].copy()
    moved = rng.uniform(size=n) < 0.1
    nodes2[moved] = rng.integers(0, n_nodes, int(moved.sum()))
    nodes1[::17] = -1
    nodes2[5::23] = -1
    has1 = (rng.uniform(size=n) < 0.7).astype(np.uint8)
    has2 = (rng.uniform(size=n) < 0.7).astype(np.uint8)
    c = dict(kf1=(k1, d1), kf2=(k2, d2), nodes1=nodes1, nodes2=nodes2, has1=has1, has2=has2, nn_ratio=0.85, ori=ori)
    got, ng = run_hip(hip, c)
    exp, ne = run_ref(oracle, c)
    np.testing.assert_array_equal(got, exp)
    assert ng == ne == int((exp >= 0).sum()) and ng > 0.2 * n
    assert len(np.unique(nodes1[nodes1 >= 0])) == n_nodes
    ok = np.nonzero(exp >= 0)[0]
    assert has1[ok].all() and has2[exp[ok]].all() and len(np.unique(exp[ok])) == len(ok)      # masks respected, no point of keyframe 2 twice
    inv = np.empty_like(perm)
    inv[perm] = np.arange(n)
    assert (exp[ok] == inv[ok]).mean() > 0.9
