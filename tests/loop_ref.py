"""numpy restatement of ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)
(ORBmatcher.cc:533-666), for tests/test_match_bow_kf.py.  Written from the reference's source text; the descriptor distances come in
from outside (the oracle's dist_matrix: DescriptorDistance in f32, component order 0..127), everything else is here:

  node join     (:561-643)  both feature vectors in ascending node id; a node present in one only is skipped (lower_bound)
  query gate    (:569-573)  keyframe 1's keypoint needs a map point that is not bad (has_mp1)
  candidate gate(:587-591)  keyframe 2's keypoint must not have been taken (vbMatched2) and needs a map point that is not bad
  best / second (:597-606)  first strict minimum from 256, second from 256
  threshold     (:609)      bestDist1 < TH_LOW, STRICT (the KeyFrame-Frame overload at :231 has <=)
  ratio         (:611)      bestDist1 < mfNNratio * bestDist2 in f32
  claim         (:613-614)  vpMatches12[idx1] = the point of idx2; vbMatched2[idx2] = true, in visiting order
  histogram     (:616-626)  rot = angle1 - angle2 (+360 if negative), bin = round(rot / 30) mod 30, holds idx1
  three maxima  (:645-663)  ComputeThreeMaxima (:1454-1510): matches outside the three fullest bins are removed; the second / third
                            bin counts only if it holds at least a tenth of the first

A keypoint index is taken from keyframe 1's feature vector at most once (DBoW2 puts a feature under one node).
"""
import math

import numpy as np

F32 = np.float32
TH_LOW = F32(0.5)        # ORBmatcher.cc:38
HISTO_LENGTH = 30        # ORBmatcher.cc:39


def feature_vector(node_of_kp):
    """node id per keypoint (-1 = none) -> [(node id, [keypoint indices ascending])] in ascending node id (DBoW2::FeatureVector)"""
    node_of_kp = np.asarray(node_of_kp)
    return [(int(nid), [int(i) for i in np.nonzero(node_of_kp == nid)[0]]) for nid in np.unique(node_of_kp[node_of_kp >= 0])]


def three_maxima(counts):
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(counts):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if F32(max2) < F32(0.1) * F32(max1):
        ind2 = ind3 = -1
    elif F32(max3) < F32(0.1) * F32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def rot_bin(angle1, angle2):
    rot = F32(angle1) - F32(angle2)
    if rot < 0.0:
        rot = F32(rot + F32(360.0))
    x = float(F32(rot * F32(1.0 / HISTO_LENGTH)))
    b = int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))   # C round(): half away from zero
    return 0 if b == HISTO_LENGTH else b


def search_by_bow_kf(dist, nodes1, nodes2, has_mp1, has_mp2, angle1, angle2, nn_ratio=0.85, check_orientation=True):
    """dist[n1][n2] f32; returns (match12[n1] = index in keyframe 2 or -1, nmatches)"""
    n1, n2 = len(nodes1), len(nodes2)
    match12 = np.full(n1, -1, np.int32)
    matched2 = np.zeros(n2, bool)
    hist = [[] for _ in range(HISTO_LENGTH)]
    fv2 = dict(feature_vector(nodes2))
    nmatches = 0
    for nid, members1 in feature_vector(nodes1):
        if nid not in fv2:
            continue
        for idx1 in members1:
            if not has_mp1[idx1]:
                continue
            best1 = best2 = F32(256)
            best_idx = -1
            for idx2 in fv2[nid]:
                if matched2[idx2] or not has_mp2[idx2]:
                    continue
                d = F32(dist[idx1, idx2])
                if d < best1:
                    best2, best1, best_idx = best1, d, idx2
                elif d < best2:
                    best2 = d
            if best1 < TH_LOW and best1 < F32(nn_ratio) * best2:
                match12[idx1] = best_idx
                matched2[best_idx] = True
                if check_orientation:
                    hist[rot_bin(angle1[idx1], angle2[best_idx])].append(idx1)
                nmatches += 1
    if check_orientation:
        keepers = three_maxima([len(h) for h in hist])
        for b in range(HISTO_LENGTH):
            if b in keepers:
                continue
            for idx1 in hist[b]:
                match12[idx1] = -1
                nmatches -= 1
    return match12, nmatches
