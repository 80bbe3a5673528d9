"""A plain sequential Python restatement of the side-effect half of ORBmatcher::Fuse and of MapPoint::Replace, the yardstick of
asd_fuse_apply, asd_map_get and asd_map_points, over tests/culling_ref.CullingMap (kf_points, obs, pt_bad).

  mode 0  Fuse(pKF, vpMapPoints, th), ORBmatcher.cc:842-957 without the search: the gate of :849 at the candidate's turn, then :939-955
  mode 1  Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) :986-1083 (spAlreadyFound is the snapshot of :979) followed by the loop of
          LoopClosing::SearchAndFuse, LoopClosing.cc:619-627
  mode 2  the loop fusion of LoopClosing::CorrectLoop, LoopClosing.cc:540-555
  Replace MapPoint.cc:206-244

Written from those lines.  The ONE thing that is not restated is action 6 (mode 2, an empty entry and a candidate that already observes
the keyframe elsewhere): AddObservation is a no-op there while AddMapPoint would write a second entry of the point into the row, a state
the table cannot hold -- the step is skipped.  The table's precondition (a point at most once per row, rows and observation dicts in
agreement) is asserted after every call.
"""
NO_STEP, ADDED, CAND_REPLACED, KF_POINT_REPLACED, BAD_IN_KF, SELF, SECOND_ENTRY, GATED = range(8)


def check_precondition(m):
    for kf, row in m.kf_points.items():
        named = [p for p in row if p >= 0]
        assert len(named) == len(set(named)), f"a point occurs twice in the row of keyframe {kf}"
        for idx, p in enumerate(row):
            if p >= 0:
                assert m.obs[p][kf] == idx
    for p, o in m.obs.items():
        for kf, idx in o.items():
            assert m.kf_points[kf][idx] == p


def observations(m, p):
    return len(m.obs.get(p, {}))


def replace(m, loser, winner):
    """loser->Replace(winner), MapPoint.cc:206-244 -> (n_moved, n_dropped), or None when both are the same point (:208-209)"""
    if loser == winner:
        return None
    obs = m.obs.get(loser, {})                                 # :216 obs = mObservations
    m.obs[loser] = {}                                          # :217 mObservations.clear()
    m.pt_bad.add(loser)                                        # :218 mbBad = true
    moved = dropped = 0
    for kf in sorted(obs):                                     # :224 (the keyframes of one point are distinct: the order changes nothing)
        idx = obs[kf]
        if kf not in m.obs.setdefault(winner, {}):             # :229 !pMP->IsInKeyFrame(pKF)
            m.kf_points[kf][idx] = winner                      # :231 ReplaceMapPointMatch
            m.obs[winner][kf] = idx                            # :232 AddObservation (no bad test)
            moved += 1
        else:
            m.kf_points[kf][idx] = -1                          # :236 EraseMapPointMatch
            dropped += 1
    return moved, dropped


def _add(m, kf, idx, p):
    m.obs.setdefault(p, {})[kf] = idx                          # pMP->AddObservation(pKF, bestIdx)
    m.kf_points[kf][idx] = p                                   # pKF->AddMapPoint(pMP, bestIdx)


def fuse_apply(m, kf, cand, best_idx, mode, apply):
    """-> dict(action, other, obs_cand, obs_other, n_moved, n_dropped, n_fused); with apply the map is mutated, without it the map is
    left as it was"""
    assert mode in (0, 1, 2) and len(cand) == len(best_idx)
    m = m if apply else m._copy()
    n = len(cand)
    action, other = [NO_STEP] * n, [-1] * n
    obs_cand, obs_other, n_moved, n_dropped = [0] * n, [0] * n, [0] * n, [0] * n
    row = m.kf_points[kf]
    already_found = set(p for p in row if p >= 0)              # ORBmatcher.cc:979
    noted = []                                                 # vpReplacePoint

    def do_replace(i, loser, winner):
        obs_cand[i], obs_other[i] = observations(m, int(cand[i])), observations(m, other[i])
        r = replace(m, loser, winner)
        if r is None:
            action[i] = SELF
        else:
            n_moved[i], n_dropped[i] = r

    for i in range(n):
        p, b = int(cand[i]), int(best_idx[i])
        if p < 0 or b < 0:                                     # null pointer / bestDist > TH_LOW
            continue
        if mode == 0 and (p in m.pt_bad or kf in m.obs.get(p, {})):      # :849
            action[i] = GATED
            continue
        if mode == 1 and (p in m.pt_bad or p in already_found):          # :992
            action[i] = GATED
            continue
        q = row[b]                                             # pKF->GetMapPoint(bestIdx)
        if q < 0:
            obs_cand[i] = observations(m, p)
            if mode == 2 and kf in m.obs.get(p, {}):
                action[i] = SECOND_ENTRY                       # not restated, see the head of the file
                continue
            _add(m, kf, b, p)
            action[i] = ADDED
            continue
        other[i] = q
        if mode == 2:                                          # LoopClosing.cc:548-549: no bad test, no comparison
            action[i] = KF_POINT_REPLACED
            do_replace(i, q, p)
        elif q in m.pt_bad:                                    # :942 / :1073: nothing happens, nFused++
            action[i] = BAD_IN_KF
            obs_cand[i], obs_other[i] = observations(m, p), observations(m, q)
        elif mode == 1:                                        # :1074
            action[i] = KF_POINT_REPLACED
            noted.append(i)
        elif observations(m, q) > observations(m, p):          # :944-945
            action[i] = CAND_REPLACED
            do_replace(i, p, q)
        else:                                                  # :946-947
            action[i] = KF_POINT_REPLACED
            do_replace(i, q, p)
    for i in noted:                                            # LoopClosing.cc:619-627: no test at all
        do_replace(i, other[i], int(cand[i]))
    check_precondition(m)
    n_fused = sum(1 for a in action if ADDED <= a <= SELF)
    return dict(action=action, other=other, obs_cand=obs_cand, obs_other=obs_other, n_moved=n_moved, n_dropped=n_dropped, n_fused=n_fused)


def map_get(m, kf):
    """KeyFrame::GetMapPointMatches()"""
    return list(m.kf_points[kf])


def map_points(m, kfs):
    """the keyframes in the order given, their entries in ascending keypoint index, a point at its first occurrence unless it is -1 or bad:
    vpFuseCandidates (LocalMapping.cc:599-615) -- UpdateLocalPoints' rule; an id that is not in the map contributes nothing"""
    return m.update_local_points([int(k) for k in kfs])


def replaced_pairs(cand, out):
    """(loser, winner) in the order the reference calls Replace with an effect on mpReplaced: what the host owes IncreaseFound /
    IncreaseVisible for.  Mode 1's pairs happen in pass 2, which keeps the list order."""
    pairs = []
    for c, a, o in zip(cand, out["action"], out["other"]):
        if a == CAND_REPLACED:
            pairs.append((int(c), int(o)))
        elif a == KF_POINT_REPLACED:
            pairs.append((int(o), int(c)))
    return pairs
