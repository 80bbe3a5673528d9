"""A plain Python restatement of the map side of Optimizer::LocalBundleAdjustment, the yardstick of asd_local_ba_graph and
asd_local_ba_apply: the three lists (Optimizer.cc:418-467), the vertices' and edges' structure (:484-593) and the erase policy
(:652-697) with MapPoint::EraseObservation (MapPoint.cc:119-142) and MapPoint::SetBadFlag (:180-197), over tests.culling_ref.CullingMap.

The loops are the reference's sequential ones -- the mnBALocalForKF / mnBAFixedForKF stamps, one erased pair after the other -- not the
closed forms the device may use.  The ONE stated rule of the section holds: every walk over a std::map<KeyFrame*, ...> is in ascending
keyframe id.  A keyframe that a list names but the map does not hold has no points and is not bad.
"""


def graph(m, kf, neigh):
    """-> dict(local_kfs, local_rows, fixed_kfs, pose_kfs, pose_fixed, point_rank, e_point, e_pose, e_kf, e_idx, e_octave)"""
    kf = int(kf)
    ba_local_kf, ba_fixed_kf, ba_local_mp = {}, {}, {}         # mnBALocalForKF, mnBAFixedForKF (keyframes), mnBALocalForKF (points)
    local_kfs = [kf]                                           # :420
    ba_local_kf[kf] = kf                                       # :421
    for nb in neigh:                                           # :425-431
        nb = int(nb)
        ba_local_kf[nb] = kf
        if nb not in m.kf_bad:
            local_kfs.append(nb)
    local_rows = []
    for k in local_kfs:                                        # :435-449
        for p in m.kf_points.get(k, []):
            if p >= 0:
                if p not in m.pt_bad:
                    if ba_local_mp.get(p) != kf:
                        local_rows.append(p)
                        ba_local_mp[p] = kf
    fixed_kfs = []
    for p in local_rows:                                       # :453-467
        observations = m.obs.get(p, {})
        for k in sorted(observations):
            if ba_local_kf.get(k) != kf and ba_fixed_kf.get(k) != kf:
                ba_fixed_kf[k] = kf                            # stamped before the bad test (:462-463)
                if k not in m.kf_bad:
                    fixed_kfs.append(k)
    # the vertices (:484-507) in asd_ba_problem's orders: poses in ascending id, points in ascending row
    pose_kfs = sorted(local_kfs + fixed_kfs)
    is_fixed = set(fixed_kfs)
    pose_fixed = [int(k in is_fixed) for k in pose_kfs]
    pose_of = {k: i for i, k in enumerate(pose_kfs)}
    rank_of = {p: i for i, p in enumerate(sorted(local_rows))}
    point_rank = [rank_of[p] for p in local_rows]
    e_point, e_pose, e_kf, e_idx, e_octave = [], [], [], [], []
    for p in local_rows:                                       # :534-593
        observations = m.obs.get(p, {})
        for k in sorted(observations):
            if k not in m.kf_bad:                              # :556
                idx = observations[k]
                e_point.append(rank_of[p]); e_pose.append(pose_of[k]); e_kf.append(k); e_idx.append(idx)
                e_octave.append(m.octave[k][idx])
    return dict(local_kfs=local_kfs, local_rows=local_rows, fixed_kfs=fixed_kfs, pose_kfs=pose_kfs, pose_fixed=pose_fixed,
                point_rank=point_rank, e_point=e_point, e_pose=e_pose, e_kf=e_kf, e_idx=e_idx, e_octave=e_octave)


def _set_bad_flag(m, p):
    """MapPoint::SetBadFlag (MapPoint.cc:180-197)"""
    m.pt_bad.add(p)
    obs = dict(m.obs[p])
    m.obs[p].clear()
    for k in sorted(obs):
        m.kf_points[k][obs[k]] = -1                            # pKF->EraseMapPointMatch(mit->second)


def _erase_observation(m, p, k, ref_kf):
    """MapPoint::EraseObservation (MapPoint.cc:119-142) -> 1 when the observation was there"""
    bad = False
    found = 0
    if k in m.obs.get(p, {}):
        found = 1
        del m.obs[p][k]                                        # nObs--, mObservations.erase(pKF)
        if ref_kf.get(p) == k:                                 # :131-132 (begin() of a std::map: the lowest id left)
            ref_kf[p] = min(m.obs[p]) if m.obs[p] else None
        if len(m.obs[p]) <= 2:
            bad = True
    if bad:
        _set_bad_flag(m, p)
    return found


def erase(m, g, flags, apply, ref_kf=None):
    """Optimizer.cc:652-697 over the edges of g = graph(...): flags[e] = chi2 > 5.991 || !isDepthPositive.  ref_kf: point -> mpRefKF
    (re-seated in place when given).  -> dict(n_erased, bad_rows, new_ref); with apply the map is mutated, without it left as it was.
    new_ref[i] states what the header promises for local_rows[i]: the lowest observer id left for a point that lost an observation and
    did not turn bad, -1 otherwise."""
    w = m if apply else m._copy()
    ref_kf = {} if ref_kf is None else (ref_kf if apply else dict(ref_kf))
    rows_sorted = sorted(g["local_rows"])
    to_erase = []
    for e, f in enumerate(flags):                              # :656-669 (the points are not bad: the map has not changed since)
        if f:
            to_erase.append((g["e_kf"][e], rows_sorted[g["e_point"][e]]))
    bad0 = set(w.pt_bad)
    bad_rows, lost, n_erased = [], set(), 0
    for k, p in to_erase:                                      # :690-696
        idx = w.obs.get(p, {}).get(k)
        if idx is not None:
            w.kf_points[k][idx] = -1                           # pKFi->EraseMapPointMatch(pMPi)
        if _erase_observation(w, p, k, ref_kf):
            n_erased += 1
            lost.add(p)
        if p in w.pt_bad and p not in bad0 and p not in bad_rows:
            bad_rows.append(p)
    new_ref = [min(w.obs[p]) if p in lost and p not in w.pt_bad else -1 for p in g["local_rows"]]
    return dict(n_erased=n_erased, bad_rows=bad_rows, new_ref=new_ref)

