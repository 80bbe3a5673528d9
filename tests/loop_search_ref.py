"""numpy restatement of the four searches that decide whether a loop is closed or a lost camera is relocalised, for
tests/test_loop_search_exits.py.  Written from the reference's source text, independently of oracle/matcher.cpp and of the
kernels:

  search_by_projection_reloc  ORBmatcher::SearchByProjection(Frame&, KeyFrame*, set, th, ORBdist) (ORBmatcher.cc:1455-1582) with
                              Frame::GetFeaturesInArea (Frame.cc:219-273) and ComputeThreeMaxima (:1584-1625)
  search_by_projection_scw    ORBmatcher::SearchByProjection(KeyFrame*, Scw, points, vpMatched, th) (:300-413)
  fuse_scw                    ORBmatcher::Fuse(KeyFrame*, Scw, points, th, vpReplacePoint), search half (:963-1086)
  search_by_sim3              ORBmatcher::SearchBySim3 (:1090-1314)
                              the three with KeyFrame::GetFeaturesInArea (KeyFrame.cc:839-878) and KeyFrame::IsInImage (:880-883);
                              all four with MapPoint::PredictScale (MapPoint.cc:421-453) and Get{Min,Max}DistanceInvariance (:409-419)

Arithmetic, as in tests/mapping_ref.py.  Descriptor distances (stereo_ref.descriptor_distance: f32, components 0..127 in order) and
every comparison between them -- the first strict minimum from the starting bestDist, the acceptance against TH_LOW / TH_HIGH /
ORBdist -- are bit-comparable f32.  The rotation histogram is loop_ref.rot_bin / three_maxima (f32 as the source writes it).  The
geometric gates are evaluated in float64 and report a MARGIN: the distance of the gate quantity from its threshold in units of
the tolerance (mapping_ref.REL_TOL for the distance range, the viewing angle and PredictScale's level boundaries, DEPTH_TOL for
|z| against the point's distance, PIXEL_TOL for the image bounds and the window edge), the minimum over the gates the element
evaluated.  An element is DECIDABLE when its margin is > 1.  The window-edge margin is taken over every keypoint of the visited
cells, whether a claim or a level gate drops it later or not, so a margin never depends on what earlier elements claimed.

The relocalisation search has no depth gate, but its pixel is fx * xc / z + cx: the f32 rounding of z is amplified by dist / |z|,
so |z| against DEPTH_TOL * dist enters its margin although no rule of the source compares it.

Where the source has undefined behaviour the library defines the result and this file states the same rule:
  * z == 0.  invz is +-inf; the pixel is +-inf (outside every bound) or, with xc == 0, NaN.  A NaN passes `u < min || u > max`
    (:1490) and reaches floor() -> int in GetFeaturesInArea.  RULE: a point with z == 0 has no match in any of the four; it is
    reported as outside_u (relocalisation) / outside_image.  Its margin is 0: whoever builds such a row with an exactly
    representable camera marks it as exact.
  * bestDist <= threshold with bestIdx == -1 cannot happen with the source's starting values and thresholds below 100; the
    mutants that exchange the starting values treat it as no match.

Exits the source has but no decidable input reaches:
  * level_clamped_low (PredictScale's nScale < 0): ceil(log(max / dist) / log 1.2) < 0 needs dist >= 1.2 * max, which has left
    through too_far unless the two f32 roundings meet exactly.  It is not in the counter lists.
  * search_by_projection_reloc, all_dropped through the level gate: there the level gate is part of GetFeaturesInArea, so a window
    whose keypoints all fail it is window_empty (:1513); all_dropped is reached through occupied keypoints only.
"""
import numpy as np

from tests.loop_ref import rot_bin, three_maxima
from tests.mapping_ref import DEPTH_TOL, GRID_COLS, GRID_ROWS, PIXEL_TOL, REL_TOL, census, grid_cells, level_tables  # noqa: F401
from tests.stereo_ref import descriptor_distance

F32 = np.float32
F64 = np.float64

TH_HIGH, TH_LOW = F32(1.5), F32(0.5)     # ORBmatcher.cc:37-38
HISTO_LENGTH = 30                        # :39
N_LEVELS, SCALE_FACTOR = 8, 1.2

RELOC_EXITS = ("invalid",                 # :1475-1477
               "outside_u",               # :1490
               "outside_v",               # :1492
               "too_near",                # :1503 dist3D < 0.8 * mfMinDistance
               "too_far",                 # :1503 dist3D > 1.2 * mfMaxDistance
               "window_empty",            # :1513
               "all_dropped",             # :1524 every candidate already holds a map point
               "above_orb_dist",          # :1538
               "matched",
               "removed_by_orientation")  # :1568-1578
RELOC_COUNTERS = ("level_below", "level_above", "occupied_on_entry", "claimed_earlier", "tie_first_wins", "level_clamped_high",
                  "behind_camera_went_on", "bin_wrapped", "rot_negative")
SCW_EXITS = ("invalid",                   # :327
             "behind",                    # :337
             "outside_image",             # :349
             "too_near",                  # :358
             "too_far",                   # :358
             "viewing_angle",             # :364
             "window_empty",              # :374
             "all_dropped",               # :385 / :390 no candidate reached the distance
             "above_th_low",              # :404
             "matched")
SCW_COUNTERS = ("matched_on_entry", "claimed_earlier", "level_below", "level_above", "tie_first_wins", "level_clamped_high")
FUSE_SCW_EXITS = SCW_EXITS                # :991, :1001, :1013, :1022, :1028, :1039, :1053, :1068
FUSE_SCW_COUNTERS = ("level_below", "level_above", "tie_first_wins", "level_clamped_high", "keypoint_chosen_twice")
SIM3_EXITS = ("no_point",                 # :1140-1144 / :1220-1224
              "behind",                   # :1151 / :1231
              "outside_image",            # :1162 / :1242
              "too_near",                 # :1170 / :1250
              "too_far",
              "window_empty",             # :1181 / :1261
              "all_dropped",              # :1195 / :1275
              "above_th_high",            # :1209 / :1289
              "one_way")                  # vnMatch1 / vnMatch2 set
SIM3_COUNTERS = ("level_below", "level_above", "tie_first_wins", "level_clamped_high")
SIM3_PAIRS = ("only_12", "only_21", "mutual")      # :1298-1311


def _rel(q, thr):
    return abs(q - thr) / (REL_TOL * abs(thr))


class Frame:
    """keypoints, descriptors and the grid of a Frame / KeyFrame"""

    def __init__(self, kps, desc, bounds):
        self.n = len(kps)
        self.kps = kps
        self.desc = np.ascontiguousarray(desc, F32).reshape(self.n, -1)
        self.bounds = tuple(F64(F32(b)) for b in bounds)
        self.cells, self.inv_w, self.inv_h = grid_cells(kps, bounds)
        self.x, self.y, self.octave = kps["x"].astype(F64), kps["y"].astype(F64), kps["octave"].astype(np.int64)
        self.angle = kps["angle"].astype(F32)


def _area(fr, u, v, r):
    """GetFeaturesInArea without a level gate (KeyFrame.cc:839-878, Frame.cc:219-273 visit the cells in the same order)
    -> (indices in visiting order, margin of the window edge, grid columns visited, the largest number of keypoints that the
    visited rows of one column hold)"""
    min_x, _, min_y, _ = fr.bounds
    c0 = max(0, int(np.floor((u - min_x - r) * fr.inv_w)))
    c1 = min(GRID_COLS - 1, int(np.ceil((u - min_x + r) * fr.inv_w)))
    r0 = max(0, int(np.floor((v - min_y - r) * fr.inv_h)))
    r1 = min(GRID_ROWS - 1, int(np.ceil((v - min_y + r) * fr.inv_h)))
    if c0 >= GRID_COLS or c1 < 0 or r0 >= GRID_ROWS or r1 < 0:
        return np.zeros(0, np.int64), np.inf, 0, 0
    out, m, widest = [], np.inf, 0
    for ix in range(c0, c1 + 1):
        col = [fr.cells[(ix, iy)] for iy in range(r0, r1 + 1) if (ix, iy) in fr.cells]
        if not col:
            continue
        col = np.concatenate(col)
        dx, dy = np.abs(fr.x[col] - u), np.abs(fr.y[col] - v)
        edge = (dx < r + PIXEL_TOL) & (dy < r + PIXEL_TOL)
        if edge.any():
            m = min(m, np.minimum(np.abs(dx[edge] - r), np.abs(dy[edge] - r)).min() / PIXEL_TOL)
        widest = max(widest, len(col))
        out.append(col[(dx < r) & (dy < r)])
    return (np.concatenate(out) if out else np.zeros(0, np.int64)), m, c1 - c0 + 1, widest


_LOG_SF = np.log(F64(F32(SCALE_FACTOR)))
_Q_TOL = np.log1p(REL_TOL) / _LOG_SF                   # REL_TOL on the ratio of distances, in units of levels
_SCALE64 = level_tables(N_LEVELS, SCALE_FACTOR)[0].astype(F64)


def _predict_scale(max_dist, dist):
    """MapPoint::PredictScale -> (level, clamped high, margin); ceil changes at the integers, those in [0, n - 2] change the level"""
    q = np.log(F64(max_dist) / dist) / _LOG_SF
    n_scale = int(np.ceil(q))
    near = np.round(q)
    m = abs(q - near) / _Q_TOL if 0 <= near <= N_LEVELS - 2 else np.inf
    return min(max(n_scale, 0), N_LEVELS - 1), n_scale >= N_LEVELS, m


def _first_minimum(md, desc, cand, start, last_wins):
    """`if (dist < bestDist)` over cand in order from bestDist = start -> (bestDist, bestIdx, the minimum is shared)"""
    if len(cand) == 0:
        return F32(start), -1, False
    dist = descriptor_distance(md, desc[cand])
    lowest = dist.min()
    if not lowest < F32(start):
        return F32(start), -1, False
    where = np.nonzero(dist == lowest)[0]
    return lowest, int(cand[where[-1] if last_wins else where[0]]), len(where) > 1


def _range_factors(min_dist, max_dist, drop_factors):
    if drop_factors:
        return F64(min_dist), F64(max_dist)
    return F64(F32(0.8)) * F64(min_dist), F64(F32(1.2)) * F64(max_dist)                 # MapPoint.cc:409-419


def _new(n, exits, counters):
    r = dict(exit=np.zeros(n, np.int32), margin=np.full(n, np.inf), best_dist=np.full(n, np.nan, F32), match=np.full(n, -1, np.int32),
             level=np.full(n, -1, np.int64), n_in_window=np.zeros(n, np.int64), n_list=np.zeros(n, np.int64), n_cols=np.zeros(n, np.int64),
             max_column=np.zeros(n, np.int64), u=np.full(n, np.nan), v=np.full(n, np.nan), radius=np.full(n, np.nan))
    for c in counters:
        r[c] = np.zeros(n, np.int64)
    return r


def _keyframe_search(fr, K, valid, pc, PO, normal, min_dist, max_dist, mp_desc, th, exits, counters, start, accept, above,
                     taken=None, claims=True, view_gate=True, accept_strict=False, closed_upper=False, level_wide=False, drop_factors=False,
                     last_wins=False):
    """the body the three KeyFrame searches share.  pc [n][3]: the point in the camera; PO [n][3]: the vector whose norm is the
    distance (p3Dw - Ow for the Scw functions, the camera-frame point for SearchBySim3).  taken: vpMatched as booleans, updated
    in visiting order, or None for the functions without claims.  -> the per-element dict; match = bestIdx where accepted"""
    n = len(valid)
    E = {name: i for i, name in enumerate(exits)}
    fx, fy, cx, cy = np.asarray(K, F32).astype(F64)
    min_x, max_x, min_y, max_y = fr.bounds
    mp_desc = np.ascontiguousarray(mp_desc, F32).reshape(n, -1)
    res = _new(n, exits, counters)
    on_entry = None if taken is None else taken.copy()
    for i in range(n):
        m = np.inf

        def leave(name):
            res["exit"][i] = E[name]
            res["margin"][i] = m

        if not valid[i]:
            leave(exits[0])
            continue
        z = pc[i, 2]
        dist3d = np.linalg.norm(PO[i])
        m = min(m, abs(z) / (DEPTH_TOL * dist3d) if dist3d > 0 else 0.0)
        if z < 0:
            leave("behind")
            continue
        if z == 0:
            leave("outside_image")
            continue
        u, v = fx * pc[i, 0] / z + cx, fy * pc[i, 1] / z + cy
        m = min(m, min(abs(u - min_x), abs(u - max_x), abs(v - min_y), abs(v - max_y)) / PIXEL_TOL)
        if closed_upper:
            inside = min_x <= u <= max_x and min_y <= v <= max_y
        else:
            inside = min_x <= u < max_x and min_y <= v < max_y
        if not inside:
            leave("outside_image")
            continue
        lo, hi = _range_factors(min_dist[i], max_dist[i], drop_factors)
        m = min(m, _rel(dist3d, lo))
        if dist3d < lo:
            leave("too_near")
            continue
        m = min(m, _rel(dist3d, hi))
        if dist3d > hi:
            leave("too_far")
            continue
        if normal is not None and view_gate:
            dot = PO[i] @ normal[i].astype(F64)
            m = min(m, _rel(dot, 0.5 * dist3d))
            if dot < 0.5 * dist3d:
                leave("viewing_angle")
                continue
        lvl, clamped, mq = _predict_scale(max_dist[i], dist3d)
        m = min(m, mq)
        res["level"][i] = lvl
        res["level_clamped_high"][i] = clamped
        res["u"][i], res["v"][i], res["radius"][i] = u, v, F64(F32(th)) * _SCALE64[lvl]
        window, me, res["n_cols"][i], res["max_column"][i] = _area(fr, u, v, res["radius"][i])
        m = min(m, me)
        res["n_in_window"][i] = res["n_list"][i] = len(window)
        if len(window) == 0:
            leave("window_empty")
            continue
        if taken is not None:
            was, now = on_entry[window], taken[window] & ~on_entry[window]
            res["matched_on_entry"][i], res["claimed_earlier"][i] = int(was.sum()), int(now.sum())
            window = window[~was & ~now]
        lo_l, hi_l = (lvl - 1, lvl + 1) if level_wide else (lvl - 1, lvl)
        below, above_l = fr.octave[window] < lo_l, fr.octave[window] > hi_l
        res["level_below"][i], res["level_above"][i] = int(below.sum()), int(above_l.sum())
        bd, bi, tie = _first_minimum(mp_desc[i], fr.desc, window[~below & ~above_l], start, last_wins)
        res["best_dist"][i] = bd
        res["tie_first_wins"][i] = tie
        if bi < 0:
            leave("all_dropped")
        elif (bd < accept) if accept_strict else (bd <= accept):
            res["match"][i] = bi
            if taken is not None and claims:
                taken[bi] = True
            leave(exits[-1])
        else:
            leave(above)
    res["decidable"] = res["margin"] > 1
    return res


def _decompose_scw(Scw, ow_scaled=False):
    """:309-313 / :972-976: the scale from row 0 alone, Ow = -Rcw.t() * tcw"""
    S = np.asarray(Scw, F32).astype(F64).reshape(4, 4)
    sR = S[:3, :3]
    s = np.sqrt(sR[0] @ sR[0])
    R, t = sR / s, S[:3, 3] / s
    return R, t, -R.T @ (S[:3, 3] if ow_scaled else t)


def search_by_projection_scw(fr, Scw, valid, Xw, normal, min_dist, max_dist, mp_desc, K, th, matched_kp, no_claims=False,
                             ow_scaled=False, start=256, **mutant):
    """-> the per-point dict of _keyframe_search plus matched_kp [fr.n] (entries set on entry untouched, the index of the point
    elsewhere, -1: free) and n_matches.  th is the source's int."""
    R, t, Ow = _decompose_scw(Scw, ow_scaled)
    X = np.asarray(Xw, F32).astype(F64)
    mk = np.asarray(matched_kp, np.int32).copy()
    taken = mk != -1
    res = _keyframe_search(fr, K, valid, X @ R.T + t, X - Ow, normal, min_dist, max_dist, mp_desc, int(th), SCW_EXITS, SCW_COUNTERS,
                           start, TH_LOW, "above_th_low", taken=taken, claims=not no_claims, **mutant)
    for i in np.nonzero(res["match"] >= 0)[0]:                  # :406 in visiting order: without claims the last writer stays
        mk[res["match"][i]] = i
    res["matched_kp"], res["n_matches"] = mk, int((res["match"] >= 0).sum())
    return res


def fuse_scw(fr, Scw, valid, Xw, normal, min_dist, max_dist, mp_desc, K, th, ow_scaled=False, start=100, **mutant):
    """-> the per-point dict plus best_idx (= match: bestIdx where bestDist <= TH_LOW, else -1); best_dist is bestDist at :1068
    (the starting value where no candidate passed, NaN where the search was not reached)"""
    R, t, Ow = _decompose_scw(Scw, ow_scaled)
    X = np.asarray(Xw, F32).astype(F64)
    res = _keyframe_search(fr, K, valid, X @ R.T + t, X - Ow, normal, min_dist, max_dist, mp_desc, F32(th), FUSE_SCW_EXITS,
                           FUSE_SCW_COUNTERS, start, TH_LOW, "above_th_low", **mutant)
    res["best_idx"] = res["match"]
    seen = set()
    for i in np.nonzero(res["match"] >= 0)[0]:
        res["keypoint_chosen_twice"][i] = res["match"][i] in seen
        seen.add(int(res["match"][i]))
    return res


def search_by_sim3(fr1, fr2, has1, has2, Xw1, Xw2, mind1, maxd1, mind2, maxd2, desc1, desc2, T1w, T2w, s12, R12, t12, K, th,
                   swap_sr=False, no_mutual=False, start=100, **mutant):
    """-> dict(match12 [n1] (i2 for the pairs that agree, else -1), n_matches, d12 / d21 (the per-point dicts of the two
    directions; match = vnMatch1 / vnMatch2), pair [n1] (index into SIM3_PAIRS or -1), only_21 [n2] flags, decidable [n1])"""
    T1, T2 = np.asarray(T1w, F32).astype(F64).reshape(4, 4), np.asarray(T2w, F32).astype(F64).reshape(4, 4)
    R12, t12, s = np.asarray(R12, F32).astype(F64).reshape(3, 3), np.asarray(t12, F32).astype(F64), F64(F32(s12))
    sR12 = s * R12                                               # :1107
    sR21 = (1.0 / s) * R12.T                                     # :1108
    t21 = -sR21 @ t12                                            # :1109
    if swap_sr:
        sR12, sR21 = sR21, sR12
    c1 = np.asarray(Xw1, F32).astype(F64) @ T1[:3, :3].T + T1[:3, 3]          # :1147
    p2 = c1 @ sR21.T + t21                                                     # :1148
    c2 = np.asarray(Xw2, F32).astype(F64) @ T2[:3, :3].T + T2[:3, 3]          # :1227
    p1 = c2 @ sR12.T + t12                                                     # :1228
    d12 = _keyframe_search(fr2, K, has1, p2, p2, None, mind1, maxd1, desc1, F32(th), SIM3_EXITS, SIM3_COUNTERS, start, TH_HIGH,
                           "above_th_high", **mutant)
    d21 = _keyframe_search(fr1, K, has2, p1, p1, None, mind2, maxd2, desc2, F32(th), SIM3_EXITS, SIM3_COUNTERS, start, TH_HIGH,
                           "above_th_high", **mutant)
    n1 = len(has1)
    match12, pair = np.full(n1, -1, np.int32), np.full(n1, -1, np.int32)
    decidable = d12["decidable"].copy()
    for i1 in np.nonzero(d12["match"] >= 0)[0]:
        i2 = d12["match"][i1]
        decidable[i1] &= d21["decidable"][i2]
        if d21["match"][i2] == i1 or no_mutual:                 # :1304-1309
            match12[i1], pair[i1] = i2, 2
        else:
            pair[i1] = 0
    only_21 = np.zeros(len(has2), bool)
    for i2 in np.nonzero(d21["match"] >= 0)[0]:
        only_21[i2] = d12["match"][d21["match"][i2]] != i2
    return dict(match12=match12, n_matches=int((match12 >= 0).sum()), d12=d12, d21=d21, pair=pair, only_21=only_21,
                decidable=decidable)


def search_by_projection_reloc(fr, valid, Xw, min_dist, max_dist, mp_desc, kf_angle, occupied, Tcw, K, th, orb_dist, check_ori=True,
                               accept_strict=False, start=256, half_open=False, depth_gate=False, level_narrow=False,
                               drop_factors=False, no_claims=False, last_wins=False, drop_tenth=False, hist_holds_mp=False):
    """fr: the current frame; the arrays run over the keyframe's keypoints.  -> the per-point dict (match = the current frame's
    keypoint the point holds after the orientation check) plus match_cur [fr.n] (the point assigned to keypoint j, or -1) and
    n_matches.  The keyword arguments from accept_strict on are the mutants of the sensitivity test."""
    n = len(valid)
    E = {name: i for i, name in enumerate(RELOC_EXITS)}
    T = np.asarray(Tcw, F32).astype(F64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    Ow = -R.T @ t                                                # :1461
    fx, fy, cx, cy = np.asarray(K, F32).astype(F64)
    min_x, max_x, min_y, max_y = fr.bounds
    mp_desc = np.ascontiguousarray(mp_desc, F32).reshape(n, -1)
    orb_dist = F32(orb_dist)
    res = _new(n, RELOC_EXITS, RELOC_COUNTERS)
    occupied = np.asarray(occupied).astype(bool)
    claimed = np.zeros(fr.n, bool)
    match_cur = np.full(fr.n, -1, np.int32)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for i in range(n):
        m = np.inf

        def leave(name):
            res["exit"][i] = E[name]
            res["margin"][i] = m

        if not valid[i]:
            leave("invalid")
            continue
        p = Xw[i].astype(F64)
        pc = R @ p + t
        PO = p - Ow
        dist3d = np.linalg.norm(PO)
        z = pc[2]
        m = min(m, abs(z) / (DEPTH_TOL * dist3d) if dist3d > 0 else 0.0)
        if z == 0 or (depth_gate and z < 0):
            leave("outside_u")
            continue
        u, v = fx * pc[0] / z + cx, fy * pc[1] / z + cy
        m = min(m, min(abs(u - min_x), abs(u - max_x)) / PIXEL_TOL)
        if u < min_x or (u >= max_x if half_open else u > max_x):              # :1490
            leave("outside_u")
            continue
        m = min(m, min(abs(v - min_y), abs(v - max_y)) / PIXEL_TOL)
        if v < min_y or (v >= max_y if half_open else v > max_y):              # :1492
            leave("outside_v")
            continue
        lo, hi = _range_factors(min_dist[i], max_dist[i], drop_factors)
        m = min(m, _rel(dist3d, lo))
        if dist3d < lo:
            leave("too_near")
            continue
        m = min(m, _rel(dist3d, hi))
        if dist3d > hi:
            leave("too_far")
            continue
        res["behind_camera_went_on"][i] = z < 0
        lvl, res["level_clamped_high"][i], mq = _predict_scale(max_dist[i], dist3d)
        m = min(m, mq)
        res["level"][i] = lvl
        res["u"][i], res["v"][i], res["radius"][i] = u, v, F64(F32(th)) * _SCALE64[lvl]
        window, me, res["n_cols"][i], res["max_column"][i] = _area(fr, u, v, res["radius"][i])
        m = min(m, me)
        res["n_in_window"][i] = len(window)
        # Frame.cc:242-262 with minLevel = lvl - 1, maxLevel = lvl + 1: bCheckLevels holds for every lvl through maxLevel >= 0
        min_level, max_level = lvl - 1, (lvl if level_narrow else lvl + 1)
        if min_level > 0 or max_level >= 0:
            below = fr.octave[window] < min_level
            above = (fr.octave[window] > max_level) if max_level >= 0 else np.zeros(len(window), bool)
            res["level_below"][i], res["level_above"][i] = int(below.sum()), int((above & ~below).sum())
            window = window[~below & ~above]
        res["n_list"][i] = len(window)                      # vIndices2
        if len(window) == 0:
            leave("window_empty")
            continue
        was = occupied[window]
        now = claimed[window] & ~was if not no_claims else np.zeros(len(window), bool)
        res["occupied_on_entry"][i], res["claimed_earlier"][i] = int(was.sum()), int(now.sum())
        bd, bi, tie = _first_minimum(mp_desc[i], fr.desc, window[~was & ~now], start, last_wins)
        res["best_dist"][i] = bd
        res["tie_first_wins"][i] = tie
        if bi < 0:
            leave("all_dropped")
        elif (bd < orb_dist) if accept_strict else (bd <= orb_dist):           # :1538
            match_cur[bi] = i
            claimed[bi] = True
            res["match"][i] = bi
            nmatches += 1
            if check_ori:
                rot = F32(kf_angle[i]) - fr.angle[bi]                          # :1545
                b = rot_bin(kf_angle[i], fr.angle[bi])
                res["rot_negative"][i] = rot < 0
                res["bin_wrapped"][i] = b == 0 and (rot + F32(360) if rot < 0 else rot) > 180
                hist[b].append(i if hist_holds_mp else bi)
            leave("matched")
        else:
            leave("above_orb_dist")
    if check_ori:
        counts = [len(h) for h in hist]
        keep = three_maxima(counts)
        if drop_tenth:
            order = sorted(range(HISTO_LENGTH), key=lambda b: (-counts[b], b))
            keep = tuple(b for b in order[:3] if counts[b] > 0)
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for j in hist[b]:                                                  # :1574 indexes the current frame's keypoints
                nmatches -= 1
                if j < fr.n and match_cur[j] >= 0:
                    res["exit"][match_cur[j]] = E["removed_by_orientation"]
                    res["match"][match_cur[j]] = -1
                    match_cur[j] = -1
    res["match_cur"], res["n_matches"] = match_cur, nmatches
    res["decidable"] = res["margin"] > 1
    return res
