"""numpy restatement of the two searches that run on every tracked frame, for tests/test_track_search_exits.py.  Written from the
reference's source text, independently of oracle/matcher.cpp, of the kernels and of test_matcher._m1_python:

  search_by_projection_frame   ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, mono) (ORBmatcher.cc:1318-1452), M1, with
                               ComputeThreeMaxima (:1584-1625, loop_ref.three_maxima)
  is_in_frustum                Frame::isInFrustum (Frame.cc:160-217) with MapPoint::PredictScale (MapPoint.cc:438-453) and
                               Get{Min,Max}DistanceInvariance (:409-419)
  search_by_projection_points  ORBmatcher::SearchByProjection(Frame, vector<MapPoint*>, th) (:44-122), M2, with RadiusByViewingCos
                               (:126-132)
  features_in_area             Frame::GetFeaturesInArea (Frame.cc:219-273), the one with the level gate

Arithmetic, as in tests/loop_search_ref.py.  Descriptor distances (stereo_ref.descriptor_distance) and every comparison between
them -- the strict minimum from the starting bestDist, the second best, TH_HIGH, the ratio test in f32 -- are bit-comparable f32, and
so is the rotation histogram (loop_ref.rot_bin / three_maxima).  The geometric gates are evaluated in float64 and report a MARGIN:
the distance of the gate quantity from its threshold in units of the tolerance (mapping_ref.PIXEL_TOL for the image bounds and the
window edge, DEPTH_TOL for |z| against the point's distance, REL_TOL for the distance range, the viewing angle and PredictScale's
level boundaries, COS_TOL -- absolute, a few f32 ulps of a cosine -- for viewCos against RadiusByViewingCos' 0.998), the minimum over
the gates the element evaluated.  An element is DECIDABLE when its margin is > 1.  The window-edge margin is taken over every keypoint
of the visited cells, whether a claim or the level gate drops it or not, so a margin never depends on what earlier elements claimed.

Where the source has undefined behaviour this file keeps loop_search_ref's rule: a point with z == 0 (invz = +-inf, the pixel +-inf
or NaN) has no match and is not in view; it leaves through outside_u with margin 0, and whoever builds such a row with an exactly
representable camera marks it as exact.

M1's two directional forms of the area query (bForward / bBackward, :1375-1378) need a stereo baseline; the entry points are monocular
(bMono), so the restatement has the third form alone.

Exits the source has but no decidable input reaches:
  * level_clamped_low (PredictScale's nScale < 0): needs dist >= 1.2 * max ... which has left through too_far (see loop_search_ref).
  * M2 above_th_high with bestIdx == -1 is all_dropped here: every candidate held a map point, bestDist stayed 256.
"""
import numpy as np

from tests.loop_ref import rot_bin, three_maxima
from tests.loop_search_ref import Frame, _predict_scale                                                  # noqa: F401
from tests.mapping_ref import COS_TOL, DEPTH_TOL, GRID_COLS, GRID_ROWS, PIXEL_TOL, REL_TOL, census, level_tables  # noqa: F401
from tests.stereo_ref import descriptor_distance

F32 = np.float32
F64 = np.float64

TH_HIGH = F32(1.5)                       # ORBmatcher.cc:37
HISTO_LENGTH = 30                        # :39
N_LEVELS, SCALE_FACTOR = 8, 1.2
_SCALE64 = level_tables(N_LEVELS, SCALE_FACTOR)[0].astype(F64)

M1_EXITS = ("invalid",                        # :1345-1347 no map point / outlier
            "behind",                         # :1357
            "outside_u",                      # :1363
            "outside_v",                      # :1365
            "window_empty",                   # :1382
            "all_dropped",                    # :1393-1395 every candidate holds an observed map point: bestDist stays 100
            "above_th_high",                  # :1408
            "matched",
            "overwritten_later",              # :1410 by a later point, the holder having no observations
            "removed_by_orientation",         # :1438-1448 its own bin was discarded
            "cleared_through_another_write")  # :1444 the last writer's bin stayed, an overwritten write to the keypoint sat in a discarded one
M1_COUNTERS = ("level_below", "level_above", "claimed_earlier", "holder_unobserved_went_on", "tie_first_wins", "bin_wrapped", "rot_negative",
               "octave_0", "octave_top")
FRUSTUM_EXITS = ("behind",                    # Frame.cc:174
                 "outside_u",                 # :182
                 "outside_v",                 # :184
                 "too_near",                  # :194
                 "too_far",                   # :194
                 "viewing_angle",             # :202
                 "in_view")
FRUSTUM_COUNTERS = tuple("level_%d" % l for l in range(N_LEVELS)) + ("level_clamped_high",)
M2_EXITS = ("not_in_view",                    # :54
            "window_empty",                   # :70
            "all_dropped",                    # :86-88 every candidate holds a map point
            "above_th_high",                  # :110
            "ratio_rejected",                 # :112
            "matched",
            "overwritten_later")              # :115 by a later point, the holder having no observations
M2_COUNTERS = ("occupied_on_entry", "claimed_earlier", "level_below", "level_above", "no_second", "second_other_level",
               "second_tie_first_by_position", "second_at_or_beyond_256", "ratio_at_equality", "tie_first_wins", "radius_2.5", "radius_4")


def _rel(q, thr):
    return abs(q - thr) / (REL_TOL * abs(thr))


def features_in_area(fr, u, v, r, min_level, max_level):
    """Frame::GetFeaturesInArea -> dict(idx (visiting order, behind the level gate), margin of the window edge, n_cols, widest (the
    largest number of keypoints the visited rows of one column hold), below, above, n_in_window (in front of the level gate))"""
    min_x, _, min_y, _ = fr.bounds
    out = dict(idx=np.zeros(0, np.int64), margin=np.inf, n_cols=0, widest=0, below=0, above=0, n_in_window=0)
    c0 = max(0, int(np.floor((u - min_x - r) * fr.inv_w)))                                     # :226
    c1 = min(GRID_COLS - 1, int(np.ceil((u - min_x + r) * fr.inv_w)))                          # :230
    r0 = max(0, int(np.floor((v - min_y - r) * fr.inv_h)))                                     # :234
    r1 = min(GRID_ROWS - 1, int(np.ceil((v - min_y + r) * fr.inv_h)))                          # :238
    if c0 >= GRID_COLS or c1 < 0 or r0 >= GRID_ROWS or r1 < 0:
        return out
    check = min_level > 0 or max_level >= 0                                                    # :242
    got, m = [], np.inf
    for ix in range(c0, c1 + 1):
        col = [fr.cells[(ix, iy)] for iy in range(r0, r1 + 1) if (ix, iy) in fr.cells]
        if not col:
            continue
        col = np.concatenate(col)
        out["widest"] = max(out["widest"], len(col))
        dx, dy = np.abs(fr.x[col] - u), np.abs(fr.y[col] - v)
        edge = (dx < r + PIXEL_TOL) & (dy < r + PIXEL_TOL)
        if edge.any():
            m = min(m, np.minimum(np.abs(dx[edge] - r), np.abs(dy[edge] - r)).min() / PIXEL_TOL)
        col = col[(dx < r) & (dy < r)]                                                         # :267
        out["n_in_window"] += len(col)
        if check:
            below = fr.octave[col] < min_level                                                 # :257
            above = (fr.octave[col] > max_level) if max_level >= 0 else np.zeros(len(col), bool)   # :259-261
            out["below"] += int(below.sum())
            out["above"] += int((above & ~below).sum())
            col = col[~below & ~above]
        got.append(col)
    out.update(idx=np.concatenate(got) if got else out["idx"], margin=m, n_cols=c1 - c0 + 1)
    return out


def _project(T, K, Xw):
    Tm = np.asarray(T, F32).astype(F64).reshape(4, 4)
    R, t = Tm[:3, :3], Tm[:3, 3]
    X = np.asarray(Xw, F32).astype(F64)
    return X @ R.T + t, -R.T @ t, np.asarray(K, F32).astype(F64)


def search_by_projection_frame(cur, last_octave, last_angle, has_mp, Xw, mp_desc, Tcw, K, th, check_ori=True, obs_positive=None,
                               last_wins=False, start=100, accept_strict=False, no_claims=False, honour_unobserved=False,
                               level_narrow=False, half_open=False, behind_at_zero=False, hist_last_writer=False, maxima_by_sort=False,
                               tenth_closed=False, count_entries=False):
    """M1.  cur: the current Frame; the arrays run over the last frame's keypoints.  -> per-point dict (exit, margin, counters,
    best_dist, write = the keypoint the point wrote to or -1, n_list, n_cols, max_column) plus match_cur [cur.n] and n_matches.
    The keyword arguments from last_wins on are the mutants of the sensitivity test."""
    n = len(has_mp)
    E = {name: i for i, name in enumerate(M1_EXITS)}
    pc_all, _, (fx, fy, cx, cy) = _project(Tcw, K, Xw)
    min_x, max_x, min_y, max_y = cur.bounds
    mp_desc = np.ascontiguousarray(mp_desc, F32).reshape(n, -1)
    obs = np.ones(n, bool) if obs_positive is None else np.asarray(obs_positive).astype(bool)
    res = dict(exit=np.zeros(n, np.int32), margin=np.full(n, np.inf), best_dist=np.full(n, np.nan, F32), write=np.full(n, -1, np.int32),
               n_list=np.zeros(n, np.int64), n_cols=np.zeros(n, np.int64), max_column=np.zeros(n, np.int64), n_free=np.zeros(n, np.int64),
               u=np.full(n, np.nan), v=np.full(n, np.nan), radius=np.full(n, np.nan))
    for c in M1_COUNTERS:
        res[c] = np.zeros(n, np.int64)
    held = np.full(cur.n, -1, np.int64)                  # CurrentFrame.mvpMapPoints
    hist = [[] for _ in range(HISTO_LENGTH)]             # (keypoint, writer)
    writes = []                                          # (writer, keypoint, bin or -1) in order
    nmatches = 0
    for i in range(n):
        m = np.inf

        def leave(name):
            res["exit"][i] = E[name]
            res["margin"][i] = m

        if not has_mp[i]:
            leave("invalid")
            continue
        pc = pc_all[i]
        z, d3 = pc[2], np.linalg.norm(pc)
        m = min(m, abs(z) / (DEPTH_TOL * d3) if d3 > 0 else 0.0)
        if z < 0 or (behind_at_zero and z == 0):                                           # :1357 invzc < 0
            leave("behind")
            continue
        if z == 0:
            leave("outside_u")
            continue
        u, v = fx * pc[0] / z + cx, fy * pc[1] / z + cy
        m = min(m, min(abs(u - min_x), abs(u - max_x)) / PIXEL_TOL)
        if u < min_x or (u >= max_x if half_open else u > max_x):                           # :1363
            leave("outside_u")
            continue
        m = min(m, min(abs(v - min_y), abs(v - max_y)) / PIXEL_TOL)
        if v < min_y or (v >= max_y if half_open else v > max_y):                           # :1365
            leave("outside_v")
            continue
        o = int(last_octave[i])
        res["octave_0"][i], res["octave_top"][i] = o == 0, o == N_LEVELS - 1
        radius = F64(F32(th)) * _SCALE64[o]                                                # :1371
        lo, hi = (o, o) if level_narrow else (o - 1, o + 1)                                # :1380
        a = features_in_area(cur, u, v, radius, lo, hi)
        m = min(m, a["margin"])
        res["u"][i], res["v"][i], res["radius"][i] = u, v, radius
        res["level_below"][i], res["level_above"][i] = a["below"], a["above"]
        res["n_list"][i], res["n_cols"][i], res["max_column"][i] = len(a["idx"]), a["n_cols"], a["widest"]
        cand = a["idx"]
        if len(cand) == 0:
            leave("window_empty")
            continue
        holder = held[cand]
        if no_claims:
            skip = np.zeros(len(cand), bool)
        elif honour_unobserved:
            skip = holder >= 0
        else:
            skip = (holder >= 0) & obs[np.maximum(holder, 0)]                              # :1393-1395
        res["claimed_earlier"][i] = int(skip.sum())
        res["holder_unobserved_went_on"][i] = int(((holder >= 0) & ~skip).sum())
        cand = cand[~skip]
        res["n_free"][i] = len(cand)
        best, bi = F32(start), -1
        if len(cand):
            dist = descriptor_distance(mp_desc[i], cur.desc[cand])
            lowest = dist.min()
            if lowest < best:                                                              # :1401 strict: the first minimum
                where = np.nonzero(dist == lowest)[0]
                best, bi = lowest, int(cand[where[-1] if last_wins else where[0]])
                res["tie_first_wins"][i] = len(where) > 1
        res["best_dist"][i] = best
        if bi < 0:
            leave("all_dropped" if len(cand) == 0 else "above_th_high")
        elif (best < TH_HIGH) if accept_strict else (best <= TH_HIGH):                     # :1408
            held[bi] = i
            res["write"][i] = bi
            nmatches += 1
            b = -1
            if check_ori:
                rot = F32(last_angle[i]) - cur.angle[bi]                                   # :1415
                b = rot_bin(last_angle[i], cur.angle[bi])
                res["rot_negative"][i] = rot < 0
                res["bin_wrapped"][i] = b == 0 and (rot + F32(360) if rot < 0 else rot) > 180
                hist[b].append((bi, i))
            writes.append((i, bi, b))
            leave("matched")
        else:
            leave("above_th_high")
    last_writer = {}
    for i, j, b in writes:
        last_writer[j] = i
    dropped = set()
    if check_ori:
        if hist_last_writer:
            hist = [[(j, i) for (j, i) in h if last_writer[j] == i] for h in hist]
        counts = [len(h) for h in hist]
        if maxima_by_sort:
            order = sorted(range(HISTO_LENGTH), key=lambda b: (counts[b], b), reverse=True)      # ties: the higher bin first
            keep = [order[0]]
            if F32(counts[order[1]]) >= F32(0.1) * F32(counts[order[0]]):
                keep.append(order[1])
                if F32(counts[order[2]]) >= F32(0.1) * F32(counts[order[0]]):
                    keep.append(order[2])
        elif tenth_closed:
            keep = _three_maxima_closed(counts)
        else:
            keep = three_maxima(counts)
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            dropped.add(b)
            for j, _ in hist[b]:                                                           # :1442-1446
                held[j] = -1
                nmatches -= 1
    for i, j, b in writes:
        if b in dropped:
            res["exit"][i] = E["removed_by_orientation"]
        elif last_writer[j] != i:
            res["exit"][i] = E["overwritten_later"]
        elif held[j] != i:
            res["exit"][i] = E["cleared_through_another_write"]
    res["match_cur"] = held.astype(np.int32)
    res["n_matches"] = int((held >= 0).sum()) if count_entries else nmatches
    res["decidable"] = res["margin"] > 1
    return res


def _three_maxima_closed(counts):
    """the mutant of ComputeThreeMaxima whose tenth rule is `<=`"""
    ind, vals = [-1, -1, -1], [0, 0, 0]
    for i, s in enumerate(counts):
        k = next((k for k in range(3) if s > vals[k]), None)
        if k is not None:
            ind[k + 1:], vals[k + 1:] = ind[k:2], vals[k:2]
            ind[k], vals[k] = i, s
    if F32(vals[1]) <= F32(0.1) * F32(vals[0]):
        ind[1] = ind[2] = -1
    elif F32(vals[2]) <= F32(0.1) * F32(vals[0]):
        ind[2] = -1
    return tuple(ind)


def is_in_frustum(bounds, Xw, normal, min_dist, max_dist, Tcw, K, cos_limit=0.5, drop_factors=False, cos_closed=False):
    """-> per-point dict: exit, margin, in_view, u, v, level, view_cos (f64) and the counters"""
    n = len(min_dist)
    E = {name: i for i, name in enumerate(FRUSTUM_EXITS)}
    pc_all, Ow, (fx, fy, cx, cy) = _project(Tcw, K, Xw)
    X = np.asarray(Xw, F32).astype(F64)
    min_x, max_x, min_y, max_y = (F64(F32(b)) for b in bounds)
    limit = F64(F32(cos_limit))
    res = dict(exit=np.zeros(n, np.int32), margin=np.full(n, np.inf), in_view=np.zeros(n, bool), u=np.full(n, np.nan), v=np.full(n, np.nan),
               level=np.full(n, -1, np.int64), view_cos=np.full(n, np.nan))
    for c in FRUSTUM_COUNTERS:
        res[c] = np.zeros(n, np.int64)
    for i in range(n):
        m = np.inf

        def leave(name):
            res["exit"][i] = E[name]
            res["margin"][i] = m

        pc, PO = pc_all[i], X[i] - Ow
        z, dist = pc[2], np.linalg.norm(PO)
        m = min(m, abs(z) / (DEPTH_TOL * dist) if dist > 0 else 0.0)
        if z < 0:                                                                          # :174
            leave("behind")
            continue
        if z == 0:
            leave("outside_u")
            continue
        u, v = fx * pc[0] / z + cx, fy * pc[1] / z + cy
        m = min(m, min(abs(u - min_x), abs(u - max_x)) / PIXEL_TOL)
        if u < min_x or u > max_x:                                                         # :182
            leave("outside_u")
            continue
        m = min(m, min(abs(v - min_y), abs(v - max_y)) / PIXEL_TOL)
        if v < min_y or v > max_y:                                                         # :184
            leave("outside_v")
            continue
        lo = F64(min_dist[i]) if drop_factors else F64(F32(0.8)) * F64(min_dist[i])        # MapPoint.cc:409-419
        hi = F64(max_dist[i]) if drop_factors else F64(F32(1.2)) * F64(max_dist[i])
        m = min(m, _rel(dist, lo))
        if dist < lo:                                                                      # :194
            leave("too_near")
            continue
        m = min(m, _rel(dist, hi))
        if dist > hi:
            leave("too_far")
            continue
        dot = PO @ np.asarray(normal[i], F32).astype(F64)
        m = min(m, _rel(dot, limit * dist))
        vc = dot / dist                                                                    # :200
        if (vc <= limit) if cos_closed else (vc < limit):                                  # :202
            leave("viewing_angle")
            continue
        lvl, clamped, mq = _predict_scale(max_dist[i], dist)                               # :206
        m = min(m, mq)
        res["in_view"][i], res["u"][i], res["v"][i], res["level"][i], res["view_cos"][i] = True, u, v, lvl, vc
        res["level_%d" % lvl][i] = 1
        res["level_clamped_high"][i] = clamped
        leave("in_view")
    res["decidable"] = res["margin"] > 1
    return res


def search_by_projection_points(cur, fru, mp_desc, occupied, th, nn_ratio, obs_positive=None, cos_f32_literal=False, no_th_factor=False,
                                level_wide=False, second_stays=False, ratio_closed=False, no_level_condition=False, admit_256=False,
                                one_count=False, last_wins=False):
    """M2 behind is_in_frustum's result `fru` (in_view, u, v, level, view_cos; exact: rows whose frustum outputs are exact by construction).
    -> per-point dict (exit, margin, counters, best_dist, best_dist2, write, n_list, n_cols, max_column, n_free) plus match_cur [cur.n]
    and n_matches"""
    n = len(fru["in_view"])
    E = {name: i for i, name in enumerate(M2_EXITS)}
    mp_desc = np.ascontiguousarray(mp_desc, F32).reshape(n, -1)
    obs = np.ones(n, bool) if obs_positive is None else np.asarray(obs_positive).astype(bool)
    occupied = np.asarray(occupied).astype(bool)
    nn_ratio, th = F32(nn_ratio), F32(th)
    res = dict(exit=np.zeros(n, np.int32), margin=np.array(fru["margin"], F64), best_dist=np.full(n, np.nan, F32), best_dist2=np.full(n, np.nan, F32),
               write=np.full(n, -1, np.int32), n_list=np.zeros(n, np.int64), n_cols=np.zeros(n, np.int64), max_column=np.zeros(n, np.int64),
               n_free=np.zeros(n, np.int64), radius=np.full(n, np.nan))
    for c in M2_COUNTERS:
        res[c] = np.zeros(n, np.int64)
    held = np.full(cur.n, -1, np.int64)
    writes = []
    nmatches = 0
    b_factor = th != 1.0 and not no_th_factor                                              # :48
    for i in range(n):
        def leave(name):
            res["exit"][i] = E[name]

        if not fru["in_view"][i]:
            leave("not_in_view")
            continue
        m = res["margin"][i]
        vc, lvl = fru["view_cos"][i], int(fru["level"][i])
        cut = F64(F32(0.998)) if cos_f32_literal else 0.998                                # :128 a double literal against a float
        m = min(m, abs(vc - cut) / COS_TOL)
        r = F32(2.5) if vc > cut else F32(4.0)
        res["radius_2.5" if vc > cut else "radius_4"][i] = 1
        if b_factor:
            r = F32(r * th)                                                                # :65
        radius = F64(r) * _SCALE64[lvl]                                                    # :68
        res["radius"][i] = radius
        a = features_in_area(cur, fru["u"][i], fru["v"][i], radius, lvl - 1, lvl + 1 if level_wide else lvl)
        m = min(m, a["margin"])
        res["margin"][i] = m
        res["level_below"][i], res["level_above"][i] = a["below"], a["above"]
        res["n_list"][i], res["n_cols"][i], res["max_column"][i] = len(a["idx"]), a["n_cols"], a["widest"]
        cand = a["idx"]
        if len(cand) == 0:
            leave("window_empty")
            continue
        was = occupied[cand]
        now = ~was & (held[cand] >= 0) & obs[np.maximum(held[cand], 0)]                    # :86-88
        res["occupied_on_entry"][i], res["claimed_earlier"][i] = int(was.sum()), int(now.sum())
        cand = cand[~was & ~now]
        res["n_free"][i] = len(cand)
        best, best2, lv1, lv2, bi = F32(256), F32(256), -1, -1, -1                         # :75-79
        tie1 = tie2 = False
        if len(cand):
            dist = descriptor_distance(mp_desc[i], cur.desc[cand])
            for k in range(len(cand)):
                d = dist[k]
                if (d <= best) if last_wins else (d < best):                               # :94
                    if not second_stays:
                        best2, lv2 = best, lv1                                             # :96-98
                    best, lv1, bi = d, int(cur.octave[cand[k]]), int(cand[k])
                elif d < best2:                                                            # :102
                    best2, lv2 = d, int(cur.octave[cand[k]])
            tie1 = int((dist == best).sum()) > 1
            rest = np.delete(dist, int(np.nonzero(cand == bi)[0][0])) if bi >= 0 else dist
            if admit_256 and bi >= 0 and lv2 == -1 and len(rest):                         # the mutant: the next entry whatever its distance
                k2 = int(np.argmin(rest))
                best2, lv2 = rest[k2], int(cur.octave[cand[cand != bi]][k2])
            tie2 = bi >= 0 and len(rest) > 0 and best2 < F32(256) and int((rest == best2).sum()) > 1
            res["second_at_or_beyond_256"][i] = bi >= 0 and len(rest) > 0 and not rest.min() < F32(256)
        res["best_dist"][i], res["best_dist2"][i] = best, best2
        res["tie_first_wins"][i], res["second_tie_first_by_position"][i] = tie1, tie2
        if bi < 0:
            leave("all_dropped" if len(cand) == 0 else "above_th_high")
            continue
        if not best <= TH_HIGH:                                                            # :110
            leave("above_th_high")
            continue
        res["no_second"][i] = lv2 == -1
        res["second_other_level"][i] = lv2 != -1 and lv2 != lv1
        prod = F32(nn_ratio * best2)
        res["ratio_at_equality"][i] = (lv1 == lv2) and best == prod
        same = True if no_level_condition else lv1 == lv2
        if same and ((best >= prod) if ratio_closed else (best > prod)):                   # :112
            leave("ratio_rejected")
            continue
        held[bi] = i                                                                       # :115
        res["write"][i] = bi
        writes.append((i, bi))
        nmatches += 1 if one_count else 2                                                  # :116-117
        leave("matched")
    for i, j in writes:
        if held[j] != i:
            res["exit"][i] = E["overwritten_later"]
    res["match_cur"], res["n_matches"] = held.astype(np.int32), nmatches
    res["decidable"] = res["margin"] > 1
    return res
