"""numpy restatement of the per-keyframe stage in front of LocalBA, for tests/test_mapping_exits.py.  Written from the
reference's source text, independently of oracle/mapping.cpp, oracle/matcher.cpp and of the kernels:

  search_for_triangulation  ORBmatcher::SearchForTriangulation (ORBmatcher.cc:669-822, bOnlyStereo = false, no orientation
                            check: LocalMapping.cc:309 builds the matcher with checkOri = false) with
                            ORBmatcher::CheckDistEpipolarLine (:136-153)
  triangulate               the per-match body of LocalMapping::CreateNewMapPoints (LocalMapping.cc:386-523, monocular branch)
  fuse_search               ORBmatcher::Fuse(KeyFrame*, vector<MapPoint*>, th), search half (ORBmatcher.cc:825-937) with
                            KeyFrame::GetFeaturesInArea (KeyFrame.cc:839-878), KeyFrame::PosInGrid (:133-143),
                            KeyFrame::IsInImage (:880-883) and MapPoint::PredictScale (MapPoint.cc:421-436)

Arithmetic.  What decides a discrete result between descriptors is bit-comparable: the descriptor distance is accumulated in
f32 in component order 0..127 (stereo_ref.descriptor_distance), the epipolar line, the epipole distance and dsqr are single f32
operations in the order the reference writes them, `dsqr < 3.84 * sigma2` compares in double.  The geometric gates of
triangulate and fuse_search are evaluated in float64 (np.linalg.svd for the 4 x 4 system): the oracle already pins OpenCV's f32
evaluation order and a second copy of that order would only copy its assumptions.  Every float64 gate reports a MARGIN instead:
the distance of the gate quantity from its threshold divided by the tolerance below, the minimum over the gates the element
evaluated.  An element is DECIDABLE when its margin is > 1; an f32 chain that moves a decidable element across a gate is off by
more than rounding.

  REL_TOL   1e-2   relative, every gate that has no rule of its own (chi-square, distance range, viewing angle, scale ratio,
                   PredictScale's level boundaries as a ratio of distances)
  COS_TOL   1e-6   absolute, the parallax cosine against 0 and 0.9998
  DEPTH_TOL 1e-3   |z| against DEPTH_TOL * (distance of the point from that camera)
  PIXEL_TOL 1e-3   pixels, the window edge |dx| < r, |dy| < r of GetFeaturesInArea and the image bounds of IsInImage (a pixel
                   coordinate <= 1241 carries about 1e-4 px of f32 rounding)

Unreachable exits of triangulate, kept in EXITS because the source has them:
  * w_zero (:444): behind the parallax gate the two rays meet at an angle of at least acos(0.9998) = 1.15 degrees, so the
    least-squares point is finite and the last component of the unit null vector is about 1 / |X| -- it would need a point
    further than 1e38 away.  x3D.at(3) == 0 can occur in the SVD itself (a matrix whose null vector has a zero last
    component, e.g. an exactly zero first column); that is covered through asd_svd4_null.
  * dist_zero (:514): dist1 == 0 needs x3D == Ow1, where z1 = 0 has already left through :466; the same holds for dist2.
"""
import numpy as np

from tests.stereo_ref import descriptor_distance

F32 = np.float32
F64 = np.float64

TH_LOW = F32(0.5)                       # ORBmatcher.cc:38
GRID_COLS, GRID_ROWS = 64, 48           # Frame.h:37-38

REL_TOL, COS_TOL, DEPTH_TOL, PIXEL_TOL = 1e-2, 1e-6, 1e-3, 1e-3

# |x_oracle - x_ref| / |x_ref| over the accepted decidable pairs, CPU oracle against the float64 triangulate() below: the
# largest value over the sets tri_exits (5.6e-7), tri_exits_mixed_k (5.9e-7) and batch_mixed (4.51e-6, neighbour 0: the short
# forward baseline) of tests/test_mapping_exits.py, rounded up; test_coordinate_bound_is_the_measured_one keeps the figure
# honest.  The HIP kernels may evaluate in another legitimate f32 order, which the factor 4 allows for.
ORACLE_COORD_ERR = 4.6e-6
COORD_BOUND = 4 * ORACLE_COORD_ERR


def level_tables(n_levels=8, scale_factor=1.2):
    """mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2 as ORBextractor.cc:460-476 fills them (f32, cumulative product)"""
    s = np.ones(n_levels, F32)
    for i in range(1, n_levels):
        s[i] = s[i - 1] * F32(scale_factor)
    sigma2 = s * s
    return s, sigma2, F32(1.0) / sigma2


# ====================================================================================== SearchForTriangulation
# one name per way a keypoint of keyframe 1 can leave the function, in source order
SFT_EXITS = ("no_node",                 # the keypoint is in no node of vFeatVec1: never visited
             "node_absent_in_kf2",      # :699-787 the node walk never pairs its node
             "has_mp1",                 # :711
             "no_candidate_passed",     # :757 bestIdx2 < 0
             "matched")
SFT_EXIT = {n: i for i, n in enumerate(SFT_EXITS)}
SFT_COUNTERS = ("has_mp2", "dist", "epipole", "den_zero", "epipolar_line")


def _fv(nodes):
    """DBoW2::FeatureVector of a keyframe from one node id per keypoint (-1: none): node id -> members in keypoint order"""
    nodes = np.asarray(nodes)
    return {int(n): np.nonzero(nodes == n)[0] for n in np.unique(nodes[nodes >= 0])}


def search_for_triangulation(k1, d1, k2, d2, nodes1, nodes2, has1, has2, F12, ex, ey, scale, sigma2,
                             first_wins=False, max_candidates=None, max_nodes=None):
    """-> dict(match [n1] (index in keyframe 2 or -1), n_matches, exit, the counters of SFT_COUNTERS [n1], tie_replaced [n1],
    list_len [n1] (members of the keypoint's node in keyframe 2), n_nodes2).  The three keyword arguments are the mutants of the
    sensitivity test: the first candidate of equal distance kept, members / nodes of keyframe 2 beyond the first N ignored."""
    n1 = len(k1)
    d1 = np.ascontiguousarray(d1, F32).reshape(n1, -1)
    d2 = np.ascontiguousarray(d2, F32).reshape(len(k2), -1)
    F = np.asarray(F12, F32).reshape(3, 3)
    ex, ey = F32(ex), F32(ey)
    x1, y1 = k1["x"].astype(F32), k1["y"].astype(F32)
    x2, y2, o2 = k2["x"].astype(F32), k2["y"].astype(F32), k2["octave"].astype(np.int64)
    fv1, fv2 = _fv(nodes1), _fv(nodes2)
    if max_nodes is not None:
        fv2 = {n: fv2[n] for n in sorted(fv2)[:max_nodes]}
    match = np.full(n1, -1, np.int32)
    exit_code = np.full(n1, SFT_EXIT["no_node"], np.int32)
    counters = {c: np.zeros(n1, np.int64) for c in SFT_COUNTERS}
    tie_replaced = np.zeros(n1, bool)
    list_len = np.zeros(n1, np.int64)
    for node in sorted(fv1):                                       # :699 the ordered walk pairs exactly the common node ids
        if node not in fv2:
            exit_code[fv1[node]] = SFT_EXIT["node_absent_in_kf2"]
            continue
        members2 = fv2[node]
        cand_all = members2 if max_candidates is None else members2[:max_candidates]
        for i1 in fv1[node]:
            list_len[i1] = len(members2)
            if has1[i1]:                                            # :711
                exit_code[i1] = SFT_EXIT["has_mp1"]
                continue
            free = has2[cand_all] == 0                              # :730 (vbMatched2 is never set: :685 is its only write)
            counters["has_mp2"][i1] = int((~free).sum())
            cand = cand_all[free]
            dist = descriptor_distance(d1[i1], d2[cand])
            # epipolar line of kp1 in image 2 (:139-141), once per kp1: the operands do not depend on the candidate
            a = x1[i1] * F[0, 0] + y1[i1] * F[1, 0] + F[2, 0]
            b = x1[i1] * F[0, 1] + y1[i1] * F[1, 1] + F[2, 1]
            c = x1[i1] * F[0, 2] + y1[i1] * F[1, 2] + F[2, 2]
            den = a * a + b * b
            best_dist, best = TH_LOW, -1
            for j in range(len(cand)):
                dj = dist[j]
                if dj > TH_LOW or (dj >= best_dist and best >= 0 if first_wins else dj > best_dist):   # :737
                    counters["dist"][i1] += 1
                    continue
                i2 = cand[j]
                dex, dey = ex - x2[i2], ey - y2[i2]
                if dex * dex + dey * dey < F32(100) * scale[o2[i2]]:                                       # :746
                    counters["epipole"][i1] += 1
                    continue
                if den == 0:                                                                               # :147
                    counters["den_zero"][i1] += 1
                    continue
                num = a * x2[i2] + b * y2[i2] + c
                dsqr = num * num / den
                if not F64(dsqr) < 3.84 * F64(sigma2[o2[i2]]):                                             # :152
                    counters["epipolar_line"][i1] += 1
                    continue
                if best >= 0 and dj == best_dist:
                    tie_replaced[i1] = True
                best, best_dist = int(i2), dj
            match[i1] = best
            exit_code[i1] = SFT_EXIT["matched" if best >= 0 else "no_candidate_passed"]
    out = dict(match=match, n_matches=int((match >= 0).sum()), exit=exit_code, tie_replaced=tie_replaced, list_len=list_len,
               n_nodes2=len(fv2), n_nodes1=len(fv1))
    out.update(counters)
    return out


# ====================================================================================== CreateNewMapPoints, per match
TRI_EXITS = ("cos_nonpositive",         # :430 cosParallaxRays > 0 fails
             "low_parallax",            # :430 cosParallaxRays < 0.9998 fails -> :460
             "w_zero",                  # :444 (unreachable, see the module text)
             "z1",                      # :466
             "z2",                      # :470
             "chi2_image1",             # :486
             "chi2_image2",             # :502
             "dist_zero",               # :514 (unreachable)
             "ratio_low",               # :522 ratioDist * ratioFactor < ratioOctave
             "ratio_high",              # :522 ratioDist > ratioOctave * ratioFactor
             "accepted")
TRI_EXIT = {n: i for i, n in enumerate(TRI_EXITS)}


def _rel(q, thr):
    return abs(q - thr) / (REL_TOL * abs(thr))


def triangulate(k1, k2, idx1, idx2, T1, T2, K1, K2, scale, sigma2, ratio_factor,
                k2_is_k1=False, sigma2_from_octave1=False, drop_gate2=False, swap_ratio=False):
    """-> dict(ok [n] u8, X [n][3] f64 (NaN where the SVD was not reached), exit [n], margin [n]).  The keyword arguments are
    the mutants of the sensitivity test."""
    n = len(idx1)
    T1, T2 = np.asarray(T1, F32).astype(F64), np.asarray(T2, F32).astype(F64)
    K1 = np.asarray(K1, F32).astype(F64)
    K2 = K1 if k2_is_k1 else np.asarray(K2, F32).astype(F64)
    scale, sigma2 = np.asarray(scale, F32).astype(F64), np.asarray(sigma2, F32).astype(F64)
    rf = F64(F32(ratio_factor))
    R1, t1, R2, t2 = T1[:3, :3], T1[:3, 3], T2[:3, :3], T2[:3, 3]
    O1, O2 = -R1.T @ t1, -R2.T @ t2
    ok = np.zeros(n, np.uint8)
    X = np.full((n, 3), np.nan)
    exit_code = np.zeros(n, np.int32)
    margin = np.full(n, np.inf)
    for i in range(n):
        a, b = k1[idx1[i]], k2[idx2[i]]
        u1, v1, o1 = F64(a["x"]), F64(a["y"]), int(a["octave"])
        u2, v2, o2 = F64(b["x"]), F64(b["y"]), int(b["octave"])
        m = np.inf

        def leave(name):
            exit_code[i] = TRI_EXIT[name]
            margin[i] = m

        xn1 = np.array([(u1 - K1[2]) / K1[0], (v1 - K1[3]) / K1[1], 1.0])         # :410-411
        xn2 = np.array([(u2 - K2[2]) / K2[0], (v2 - K2[3]) / K2[1], 1.0])
        ray1, ray2 = R1.T @ xn1, R2.T @ xn2
        cos = ray1 @ ray2 / (np.linalg.norm(ray1) * np.linalg.norm(ray2))          # :416
        m = min(m, abs(cos) / COS_TOL)
        if not cos > 0:
            leave("cos_nonpositive")
            continue
        m = min(m, abs(cos - 0.9998) / COS_TOL)
        if not cos < 0.9998:
            leave("low_parallax")
            continue
        A = np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1],             # :434-437
                      xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]])
        v = np.linalg.svd(A)[2][3]
        if v[3] == 0:
            leave("w_zero")
            continue
        x = v[:3] / v[3]
        X[i] = x
        d1, d2 = np.linalg.norm(x - O1), np.linalg.norm(x - O2)
        z1 = R1[2] @ x + t1[2]
        m = min(m, abs(z1) / (DEPTH_TOL * d1))
        if z1 <= 0:
            leave("z1")
            continue
        z2 = R2[2] @ x + t2[2]
        m = min(m, abs(z2) / (DEPTH_TOL * d2))
        if z2 <= 0:
            leave("z2")
            continue
        e1 = np.array([K1[0] * (R1[0] @ x + t1[0]) / z1 + K1[2] - u1, K1[1] * (R1[1] @ x + t1[1]) / z1 + K1[3] - v1])
        m = min(m, _rel(e1 @ e1, 5.991 * sigma2[o1]))
        if e1 @ e1 > 5.991 * sigma2[o1]:
            leave("chi2_image1")
            continue
        if not drop_gate2:
            s2 = sigma2[o1] if sigma2_from_octave1 else sigma2[o2]
            e2 = np.array([K2[0] * (R2[0] @ x + t2[0]) / z2 + K2[2] - u2, K2[1] * (R2[1] @ x + t2[1]) / z2 + K2[3] - v2])
            m = min(m, _rel(e2 @ e2, 5.991 * s2))
            if e2 @ e2 > 5.991 * s2:
                leave("chi2_image2")
                continue
        if d1 == 0 or d2 == 0:
            leave("dist_zero")
            continue
        ratio_dist = d1 / d2 if swap_ratio else d2 / d1                             # :517
        ratio_octave = scale[o1] / scale[o2]
        m = min(m, _rel(ratio_dist * rf, ratio_octave))
        if ratio_dist * rf < ratio_octave:
            leave("ratio_low")
            continue
        m = min(m, _rel(ratio_dist, ratio_octave * rf))
        if ratio_dist > ratio_octave * rf:
            leave("ratio_high")
            continue
        ok[i] = 1
        leave("accepted")
    return dict(ok=ok, X=X, exit=exit_code, margin=margin, decidable=margin > 1)


# ====================================================================================== Fuse, search half
FUSE_EXITS = ("invalid",                # :846-850 !pMP || isBad() || IsInKeyFrame(pKF)
              "behind",                 # :856
              "outside_image",          # :867
              "too_near",               # :878 dist3D < 0.8 * mfMinDistance
              "too_far",                # :878 dist3D > 1.2 * mfMaxDistance
              "viewing_angle",          # :884
              "window_empty",           # :894
              "no_candidate_passed",    # :937 with bestIdx == -1: every window candidate failed the level or the 5.99 gate
              "above_th_low",           # :937 bestDist > TH_LOW
              "matched")
FUSE_EXIT = {n: i for i, n in enumerate(FUSE_EXITS)}
FUSE_COUNTERS = ("level_below", "level_above", "chi2")


def _c_round(x):
    """C round() of f32 values: halfway cases away from zero"""
    x = np.asarray(x, F32)
    t = np.trunc(x)
    return (t + np.where(np.abs(x - t) >= F32(0.5), np.copysign(F32(1), x), F32(0))).astype(np.int64)


def grid_cells(kps, bounds):
    """(col, row) -> keypoint indices in index order, as the KeyFrame constructor fills mGrid (KeyFrame.cc:120-131) through
    PosInGrid (:133-143, f32, C round, cells outside the grid dropped)"""
    min_x, max_x, min_y, max_y = (F32(b) for b in bounds)
    inv_w = F32(GRID_COLS) / (max_x - min_x)
    inv_h = F32(GRID_ROWS) / (max_y - min_y)
    cx = _c_round((kps["x"].astype(F32) - min_x) * inv_w)
    cy = _c_round((kps["y"].astype(F32) - min_y) * inv_h)
    cells = {}
    for i in range(len(kps)):
        if 0 <= cx[i] < GRID_COLS and 0 <= cy[i] < GRID_ROWS:
            cells.setdefault((int(cx[i]), int(cy[i])), []).append(i)
    return {k: np.array(v, np.int64) for k, v in cells.items()}, F64(inv_w), F64(inv_h)


def fuse_search(kps, desc, bounds, valid, Xw, normal, min_dist, max_dist, mp_desc, Tcw, K, th, scale, inv_sigma2, n_levels,
                scale_factor, closed_upper=False, level_wide=False, last_wins=False, column_cap=None):
    """-> dict(best_idx [n] (-1 unless matched), best_dist [n] f32 (bestDist at :937, 256 where no candidate passed, NaN where
    the search was not reached; the library returns it for matched points and 256 for every other), exit, margin, decidable, the counters of FUSE_COUNTERS, level (-1: not reached),
    level_clamped_low / _high, tie_first_wins, n_in_window, max_column (the largest number of window candidates one cell
    column contributed).  The keyword arguments are the mutants of the sensitivity test; column_cap ignores the members of one
    cell column's row range beyond the first N."""
    n = len(valid)
    desc = np.ascontiguousarray(desc, F32).reshape(len(kps), -1)
    mp_desc = np.ascontiguousarray(mp_desc, F32).reshape(n, -1)
    T = np.asarray(Tcw, F32).astype(F64)
    R, t = T[:3, :3], T[:3, 3]
    Ow = -R.T @ t
    fx, fy, cx, cy = np.asarray(K, F32).astype(F64)
    min_x, max_x, min_y, max_y = (F64(F32(b)) for b in bounds)
    cells, inv_w, inv_h = grid_cells(kps, bounds)
    kx, ky, ko = kps["x"].astype(F64), kps["y"].astype(F64), kps["octave"].astype(np.int64)
    scale64, inv_sigma2_64 = np.asarray(scale, F32).astype(F64), np.asarray(inv_sigma2, F32).astype(F64)
    log_sf = np.log(F64(F32(scale_factor)))
    q_tol = np.log1p(REL_TOL) / log_sf                        # REL_TOL on the ratio of distances, in units of levels
    best_idx = np.full(n, -1, np.int32)
    best_dist = np.full(n, np.nan, F32)
    exit_code = np.zeros(n, np.int32)
    margin = np.full(n, np.inf)
    counters = {c: np.zeros(n, np.int64) for c in FUSE_COUNTERS}
    level = np.full(n, -1, np.int64)
    clamp_lo, clamp_hi, tie = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    n_in_window, max_column = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        m = np.inf

        def leave(name):
            exit_code[i] = FUSE_EXIT[name]
            margin[i] = m

        if not valid[i]:
            leave("invalid")
            continue
        p = Xw[i].astype(F64)
        pc = R @ p + t
        PO = p - Ow
        dist3d = np.linalg.norm(PO)
        m = min(m, abs(pc[2]) / (DEPTH_TOL * dist3d))
        if pc[2] < 0:
            leave("behind")
            continue
        u, v = fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy
        m = min(m, min(abs(u - min_x), abs(u - max_x), abs(v - min_y), abs(v - max_y)) / PIXEL_TOL)
        if closed_upper:
            inside = min_x <= u <= max_x and min_y <= v <= max_y
        else:
            inside = min_x <= u < max_x and min_y <= v < max_y
        if not inside:
            leave("outside_image")
            continue
        lo, hi = F64(F32(0.8)) * F64(min_dist[i]), F64(F32(1.2)) * F64(max_dist[i])     # MapPoint.cc:409-419
        m = min(m, _rel(dist3d, lo))
        if dist3d < lo:
            leave("too_near")
            continue
        m = min(m, _rel(dist3d, hi))
        if dist3d > hi:
            leave("too_far")
            continue
        dot = PO @ normal[i].astype(F64)
        m = min(m, _rel(dot, 0.5 * dist3d))
        if dot < 0.5 * dist3d:
            leave("viewing_angle")
            continue
        q = np.log(F64(max_dist[i]) / dist3d) / log_sf                                   # MapPoint.cc:426-429
        n_scale = int(np.ceil(q))
        # ceil(q) changes at the integers; those in [0, n_levels - 2] change the clamped level
        near = np.round(q)
        if 0 <= near <= n_levels - 2:
            m = min(m, abs(q - near) / q_tol)
        clamp_lo[i], clamp_hi[i] = n_scale < 0, n_scale >= n_levels
        lvl = min(max(n_scale, 0), n_levels - 1)
        level[i] = lvl
        r = F64(F32(th)) * scale64[lvl]
        # GetFeaturesInArea (KeyFrame.cc:844-858)
        window = []
        c0, c1 = max(0, int(np.floor((u - min_x - r) * inv_w))), min(GRID_COLS - 1, int(np.ceil((u - min_x + r) * inv_w)))
        r0, r1 = max(0, int(np.floor((v - min_y - r) * inv_h))), min(GRID_ROWS - 1, int(np.ceil((v - min_y + r) * inv_h)))
        if c0 < GRID_COLS and c1 >= 0 and r0 < GRID_ROWS and r1 >= 0:
            for ix in range(c0, c1 + 1):
                col = [cells[(ix, iy)] for iy in range(r0, r1 + 1) if (ix, iy) in cells]
                if not col:
                    continue
                col = np.concatenate(col)
                if column_cap is not None:
                    col = col[:column_cap]
                dx, dy = np.abs(kx[col] - u), np.abs(ky[col] - v)
                edge = (dx < r + PIXEL_TOL) & (dy < r + PIXEL_TOL)
                if edge.any():
                    m = min(m, np.minimum(np.abs(dx[edge] - r), np.abs(dy[edge] - r)).min() / PIXEL_TOL)
                inside = col[(dx < r) & (dy < r)]
                max_column[i] = max(max_column[i], len(inside))
                window.append(inside)
        window = np.concatenate(window) if window else np.zeros(0, np.int64)
        n_in_window[i] = len(window)
        if len(window) == 0:
            leave("window_empty")
            continue
        lo_l, hi_l = (lvl - 2, lvl + 1) if level_wide else (lvl - 1, lvl)
        below, above = ko[window] < lo_l, ko[window] > hi_l                                # :911
        counters["level_below"][i], counters["level_above"][i] = int(below.sum()), int(above.sum())
        cand = window[~below & ~above]
        e2 = (u - kx[cand]) ** 2 + (v - ky[cand]) ** 2
        chi = e2 * inv_sigma2_64[ko[cand]]
        if len(cand):
            m = min(m, (np.abs(chi - 5.99) / (REL_TOL * 5.99)).min())
        counters["chi2"][i] = int((chi > 5.99).sum())                                      # :921
        cand = cand[~(chi > 5.99)]
        bd, bi = F32(256), -1
        if len(cand):
            dist = descriptor_distance(mp_desc[i], desc[cand])
            lowest = dist.min()
            where = np.nonzero(dist == lowest)[0]
            j = where[-1] if last_wins else where[0]                                       # :929 strict <: the first of equals
            if lowest < bd:
                bd, bi = lowest, int(cand[j])
                tie[i] = len(where) > 1
        best_dist[i] = bd
        if bi < 0:
            leave("no_candidate_passed")
        elif bd <= TH_LOW:                                                                 # :937
            best_idx[i] = bi
            leave("matched")
        else:
            leave("above_th_low")
    out = dict(best_idx=best_idx, best_dist=best_dist, exit=exit_code, margin=margin, decidable=margin > 1, level=level,
               level_clamped_low=clamp_lo, level_clamped_high=clamp_hi, tie_first_wins=tie, n_in_window=n_in_window,
               max_column=max_column)
    out.update(counters)
    return out


def census(res, exits, extra=()):
    """exit name -> number of elements, plus the sums of the named counters / flags"""
    out = {name: int((res["exit"] == i).sum()) for i, name in enumerate(exits)}
    for name in extra:
        out[name] = int(np.asarray(res[name]).astype(np.int64).sum())
    return out
