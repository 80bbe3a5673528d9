"""numpy restatement of Frame::ComputeStereoMatches (Frame.cc:360-535), for tests/test_stereo.py.  Written from the
reference's source text, independently of oracle/stereo.cpp and of k_stereo_match:

  row table    (:370-388)  right keypoint iR is a candidate of every row in [floor(y - r), ceil(y + r)], r = 2 * scale[octave]
  search       (:399-444)  octave window levelL +- 1, inclusive gate uL - maxD <= uR <= uL, first strict minimum from TH_HIGH
  threshold    (:366,:447) thOrbDist = int((TH_HIGH + TH_LOW) / 2) = 1
  SAD slide    (:449-487)  11 x 11 windows, centre pixel subtracted, 11 positions, first strict minimum
  parabola fit (:489-503)
  gates        (:505-517)  0 <= disparity < maxD, disparity <= 0 -> 0.01
  median       (:521-534)  matches whose SAD is >= 1.5 * 1.4 * median are removed

Arithmetic that makes the results bit-comparable: the descriptor distance is accumulated in f32 in component order 0..127
(np.float32 array operations: numpy does not fuse a multiply into an add), the SAD values are integers (cv::norm sums
|a - b| of integer-valued floats <= 510: exact in any order and in any type), the parabola fit, the rescale and
mbf / disparity are single f32 operations in the order the reference writes them, `round` is C roundf.

Where the reference has undefined behaviour or throws, the library defines the result and this file states the same rule:
  * rows of the table outside the image are not filled (:386 writes vRowIndices[yi] unchecked), a left keypoint whose
    truncated row lies outside the image has no match (:406 reads vRowIndices[vL] unchecked);
  * WINDOW RULE: an 11 x 11 window that would leave the level image (cv::Mat::rowRange / colRange throw) leaves the
    keypoint unmatched, see _window_outside;
  * no match at all: the median filter is skipped (:522 reads vDistIdx[0] of an empty vector), n_matched = 0.
"""
import numpy as np

F32 = np.float32

# one name per way a left keypoint can leave the function, in source order
EXITS = ("row_outside",       # truncated row not in [0, nRows)
         "row_empty",         # :408 no right keypoint covers the row
         "maxu_negative",     # :414
         "dist_threshold",    # :447 best distance >= 1 (also: no candidate passed the octave window and the uR gate)
         "iniu_endu",         # :470
         "window_guard",      # the window rule
         "bestinc_edge",      # :489
         "delta_range",       # :499 (unreachable: |deltaR| <= 0.5 after :489, see test_stereo.py)
         "disparity_range",   # :507
         "median_removed",    # :527-533
         "matched")
EXIT = {name: i for i, name in enumerate(EXITS)}

TH_HIGH, TH_LOW = F32(1.5), F32(0.5)
TH_ORB_DIST = int((TH_HIGH + TH_LOW) / F32(2))          # `const int thOrbDist` (:366) truncates 1.0f
INT_MAX = (1 << 31) - 1


def roundf(x):
    """C roundf on one f32: nearest, halfway cases away from zero (x - trunc(x) is exact)"""
    x = F32(x)
    t = np.trunc(x)
    if abs(x - t) >= F32(0.5):
        t = t + np.copysign(F32(1), x)
    return F32(t)


def descriptor_distance(a, B):
    """ORBmatcher::DescriptorDistance of one descriptor against the rows of B: sum_k (a_k - b_k)^2, f32, k = 0..127 in order"""
    acc = np.zeros(len(B), F32)
    for k in range(B.shape[1]):
        d = a[k] - B[:, k]
        acc = acc + d * d
    return acc


def _window_outside(xl, yl, xr, w, h):
    """WINDOW RULE (the library's defined behaviour where the reference would throw from cv::Mat::rowRange / colRange):
    the left window is [xl-5, xl+5] x [yl-5, yl+5], the right windows span [xr-10, xr+10] on the same rows, all on one level
    image of w x h pixels.  Evaluated after the iniu / endu test of :470."""
    return xl - 5 < 0 or xl + 5 >= w or yl - 5 < 0 or yl + 5 >= h or xr - 10 < 0 or xr + 10 >= w


def stereo_match(kps_l, desc_l, kps_r, desc_r, pyr_l, pyr_r, scale, inv_scale, mb, mbf):
    """kps_*: structured arrays with x, y, octave; desc_*: [n, 128] f32; pyr_*: per level u8 [h, w] (mvImagePyramid of the left
    and the right extractor); scale / inv_scale: mvScaleFactors / mvInvScaleFactors; mb, mbf as Frame keeps them (f32).
    Returns a dict: u_right, depth (f32 [N]), n_matched, exit (index into EXITS per left keypoint), the intermediate values
    best_iR (-1: search not reached), best_dist, bestincR, deltaR (NaN: not reached), sad (-1: not reached), and the properties
    n_cand (size of the keypoint's row), tie (the minimum distance is shared by several gated candidates), clamped
    (disparity <= 0 -> 0.01), median_skipped (no match at all)."""
    N, Nr = len(kps_l), len(kps_r)
    desc_l = np.ascontiguousarray(desc_l, F32).reshape(N, -1)
    desc_r = np.ascontiguousarray(desc_r, F32).reshape(Nr, -1)
    scale, inv_scale = np.asarray(scale, F32), np.asarray(inv_scale, F32)
    mb, mbf = F32(mb), F32(mbf)
    xr_all, yr_all, or_all = kps_r["x"].astype(F32), kps_r["y"].astype(F32), kps_r["octave"].astype(np.int64)
    u_right, depth = np.full(N, -1, F32), np.full(N, -1, F32)
    exit_code = np.full(N, -1, np.int32)
    best_iR, bestincR = np.full(N, -1, np.int64), np.zeros(N, np.int64)
    best_dist = np.full(N, TH_HIGH, F32)
    deltaR_out = np.full(N, np.nan, F32)
    sad_out = np.full(N, -1, np.int64)
    n_cand = np.zeros(N, np.int64)
    tie, clamped = np.zeros(N, bool), np.zeros(N, bool)

    nRows = pyr_l[0].shape[0]
    rows = [[] for _ in range(nRows)]
    for iR in range(Nr):
        r = F32(2.0) * scale[or_all[iR]]
        maxr = int(np.ceil(yr_all[iR] + r))
        minr = int(np.floor(yr_all[iR] - r))
        for yi in range(max(minr, 0), min(maxr, nRows - 1) + 1):
            rows[yi].append(iR)
    rows = [np.array(c, np.int64) for c in rows]

    minZ = mb
    minD = F32(0)
    maxD = mbf / minZ
    vDistIdx = []
    for iL in range(N):
        levelL = int(kps_l["octave"][iL])
        vL, uL = F32(kps_l["y"][iL]), F32(kps_l["x"][iL])
        row = int(vL)                                             # truncation toward zero, like the float -> index conversion
        if row < 0 or row >= nRows:
            exit_code[iL] = EXIT["row_outside"]
            continue
        cand = rows[row]
        n_cand[iL] = len(cand)
        if len(cand) == 0:
            exit_code[iL] = EXIT["row_empty"]
            continue
        minU = uL - maxD
        maxU = uL - minD
        if maxU < 0:
            exit_code[iL] = EXIT["maxu_negative"]
            continue
        gate = (or_all[cand] >= levelL - 1) & (or_all[cand] <= levelL + 1) & (xr_all[cand] >= minU) & (xr_all[cand] <= maxU)
        cand = cand[gate]                                         # candidate order kept
        bestDist, bestIdxR = TH_HIGH, 0
        if len(cand):
            dist = descriptor_distance(desc_l[iL], desc_r[cand])
            j = int(np.argmin(dist))                              # first occurrence of the minimum = first strict `<`
            if dist[j] < bestDist:
                bestDist, bestIdxR = dist[j], int(cand[j])
                tie[iL] = int((dist == dist[j]).sum()) > 1
        best_dist[iL] = bestDist
        if not bestDist < TH_ORB_DIST:
            exit_code[iL] = EXIT["dist_threshold"]
            continue
        best_iR[iL] = bestIdxR
        uR0 = xr_all[bestIdxR]
        scaleFactor = inv_scale[levelL]
        scaleduL = roundf(uL * scaleFactor)
        scaledvL = roundf(vL * scaleFactor)
        scaleduR0 = roundf(uR0 * scaleFactor)
        w, L = 5, 5
        imL, imR = pyr_l[levelL], pyr_r[levelL]
        iniu = scaleduR0 + F32(L) - F32(w)
        endu = scaleduR0 + F32(L) + F32(w) + F32(1)
        if iniu < 0 or endu >= imR.shape[1]:
            exit_code[iL] = EXIT["iniu_endu"]
            continue
        xl, yl, xr = int(scaleduL), int(scaledvL), int(scaleduR0)
        if _window_outside(xl, yl, xr, imL.shape[1], imL.shape[0]):
            exit_code[iL] = EXIT["window_guard"]
            continue
        IL = imL[yl - w:yl + w + 1, xl - w:xl + w + 1].astype(np.int64)
        IL = IL - IL[w, w]
        bestDistS, binc = F32(INT_MAX), 0
        vDists = np.zeros(2 * L + 1, F32)
        for incR in range(-L, L + 1):
            IR = imR[yl - w:yl + w + 1, xr + incR - w:xr + incR + w + 1].astype(np.int64)
            IR = IR - IR[w, w]
            d = F32(np.abs(IL - IR).sum())
            if d < bestDistS:
                bestDistS, binc = d, incR
            vDists[L + incR] = d
        bestincR[iL] = binc
        sad_out[iL] = int(bestDistS)
        if binc == -L or binc == L:
            exit_code[iL] = EXIT["bestinc_edge"]
            continue
        dist1, dist2, dist3 = vDists[L + binc - 1], vDists[L + binc], vDists[L + binc + 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            deltaR = (dist1 - dist3) / (F32(2.0) * (dist1 + dist3 - F32(2.0) * dist2))
        deltaR_out[iL] = deltaR
        if deltaR < -1 or deltaR > 1:
            exit_code[iL] = EXIT["delta_range"]
            continue
        bestuR = scale[levelL] * (scaleduR0 + F32(binc) + deltaR)
        disparity = uL - bestuR
        if disparity >= minD and disparity < maxD:
            if disparity <= 0:
                disparity = F32(0.01)
                bestuR = F32(np.float64(uL) - 0.01)               # `uL-0.01` is a double expression stored to a float
                clamped[iL] = True
            depth[iL] = mbf / disparity
            u_right[iL] = bestuR
            vDistIdx.append((int(bestDistS), iL))
            exit_code[iL] = EXIT["matched"]
        else:
            exit_code[iL] = EXIT["disparity_range"]

    kept = 0
    if vDistIdx:
        vDistIdx.sort()
        median = F32(vDistIdx[len(vDistIdx) // 2][0])
        thDist = F32(1.5) * F32(1.4) * median
        kept = len(vDistIdx)
        for first, second in reversed(vDistIdx):
            if F32(first) < thDist:
                break
            u_right[second] = -1
            depth[second] = -1
            exit_code[second] = EXIT["median_removed"]
            kept -= 1
    assert (exit_code >= 0).all()
    return dict(u_right=u_right, depth=depth, n_matched=kept, exit=exit_code, best_iR=best_iR, best_dist=best_dist,
                bestincR=bestincR, deltaR=deltaR_out, sad=sad_out, n_cand=n_cand, tie=tie, clamped=clamped,
                median_skipped=not vDistIdx)


def census(res):
    """exit name -> number of left keypoints, plus the properties of the coverage table"""
    out = {name: int((res["exit"] == i).sum()) for i, name in enumerate(EXITS)}
    out["clamped_0.01"] = int(res["clamped"].sum())
    out["tie"] = int(res["tie"].sum())
    out["rows_gt_64"] = int((res["n_cand"] > 64).sum())
    out["rows_gt_128"] = int((res["n_cand"] > 128).sum())
    out["median_skipped"] = int(res["median_skipped"])
    return out
