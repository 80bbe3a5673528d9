"""numpy restatement of OpenCV 3.2.0's cv::undistort as the reference calls it (Tracking.cc:104,125: newCameraMatrix empty,
CV_32F mK / mDistCoef with four coefficients), for tests/test_undistort.py.  Written from the semantics listed at the top of
asd-slam_amd/csrc/undistort.hip, independently of that code:

  undistort_map -- initUndistortRectifyMap stripe by stripe into the CV_16SC2 + CV_16UC1 pair (cv::invert's closed-form 3x3
                   inverse, _x / _y / _w accumulated column by column: np.add.accumulate over float64 is sequential);
  remap         -- remap INTER_LINEAR with 15-bit fixed-point weights, BORDER_CONSTANT 0.

Every float operation below is one IEEE double operation in the order OpenCV writes it (numpy does not fuse).
"""
import numpy as np

INT_MIN = -(1 << 31)


def _round_sat(v):
    """saturate_cast<int>(double) = cvRound (cvtsd2si): half to even, INT_MIN for NaN / out of range"""
    r = np.rint(v)
    ok = (r >= INT_MIN) & (r <= (1 << 31) - 1)
    return np.where(ok, np.nan_to_num(r), INT_MIN).astype(np.int64)


def _inv3(S):
    """cv::invert(DECOMP_LU) of a 3x3 double matrix: det3, cofactors, times 1/det"""
    d = (S[0][0] * (S[1][1] * S[2][2] - S[1][2] * S[2][1]) - S[0][1] * (S[1][0] * S[2][2] - S[1][2] * S[2][0]) +
         S[0][2] * (S[1][0] * S[2][1] - S[1][1] * S[2][0]))
    d = 1.0 / d
    return [(S[1][1] * S[2][2] - S[1][2] * S[2][1]) * d, (S[0][2] * S[2][1] - S[0][1] * S[2][2]) * d,
            (S[0][1] * S[1][2] - S[0][2] * S[1][1]) * d, (S[1][2] * S[2][0] - S[1][0] * S[2][2]) * d,
            (S[0][0] * S[2][2] - S[0][2] * S[2][0]) * d, (S[0][2] * S[1][0] - S[0][0] * S[1][2]) * d,
            (S[1][0] * S[2][1] - S[1][1] * S[2][0]) * d, (S[0][1] * S[2][0] - S[0][0] * S[2][1]) * d,
            (S[0][0] * S[1][1] - S[0][1] * S[1][0]) * d]


def _row_accumulate(first, step, rows, w):
    a = np.empty((rows, w), np.float64)
    a[:, 0] = first
    a[:, 1:] = step
    return np.add.accumulate(a, axis=1)


def undistort_map(K, dist, w, h):
    """-> (xy int16 [h, w, 2], frac uint16 [h, w]) as cv::undistort's internal map pair"""
    fx, fy, u0, v0 = (float(np.float32(k)) for k in K)
    k1, k2, p1, p2 = (float(np.float32(c)) for c in (dist if dist is not None else (0, 0, 0, 0)))
    k3 = 0.0
    xy = np.empty((h, w, 2), np.int16)
    frac = np.empty((h, w), np.uint16)
    stripe0 = min(max(1, 4096 // w), h)
    for ys in range(0, h, stripe0):
        rows = min(stripe0, h - ys)
        ir = _inv3([[fx, 0.0, u0], [0.0, fy, v0 - ys], [0.0, 0.0, 1.0]])
        i = np.arange(rows, dtype=np.float64)
        _x = _row_accumulate(i * ir[1] + ir[2], ir[0], rows, w)
        _y = _row_accumulate(i * ir[4] + ir[5], ir[3], rows, w)
        _w = _row_accumulate(i * ir[7] + ir[8], ir[6], rows, w)
        ww = 1.0 / _w
        x = _x * ww
        y = _y * ww
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = 2 * x * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
        yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
        u = fx * xd + u0
        v = fy * yd + v0
        iu = _round_sat(u * 32)
        iv = _round_sat(v * 32)
        xy[ys:ys + rows, :, 0] = (iu >> 5).astype(np.int16)
        xy[ys:ys + rows, :, 1] = (iv >> 5).astype(np.int16)
        frac[ys:ys + rows] = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return xy, frac


def remap(img, xy, frac):
    """remap(img, map1 = xy, map2 = frac, INTER_LINEAR, BORDER_CONSTANT 0) for a u8 image; output of the map's size"""
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    sx = xy[..., 0].astype(np.int64)
    sy = xy[..., 1].astype(np.int64)
    a = (frac & 31).astype(np.int64)
    b = ((frac >> 5) & 31).astype(np.int64)

    def px(x, y):
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(inside, img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.int64), 0)

    s = ((32 - a) * (32 - b) * 32 * px(sx, sy) + a * (32 - b) * 32 * px(sx + 1, sy) +
         (32 - a) * b * 32 * px(sx, sy + 1) + a * b * 32 * px(sx + 1, sy + 1))
    return ((s + (1 << 14)) >> 15).astype(np.uint8)


def undistort(img, K, dist):
    h, w = np.asarray(img).shape
    return remap(img, *undistort_map(K, dist, w, h))
