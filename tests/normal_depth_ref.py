"""A literal NumPy restatement of MapPoint::UpdateNormalAndDepth (MapPoint.cc:361-407), the yardstick of asd_update_normal_and_depth
and asd_normal_and_depth_point.

The reference leaves the arithmetic to OpenCV (cv::norm, Mat / double, Mat / int); the rule restated here is the library's own, as
include/asd_slam.h states it, step by step in np.float32 / np.float64 scalars:

    d      = Pos - Ow_kf                                            f32, per component
    nrm    = sqrt(((double)dx*dx + (double)dy*dy) + (double)dz*dz)  f64
    unit_k = (float)((double)d_k * (1.0 / nrm))
    normal = normal + unit                                          f32, one observer after the other in ascending keyframe id, from zero
    mNormalVector_k = (float)((double)normal_k * (1.0 / (double)n_obs))
    dist          = (float)nrm  with kf = ref_kf
    mfMaxDistance = dist * scaleFactor[level]                       one f32 product
    mfMinDistance = mfMaxDistance / scaleFactor[nLevels - 1]        one f32 division (NumPy's is correctly rounded)

The map is a tests.culling_ref.CullingMap (observations, bad points, octaves) plus a dict of camera centres; the bank is an array
[rows][8] = Xw, normal, min_dist, max_dist as asd_mpbank_put stores it.  The ONE stated rule: mObservations is walked in ascending
keyframe id.  Status 3 (mpRefKF does not observe the point) is a state the reference cannot reach and is left untouched here.
"""
import numpy as np

UPDATED, BAD, NO_OBSERVATIONS, NO_REFERENCE = 0, 1, 2, 3
f32, f64 = np.float32, np.float64


def scale_table(scale_factor=1.2, n_levels=8):
    """mvScaleFactors (ORBextractor.cc:459-466): the float factor widened to double for the product, the product stored as float"""
    s = [f32(1.0)]
    for _ in range(1, n_levels):
        s.append(f32(f64(s[-1]) * f64(f32(scale_factor))))
    return np.array(s, np.float32)


def point(Ow, ref, Pos, scale_level, scale_top, order=None):
    """the rule for one point: Ow = the observers' centres in walk order, ref = the reference keyframe's index among them
    -> (normal [3] f32, min_dist f32, max_dist f32).  order: test aid, another order of the sum (indices into Ow)"""
    Ow = np.asarray(Ow, np.float32).reshape(-1, 3)
    Pos = np.asarray(Pos, np.float32)
    with np.errstate(all="ignore"):
        normal = [f32(0.0), f32(0.0), f32(0.0)]
        nrm_ref = None
        for k in (range(len(Ow)) if order is None else order):
            d = [f32(Pos[c] - Ow[k][c]) for c in range(3)]                         # :390
            dd = [f64(x) for x in d]
            nrm = np.sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2])         # cv::norm
            inv = f64(1.0) / nrm
            unit = [f32(dd[c] * inv) for c in range(3)]
            normal = [f32(normal[c] + unit[c]) for c in range(3)]                 # :391
            if k == ref:
                nrm_ref = nrm                                                       # :395-396
        inv_n = f64(1.0) / f64(len(Ow))
        out = np.array([f32(f64(normal[c]) * inv_n) for c in range(3)], np.float32)  # :405
        dist = f32(nrm_ref)
        mx = f32(dist * f32(scale_level))                                           # :403
        mn = f32(mx / f32(scale_top))                                               # :404
    return out, mn, mx


def update_normal_and_depth(m, centres, bank, rows, ref_kf, scale, Xw=None):
    """MapPoint.cc:361-407 for every point of `rows`, over the map m, the centres (keyframe -> [3]) and the bank [R][8], which is changed
    in place (with Xw: SetWorldPos first, whatever the status) -> dict(normal, min_dist, max_dist, status): what the bank now holds"""
    scale = np.asarray(scale, np.float32)
    status = []
    for i, (r, ref) in enumerate(zip(rows, ref_kf)):
        r, ref = int(r), int(ref)
        if Xw is not None:
            bank[r, 0:3] = np.asarray(Xw[i], np.float32)                            # SetWorldPos has no bad test
        obs = m.obs.get(r, {})
        if r in m.pt_bad:                                                           # :369
            status.append(BAD)
        elif not obs:                                                               # :381
            status.append(NO_OBSERVATIONS)
        elif ref not in m.kf_points or ref not in obs:
            status.append(NO_REFERENCE)
        else:
            kfs = sorted(obs)                                                       # ascending keyframe id
            level = m.octave[ref][obs[ref]]                                         # :397
            s_level = scale[level] if level < len(scale) else f32(0.0)
            normal, mn, mx = point([centres[k] for k in kfs], kfs.index(ref), bank[r, 0:3], s_level, scale[-1])
            bank[r, 3:6], bank[r, 6], bank[r, 7] = normal, mn, mx
            status.append(UPDATED)
    idx = [int(r) for r in rows]
    return dict(normal=bank[idx, 3:6].copy(), min_dist=bank[idx, 6].copy(), max_dist=bank[idx, 7].copy(), status=np.array(status, np.uint8))


def assert_bits(got, exp, what=""):
    """NaN positions coincide, every other value is equal bit for bit"""
    got, exp = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(exp, np.float32)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    ng, ne = np.isnan(got), np.isnan(exp)
    assert np.array_equal(ng, ne), f"{what}: NaN positions differ"
    a, b = got.view(np.uint32)[~ng], exp.view(np.uint32)[~ne]
    bad = np.nonzero(a != b)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {a.size} values differ, first {got[~ng][bad[0]]!r} != {exp[~ne][bad[0]]!r}"


def random_centres(m, seed, lo=-50.0, hi=50.0):
    rng = np.random.default_rng(seed)
    return {kf: rng.uniform(lo, hi, 3).astype(np.float32) for kf in sorted(m.kf_points)}


def random_bank(n_rows, seed, lo=-50.0, hi=50.0):
    """positions in [lo, hi), normals / ranges filled with recognisable values that no update produces"""
    rng = np.random.default_rng(seed)
    bank = np.empty((n_rows, 8), np.float32)
    bank[:, 0:3] = rng.uniform(lo, hi, (n_rows, 3))
    bank[:, 3:6] = rng.uniform(2.0, 3.0, (n_rows, 3))
    bank[:, 6] = -1.0
    bank[:, 7] = -2.0
    return bank
