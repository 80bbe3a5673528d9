"""Every way out of the per-keyframe stage in front of LocalBA -- SearchForTriangulation, the triangulation body of
CreateNewMapPoints, the search half of Fuse -- reached by a crafted input and compared with tests/mapping_ref.py, a plain
restatement written from the reference's source text.  On the CPU the reference is compared with the oracle, on the GPU the
HIP entry points with both.

Coverage the reference reports over the crafted sets (test_coverage asserts >= 3 of each; counts of this revision):

  SearchForTriangulation   no_node 240, node_absent_in_kf2 3936, has_mp1 1099, no_candidate_passed 3274, matched 1069;
                           candidates dropped for has_mp2 55180, dist 83525, epipole 60, den_zero 16 (F_DEGENERATE),
                           epipolar_line 1055; tie_replaced 124; a member list of 268 (five chunks of 64), 143 node ids
  triangulate              cos_nonpositive 234, low_parallax 561, z1 234, z2 234, chi2_image1 234, chi2_image2 468,
                           ratio_low 235, ratio_high 250, accepted 1415
                           (w_zero, dist_zero: unreachable, see mapping_ref.py; w == 0 is covered in the SVD itself)
  Fuse                     invalid 12, behind 12, outside_image 19, too_near 12, too_far 12, viewing_angle 12, window_empty 12,
                           no_candidate_passed 36 (level_below 30360, level_above 8115, chi2 6107), above_th_low 12,
                           matched 315; level_clamped_high 21, tie_first_wins 40 (31 won by the larger index), 842 window
                           candidates, 497 of them from one cell column
                           (level_clamped_low: unreachable on a decidable element.  ceil(log(max / dist) / log 1.2) < 0 needs
                           max / dist <= 1 / 1.2, and then dist >= 1.2 * max has left through too_far, :878, unless the two
                           f32 roundings meet exactly.)

Undecidable share per set (margin <= 1 in mapping_ref's terms; the cap is 2 %, and 0 on the rows crafted for an exit), as
test_undecidable_share prints it: tri_exits 0 %, tri_exits_mixed_k 0 %, batch_mixed 0.47 % of neighbour 0's 851 matches and 0 %
of the others', fuse_exits 0 % (its six image-bound rows sit exactly on v = 376 / v = 0 by construction and are compared
regardless), fuse_crowded 0 % (its map points are chosen clear of every threshold with the reference alone: at two keypoints
per square pixel a large window otherwise has a candidate within 1e-3 px of its edge more often than not).
Sensitivity (results changed per mutant of the reference): K2 := K1 338, sigma2[o1] in the image-2 gate 234, second gate
dropped 215, ratio of distances inverted 762 (the two ratio tests as written are symmetric under exchanging them: the swap that
changes anything is dist1 / dist2 for dist2 / dist1), first-wins in SearchForTriangulation 122, members beyond 64 ignored 117,
nodes beyond 64 ignored 509, IsInImage closed above 3, level gate widened 24, last-wins in Fuse 40, column members beyond 64
ignored 229.
"""
import functools

import numpy as np
import pytest

from tests import mapping_ref as ref
from tests.test_matcher import BOUNDS, make_frame, perturbed_descriptors, pose_T

F32 = np.float32
K_KITTI = np.array([718.856, 718.856, 607.1928, 185.2157], F32)
K_EUROC = np.array([458.654, 457.296, 367.215, 248.375], F32)
BOUNDS_EUROC = (0.0, 752.0, 0.0, 480.0)
SCALE, SIGMA2, INV_SIGMA2 = ref.level_tables(8, 1.2)
RATIO_FACTOR = F32(1.5) * F32(1.2)                       # LocalMapping.cc:327
UNDECIDABLE_CAP = 0.02


def _kp_dtype():
    from tests.conftest import load_package
    return load_package().capi.KP_DTYPE


def _rt(T):
    T = np.asarray(T, F32).astype(np.float64)
    return T[:3, :3], T[:3, 3]


def _project(T, K, X):
    """pinhole projection through the centre: a point behind the camera still has a pixel"""
    R, t = _rt(T)
    K = np.asarray(K, F32).astype(np.float64)
    Xc = X @ R.T + t
    return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], 1), Xc[:, 2]


def _backproject(T, K, uv, depth):
    R, t = _rt(T)
    K = np.asarray(K, F32).astype(np.float64)
    Xc = np.stack([(uv[:, 0] - K[2]) / K[0] * depth, (uv[:, 1] - K[3]) / K[1] * depth, depth], 1)
    return (Xc - t) @ R


def _compose(T21, T1):
    return (np.asarray(T21, np.float64) @ np.asarray(T1, np.float64)).astype(F32)


def _relative(rv, centre):
    """pose of camera 2 relative to camera 1: rotation vector rv, camera 2's centre at `centre` in camera 1's frame"""
    T = pose_T(rv, (0, 0, 0)).astype(np.float64)
    T[:3, 3] = -T[:3, :3] @ np.asarray(centre, np.float64)
    return T


def _epipole(T1, T2, K2):
    """:675-683 camera 1's centre in image 2"""
    R1, t1 = _rt(T1)
    uv, _ = _project(T2, K2, (-R1.T @ t1)[None])
    return F32(uv[0, 0]), F32(uv[0, 1])


def _f12(T1, T2, K1, K2):
    """LocalMapping::ComputeF12 (LocalMapping.cc:638-655): K1^-T [t12]x R12 K2^-1"""
    R1, t1 = _rt(T1)
    R2, t2 = _rt(T2)
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    Km = [np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], np.float64) for K in (K1, K2)]
    return (np.linalg.inv(Km[0]).T @ tx @ R12 @ np.linalg.inv(Km[1])).astype(F32)


def _inside(uv, bounds, inset=20):
    return (uv[:, 0] > bounds[0] + inset) & (uv[:, 0] < bounds[1] - inset) & (uv[:, 1] > bounds[2] + inset) & (uv[:, 1] < bounds[3] - inset)


def _perpendicular(uv, e, px):
    """uv moved by px pixels across its epipolar line (the line through the epipole e)"""
    d = uv - np.asarray(e, np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return uv + px * np.stack([-d[:, 1], d[:, 0]], 1)


# ====================================================================================== tri_exits
T1_TRI = pose_T((0.01, -0.02, 0.005), (0.1, -0.05, 0.3))
T2_TRI = _compose(_relative((0.01, 0.5, 0.02), (0.5, -0.3, 40.0)), T1_TRI)     # 40 units ahead along z, 0.5 rad of yaw
PER_EXIT = 117


def _consistent_octaves(rng, rd):
    """octaves whose scale ratio follows the ratio of distances rd = dist2 / dist1"""
    k = np.clip(np.round(-np.log(rd) / np.log(1.2)).astype(int), -7, 7)
    o1 = np.array([rng.integers(max(0, -kk), 8 - max(0, kk)) for kk in k])
    return o1, o1 + k


@functools.lru_cache(None)
def tri_exits(mixed_k=False):
    """pairs crafted for each reachable exit of the triangulation body, joined in one call in mixed order; mixed_k: the two
    views are made with different intrinsics (batch_mixed has them the other way round).  -> dict(k1, k2, idx1, idx2, T1, T2, K1, K2, b1, b2, crafted [n] (exit the row was built
    for, -1: the noisy accepted population), ref)"""
    rng = np.random.default_rng(4100 + mixed_k)
    K1, K2, b1, b2 = (K_EUROC if mixed_k else K_KITTI), K_KITTI, (BOUNDS_EUROC if mixed_k else BOUNDS), BOUNDS
    T1, T2 = T1_TRI, T2_TRI
    R1, t1 = _rt(T1)
    R2, t2 = _rt(T2)
    O1, O2 = -R1.T @ t1, -R2.T @ t2
    e2 = _epipole(T1, T2, K2)
    e1 = _epipole(T2, T1, K1)

    def sample(lo, hi, z2_sign, want):
        uv1 = np.stack([rng.uniform(b1[0] + 20, b1[1] - 20, 60000), rng.uniform(b1[2] + 20, b1[3] - 20, 60000)], 1)
        X = _backproject(T1, K1, uv1, rng.uniform(lo, hi, 60000))
        uv2, z2 = _project(T2, K2, X)
        r1, r2 = (X - O1) * np.sign(lo), (X - O2) * z2_sign
        cos = (r1 * r2).sum(1) / np.linalg.norm(r1, axis=1) / np.linalg.norm(r2, axis=1)
        keep = np.nonzero(_inside(uv2, b2) & (z2 * z2_sign > 3) & (cos > 0.05) & ((cos < 0.999) | (abs(lo) > 1000)))[0][:want]
        assert len(keep) == want
        rd = np.linalg.norm(X[keep] - O2, axis=1) / np.linalg.norm(X[keep] - O1, axis=1)
        return uv1[keep], uv2[keep], rd

    E = ref.TRI_EXIT
    rows = []                                            # (uv1, uv2, o1, o2, crafted)
    want = 2 * PER_EXIT
    uv1, uv2, rd = sample(45, 90, 1, 2 * PER_EXIT)       # the accepted population: consistent octaves, 0.3 px of noise
    o1, o2 = _consistent_octaves(rng, rd)
    rows.append((uv1 + rng.normal(0, 0.3, uv1.shape), uv2 + rng.normal(0, 0.3, uv2.shape), o1, o2, -1))
    uv1, uv2, rd = sample(3000, 9000, 1, want)           # far away: the rays are parallel
    rows.append((uv1, uv2, *_consistent_octaves(rng, rd), E["low_parallax"]))
    uv1, uv2, rd = sample(-90, -45, -1, want)            # behind both cameras
    rows.append((uv1, uv2, *_consistent_octaves(rng, rd), E["z1"]))
    uv1, uv2, rd = sample(5, 35, -1, want)               # between the cameras: in front of the first, behind the second
    rows.append((uv1, uv2, *_consistent_octaves(rng, rd), E["z2"]))
    # rays more than 90 degrees apart: no point at all, two pixels on opposite sides of the yaw
    a = np.stack([rng.uniform(b1[0] + 20, b1[1] - 20, 60000), rng.uniform(b1[2] + 20, b1[3] - 20, 60000)], 1)
    b = np.stack([rng.uniform(b2[0] + 20, b2[1] - 20, 60000), rng.uniform(b2[2] + 20, b2[3] - 20, 60000)], 1)
    ray1 = np.stack([(a[:, 0] - K1[2]) / K1[0], (a[:, 1] - K1[3]) / K1[1], np.ones(len(a))], 1) @ R1
    ray2 = np.stack([(b[:, 0] - K2[2]) / K2[0], (b[:, 1] - K2[3]) / K2[1], np.ones(len(b))], 1) @ R2
    cos = (ray1 * ray2).sum(1) / np.linalg.norm(ray1, axis=1) / np.linalg.norm(ray2, axis=1)
    keep = np.nonzero(cos < -0.02)[0][:want]
    assert len(keep) == want
    rows.append((a[keep], b[keep], rng.integers(0, 8, want), rng.integers(0, 8, want), E["cos_nonpositive"]))
    uv1, uv2, rd = sample(45, 90, 1, want)               # 30 px across the epipolar line in image 1 at octave 0
    rows.append((_perpendicular(uv1, e1, 30.0), uv2, np.zeros(want, int), np.full(want, 3), E["chi2_image1"]))
    uv1, uv2, rd = sample(45, 90, 1, want)               # octave 7 / octave 0, 6 px across the line in image 2
    rows.append((uv1, _perpendicular(uv2, e2, 6.0), np.full(want, 7), np.zeros(want, int), E["chi2_image2"]))
    uv1, uv2, rd = sample(45, 90, 1, want)               # the same octaves without the offset
    rows.append((uv1, uv2, np.full(want, 7), np.zeros(want, int), E["ratio_low"]))
    uv1, uv2, rd = sample(110, 250, 1, want)             # octave 0 / octave 7 at dist2 / dist1 > 0.6
    rows.append((uv1, uv2, np.zeros(want, int), np.full(want, 7), E["ratio_high"]))
    # an offset of 8 px in image 2 leaves 4 px there and 4 px * z2 / z1 in image 1
    uv1, uv2, rd = sample(65, 110, 1, want)              # octave 1 / octave 2: the second gate alone rejects
    rows.append((uv1, _perpendicular(uv2, e2, 8.0), np.full(want, 1), np.full(want, 2), E["chi2_image2"]))
    uv1, uv2, rd = sample(52, 65, 1, want)               # octave 0 / octave 5: accepted with sigma2[5], not with sigma2[0]
    rows.append((uv1, _perpendicular(uv2, e2, 8.0), np.zeros(want, int), np.full(want, 5), E["accepted"]))

    KP = _kp_dtype()

    def frames(rows):
        n = sum(len(r[0]) for r in rows)
        k1, k2 = np.zeros(n, KP), np.zeros(n, KP)
        k1["size"] = k2["size"] = 31
        uv1, uv2 = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
        k1["x"], k1["y"], k1["octave"] = uv1[:, 0], uv1[:, 1], np.concatenate([r[2] for r in rows])
        k2["x"], k2["y"], k2["octave"] = uv2[:, 0], uv2[:, 1], np.concatenate([r[3] for r in rows])
        crafted = np.concatenate([np.full(len(r[0]), r[4]) for r in rows])
        return k1, k2, crafted

    # the rows built for an exit keep a clear margin (chosen with the reference alone), PER_EXIT of each
    k1, k2, crafted = frames(rows)
    ident = np.arange(len(k1), dtype=np.int32)
    pre = ref.triangulate(k1, k2, ident, ident, T1, T2, K1, K2, SCALE, SIGMA2, RATIO_FACTOR)
    keep, start = [np.arange(len(rows[0][0]))], len(rows[0][0])
    for r in rows[1:]:
        sel = start + np.nonzero((pre["margin"][start: start + len(r[0])] > 2) & (pre["exit"][start: start + len(r[0])] == r[4]))[0]
        assert len(sel) >= PER_EXIT, (r[4], len(sel), np.bincount(pre["exit"][start: start + len(r[0])], minlength=len(ref.TRI_EXITS)))
        keep.append(sel[:PER_EXIT])
        start += len(r[0])
    keep = np.concatenate(keep)
    k1, k2, crafted = k1[keep], k2[keep], crafted[keep]
    n = len(k1)
    assert n % 64 != 0 and n <= 2000
    perm2 = rng.permutation(n)                           # keyframe 2 stores its keypoints in another order
    inv2 = np.empty(n, np.int32)
    inv2[perm2] = np.arange(n, dtype=np.int32)
    k2 = k2[perm2].copy()
    idx1 = rng.permutation(n).astype(np.int32)           # one launch holds every exit in mixed order
    idx2 = inv2[idx1]
    s = dict(k1=k1, k2=k2, idx1=idx1, idx2=idx2, T1=T1, T2=T2, K1=K1, K2=K2, b1=b1, b2=b2, crafted=crafted[idx1])
    s["ref"] = ref.triangulate(k1, k2, idx1, idx2, T1, T2, K1, K2, SCALE, SIGMA2, RATIO_FACTOR)
    return s


def _check_tri(r, ok, x):
    """accept flags on the decidable pairs, rejected pairs zeroed; -> the largest relative coordinate error on the accepted
    decidable pairs"""
    dec = r["decidable"]
    np.testing.assert_array_equal(np.asarray(ok)[dec], r["ok"][dec])
    assert not np.asarray(x)[np.asarray(ok) == 0].any()
    acc = dec & (r["ok"] == 1) & (np.asarray(ok) == 1)
    if not acc.any():
        return 0.0
    return float((np.linalg.norm(np.asarray(x, np.float64)[acc] - r["X"][acc], axis=1) / np.linalg.norm(r["X"][acc], axis=1)).max())


# ====================================================================================== sft_crowded / batch_mixed
NODE_IDS = 7 + 13 * np.arange(150)                       # non-contiguous node ids; 144 of them are used by both keyframes
T1_SFT = pose_T((0.01, -0.02, 0.005), (0.1, -0.05, 0.3))
N_CUR = 1603


@functools.lru_cache(None)
def sft_current():
    """the current keyframe of sft_crowded and batch_mixed: keypoints, descriptors, the 3-D points behind them, nodes, has_mp"""
    rng = np.random.default_rng(5200)
    kc, dc = make_frame(N_CUR, 5201)
    X = _backproject(T1_SFT, K_KITTI, np.stack([kc["x"], kc["y"]], 1).astype(np.float64), rng.uniform(6, 40, N_CUR))
    kc["x"] += rng.normal(0, 0.3, N_CUR).astype(F32)
    kc["y"] += rng.normal(0, 0.3, N_CUR).astype(F32)
    node = NODE_IDS[np.arange(N_CUR) % 140]
    node[:400:2] = NODE_IDS[141]                          # one crowded node: 200 members here, 235 in the neighbour
    node[1400:1440] = -1                                  # keypoints without a node
    node[1440:1460] = NODE_IDS[145]                       # nodes the neighbour does not have
    node[1460:1480] = NODE_IDS[146]
    kc["x"][1500:1520] = 400.0                            # den == 0 under F_DEGENERATE
    has = (rng.uniform(size=N_CUR) < 0.2).astype(np.uint8)
    has[1500:1520] = 0
    return dict(kps=kc, desc=dc, X=X, nodes=node.astype(np.int32), has=has, T=T1_SFT, K=K_KITTI)


# a = 0, b = x1 - 400, c = -200 b: den == 0 exactly where x1 == 400, elsewhere dsqr = (y2 - 200)^2
F_DEGENERATE = np.array([[0, 1, -200], [0, 0, 0], [0, -400, 80000]], F32)


def _neighbour(seed, T2, K2, n_keep, crowded=False, node_limit=None):
    """a neighbour keyframe observing the current keyframe's points: shuffled, perturbed descriptors, its own has_mp"""
    cur = sft_current()
    rng = np.random.default_rng(seed)
    uv2, z2 = _project(T2, K2, cur["X"])
    src = rng.permutation(N_CUR)[:n_keep]                 # which point each neighbour keypoint observes
    kb = cur["kps"][src].copy()
    uv = uv2[src] + rng.normal(0, 0.3, (n_keep, 2))
    db = perturbed_descriptors(cur["desc"][src], 0.03, seed + 1)
    node = cur["nodes"][src].copy()
    has = (rng.uniform(size=n_keep) < 0.2).astype(np.uint8)
    e = _epipole(cur["T"], T2, K2)
    if crowded:
        # candidates a few pixels off the epipolar line: 3 px passes 3.84 * sigma2 at octave 7 and fails at octave 0
        off = np.nonzero((node != NODE_IDS[141]) & (node >= 0))[0][:120]
        uv[off] = _perpendicular(uv2[src[off]], e, 3.0)
        kb["octave"][off[:60]], kb["octave"][off[60:]] = 0, 7
        has[off] = 0
        # candidates within sqrt(100 * scale) of the epipole
        near = np.nonzero((node != NODE_IDS[141]) & (node >= 0))[0][120:150]
        ang = rng.uniform(0, 2 * np.pi, len(near))
        uv[near] = np.stack([e[0] + 4 * np.cos(ang), e[1] + 4 * np.sin(ang)], 1)
        has[near] = 0
        node[node == NODE_IDS[145]] = NODE_IDS[147]       # nodes present on one side only, both ways
        node[node == NODE_IDS[146]] = NODE_IDS[148]
    kb["x"], kb["y"] = uv[:, 0], uv[:, 1]
    if crowded:
        # duplicated rows: the same descriptor and position later in the same member list -> ties, the later candidate wins
        dup = np.concatenate([np.nonzero(node == NODE_IDS[141])[0][:80], np.nonzero((node != NODE_IDS[141]) & (node >= 0))[0][150:270]])
        kb, db, node, has = np.concatenate([kb, kb[dup]]), np.concatenate([db, db[dup]]), np.concatenate([node, node[dup]]), np.concatenate([has, has[dup]])
    if node_limit is not None:
        node = np.where(np.isin(node, NODE_IDS[:node_limit]), node, -1)
    return dict(kps=kb, desc=db, nodes=node.astype(np.int32), has=has, T=T2, K=K2, F12=_f12(cur["T"], T2, cur["K"], K2),
                ex=e[0], ey=e[1], bounds=BOUNDS_EUROC if K2 is K_EUROC else BOUNDS)


@functools.lru_cache(None)
def batch_mixed():
    """5 neighbours of sft_current(): [0] is sft_crowded's (more than 128 nodes, a member list of 235, ties, every candidate
    rejection), [1] tiny with other intrinsics, [2] at most 64 nodes, [3] an empty FeatureVector, [4] has_mp set everywhere"""
    T = [_compose(_relative(rv, c), T1_SFT) for rv, c in (((0.004, -0.01, 0.002), (0.3, 0.1, 1.6)), ((0.0, 0.03, 0.0), (0.9, 0.0, 0.2)),
                                                        ((0.01, 0.02, -0.01), (-0.8, 0.1, 0.5)), ((0.0, -0.02, 0.0), (0.7, -0.2, 0.3)),
                                                        ((0.02, 0.0, 0.01), (-0.6, 0.0, 0.9)))]
    nb = [_neighbour(5300, T[0], K_KITTI, 1500, crowded=True), _neighbour(5310, T[1], K_EUROC, 7),
          _neighbour(5320, T[2], K_EUROC, 900, node_limit=60), _neighbour(5330, T[3], K_KITTI, 500, node_limit=0),
          _neighbour(5340, T[4], K_KITTI, 1200)]
    nb[4]["has"][:] = 1
    return nb


def _ref_sft(nb, F12=None, **mutant):
    cur = sft_current()
    return ref.search_for_triangulation(cur["kps"], cur["desc"], nb["kps"], nb["desc"], cur["nodes"], nb["nodes"], cur["has"], nb["has"],
                                        nb["F12"] if F12 is None else F12, nb["ex"], nb["ey"], SCALE, SIGMA2, **mutant)


@functools.lru_cache(None)
def ref_batch():
    """per neighbour: the reference's matches, and its triangulation of them"""
    cur, out = sft_current(), []
    for nb in batch_mixed():
        s = _ref_sft(nb)
        i1 = np.nonzero(s["match"] >= 0)[0].astype(np.int32)
        t = ref.triangulate(cur["kps"], nb["kps"], i1, s["match"][i1], cur["T"], nb["T"], cur["K"], nb["K"], SCALE, SIGMA2, RATIO_FACTOR)
        out.append((s, i1, t))
    return out


@functools.lru_cache(None)
def ref_sft_degenerate():
    return _ref_sft(batch_mixed()[0], F12=F_DEGENERATE)


# ====================================================================================== fuse_exits / fuse_crowded
K_DYADIC = np.array([512.0, 512.0, 601.0, 183.0], F32)   # exactly representable: the image-bound rows are exact in f32 and f64
T_DYADIC = pose_T((0, 0, 0), (0.5, -0.25, 1.0))
T_CROWD = pose_T((0.01, -0.02, 0.005), (0.1, -0.05, 0.3))


def _map_points(rng, kps, desc, T, K, src, uv, depth, g, sigma=0.04):
    """map points aimed at pixel uv of the keyframe; max_dist = dist * scale[octave of src] * 1.2^g puts PredictScale at
    octave + g before ceil"""
    n = len(src)
    Xw = _backproject(T, K, uv, depth).astype(F32)
    R, t = _rt(T)
    Ow = -R.T @ t
    PO = Xw.astype(np.float64) - Ow
    dist = np.linalg.norm(PO, axis=1)
    nrm = (PO / dist[:, None] + rng.normal(0, 0.05, PO.shape))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    maxd = (dist * SCALE[kps["octave"][src]].astype(np.float64) * 1.2 ** g).astype(F32)
    mind = (maxd / SCALE[7]).astype(F32)
    mpd = perturbed_descriptors(desc[src], sigma, int(rng.integers(1 << 30)))
    return dict(valid=np.ones(n, np.uint8), Xw=Xw, normal=nrm, min_dist=mind, max_dist=maxd, mp_desc=mpd,
                crafted=np.full(n, -1), exact=np.zeros(n, bool))


def _away_from_integers(rng, n, lo=-0.85, hi=0.85):
    g = rng.uniform(0.15, hi, n)
    return np.where(rng.uniform(size=n) < 0.5, g, -rng.uniform(0.15, -lo, n))


def _cat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


@functools.lru_cache(None)
def fuse_exits():
    """one sparse keyframe (a jittered lattice: every keypoint is alone in any window) and map points built to leave through
    each exit and property of Fuse's search half"""
    rng = np.random.default_rng(6100)
    E = ref.FUSE_EXIT
    KP = _kp_dtype()
    gx, gy = np.meshgrid(40 + 60 * np.arange(20), 20 + 22 * np.arange(16))
    n = gx.size
    kps = np.zeros(n, KP)
    kps["x"] = (gx.ravel() + rng.uniform(-3, 3, n)).astype(F32)
    kps["y"] = (gy.ravel() + rng.uniform(-3, 3, n)).astype(F32)
    kps["octave"], kps["size"] = rng.integers(0, 8, n), 31
    # keypoints beside the image bounds for the exact rows: v == 376 (open bound) and v == 0 (closed bound)
    edge = np.zeros(6, KP)
    edge["x"] = [729, 473, 857, 729, 473, 857]
    edge["y"] = [371.5, 371.5, 371.5, 4.4, 4.4, 4.4]
    edge["octave"], edge["size"] = 4, 31
    kps = np.concatenate([kps, edge])
    desc = make_frame(len(kps), 6101)[1]
    T, K = T_DYADIC, K_DYADIC
    P = []

    def base(src, g=None, sigma=0.04, off=None):
        uv = np.stack([kps["x"][src], kps["y"][src]], 1).astype(np.float64) + (rng.uniform(-0.8, 0.8, (len(src), 2)) if off is None else off)
        return _map_points(rng, kps, desc, T, K, src, uv, rng.uniform(3, 60, len(src)), _away_from_integers(rng, len(src)) if g is None else g, sigma)

    def pick(m, cond=None):
        ok = np.arange(n) if cond is None else np.nonzero(cond(kps["octave"][:n]))[0]
        return rng.choice(ok, m, replace=False)

    p = base(pick(40)); p["crafted"][:] = E["matched"]; P.append(p)
    p = base(pick(12)); p["valid"][:] = 0; p["crafted"][:] = E["invalid"]; P.append(p)
    p = base(pick(12)); p["crafted"][:] = E["behind"]                       # the same pixel from behind the camera
    p["Xw"] = _backproject(T, K, np.stack([kps["x"][:12], kps["y"][:12]], 1).astype(np.float64), -rng.uniform(3, 60, 12)).astype(F32); P.append(p)
    src = pick(16)
    p = base(src); p["crafted"][:] = E["outside_image"]
    uv = np.stack([kps["x"][src], kps["y"][src]], 1).astype(np.float64)
    uv[0:4, 0], uv[4:8, 0], uv[8:12, 1], uv[12:16, 1] = 1241 + 5, -5, 376 + 3, -3
    p["Xw"] = _backproject(T, K, uv, rng.uniform(3, 60, 16)).astype(F32); P.append(p)
    p = base(pick(12)); p["min_dist"] = (p["min_dist"] * 0 + np.linalg.norm(p["Xw"] + T[:3, 3], axis=1) * 1.4).astype(F32)
    p["crafted"][:] = E["too_near"]; P.append(p)
    p = base(pick(12)); p["max_dist"] = (np.linalg.norm(p["Xw"] + T[:3, 3], axis=1) / 1.2 / 1.1).astype(F32)
    p["min_dist"] = (p["max_dist"] / SCALE[7]).astype(F32); p["crafted"][:] = E["too_far"]; P.append(p)
    p = base(pick(12)); p["crafted"][:] = E["viewing_angle"]               # 75 degrees between the normal and the viewing ray
    po = p["Xw"].astype(np.float64) + T[:3, 3]
    po /= np.linalg.norm(po, axis=1, keepdims=True)
    side = np.cross(po, [0.0, 1.0, 0.0]); side /= np.linalg.norm(side, axis=1, keepdims=True)
    p["normal"] = (np.cos(np.deg2rad(75)) * po + np.sin(np.deg2rad(75)) * side).astype(F32); P.append(p)
    src = pick(12)                                                          # aimed between the lattice points
    p = base(src, off=np.tile([30.0, 0.0], (12, 1))); p["crafted"][:] = E["window_empty"]; P.append(p)
    src = pick(12, lambda o: o <= 4)                                        # predicted level = octave + 2: one below the gate
    p = base(src, g=rng.uniform(1.2, 1.8, 12)); p["crafted"][:] = E["no_candidate_passed"]; P.append(p)
    src = pick(12, lambda o: o >= 3)                                        # predicted level = octave - 1: one above the gate
    p = base(src, g=-rng.uniform(1.2, 1.8, 12)); p["crafted"][:] = E["no_candidate_passed"]; P.append(p)
    src = pick(12)                                                          # 2.69 sigma away: inside the window, outside 5.99
    p = base(src, off=(1.9 * SCALE[kps["octave"][src]].astype(np.float64))[:, None] * np.ones((12, 2)), g=rng.uniform(0.15, 0.85, 12))
    p["crafted"][:] = E["no_candidate_passed"]; P.append(p)
    p = base(pick(12), sigma=0.12); p["crafted"][:] = E["above_th_low"]; P.append(p)
    src = pick(12, lambda o: o >= 6)                                        # ceil(.) >= 8: clamped to the top level
    p = base(src, g=7.5 - kps["octave"][src]); p["crafted"][:] = E["matched"]; P.append(p)
    # the exact rows: pc = (x, 193/128 or -183/128, 4) projects to v = 376 or v = 0 without rounding in f32 or f64
    src = np.arange(n, n + 6)
    p = base(src, g=rng.uniform(0.2, 0.8, 6))
    pc = np.array([[1.0, 193 / 128, 4], [-1.0, 193 / 128, 4], [2.0, 193 / 128, 4], [1.0, -183 / 128, 4], [-1.0, -183 / 128, 4], [2.0, -183 / 128, 4]])
    p["Xw"] = (pc - T[:3, 3].astype(np.float64)).astype(F32)
    dist = np.linalg.norm(pc, axis=1)
    p["normal"] = (pc / dist[:, None]).astype(F32)
    p["max_dist"] = (dist * SCALE[4] * 1.2 ** 0.5).astype(F32); p["min_dist"] = (p["max_dist"] / SCALE[7]).astype(F32)
    p["exact"][:] = True
    p["crafted"][:3], p["crafted"][3:] = E["outside_image"], E["matched"]; P.append(p)
    pts = _cat(P)
    order = rng.permutation(len(pts["valid"]))
    pts = {k: v[order] for k, v in pts.items()}
    s = dict(kps=kps, desc=desc, bounds=BOUNDS, T=T, K=K, **pts)
    s["ref"] = _ref_fuse(s)
    return s


@functools.lru_cache(None)
def fuse_crowded():
    """1600 keypoints inside 40 x 20 px: one cell column's row range holds hundreds of window candidates, every window spans
    several cell columns; twins with one descriptor sit on both sides of a cell boundary so that the first in
    GetFeaturesInArea order has the larger keypoint index"""
    rng = np.random.default_rng(6200)
    n = 1600
    kps, desc = make_frame(n, 6201)
    kps["octave"] = np.where(rng.uniform(size=n) < 0.7, 0, rng.integers(0, 8, n))     # most candidates stop at the level gate
    kps["x"] = rng.uniform(600, 640, n).astype(F32)
    kps["y"] = rng.uniform(180, 200, n).astype(F32)
    col_edge, row_edge = 31.5 * 1241 / 64, 24.5 * 376 / 48          # PosInGrid rounds: the cells change at the half
    for i in range(90):
        a, b = n - 1 - i, i                                         # a comes first in the area order and has the larger index
        kps["octave"][a] = kps["octave"][b] = 1 + i % 7
        desc[a] = desc[b]
        if i < 40:                                                  # across a column boundary
            kps["x"][a], kps["x"][b] = col_edge - 1, col_edge + 1
            kps["y"][a] = kps["y"][b] = 181 + 0.45 * i
        elif i < 70:                                                # across a row boundary inside one column
            kps["y"][a], kps["y"][b] = row_edge - 0.6, row_edge + 0.6
            kps["x"][a] = kps["x"][b] = 601 + 1.2 * (i - 40)
        else:                                                       # inside one cell: the smaller index comes first
            kps["x"][a], kps["x"][b] = 625.0 + 0.5 * (i - 70), 625.6 + 0.5 * (i - 70)
            kps["y"][a] = kps["y"][b] = 186.0
    twins = np.arange(90)
    uv = np.stack([(kps["x"][twins] + kps["x"][n - 1 - twins]) / 2, kps["y"][twins] * 0.5 + kps["y"][n - 1 - twins] * 0.5], 1).astype(np.float64)
    P = [_map_points(rng, kps, desc, T_CROWD, K_KITTI, twins, uv, rng.uniform(3, 60, 90), _away_from_integers(rng, 90))]
    src = rng.choice(np.arange(90, n - 90), 700, replace=False)
    uv = np.stack([kps["x"][src], kps["y"][src]], 1).astype(np.float64) + rng.uniform(-0.8, 0.8, (700, 2))
    P.append(_map_points(rng, kps, desc, T_CROWD, K_KITTI, src, uv, rng.uniform(3, 60, 700), _away_from_integers(rng, 700)))
    pts = _cat(P)
    s = dict(kps=kps, desc=desc, bounds=BOUNDS, T=T_CROWD, K=K_KITTI, **pts)
    # at two keypoints per square pixel a large window has a candidate within the tolerance of its edge or of the 5.99 circle
    # more often than not: keep the map points that the reference alone finds clear of every threshold, the large windows first
    pre = _ref_fuse(s)
    clear = np.nonzero(pre["margin"] > 2)[0]
    clear = clear[np.argsort(-pre["n_in_window"][clear], kind="stable")][:260]
    clear.sort()
    for k in pts:
        s[k] = s[k][clear]
    s["ref"] = _ref_fuse(s)
    return s


def _ref_fuse(s, **mutant):
    return ref.fuse_search(s["kps"], s["desc"], s["bounds"], s["valid"], s["Xw"], s["normal"], s["min_dist"], s["max_dist"],
                           s["mp_desc"], s["T"], s["K"], 3.0, SCALE, INV_SIGMA2, 8, 1.2, **mutant)


def _fuse_args(s):
    return s["valid"], s["Xw"], s["normal"], s["min_dist"], s["max_dist"], s["mp_desc"]


def _check_fuse(s, bi, bd):
    """best_idx on the decidable points (the exact rows are decided by construction), the bits of best_dist where the reference
    matched, 256 on every other point"""
    r = s["ref"]
    dec = r["decidable"] | s["exact"]
    np.testing.assert_array_equal(np.asarray(bi)[dec], r["best_idx"][dec])
    m = dec & (r["best_idx"] >= 0)
    np.testing.assert_array_equal(np.asarray(bd)[m].view(np.int32), r["best_dist"][m].view(np.int32))
    assert (np.asarray(bd)[np.asarray(bi) < 0] == 256).all()


def _svd_w_zero():
    """4 x 4 matrices whose null vector has a zero last component: x3D.at(3) == 0 at LocalMapping.cc:444"""
    rng = np.random.default_rng(7100)
    A = rng.standard_normal((12, 4, 4)).astype(F32)
    A[0:4, :, 0] = 0                                     # null vector e0
    A[4:8, :, 1] = 0                                     # e1
    A[8:12, :, 1] = A[8:12, :, 0] * 2                    # (2, -1, 0, 0) / sqrt 5
    return A


# ------------------------------------------------------------------ CPU: the plain reference against the oracle
@pytest.mark.parametrize("mixed_k", [False, True])
@pytest.mark.parametrize("n_pairs", [None, 1, 65])
def test_reference_equals_oracle_triangulation(oracle, mixed_k, n_pairs):
    s = tri_exits(mixed_k)
    sl = slice(None, n_pairs)
    x, ok, nok = oracle.triangulate_pairs(s["k1"], s["k2"], s["idx1"][sl], s["idx2"][sl], s["T1"], s["T2"], s["K1"], s["K2"])
    r = {k: v[sl] for k, v in s["ref"].items()}
    assert nok == ok.sum()
    assert _check_tri(r, ok, x) <= ref.ORACLE_COORD_ERR


def test_reference_equals_oracle_search_for_triangulation(oracle):
    cur = sft_current()
    ofc = oracle.frame(cur["kps"], cur["desc"], BOUNDS)
    for nb, (s, i1, t) in zip(batch_mixed(), ref_batch()):
        of2 = oracle.frame(nb["kps"], nb["desc"], nb["bounds"])
        m, n = oracle.match_triangulate(ofc, of2, cur["nodes"], nb["nodes"], cur["has"], nb["has"], nb["F12"], nb["ex"], nb["ey"], False)
        np.testing.assert_array_equal(m, s["match"])
        assert n == s["n_matches"]
        x, ok, _ = oracle.triangulate_pairs(cur["kps"], nb["kps"], i1, s["match"][i1], cur["T"], nb["T"], cur["K"], nb["K"])
        assert _check_tri(t, ok, x) <= ref.ORACLE_COORD_ERR
    nb, d = batch_mixed()[0], ref_sft_degenerate()
    m, n = oracle.match_triangulate(ofc, oracle.frame(nb["kps"], nb["desc"], nb["bounds"]), cur["nodes"], nb["nodes"], cur["has"], nb["has"],
                                    F_DEGENERATE, nb["ex"], nb["ey"], False)
    np.testing.assert_array_equal(m, d["match"])
    assert n == d["n_matches"]


@pytest.mark.parametrize("name", ["fuse_exits", "fuse_crowded"])
def test_reference_equals_oracle_fuse(oracle, name):
    s = globals()[name]()
    bi, bd = oracle.fuse_search(oracle.frame(s["kps"], s["desc"], s["bounds"]), *_fuse_args(s), s["T"], s["K"], 3.0)
    _check_fuse(s, bi, bd)


def test_oracle_svd4_w_zero(oracle):
    v = oracle.svd4_vt(_svd_w_zero())[:, 3]
    assert (v[:, 3] == 0).all() and (v[:, 2] == 0).all()
    np.testing.assert_allclose(np.linalg.norm(v, axis=1), 1, atol=1e-6)
    np.testing.assert_array_equal(np.abs(v[:4]), np.tile(np.array([1, 0, 0, 0], F32), (4, 1)))
    np.testing.assert_allclose(np.abs(v[8:]), np.tile(np.array([2, 1, 0, 0]) / np.sqrt(5), (4, 1)), atol=1e-6)


def test_coordinate_bound_is_the_measured_one(oracle):
    """ORACLE_COORD_ERR is what the CPU oracle shows against the float64 reference over the triangulation sets, not a figure
    taken from the kernels: the largest value lies in (ORACLE_COORD_ERR / 2, ORACLE_COORD_ERR]"""
    cur, worst = sft_current(), 0.0
    for mixed_k in (False, True):
        s = tri_exits(mixed_k)
        x, ok, _ = oracle.triangulate_pairs(s["k1"], s["k2"], s["idx1"], s["idx2"], s["T1"], s["T2"], s["K1"], s["K2"])
        worst = max(worst, _check_tri(s["ref"], ok, x))
    for nb, (sft, i1, t) in zip(batch_mixed(), ref_batch()):
        x, ok, _ = oracle.triangulate_pairs(cur["kps"], nb["kps"], i1, sft["match"][i1], cur["T"], nb["T"], cur["K"], nb["K"])
        worst = max(worst, _check_tri(t, ok, x))
    print("oracle coordinate error", worst)
    assert ref.ORACLE_COORD_ERR / 2 < worst <= ref.ORACLE_COORD_ERR
    assert ref.COORD_BOUND == 4 * ref.ORACLE_COORD_ERR


def test_coverage():
    """a condition, not a measurement: over the crafted sets the reference reports every reachable exit, counter and property
    at least 3 times, and the sizes that make the kernels' chunk loops take a second and a third step"""
    sft = [s for s, _, _ in ref_batch()] + [ref_sft_degenerate()]
    got = {}
    for s in sft:
        for k, v in ref.census(s, ref.SFT_EXITS, ref.SFT_COUNTERS + ("tie_replaced",)).items():
            got["sft." + k] = got.get("sft." + k, 0) + v
    tri = [tri_exits(False)["ref"], tri_exits(True)["ref"]] + [t for _, _, t in ref_batch()]
    for t in tri:
        for k, v in ref.census(t, ref.TRI_EXITS).items():
            got["tri." + k] = got.get("tri." + k, 0) + v
    for s in (fuse_exits(), fuse_crowded()):
        for k, v in ref.census(s["ref"], ref.FUSE_EXITS, ref.FUSE_COUNTERS + ("level_clamped_low", "level_clamped_high", "tie_first_wins")).items():
            got["fuse." + k] = got.get("fuse." + k, 0) + v
    print(got)
    unreachable = {"tri.w_zero", "tri.dist_zero", "fuse.level_clamped_low"}      # the arguments: mapping_ref.py and the module text
    for k, v in got.items():
        assert (v == 0) if k in unreachable else (v >= 3), (k, v)
    s0 = ref_batch()[0][0]
    assert s0["list_len"].max() >= 129 and s0["n_nodes2"] >= 130 and s0["n_nodes1"] >= 130
    assert (s0["tie_replaced"] & (s0["list_len"] >= 129)).sum() >= 3               # ties inside the three-chunk list as well
    fc = fuse_crowded()
    assert fc["ref"]["max_column"].max() >= 129 and len(fc["kps"]) >= 1500
    won = fc["ref"]["tie_first_wins"] & (fc["ref"]["best_idx"] >= len(fc["kps"]) - 90)
    assert won.sum() >= 3                                                         # the first in area order has the larger index
    # every set fits the limits of a frame and no pair count is a multiple of the block
    assert N_CUR % 4 != 0 and all(len(nb["kps"]) <= 2000 for nb in batch_mixed())
    nbs = batch_mixed()
    assert len(nbs[1]["kps"]) < 10 and len(np.unique(nbs[2]["nodes"][nbs[2]["nodes"] >= 0])) <= 64 and (nbs[3]["nodes"] < 0).all() and nbs[4]["has"].all()


def test_undecidable_share():
    """a condition, not a measurement: at most 2 % of a set's elements lie within the tolerances of a gate, none of the
    elements crafted for an exit does, and every crafted element leaves where it was built to"""
    shares = {}
    for name, s in (("tri_exits", tri_exits(False)), ("tri_exits_mixed_k", tri_exits(True))):
        shares[name] = float((~s["ref"]["decidable"]).mean())
        c = s["crafted"] >= 0
        assert s["ref"]["decidable"][c].all()
        np.testing.assert_array_equal(s["ref"]["exit"][c], s["crafted"][c])
    for b, (_, i1, t) in enumerate(ref_batch()):
        if len(i1):
            shares["batch_mixed[%d]" % b] = float((~t["decidable"]).mean())
    for name, s in (("fuse_exits", fuse_exits()), ("fuse_crowded", fuse_crowded())):
        dec = s["ref"]["decidable"] | s["exact"]
        shares[name] = float((~dec).mean())
        c = s["crafted"] >= 0
        assert dec[c].all()
        np.testing.assert_array_equal(s["ref"]["exit"][c], s["crafted"][c])
    print(shares)
    for name, v in shares.items():
        assert v <= UNDECIDABLE_CAP, (name, v)


def test_sensitivity():
    """mutants of the REFERENCE must each change a result the library returns (matches, accept flags, best_idx) on the crafted
    sets: a mutant that does not means the inputs could not catch that bug in a kernel"""
    changed = {}
    for mutant in ("k2_is_k1", "sigma2_from_octave1", "drop_gate2", "swap_ratio"):
        n = 0
        for mixed_k in (False, True):
            s = tri_exits(mixed_k)
            m = ref.triangulate(s["k1"], s["k2"], s["idx1"], s["idx2"], s["T1"], s["T2"], s["K1"], s["K2"], SCALE, SIGMA2, RATIO_FACTOR, **{mutant: True})
            n += int((m["ok"] != s["ref"]["ok"])[s["ref"]["decidable"] & m["decidable"]].sum())
        changed["tri." + mutant] = n
    nb, base = batch_mixed()[0], ref_batch()[0][0]
    for mutant in (dict(first_wins=True), dict(max_candidates=64), dict(max_nodes=64)):
        changed["sft.%s" % list(mutant)[0]] = int((_ref_sft(nb, **mutant)["match"] != base["match"]).sum())
    for mutant in (dict(closed_upper=True), dict(level_wide=True), dict(last_wins=True), dict(column_cap=64)):
        n = 0
        for s in (fuse_exits(), fuse_crowded()):
            m = _ref_fuse(s, **mutant)
            dec = (s["ref"]["decidable"] & m["decidable"]) | s["exact"]
            n += int((m["best_idx"] != s["ref"]["best_idx"])[dec].sum())
        changed["fuse.%s" % list(mutant)[0]] = n
    print(changed)
    for k, v in changed.items():
        assert v >= 3, (k, v)


# ------------------------------------------------------------------ GPU: the HIP entry points against the oracle and the reference
@pytest.mark.gpu
@pytest.mark.parametrize("mixed_k", [False, True])
def test_hip_triangulate_pairs_exits(hip, oracle, mixed_k):
    """asd_triangulate_pairs over every exit in one launch, then the one-pair and the 65-pair call"""
    s = tri_exits(mixed_k)
    hip.frame_set(4, s["k1"], np.zeros((len(s["k1"]), 128), F32), s["b1"])
    hip.frame_set(5, s["k2"], np.zeros((len(s["k2"]), 128), F32), s["b2"])
    for n_pairs in (None, 1, 65):
        sl = slice(None, n_pairs)
        gx, gok, gn = hip.triangulate_pairs(4, 5, s["idx1"][sl], s["idx2"][sl], s["T1"], s["T2"], s["K1"], s["K2"])
        ex, eok, en = oracle.triangulate_pairs(s["k1"], s["k2"], s["idx1"][sl], s["idx2"][sl], s["T1"], s["T2"], s["K1"], s["K2"])
        np.testing.assert_array_equal(gok, eok)
        np.testing.assert_array_equal(gx, ex)
        assert gn == en == gok.sum()
        err = _check_tri({k: v[sl] for k, v in s["ref"].items()}, gok, gx)
        print("hip coordinate error", mixed_k, n_pairs, err)
        assert err <= ref.COORD_BOUND


@pytest.mark.gpu
def test_hip_match_triangulate_crowded(hip, oracle):
    """asd_match_triangulate (check_orientation = 0) per neighbour of batch_mixed, and sft_crowded again under F_DEGENERATE"""
    cur = sft_current()
    hip.frame_set(0, cur["kps"], cur["desc"], BOUNDS)
    ofc = oracle.frame(cur["kps"], cur["desc"], BOUNDS)
    cases = [(nb, nb["F12"], s) for nb, (s, _, _) in zip(batch_mixed(), ref_batch())] + [(batch_mixed()[0], F_DEGENERATE, ref_sft_degenerate())]
    for nb, F12, s in cases:
        hip.frame_set(1, nb["kps"], nb["desc"], nb["bounds"])
        gm, gn = hip.match_triangulate(0, 1, N_CUR, cur["nodes"], nb["nodes"], cur["has"], nb["has"], F12, nb["ex"], nb["ey"], False)
        om, on = oracle.match_triangulate(ofc, oracle.frame(nb["kps"], nb["desc"], nb["bounds"]), cur["nodes"], nb["nodes"], cur["has"], nb["has"],
                                          F12, nb["ex"], nb["ey"], False)
        np.testing.assert_array_equal(gm, om)
        np.testing.assert_array_equal(gm, s["match"])
        assert gn == on == s["n_matches"]


@pytest.mark.gpu
def test_hip_create_map_points_batch_mixed(hip, oracle):
    """asd_create_map_points_batch over 5 neighbours that differ in size, intrinsics and node count, against the per-pair HIP
    calls, the oracle and the reference"""
    cur, nbs = sft_current(), batch_mixed()
    hip.frame_set(0, cur["kps"], cur["desc"], BOUNDS)
    hip.frame_set_bow(0, cur["nodes"])
    for b, nb in enumerate(nbs):
        hip.frame_set(1 + b, nb["kps"], nb["desc"], nb["bounds"])
        hip.frame_set_bow(1 + b, nb["nodes"])
    m, nm, x, ok = hip.create_map_points_batch(0, N_CUR, cur["has"], cur["T"], cur["K"],
                                               [dict(slot=1 + b, has_mp=nb["has"], F12=nb["F12"], ex=nb["ex"], ey=nb["ey"], Tcw=nb["T"], K=nb["K"])
                                                for b, nb in enumerate(nbs)])
    for b, (nb, (s, i1, t)) in enumerate(zip(nbs, ref_batch())):
        np.testing.assert_array_equal(m[b], s["match"])
        assert nm[b] == s["n_matches"]
        assert not ok[b][s["match"] < 0].any() and not x[b][s["match"] < 0].any()
        ox, ook, _ = oracle.triangulate_pairs(cur["kps"], nb["kps"], i1, s["match"][i1], cur["T"], nb["T"], cur["K"], nb["K"])
        np.testing.assert_array_equal(ok[b][i1], ook)
        np.testing.assert_array_equal(x[b][i1], ox)
        px, pok, _ = hip.triangulate_pairs(0, 1 + b, i1, s["match"][i1], cur["T"], nb["T"], cur["K"], nb["K"])
        np.testing.assert_array_equal(ok[b][i1], pok)
        np.testing.assert_array_equal(x[b][i1], px)
        err = _check_tri(t, ok[b][i1], x[b][i1])
        print("hip coordinate error, neighbour", b, err)
        assert err <= ref.COORD_BOUND


@pytest.mark.gpu
def test_hip_fuse_search_exits_and_crowded(hip, oracle):
    """asd_fuse_search per set, asd_fuse_search_batch as two calls over shared tables, and again with desc_rows into the bank"""
    sets = [fuse_crowded(), fuse_exits()]
    calls, first = [], 0
    for c, s in enumerate(sets):
        hip.frame_set(10 + c, s["kps"], s["desc"], s["bounds"])
        gi, gd = hip.fuse_search(10 + c, *_fuse_args(s), s["T"], s["K"], 3.0)
        oi, od = oracle.fuse_search(oracle.frame(s["kps"], s["desc"], s["bounds"]), *_fuse_args(s), s["T"], s["K"], 3.0)
        np.testing.assert_array_equal(gi, oi)
        np.testing.assert_array_equal(gd, od)
        _check_fuse(s, gi, gd)
        calls.append(dict(slot_kf=10 + c, first=first, n=len(s["valid"]), Tcw=s["T"], K=s["K"]))
        first += len(s["valid"])
    cat = [np.concatenate([_fuse_args(s)[k] for s in sets]) for k in range(6)]
    bi, bd = hip.fuse_search_batch(calls, *cat, th=3.0)
    hip.bank_put(2000, cat[5])
    ri, rd = hip.fuse_search_batch(calls, *cat[:5], np.arange(2000, 2000 + len(cat[5]), dtype=np.int32), th=3.0)
    for got_i, got_d in ((bi, bd), (ri, rd)):
        for c, s in zip(calls, sets):
            _check_fuse(s, got_i[c["first"]: c["first"] + c["n"]], got_d[c["first"]: c["first"] + c["n"]])
    np.testing.assert_array_equal(ri, bi)
    np.testing.assert_array_equal(rd, bd)


@pytest.mark.gpu
def test_hip_svd4_w_zero(hip, oracle):
    A = _svd_w_zero()
    v = hip.svd4_null(A)
    np.testing.assert_array_equal(v, oracle.svd4_vt(A)[:, 3])
    assert (v[:, 3] == 0).all()
