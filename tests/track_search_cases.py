"""Crafted inputs for tests/test_track_search_exits.py: the sets, and drivers with one interface over the restatement
(tests/track_search_ref.py), the CPU oracle and the library's entry points.  The frame builder, the query builder, the descriptor
codes and the cameras are the ones of tests/loop_search_cases.py.

A set is a dict.  fn "m1": the current frame (kps, desc, bounds), the last frame's octaves and angles, the call's arrays, `crafted`
(per point the exit its row was built for, "" where none; "chain..." rows are checked by their own rule) and `exact` (rows that sit on
a bound by construction and are compared regardless of margin).  fn "m2": the frame, the map points as Frame::isInFrustum sees them
(Xw, normal, min / max distance), occupied, th, nn_ratio; `crafted` names the M2 exit, `crafted_f` the frustum exit.

Exit sets.  One row per rule at a SITE of its own (40 px apart, keypoints within 2 px of the site, windows of levels 0..2 never
reach the next site; rows at the top level keep their neighbours free).  Descriptors: a keypoint's identity is three components of
value 2, a query copies its target's identity and adds components that are multiples of 2^-10 in rows 0..7, so every distance is a
short sum of multiples of 2^-20 below 2^9: exact in f32 in any order.  1 + 0.25 + 0.25 is TH_HIGH, a further component 2^-10 puts the
neighbour 2^-20 beyond.  The first camera is a pure translation with K = (512, 512, 601, 183): the rows on a bound use dyadic camera
coordinates and their f32 pixel is exact.  The second camera (rotated, KITTI intrinsics) repeats the sets without those rows.
M2 is called with nn_ratio = 0.75 (dyadic: best == nn_ratio * best2 is reachable exactly) and th = 1 or the next f32 above it.

Claim chains.  A site with n keypoints whose distances to the site's points rise with the keypoint's number (component 4 = j / 16;
octaves alternate, so M2's ratio test never sees two of one level), and n + 1 points with that one preference list: point k finds the
first k entries held and takes entry k + 1 (depths 0..n-1), the last finds the list exhausted.  n = 10 gives depths 1..9 -- across the
four (M1) or two (M2) heads the replay keeps in registers and across its groups of four -- n = 4, 5, 8, 9 the exhausted lists of those
lengths.  "broken" chains: one holder has no observations, so the next point takes the same keypoint.
"""
import functools

import numpy as np

from tests import track_search_ref as ref
from tests.loop_search_cases import (BOUNDS_KITTI, K_DYADIC, K_KITTI, NEIGHBOUR, SCALE, T_CROWD, _bound_rows, _Frame, _pack, _rescaled_frame,
                                     _rigid_inverse, _shape_frame, code, fuse_grow, near, query, translation)
from tests.test_matcher import perturbed_descriptors, pose_T

F32 = np.float32
EQ_HIGH = (1.0, 0.5, 0.5)
TH_M1 = 10.0                                       # as the relocalisation rows: _bound_rows places its keypoints for this radius
NN_CRAFTED = 0.75
T_ROT = pose_T((0.03, -0.02, 0.01), (0.5, -0.25, 1.0))
CAMERAS = {"dyadic": (K_DYADIC, translation()), "kitti": (K_KITTI, T_ROT)}
CHAIN_LENGTHS = (10, 4, 5, 8, 9)
_CHAIN_XY = [(-1.6, -0.9), (-0.8, -0.9), (0.0, -0.9), (0.8, -0.9), (1.6, -0.9), (-1.6, 0.9), (-0.8, 0.9), (0.0, 0.9), (0.8, 0.9), (1.6, 0.9)]


def _octave_of(q):
    """the level PredictScale gives the row: the last frame's keypoint of an M1 row is at that octave"""
    d = np.linalg.norm(q["pc"])
    return int(np.clip(np.ceil(np.log(q["maxd"] / d) / np.log(1.2)), 0, 7)) if d > 0 else 3


class _Rows:
    """the rows of a set in order, with what M1 / M2 need beside loop_search_cases.query's fields"""

    def __init__(self):
        self.rows = []

    def __call__(self, q, obs=1, name_f="in_view", octave=None, tied=False, kp=-2):
        """tied: the row keeps its place among the other tied rows; kp: the keypoint the point must write (-1: none, -2: not stated)"""
        q = dict(q, obs=obs, name_f=name_f, octave=_octave_of(q) if octave is None else octave, tied=tied, kp=kp)
        self.rows.append(q)


def _ident(j):
    j[0] += 1
    return code(j[0])


def _chain_site(fr, Q, L, n, j, broken=None, exhausted=True, m2=False):
    """n keypoints and n (+ 1) points with one preference list; broken: the number of the point that has no observations"""
    c, d = fr.site(), _ident(j)
    first = len(fr.rows)
    for k in range(n):
        fr.kp(c[0] + _CHAIN_XY[k][0], c[1] + _CHAIN_XY[k][1], L - (k % 2), near(d, 0, 0, 0, 0, k / 16))
    for k in range(n + (1 if exhausted else 0)):
        entry = k if broken is None or k <= broken else k - 1          # the point behind an unobserved holder takes the same keypoint
        Q(query(fr, c, L, near(d, 0.125 + k / 1024), "chain%s:%d:%d" % ("b" if broken is not None else "", n, k)), obs=0 if k == broken else 1,
          tied=True, kp=first + entry if entry < n else -1)


def _shared_rows(fr, Q, m2, j, n_each=3):
    """the rows M1 and M2 have in common; the level gate is [o - 1, o + 1] for M1 and [l - 1, l] for M2"""
    top = 0 if m2 else 1
    empty = "window_empty"
    for k in range(n_each):
        L = 1 + k % 2 if m2 else k % 3
        for delta, name in (((0.25,), "matched"), (EQ_HIGH, "matched"), (EQ_HIGH + (NEIGHBOUR,), "above_th_high")):
            c, d = fr.site(), _ident(j)
            fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
            Q(query(fr, c, L, near(d, *delta), name))
        c, d = fr.site(), _ident(j)                            # one octave below is accepted, two below is not
        fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
        Q(query(fr, c, L + 1, near(d, 0.25), "matched"))
        c, d = fr.site(), _ident(j)
        fr.kp(c[0] + 0.7, c[1] + 0.7, 0, d)
        Q(query(fr, c, 2, near(d, 0.25), empty))
        c, d = fr.site(), _ident(j)                            # the highest accepted octave and the one above it
        fr.kp(c[0] + 0.7, c[1] + 0.7, L + top, d)
        Q(query(fr, c, L, near(d, 0.25), "matched"))
        c, d = fr.site(), _ident(j)
        fr.kp(c[0] + 0.7, c[1] + 0.7, L + top + 1, d)
        Q(query(fr, c, L, near(d, 0.25), empty))
        c, d = fr.site(), _ident(j)                            # the closer keypoint is one octave too high
        fr.kp(c[0] + 0.7, c[1] + 0.7, L + top + 1, d)
        fr.kp(c[0] - 1.2, c[1] + 1.0, L, near(d, 0, 0, 0, 0, 0.5))
        Q(query(fr, c, L, near(d, 0.25), "matched"))
        Q(query(fr, fr.site(), L, _ident(j), empty))           # no keypoint at all
        # octave 0 (minLevel = -1: the gate holds through maxLevel >= 0) and the top octave
        c, d = fr.site(), _ident(j)
        fr.kp(c[0] + 0.7, c[1] + 0.7, 0, d)
        Q(query(fr, c, 0, near(d, 0.25), "matched"))
        c, d = fr.site(gap=True), _ident(j)
        fr.kp(c[0] + 0.7, c[1] + 0.7, 7, d)
        Q(query(fr, c, 8 if m2 else 7, near(d, 0.25), "matched"))          # M2: ceil(7.5) = 8 is clamped to 7
        # two keypoints with one descriptor on both sides of a column boundary (the first in area order has the larger index), and
        # inside one cell; M2: at two octaves, or the ratio test would refuse the pair
        c, d = fr.site(on_column_edge=True), _ident(j)
        fr.kp(c[0] - 0.3 + 1.0, c[1], L, d)
        fr.kp(c[0] - 0.3 - 1.0, c[1], L - 1 if m2 else L, d)
        Q(query(fr, c, L, near(d, 0.25), "matched"))
        c, d = fr.site(), _ident(j)
        fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
        fr.kp(c[0] + 1.2, c[1] + 0.9, L - 1 if m2 else L, d)
        Q(query(fr, c, L, near(d, 0.25), "matched"))
        # a holder without observations: the next point writes the same keypoint
        c, d = fr.site(), _ident(j)
        fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
        Q(query(fr, c, L, near(d, 0.25), "overwritten_later"), obs=0, tied=True)
        Q(query(fr, c, L, near(d, 0.125), "matched"), tied=True)
    for n in CHAIN_LENGTHS:
        for k in range(n_each if n == 10 else 1):
            _chain_site(fr, Q, 1 + k % 2, n, j, m2=m2)
    for broken in (0, 2, 3, 4):
        _chain_site(fr, Q, 1, 6, j, broken=broken, m2=m2)


def _finish(fr, R, cam, seed):
    """-> the point arrays in the world of camera `cam`, the chains in their order and the other rows shuffled between them"""
    K, T = CAMERAS[cam]
    Rm = np.asarray(T, F32).astype(np.float64)[:3, :3]
    p = _pack(R.rows, _rigid_inverse(T), lambda nrm: np.asarray(nrm) @ Rm)
    for key, dt in (("obs", np.uint8), ("octave", np.int32), ("kp", np.int32)):
        p[key] = np.array([q[key] for q in R.rows], dt)
    p["crafted_f"] = np.array([q["name_f"] for q in R.rows])
    n = len(R.rows)
    coupled = np.array([q["tied"] for q in R.rows])
    free = np.nonzero(~coupled)[0]
    order = np.arange(n)
    order[free] = np.random.default_rng(seed).permutation(free)
    return {k: v[order] for k, v in p.items()}, K, T


def _m1_set(name, fr, R, cam, seed, th=TH_M1, check_ori=True):
    p, K, T = _finish(fr, R, cam, seed)
    kps, desc, _ = fr.arrays()
    n = len(p["valid"])
    kl = np.zeros(n, kps.dtype)
    kl["octave"], kl["angle"], kl["size"] = p["octave"], p["angle"], 31
    kl["x"], kl["y"] = 20.0 + np.arange(n) % 1200, 20.0 + np.arange(n) % 330
    return dict(fn="m1", name=name, kps=kps, desc=desc, bounds=fr.bounds, kps_last=kl, desc_last=np.zeros((n, 128), F32), has=p["valid"],
                Xw=p["Xw"], mp_desc=p["mp_desc"], obs=p["obs"], T=T, K=K, th=th, check_ori=check_ori, crafted=p["crafted"], exact=p["exact"],
                expect_kp=p["kp"])


def _m2_set(name, fr, R, cam, seed, th=1.0, nn_ratio=NN_CRAFTED):
    p, K, T = _finish(fr, R, cam, seed)
    kps, desc, taken = fr.arrays()
    return dict(fn="m2", name=name, kps=kps, desc=desc, bounds=fr.bounds, Xw=p["Xw"], normal=p["normal"], mind=p["mind"], maxd=p["maxd"],
                mp_desc=p["mp_desc"], obs=p["obs"], occupied=taken.astype(np.uint8), T=T, K=K, th=th, nn_ratio=nn_ratio,
                crafted=p["crafted"], crafted_f=p["crafted_f"], exact=p["exact"], expect_kp=p["kp"])


# ====================================================================================== M1
@functools.lru_cache(None)
def m1_exits(cam="dyadic"):
    """the shared rows, the gates in front of the search, the rows on a bound (first camera), and the orientation rows: the bulk of the
    matches falls into bin 5 (angles 200 and 50); three rows with a negative rot fall there too, three at 950 degrees go through bin 30
    into bin 0 and are removed, and three keypoints are written twice -- by a point without observations whose bin (2) is discarded and
    by a later point whose bin stays -- and end empty"""
    K, _ = CAMERAS[cam]
    fr, R, j = _Frame(K, BOUNDS_KITTI, 8810), _Rows(), [1000]
    _shared_rows(fr, R, False, j)
    for k in range(3):
        L = k % 3
        for kw, name in ((dict(valid=0), "invalid"), (dict(behind=True), "behind")):
            c, d = fr.site(), _ident(j)
            fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
            R(query(fr, c, L, near(d, 0.25), name, **kw))
        c, d = fr.site(), _ident(j)
        fr.kp(c[0] + 0.7, c[1] + 0.7, L, d, angle=230.0)
        R(query(fr, c, L, near(d, 0.25), "matched", angle=20.0))
        c, d = fr.site(), _ident(j)
        fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
        R(query(fr, c, L, near(d, 0.25), "removed_by_orientation", angle=950.0))
        c, d = fr.site(), _ident(j)
        fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
        R(query(fr, c, L, near(d, 0.25), "removed_by_orientation", angle=110.0), obs=0, tied=True)
        R(query(fr, c, L, near(d, 0.125), "cleared_through_another_write"), tied=True)
    b = fr.bounds
    for k, uv in enumerate(((b[0] - 5, 100.3), (b[1] + 5, 120.3), (300.3, b[2] - 5), (340.3, b[3] + 5)) * 2):
        R(query(fr, np.array(uv), k % 3, _ident(j), "outside_u" if k % 4 < 2 else "outside_v"))
    if cam == "dyadic":
        _bound_rows(fr, R, "reloc")
    return _m1_set("m1_exits_" + cam, fr, R, cam, 8811)


ORI_CASES = {  # name -> ((bin, number of matches), ...), kept bins
    "tie_first": (((2, 10), (5, 10), (9, 10), (11, 10)), (2, 5, 9)),
    "tie_second": (((5, 12), (2, 8), (9, 8), (11, 8)), (5, 2, 9)),
    "tie_third": (((5, 12), (2, 9), (9, 6), (11, 6)), (5, 2, 9)),
    "tenth_at": (((5, 30), (0, 3), (9, 3), (2, 2)), (5, 0, 9)),
    "tenth_second_below": (((5, 30), (0, 2), (9, 2), (2, 1)), (5,)),
    "tenth_second_above": (((5, 30), (0, 4), (9, 4), (2, 1)), (5, 0, 9)),
    "tenth_third_below": (((5, 30), (0, 3), (9, 2), (2, 1)), (5, 0)),
    "tenth_third_above": (((5, 30), (0, 5), (9, 4), (2, 1)), (5, 0, 9)),
}


@functools.lru_cache(None)
def m1_ori(case):
    """matches per rotation bin as ORI_CASES names them (the keypoints' angle is 10, a point of bin b has 10 + 30 b; bin 0 is reached
    through bin 30 with an angle of 910): tied counts in the first, second and third place -- ComputeThreeMaxima's strict `>` keeps the
    lower bin -- and second / third maxima at, below and above a tenth of the first"""
    bins, keep = ORI_CASES[case]
    fr, R, j = _Frame(K_DYADIC, BOUNDS_KITTI, 8820), _Rows(), [3000]
    for b, n in bins:
        for k in range(n):
            c, d = fr.site(), _ident(j)
            fr.kp(c[0] + 0.7, c[1] + 0.7, k % 3, d, angle=10.0)
            R(query(fr, c, k % 3, near(d, 0.25), "matched" if b in keep else "removed_by_orientation", angle=910.0 if b == 0 else 10.0 + 30 * b))
    return _m1_set("m1_ori_" + case, fr, R, "dyadic", 8821)


# ====================================================================================== frustum and M2
def _frustum_rows(fr, Q, j, dyadic):
    """every gate of isInFrustum three times, every level, the clamp, and (first camera) viewCos == limit, the bounds, z == 0"""
    for k in range(3):
        L = 1 + k % 2
        gates = ((dict(behind=True), "behind"), (dict(near_far=-1), "too_near"), (dict(near_far=1), "too_far"), (dict(off_normal=True), "viewing_angle"))
        for kw, name in gates:
            c, d = fr.site(), _ident(j)
            fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
            Q(query(fr, c, L, near(d, 0.25), "not_in_view", **kw), name_f=name)
    b = fr.bounds
    for k, uv in enumerate(((b[0] - 5, 100.3), (b[1] + 5, 120.3), (300.3, b[2] - 5), (340.3, b[3] + 5)) * 2):
        Q(query(fr, np.array(uv), 1 + k % 2, _ident(j), "not_in_view"), name_f="outside_u" if k % 4 < 2 else "outside_v")
    for L in range(3, 8):                                       # the levels the shared rows do not reach
        for k in range(3):
            c, d = fr.site(gap=L == 7), _ident(j)
            fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
            Q(query(fr, c, L, near(d, 0.25), "matched"))
    if not dyadic:
        return
    for z in (2.0, 4.0, 8.0):
        # PO = (0, 0, z): viewCos = n_z exactly.  n_z = 0.5 is the limit (inside), 0.5 - 2^-20 is beyond it; n_z = float32(0.998) is above
        # the double 0.998 of RadiusByViewingCos: radius 2.5 * 1.2, and the keypoints 3.5 px from the principal point are outside the window
        # (radius 4 * 1.2 holds them)
        Q(query(fr, None, 1, near(code(9000), 0.5) if z == 2.0 else _ident(j), "matched" if z == 2.0 else "above_th_high", pc=(0.0, 0.0, z), exact=True))
        Q.rows[-1]["normal_c"] = np.array([0.25, 0.0, 0.5])
        Q(query(fr, None, 1, _ident(j), "not_in_view", pc=(0.0, 0.0, z), exact=True), name_f="viewing_angle")
        Q.rows[-1]["normal_c"] = np.array([0.25, 0.0, 0.5 - 2.0 ** -20])
        Q(query(fr, None, 1, near(code(9000), 0.25), "window_empty", pc=(0.0, 0.0, z), exact=True))
        Q.rows[-1]["normal_c"] = np.array([0.0, 0.0, float(F32(0.998))])
    fr.kp(601.0 + 3.5, 183.0, 1, code(9000))
    fr.kp(601.0, 183.0 - 3.5, 0, code(9000))
    # the closed bounds: u = 0 / 1241 and v = 0 / 376 are inside (K_DYADIC: pc = (-601 / 128, y, 4), (5, y, 4), (x, -183 / 128, 4), (x, 193 / 128, 4))
    for y in (0.25, 0.5, -0.75):
        Q(query(fr, None, 1, _ident(j), "window_empty", pc=(-601 / 128, y, 4), exact=True))
        Q(query(fr, None, 1, _ident(j), "window_empty", pc=(5, y, 4), exact=True))
    for x in (1.0, -1.0, 2.0):
        Q(query(fr, None, 1, _ident(j), "window_empty", pc=(x, -183 / 128, 4), exact=True))
        Q(query(fr, None, 1, _ident(j), "window_empty", pc=(x, 193 / 128, 4), exact=True))
    # z == 0 with xc != 0: the pixel is +-inf.  (xc == 0 makes it NaN, which passes every comparison of the source and ends in a float -> int
    # conversion of NaN: not built)
    for pc in ((1.0, 1.0, 0.0), (-1.0, 0.5, 0.0), (2.0, -1.0, 0.0)):
        Q(query(fr, None, 1, _ident(j), "not_in_view", pc=pc, exact=True), name_f="outside_u")


def _m2_rows(fr, Q, j, dyadic, th):
    for k in range(3):
        L = 1 + k % 2
        # occupied on entry: alone; with a free second
        c, d = fr.site(), _ident(j)
        fr.kp(c[0] + 0.7, c[1] + 0.7, L, d, taken=True)
        Q(query(fr, c, L, near(d, 0.25), "all_dropped"))
        c, d = fr.site(), _ident(j)
        fr.kp(c[0] + 0.7, c[1] + 0.7, L, d, taken=True)
        fr.kp(c[0] - 1.2, c[1] + 1.0, L, near(d, 0, 0, 0, 0, 0.5))
        Q(query(fr, c, L, near(d, 0.25), "matched"))
        # the ratio test at nn_ratio = 0.75 against a second of the same level at distance 1: best 0.5 passes, 0.75 is the equality
        # and passes, 0.75 + 2^-20 and 1 - 2^-5 are refused; the second at the other level: no test
        for delta, name in (((0.5, 0.5), "matched"), ((0.5, 0.5, 0.5), "matched"), ((0.5, 0.5, 0.5, NEIGHBOUR), "ratio_rejected"),
                            ((0.875, 0.25, 0.375), "ratio_rejected")):
            c, d = fr.site(), _ident(j)
            q = near(d, *delta)
            second = q.copy()
            second[5] = 1.0
            fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
            fr.kp(c[0] - 1.2, c[1] + 1.0, L, second)
            Q(query(fr, c, L, q, name))
        c, d = fr.site(), _ident(j)
        q = near(d, 0.875, 0.25, 0.375)
        second = q.copy()
        second[5] = 1.0
        fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
        fr.kp(c[0] - 1.2, c[1] + 1.0, L - 1, second)
        Q(query(fr, c, L, q, "matched"))
        # two seconds at one distance (1.25) and two levels behind a best at 1: the first in area order gives the level -- the same level
        # refuses (1 > 0.9375), the other one lets the match through
        for first_same, name in ((True, "ratio_rejected"), (False, "matched")):
            c, d = fr.site(on_column_edge=True), _ident(j)
            q = near(d, 1.0)
            second = q.copy()
            second[5] = 1.0
            second[6] = 0.5
            fr.kp(c[0] - 0.3 + 0.4, c[1] + 0.7, L, d)
            fr.kp(c[0] - 0.3 - 1.0, c[1], L if first_same else L - 1, second)          # the lower column is visited first
            fr.kp(c[0] - 0.3 + 1.0, c[1], L - 1 if first_same else L, second)
            Q(query(fr, c, L, q, name))
        # a refused point posts no claim: the next point takes its keypoint (had it been claimed, the second keypoint)
        c, d = fr.site(), _ident(j)
        fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
        fr.kp(c[0] - 1.2, c[1] + 1.0, L, near(d, 0, 0, 0, 0, 0.25))
        Q(query(fr, c, L, near(d, 1.0), "ratio_rejected"), tied=True)
        Q(query(fr, c, L, near(d, 0.25), "chain_after_refusal"), tied=True, kp=len(fr.rows) - 2)
        # the second best changes its level because an earlier point holds the old one: 0.5625 > 0.75 * 0.625 would be refused
        c, d = fr.site(), _ident(j)
        two = near(d, 0, 0, 0, 0, 0.25)
        fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
        fr.kp(c[0] - 1.2, c[1] + 1.0, L, two)
        fr.kp(c[0] + 0.5, c[1] - 1.5, L - 1, near(d, 0, 0, 0, 0, 0.75))
        Q(query(fr, c, L, near(two, 0.125), "chain_takes_second"), tied=True, kp=len(fr.rows) - 2)
        Q(query(fr, c, L, near(d, 0.75), "chain_second_moved"), tied=True, kp=len(fr.rows) - 3)
        # RadiusByViewingCos: the keypoint is 3 px away, inside 4 * th and outside 2.5 * th (levels 0: the factor is 1)
        for off, name in ((False, "window_empty"), (True, "matched")):
            c, d = fr.site(), _ident(j)
            fr.kp(c[0] + 3.0, c[1] + 0.5, 0, d)
            Q(query(fr, c, 0, near(d, 0.25), name))
            if off:                                             # 10 degrees between the normal and the ray: viewCos = 0.985
                nrm = Q.rows[-1]["normal_c"]
                side = np.cross(nrm, [0.0, 1.0, 0.0])
                Q.rows[-1]["normal_c"] = np.cos(np.deg2rad(10)) * nrm + np.sin(np.deg2rad(10)) * side / np.linalg.norm(side)
    if dyadic:
        # th: the keypoint is exactly 2.5 px from an exact pixel, at level 0.  th == 1 leaves the radius at 2.5 (outside: the window is
        # open); the next f32 above 1 is a factor and makes it 2.5000002 (inside)
        for x in (1.0, -1.0, 2.0):
            d = _ident(j)
            fr.kp(512 * x / 4 + 601 + 2.5, 512 * 0.25 / 4 + 183 + 0.5, 0, d)
            Q(query(fr, None, 0, near(d, 0.25), "window_empty" if th == 1.0 else "matched", pc=(x, 0.25, 4), exact=True))


@functools.lru_cache(None)
def m2_exits(cam="dyadic", th=1.0):
    K, _ = CAMERAS[cam]
    fr, R, j = _Frame(K, BOUNDS_KITTI, 8830), _Rows(), [5000]
    _shared_rows(fr, R, True, j)
    _frustum_rows(fr, R, j, cam == "dyadic")
    _m2_rows(fr, R, j, cam == "dyadic", th)
    return _m2_set("m2_exits_%s_%s" % (cam, "1" if th == 1.0 else "1ulp"), fr, R, cam, 8831, th=th)


@functools.lru_cache(None)
def m2_ratio_256():
    """nn_ratio = 2^-9.  A best at 1 with a second of the same level at 256 (16^2) or 260: the source's bestDist2 starts at 256, so such a
    candidate is no second best and the match stands; a second at 255.75 is one, and 1 > 2^-9 * 255.75 refuses"""
    fr, R, j = _Frame(K_DYADIC, BOUNDS_KITTI, 8840), _Rows(), [7000]
    for k in range(3):
        L = 1 + k % 2
        for delta, name in (((16.0,), "matched"), ((16.0, 2.0), "matched"), ((15.0, 5.0, 2.0, 1.0, 0.5, 0.5, 0.5), "ratio_rejected")):
            c, d = fr.site(), _ident(j)
            q = near(d, 0, 0, 0, 0, 0, 0, 0, 1.0)
            fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
            fr.kp(c[0] - 1.2, c[1] + 1.0, L, near(q, *delta))
            R(query(fr, c, L, q, name))
        c, d = fr.site(), _ident(j)
        fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
        R(query(fr, c, L, near(d, 0.25), "matched"))
    return _m2_set("m2_ratio_256", fr, R, "dyadic", 8841, nn_ratio=2.0 ** -9)


# ====================================================================================== crowded, sized and shape sets
def _crowd(kind, n, n_kp, seed, width, cam="kitti", lead_empty=0):
    """n points aimed within 1.5 px at n_kp keypoints in the middle of the image; lead_empty: that many points in front of them whose
    window holds nothing"""
    K, bounds = K_KITTI, BOUNDS_KITTI
    rng = np.random.default_rng(seed)
    kps, desc = _rescaled_frame(n_kp, seed + 1, bounds, width)
    src = rng.integers(0, n_kp, n)
    uv = np.stack([kps["x"][src], kps["y"][src]], 1).astype(np.float64) + rng.uniform(-1.5, 1.5, (n, 2))
    uv[:lead_empty] = np.stack([rng.uniform(30, 200, lead_empty), rng.uniform(30, 340, lead_empty)], 1)
    depth = rng.uniform(3, 60, n)
    Kd = K.astype(np.float64)
    pc = np.stack([(uv[:, 0] - Kd[2]) / Kd[0] * depth, (uv[:, 1] - Kd[3]) / Kd[1] * depth, depth], 1)
    inv = _rigid_inverse(T_CROWD)
    Rm = T_CROWD[:3, :3].astype(np.float64)
    dist = np.linalg.norm(pc, axis=1)
    level = kps["octave"][src] + rng.integers(0, 2, n)
    maxd = (dist * 1.2 ** (level + rng.uniform(-0.8, -0.2, n))).astype(F32)
    nrm = pc / dist[:, None] + rng.normal(0, 0.04, pc.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    base = dict(name="%s_crowd_%d_%d" % (kind, n, n_kp), kps=kps, desc=desc, bounds=bounds, T=T_CROWD, K=K, Xw=inv(pc).astype(F32),
                mp_desc=perturbed_descriptors(desc[src], 0.04, seed + 2), obs=(rng.uniform(size=n) < 0.8).astype(np.uint8),
                crafted=np.full(n, ""), exact=np.zeros(n, bool))
    if kind == "m1":
        kl = np.zeros(n, kps.dtype)
        kl["octave"], kl["size"] = np.clip(level, 0, 7), 31
        kl["angle"] = ((kps["angle"][src] + rng.normal(0, 12, n)) % 360).astype(F32)
        kl["x"], kl["y"] = 20.0 + np.arange(n) % 1200, 20.0 + np.arange(n) % 330
        return dict(base, fn="m1", kps_last=kl, desc_last=np.zeros((n, 128), F32), has=(rng.uniform(size=n) < 0.95).astype(np.uint8), th=7.0, check_ori=True)
    return dict(base, fn="m2", normal=(nrm @ Rm).astype(F32), mind=(maxd / SCALE[7]).astype(F32), maxd=maxd,
                occupied=(rng.uniform(size=n_kp) < 0.1).astype(np.uint8), th=3.0, nn_ratio=0.8, crafted_f=np.full(n, ""))


POINT_KEYS = {"m1": ("has", "Xw", "mp_desc", "obs", "crafted", "exact", "kps_last", "desc_last"),
              "m2": ("Xw", "normal", "mind", "maxd", "mp_desc", "obs", "crafted", "crafted_f", "exact")}


def take(s, keep, name=None):
    """the set with the points `keep` (a mask or indices)"""
    out = dict(s, name=name or s["name"])
    for k in POINT_KEYS[s["fn"]]:
        out[k] = s[k][keep]
    return out


def _clear(s, n=None):
    """the points the reference alone finds clear of every threshold (margin > 2), cut to the first n; `dropped`: the share that went"""
    keep = np.nonzero(run_ref(s)["margin"] > 2)[0]
    assert n is None or len(keep) >= n, (s["name"], len(keep), n)
    out = take(s, keep if n is None else keep[:n])
    total = len(s["Xw"]) if n is None else (int(keep[n - 1]) + 1 if n else 0)
    out["dropped"] = 1.0 - len(out["Xw"]) / total
    return out


CROWD_WIDTH = {60: 40.0, 300: 200.0}                # px: the region the keypoints lie in


def crowd_seed(kind, n_kp):
    return 9500 + n_kp + (7 if kind == "m2" else 0)


@functools.lru_cache(None)
def crowded(kind, n_kp):
    """about 1800 points on n_kp keypoints: claims decide most matches"""
    return _clear(_crowd(kind, 1800, n_kp, crowd_seed(kind, n_kp), CROWD_WIDTH[n_kp]))


SIZES = {"m1": (1024, 1025, 2048, 2049, 4096, 4097), "m2": (512, 513, 1025, 2048, 2049)}


@functools.lru_cache(None)
def sized(kind, n):
    """a call of exactly n points on 300 keypoints"""
    return _clear(_crowd(kind, n + n // 8 + 40, 300, 9600 + n, 400.0), n)


@functools.lru_cache(None)
def m2_many_active(n_active_before=4090, lead_empty=300):
    """more than 4096 map points with a candidate list, 300 points with an empty window in front of them, and a claim chain of ten whose
    points stand at the active ranks n_active_before .. n_active_before + 10: it crosses 4095 -> 4096, the end of the replay's first chunk"""
    s = _clear(_crowd("m2", 5600, 400, 9700, 260.0, lead_empty=lead_empty))
    r = run_ref(s)
    active = (r["n_list"] - r["occupied_on_entry"]) > 0
    cut = int(np.nonzero(np.cumsum(active) == n_active_before)[0][0]) + 1
    # the chain: ten keypoints at a site of its own beside the crowd, as _chain_site builds them
    fr = _Frame(K_KITTI, BOUNDS_KITTI, 9701)
    R = _Rows()
    fr.site_k = 7 * 30 + 25                                     # (1040.3, 319.8): no crowd window reaches it
    _chain_site(fr, R, 2, 10, [9100])
    kps2, desc2, _ = fr.arrays()
    Rm = T_CROWD[:3, :3].astype(np.float64)
    p2 = _pack(R.rows, _rigid_inverse(T_CROWD), lambda nrm: np.asarray(nrm) @ Rm)
    out = dict(s, name="m2_many_active")
    n0 = len(s["kps"])
    out["kps"], out["desc"] = np.concatenate([s["kps"], kps2]), np.concatenate([s["desc"], desc2])
    out["occupied"] = np.concatenate([s["occupied"], np.zeros(len(kps2), np.uint8)])
    ins = dict(Xw=p2["Xw"], normal=p2["normal"], mind=p2["mind"], maxd=p2["maxd"], mp_desc=p2["mp_desc"], obs=np.ones(11, np.uint8),
               crafted=p2["crafted"], crafted_f=np.full(11, "in_view"), exact=np.zeros(11, bool))
    kp = np.array([q["kp"] for q in R.rows], np.int32)
    out["expect_kp"] = np.where(kp >= 0, kp + n0, kp)
    for k in POINT_KEYS["m2"]:
        out[k] = np.concatenate([s[k][:cut], ins[k], s[k][cut:]])
    out["chain_at"], out["n_kp_crowd"] = cut, n0
    return out


LIST_LENGTHS = (1, 2, 3, 4, 5, 64, 65, 128, 129, 256, 257)


@functools.lru_cache(None)
def lists(kind):
    """one site per list length: n keypoints of octave 1 within 8 px of the site and one point of level 1 whose window (radius 12: th = 10
    for M1, 2.5 * 4 for M2) holds them all.  The sites of 64 and 65 lie in the middle of a grid column (a column range of 64 and of 65
    items: the search's fast form ends at 64), the site of 128 on the boundary between two columns with 64 keypoints on either side (the
    longest list of the fast form), 129 one more.  A field of 1300 keypoints of octaves 6 and 7 inside a level-7 window gives a list of
    about 1300."""
    fr, R = _Frame(K_KITTI, BOUNDS_KITTI, 9800), _Rows()
    rng = fr.rng
    w = fr.cell_w

    def rand_desc(n):
        d = rng.standard_normal((n, 128)).astype(F32)
        return d / np.linalg.norm(d, axis=1, keepdims=True)
    for k, n in enumerate(LIST_LENGTHS):
        col = 4 + 4 * k
        on_edge = n in (128, 129)
        cx_, cy_ = (col + (0.5 if on_edge else 0.0)) * w, 60.0 + 90.0 * (k % 3)
        d = rand_desc(n)
        m = min(n, 128) // 2 if on_edge else n
        xs = np.concatenate([cx_ - 0.5 - rng.uniform(0, 7, m), cx_ + 0.5 + rng.uniform(0, 7, n - m)]) if on_edge else cx_ + rng.uniform(-7, 7, n)
        ys = cy_ + rng.uniform(-7, 7, n)
        for i in range(n):
            fr.kp(xs[i], ys[i], 1, d[i])
        R(query(fr, np.array([cx_ + 0.013, cy_ + 0.021]), 1, perturbed_descriptors(d[:1], 0.04, 9801 + k)[0], "list%d" % n))
    nf = 1300
    d = rand_desc(nf)
    fx_, fy_ = rng.uniform(1000, 1060, nf), rng.uniform(280, 340, nf)
    fo = rng.integers(6, 8, nf)
    for i in range(nf):
        fr.kp(fx_[i], fy_[i], int(fo[i]), d[i])
    for k in range(3):
        R(query(fr, np.array([1030.0 + k, 310.0 - k]), 8 if kind == "m2" else 7, perturbed_descriptors(d[k:k + 1], 0.04, 9850 + k)[0], "field"))
    if kind == "m1":
        return _m1_set("m1_lists", fr, R, "kitti", 9802, th=10.0)
    return _m2_set("m2_lists", fr, R, "kitti", 9802, th=4.0, nn_ratio=0.8)


PREFIXES = (1, 7, 8, 9)


@functools.lru_cache(None)
def wide(kind, n_first=None):
    """loop_search_cases' shape frame (a clump of 100 keypoints in one cell: a column range of more than 64 items; a lattice of 128 with a
    129th; a field of 1400; keypoints beside every border) under M1 (th = 10) or M2 (th = 4, radius factor 2.5); n_first: the first
    queries alone (calls of 1, 7, 8 and 9)"""
    fr, first, field_q = _shape_frame(10.0, 8700)
    R = _Rows()
    for q in (first + field_q if n_first is None else first[:n_first]):
        R(q)
    if n_first is None:
        # windows of 16 and of 17 grid columns (the search's fast form ends at 16): level-3 windows, 15.4 cells wide, cut by the left border, over
        # the keypoint beside it
        c = fr.cell_w
        e = next(k for k, row in enumerate(fr.rows) if abs(row["x"] - 0.4 * c) < 1e-6 and abs(row["y"] - 14 * c) < 1e-6)
        for cols, u in ((16, 7.0 * c), (17, 7.95 * c)):
            R(query(fr, np.array([u, 14.1 * c]), 3, perturbed_descriptors(fr.rows[e]["desc"][None], 0.04, 8710 + cols)[0], "cols%d" % cols))
    name = "%s_wide_%s" % (kind, "all" if n_first is None else n_first)
    if kind == "m1":
        s = _m1_set(name, fr, R, "dyadic", 0, th=10.0)
        s["K"] = fr.K
        s["kps_last"]["angle"] = (s["kps_last"]["angle"] + fr.rng.uniform(-100, 100, len(s["has"]))).astype(F32)
    else:
        s = _m2_set(name, fr, R, "dyadic", 0, th=4.0, nn_ratio=0.8)
        s["K"] = fr.K
    return _clear(s) if n_first is None else s


@functools.lru_cache(None)
def grow(kind):
    """loop_search_cases.fuse_grow's frame -- 2000 keypoints, 200 level-7 windows over all of them -- under M1 (th = 3, octave 7) and M2
    (th = 1.2, radius factor 2.5): 400000 candidates, more than the 2^18 a fresh context has room for"""
    g = fuse_grow()
    n = len(g["valid"])
    base = dict(name=kind + "_grow", kps=g["kps"], desc=g["desc"], bounds=g["bounds"], T=g["T"], K=g["K"], Xw=g["Xw"], mp_desc=g["mp_desc"],
                obs=np.ones(n, np.uint8), crafted=np.full(n, ""), exact=np.zeros(n, bool))
    if kind == "m1":
        kl = np.zeros(n, g["kps"].dtype)
        kl["octave"], kl["size"], kl["angle"] = 7, 31, 100.0
        kl["x"], kl["y"] = 20.0 + np.arange(n), 20.0
        return dict(base, fn="m1", kps_last=kl, desc_last=np.zeros((n, 128), F32), has=g["valid"], th=3.0, check_ori=True)
    return dict(base, fn="m2", normal=g["normal"], mind=g["mind"], maxd=g["maxd"], occupied=np.zeros(len(g["kps"]), np.uint8), th=1.2, nn_ratio=0.8,
                crafted_f=np.full(n, ""))


# ====================================================================================== drivers
_FRAMES = {}


def _frame(s):
    key = (id(s["kps"]), id(s["desc"]))
    if key not in _FRAMES:
        _FRAMES[key] = (ref.Frame(s["kps"], s["desc"], s["bounds"]), s["kps"], s["desc"])
    return _FRAMES[key][0]


def run_ref(s, **mutant):
    """M1: the per-point dict.  M2: the per-point dict of the search with `frustum` (is_in_frustum's) beside it; the frustum's mutants are
    drop_factors and cos_closed"""
    fr = _frame(s)
    if s["fn"] == "m1":
        return ref.search_by_projection_frame(fr, s["kps_last"]["octave"], s["kps_last"]["angle"], s["has"], s["Xw"], s["mp_desc"], s["T"], s["K"],
                                              s["th"], s["check_ori"], s["obs"], **mutant)
    fkw = {k: mutant.pop(k) for k in ("drop_factors", "cos_closed") if k in mutant}
    f = ref.is_in_frustum(s["bounds"], s["Xw"], s["normal"], s["mind"], s["maxd"], s["T"], s["K"], **fkw)
    r = ref.search_by_projection_points(fr, f, s["mp_desc"], s["occupied"], s["th"], s["nn_ratio"], s["obs"], **mutant)
    r["frustum"] = f
    return r


def run_oracle(oracle, s):
    """-> (match_cur, n_matches) and, M2, the frustum's four outputs"""
    f = oracle.frame(s["kps"], s["desc"], s["bounds"])
    if s["fn"] == "m1":
        last = oracle.frame(s["kps_last"], s["desc_last"], s["bounds"])
        return oracle.match_project_frame(f, last, s["has"], s["Xw"], s["mp_desc"], s["T"], s["K"], s["th"], s["check_ori"], obs_positive=s["obs"])
    fo = oracle.frustum(f, s["Xw"], s["normal"], s["mind"], s["maxd"], s["T"], s["K"])
    return oracle.match_project_points(f, *fo, s["mp_desc"], s["occupied"], s["th"], s["nn_ratio"], obs_positive=s["obs"]) + (fo,)


def decided(s, r):
    return r["decidable"] | s["exact"]


def check(s, r, got, fo=None):
    """match table and count against the reference: both searches are claim-coupled (one undecided row may change every later one), so
    every point of a set must be decided, and then every element is compared.  fo: the frustum's outputs, compared on the same rule"""
    dec = decided(s, r)
    assert dec.all(), (s["name"], np.nonzero(~dec)[0][:10])
    np.testing.assert_array_equal(got[0], r["match_cur"], err_msg=s["name"])
    assert got[1] == r["n_matches"], (s["name"], got[1], r["n_matches"])
    if fo is not None:
        f = r["frustum"]
        np.testing.assert_array_equal(np.asarray(fo[0]).astype(bool), f["in_view"], err_msg=s["name"])
        iv = f["in_view"]
        np.testing.assert_array_equal(np.asarray(fo[2])[iv], f["level"][iv], err_msg=s["name"])
        assert np.abs(np.asarray(fo[1], np.float64)[iv] - np.stack([f["u"], f["v"]], 1)[iv]).max(initial=0) <= ref.PIXEL_TOL, s["name"]
        assert np.abs(np.asarray(fo[3], np.float64)[iv] - f["view_cos"][iv]).max(initial=0) <= ref.COS_TOL, s["name"]


def n_candidates(s, r):
    """what k_window_search<true> writes for the call: the keypoints inside every window behind the level gate, without the ones
    occupied on entry"""
    return int(r["n_list"].sum() - (r["occupied_on_entry"].sum() if s["fn"] == "m2" else 0))
