"""Crafted inputs for tests/test_loop_search_exits.py: the sets, and drivers with one interface over the restatement
(tests/loop_search_ref.py), the CPU oracle and the library's four entry points.

A set is a dict: fn ("reloc", "scw", "fuse", "sim3"), the frame(s), the call's arrays, `crafted` (per query the exit its row
was built for, "" where none) and `exact` (rows that sit on a bound by construction and are compared regardless of margin).

Exit sets.  One row per rule, each at a SITE of its own: sites lie 40 px apart, a row's keypoints within 2 px of its site and
its window (levels 0..2; the clamped rows keep their neighbours free) never reaches the next site, so a row's result is what its
own keypoints make it.  The camera is a
pure translation and the exact rows use dyadic camera coordinates with K = (512, 512, 601, 183): their f32 pixel is exactly on
the bound.  Descriptors are sparse: a keypoint's identity is three components of value 2 (two different keypoints are at least
8 apart), a query copies its target's identity and adds a few components that are multiples of 2^-10 in rows 0..7, so every
distance is a short sum of multiples of 2^-20 below 2^7: exact in f32 in any order.  0.25 + 0.25 is TH_LOW, 1 + 0.25 + 0.25 is
TH_HIGH, and a further component 2^-10 puts the neighbour 2^-20 beyond.

Shape sets.  Frames whose bounds are 64 x 48 cells of c = th * 1.2^7 / 16 pixels, so that a level-7 window spans 32 grid
columns whatever th the function is called with: a clump of 100 keypoints in one cell (a column range of more than 64 items in
a window of fewer than 16 columns), a lattice of 128 keypoints with a 129th just outside the smaller of two windows (lists of
128 and 129), a field of 1400 keypoints (lists beyond 256, windows of more than 16 columns, totals beyond 4096) and keypoints
beside the four borders and in two corners (clipped windows).  A window wholly outside the grid cannot be asked for through
these entry points: the image gate in front of the search uses the bounds the grid was built with, so a query that passes it
has its centre inside the grid.

Crowded sets.  Random frames with 3 map points aimed at every keypoint (relocalisation, Scw search: most matches are decided
by claims) or one (Fuse, SearchBySim3); the map points are the ones the reference alone finds clear of every threshold
(margin > 2).
"""
import functools

import numpy as np

from tests import loop_search_ref as ref
from tests.test_matcher import make_frame, perturbed_descriptors, pose_T

F32 = np.float32
SCALE = ref.level_tables(8, 1.2)[0]
K_KITTI = np.array([718.856, 718.856, 607.1928, 185.2157], F32)
K_EUROC = np.array([458.654, 457.296, 367.215, 248.375], F32)
K_DYADIC = np.array([512.0, 512.0, 601.0, 183.0], F32)
BOUNDS_KITTI = (0.0, 1241.0, 0.0, 376.0)
BOUNDS_EUROC = (0.0, 752.0, 0.0, 480.0)
TH = dict(reloc=10.0, scw=4, fuse=3.0, sim3=7.5)
SCW_SCALES = (1.0, 0.37, 2.5)
S12 = F32(1.3)
EQ_LOW, EQ_HIGH = (0.5, 0.5), (1.0, 0.5, 0.5)            # squared: TH_LOW, TH_HIGH
NEIGHBOUR = 2.0 ** -10                                    # squared: 2^-20
PITCH = 40.0


def _kp_dtype():
    from tests.conftest import load_package
    return load_package().capi.KP_DTYPE


def code(j):
    """the identity of keypoint j: three components of value 2"""
    d = np.zeros(128, F32)
    d[8 + j % 40] = d[48 + (j // 40) % 40] = d[88 + (j // 1600) % 40] = 2
    return d


def near(d, *delta):
    """d with `delta` written into its components 0, 1, ...: the squared distance to d is the sum of delta^2"""
    d = d.copy()
    d[:len(delta)] = delta
    return d


def translation(t=(0.5, -0.25, 1.0)):
    T = np.eye(4, dtype=F32)
    T[:3, 3] = t
    return T


def sim3_of(T, s):
    S = np.asarray(T, F32).copy()
    S[:3, :] = (F32(s) * S[:3, :]).astype(F32)
    return S


def _rigid_inverse(T):
    R, t = np.asarray(T, F32).astype(np.float64)[:3, :3], np.asarray(T, F32).astype(np.float64)[:3, 3]
    return lambda pc: (np.asarray(pc, np.float64) - t) @ R


class _Frame:
    """keypoints of one frame with, for SearchBySim3, the query each may carry"""

    def __init__(self, K, bounds, seed):
        self.K, self.bounds = np.asarray(K, F32), bounds
        self.rng = np.random.default_rng(seed)
        self.rows, self.site_k = [], 0
        w = (bounds[1] - bounds[0]) / 64
        self.cell_w = w

    def kp(self, x, y, octave, desc, taken=False, angle=50.0, query=None):
        self.rows.append(dict(x=x, y=y, octave=octave, desc=desc, taken=taken, angle=angle, query=query))
        return len(self.rows) - 1

    def site(self, gap=False, on_column_edge=False):
        """the next free site; gap: its neighbours stay free; on_column_edge: moved onto the nearest boundary between two grid
        columns (PosInGrid rounds: the cells change at the half)"""
        per_row = int((self.bounds[1] - self.bounds[0] - 2 * PITCH) // PITCH) + 1
        if gap:
            self.site_k += 1
            if self.site_k % per_row == 0:
                self.site_k += 1
        k = self.site_k
        self.site_k += 2 if gap else 1
        u, v = self.bounds[0] + PITCH * (1 + k % per_row), self.bounds[2] + PITCH * (1 + k // per_row)
        assert v <= self.bounds[3] - PITCH, "out of sites"
        if on_column_edge:
            u = (np.round(u / self.cell_w - 0.5) + 0.5) * self.cell_w
        return np.array([u + 0.3, v - 0.2])

    def arrays(self):
        kps = np.zeros(len(self.rows), _kp_dtype())
        for f in ("x", "y", "octave", "angle"):
            kps[f] = [r[f] for r in self.rows]
        kps["size"] = 31
        return kps, np.stack([r["desc"] for r in self.rows]).astype(F32), np.array([r["taken"] for r in self.rows])


def query(fr, uv, level, desc, name="", g=-0.5, depth=None, behind=False, pc=None, near_far=0, off_normal=False, valid=1,
          angle=200.0, exact=False):
    """a map point aimed at pixel uv of frame fr, in the camera's coordinates: PredictScale sees level + g before ceil"""
    fx, fy, cx, cy = fr.K.astype(np.float64)
    if pc is None:
        d = fr.rng.uniform(4, 30) if depth is None else depth
        pc = np.array([(uv[0] - cx) / fx * d, (uv[1] - cy) / fy * d, d]) * (-1 if behind else 1)
    pc = np.asarray(pc, np.float64)
    dist = np.linalg.norm(pc)
    maxd = dist * 1.2 ** (level + g)
    mind = maxd / float(SCALE[7])
    if near_far < 0:                                       # dist = 0.8 * min / 1.12
        mind = dist * 1.4
        maxd = mind * float(SCALE[7])
    elif near_far > 0:                                     # dist = 1.2 * max * 1.1
        maxd = dist / 1.2 / 1.1
        mind = maxd / float(SCALE[7])
    nrm = pc / dist if dist > 0 else np.array([0.0, 0.0, 1.0])
    if off_normal:                                         # 75 degrees between the normal and the viewing ray
        side = np.cross(nrm, [0.0, 1.0, 0.0])
        side /= np.linalg.norm(side)
        nrm = np.cos(np.deg2rad(75)) * nrm + np.sin(np.deg2rad(75)) * side
    return dict(pc=pc, mind=mind, maxd=maxd, normal_c=nrm, desc=desc, valid=valid, name=name, angle=angle, exact=exact)


def _pack(queries, to_world, rotate):
    """queries -> the call's arrays; to_world maps camera coordinates to the world, rotate maps a camera direction"""
    n = len(queries)
    out = dict(valid=np.array([q["valid"] for q in queries], np.uint8), Xw=np.zeros((n, 3), F32), normal=np.zeros((n, 3), F32),
               mind=np.array([q["mind"] for q in queries], F32), maxd=np.array([q["maxd"] for q in queries], F32),
               mp_desc=np.stack([q["desc"] for q in queries]).astype(F32) if n else np.zeros((0, 128), F32),
               angle=np.array([q["angle"] for q in queries], F32), crafted=np.array([q["name"] for q in queries]),
               exact=np.array([q["exact"] for q in queries], bool))
    for i, q in enumerate(queries):
        out["Xw"][i], out["normal"][i] = to_world(q["pc"]), rotate(q["normal_c"])
    return out


# ====================================================================================== the rows the four functions share
def _common_rows(fr, Q, kind, eq, n_each=3):
    """kind: "scw", "fuse", "sim3" (level gate [pred - 1, pred] in the loop) or "reloc" ([pred - 1, pred + 1] in the area query).
    Q(q, site_keypoints...) appends a query.  eq: the components whose squares sum to the acceptance threshold."""
    claims = kind in ("scw", "reloc")
    matched = "matched" if kind != "sim3" else "one_way"
    above = dict(scw="above_th_low", fuse="above_th_low", sim3="above_th_high", reloc="above_orb_dist")[kind]
    top = 1 if kind == "reloc" else 0                      # the highest accepted octave is pred + top
    j = [1000]

    def ident():
        j[0] += 1
        return code(j[0])

    for k in range(n_each):
        L = k % 3
        # a keypoint alone, close / exactly at the threshold / 2^-20 beyond it
        for delta, name in (((0.25,), matched), (eq, matched), (eq + (NEIGHBOUR,), above)):
            c, d = fr.site(), ident()
            fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
            Q(query(fr, c, L, near(d, *delta), name))
        # the keypoint one octave below the prediction is accepted, two below is not
        c, d = fr.site(), ident()
        fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
        Q(query(fr, c, L + 1, near(d, 0.25), matched))
        c, d = fr.site(), ident()
        fr.kp(c[0] + 0.7, c[1] + 0.7, 0, d)
        Q(query(fr, c, 2, near(d, 0.25), "window_empty" if kind == "reloc" else "all_dropped"))
        # the highest accepted octave, and the one above it
        c, d = fr.site(), ident()
        fr.kp(c[0] + 0.7, c[1] + 0.7, L + top, d)
        Q(query(fr, c, L, near(d, 0.25), matched))
        c, d = fr.site(), ident()
        fr.kp(c[0] + 0.7, c[1] + 0.7, L + top + 1, d)
        Q(query(fr, c, L, near(d, 0.25), "window_empty" if kind == "reloc" else "all_dropped"))
        # the closer keypoint is one octave too high, the other one is taken
        c, d = fr.site(), ident()
        fr.kp(c[0] + 0.7, c[1] + 0.7, L + top + 1, d)
        fr.kp(c[0] - 1.2, c[1] + 1.0, L, near(d, 0, 0, 0, 0, 0.5))
        Q(query(fr, c, L, near(d, 0.25), matched))
        # no keypoint at all
        Q(query(fr, fr.site(), L, ident(), "window_empty"))
        # gates in front of the search; each aims at a keypoint that would match
        gates = [(dict(valid=0), "invalid" if kind != "sim3" else "no_point"), (dict(near_far=-1), "too_near"), (dict(near_far=1), "too_far")]
        if kind in ("scw", "fuse"):
            gates.append((dict(off_normal=True), "viewing_angle"))
        if kind != "reloc":
            gates.append((dict(behind=True), "behind"))
        for kw, name in gates:
            c, d = fr.site(), ident()
            fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
            Q(query(fr, c, L, near(d, 0.25), name, **kw))
        # PredictScale beyond the top level: ceil(7.5) = 8 is clamped to 7 (and dist lies between 0.8 * min and min)
        c, d = fr.site(gap=True), ident()
        fr.kp(c[0] + 0.7, c[1] + 0.7, 7, d)
        Q(query(fr, c, 8, near(d, 0.25), matched))
        # two keypoints with one descriptor on both sides of a column boundary: the first in area order has the larger index
        c, d = fr.site(on_column_edge=True), ident()
        fr.kp(c[0] - 0.3 + 1.0, c[1], L, d)
        fr.kp(c[0] - 0.3 - 1.0, c[1], L, d)
        Q(query(fr, c, L, near(d, 0.25), matched))
        # ... and inside one cell
        c, d = fr.site(), ident()
        fr.kp(c[0] + 0.7, c[1] + 0.7, L, d)
        fr.kp(c[0] + 1.2, c[1] + 0.9, L, d)
        Q(query(fr, c, L, near(d, 0.25), matched))
        # four points whose best keypoint is the same; the keypoints differ in component 4 alone
        c, d = fr.site(), ident()
        for x, y, c4 in ((0.7, 0.7, 0.0), (-1.2, 1.0, 0.25), (0.5, -1.5, 0.5)):
            fr.kp(c[0] + x, c[1] + y, L, near(d, 0, 0, 0, 0, c4))
        for n, c0 in enumerate((0.125, 0.25, 0.375, 0.0625)):
            Q(query(fr, c, L, near(d, c0), "chain%d" % n if claims else matched))
        if claims:
            # the only keypoint holds a point on entry; the closer one does and the second is taken
            c, d = fr.site(), ident()
            fr.kp(c[0] + 0.7, c[1] + 0.7, L, d, taken=True)
            Q(query(fr, c, L, near(d, 0.25), "all_dropped"))
            c, d = fr.site(), ident()
            fr.kp(c[0] + 0.7, c[1] + 0.7, L, d, taken=True)
            fr.kp(c[0] - 1.2, c[1] + 1.0, L, near(d, 0, 0, 0, 0, 0.5))
            Q(query(fr, c, L, near(d, 0.25), matched))
    # pixels 5 px beyond each bound
    b = fr.bounds
    for k, uv in enumerate(((b[0] - 5, 100.3), (b[1] + 5, 120.3), (300.3, b[2] - 5), (340.3, b[3] + 5)) * 2):
        Q(query(fr, np.array(uv), k % 3, ident(), ("outside_u" if k % 4 < 2 else "outside_v") if kind == "reloc" else "outside_image"))


def _bound_rows(fr, Q, kind):
    """pixels exactly on min_x, max_x, min_y, max_y (K_DYADIC, KITTI bounds, camera coordinates with few bits), each with a
    matching keypoint inside its window, and points on the camera plane.  PosInGrid drops a keypoint beyond column 63.5, 9.7 px
    inside max_x, so the rows are at the lowest level whose window reaches further than that."""
    matched = "matched" if kind != "sim3" else "one_way"
    on_max = (matched,) * 2 if kind == "reloc" else ("outside_image",) * 2
    on_plane = "outside_u" if kind == "reloc" else "outside_image"
    L = min(lv for lv in range(3, 8) if float(TH[kind]) * float(SCALE[lv]) - 0.6 > 9.95)
    reach = float(TH[kind]) * float(SCALE[L]) - 0.6        # a keypoint this far from the pixel is inside the window
    assert 1241 - reach < 63.49 * fr.cell_w
    j = 5000
    for y in (0.25, 0.5, -0.75):                           # u = 0 and u = 1241: pc = (-601 / 128, y, 4), (5, y, 4)
        v = 512 * y / 4 + 183
        j += 2
        fr.kp(4.0, v + 0.5, L, code(j))
        Q(query(fr, None, L, near(code(j), 0.25), matched, pc=(-601 / 128, y, 4), exact=True))
        fr.kp(1241 - reach, v + 0.5, L, code(j + 1))
        Q(query(fr, None, L, near(code(j + 1), 0.25), on_max[0], pc=(5, y, 4), exact=True))
    for x in (1.0, -1.0, 2.0):                             # v = 0 and v = 376: pc = (x, -183 / 128, 4), (x, 193 / 128, 4)
        u = 512 * x / 4 + 601
        j += 2
        fr.kp(u + 0.5, 3.0, L, code(j))
        Q(query(fr, None, L, near(code(j), 0.25), matched, pc=(x, -183 / 128, 4), exact=True))
        fr.kp(u + 0.5, 376 - 4.5, L, code(j + 1))          # row 47 ends at 47.5 * 376 / 48 = 372.08
        Q(query(fr, None, L, near(code(j + 1), 0.25), on_max[1], pc=(x, 193 / 128, 4), exact=True))
    for pc in ((1.0, 1.0, 0.0), (-1.0, 0.5, 0.0), (0.0, 0.0, 0.0), (0.0, 2.0, 0.0)):
        Q(query(fr, None, L, code(j), on_plane, pc=pc, exact=True))


def _shuffle(p, rng):
    """the queries in another order than their keypoints; chains keep their index order"""
    n = len(p["valid"])
    order = rng.permutation(n)
    chain = np.array([c.startswith("chain") for c in p["crafted"]])
    order[np.isin(order, np.nonzero(chain)[0])] = np.nonzero(chain)[0]      # the chain rows keep their relative order
    return {k: v[order] for k, v in p.items()}


# ====================================================================================== exit sets
@functools.lru_cache(None)
def scw_exits(kind="scw"):
    """SearchByProjection(KeyFrame, Scw) / Fuse(KeyFrame, Scw): the rows of _common_rows and _bound_rows.  The camera is T at
    scale 1; run_* applies s["scale"]"""
    fr = _Frame(K_DYADIC, BOUNDS_KITTI, 8100)
    qs = []
    _common_rows(fr, qs.append, kind, EQ_LOW)
    _bound_rows(fr, qs.append, kind)
    T = translation()
    inv = _rigid_inverse(T)
    p = _shuffle(_pack(qs, inv, lambda n: n), fr.rng)
    kps, desc, taken = fr.arrays()
    return dict(fn=kind, name=kind + "_exits", kps=kps, desc=desc, bounds=fr.bounds, T=T, K=fr.K, th=TH[kind], scale=1.0,
                matched_kp=np.where(taken, -2, -1).astype(np.int32), **p)


def fuse_exits():
    return scw_exits("fuse")


@functools.lru_cache(None)
def reloc_exits():
    """SearchByProjection(Frame, KeyFrame): the common rows, the bound rows, points behind the camera whose mirrored pixel holds a
    matching keypoint, a negative rot, and three points whose angle puts them into bin 30 -> 0 (an angle of 950 degrees: the
    extractor makes none, the array may hold one), which the orientation check then removes: bin 0 holds less than a tenth"""
    fr = _Frame(K_DYADIC, BOUNDS_KITTI, 8200)
    qs = []
    _common_rows(fr, qs.append, "reloc", (1.0,))
    _bound_rows(fr, qs.append, "reloc")
    for k in range(3):
        c, d = fr.site(), code(7000 + k)
        fr.kp(c[0] + 0.7, c[1] + 0.7, k, d)
        qs.append(query(fr, c, k, near(d, 0.25), "matched", behind=True))
        c, d = fr.site(), code(7010 + k)
        fr.kp(c[0] + 0.7, c[1] + 0.7, k, d, angle=230.0)
        qs.append(query(fr, c, k, near(d, 0.25), "matched", angle=20.0))
        c, d = fr.site(), code(7020 + k)
        fr.kp(c[0] + 0.7, c[1] + 0.7, k, d)
        qs.append(query(fr, c, k, near(d, 0.25), "removed_by_orientation", angle=950.0))
    T = translation()
    p = _shuffle(_pack(qs, _rigid_inverse(T), lambda n: n), fr.rng)
    kps, desc, taken = fr.arrays()
    return dict(fn="reloc", name="reloc_exits", kps=kps, desc=desc, bounds=fr.bounds, T=T, K=fr.K, th=TH["reloc"], orb_dist=1.0,
                check_ori=True, occupied=taken.astype(np.uint8), **p)


@functools.lru_cache(None)
def reloc_orb(orb_dist):
    """ORBdist = 0.25: a row at, and one 2^-20 beyond.  ORBdist = 200: a row at 10^2 + 10^2 and one at 11^2 = 121, which a
    starting bestDist of 100 would never take"""
    fr = _Frame(K_DYADIC, BOUNDS_KITTI, 8300)
    qs = []
    eq = (0.5,) if orb_dist == 0.25 else (10.0, 10.0)
    for k in range(3):
        for delta, name in ((eq, "matched"), (eq + (NEIGHBOUR if orb_dist == 0.25 else 2.0 ** -6,), "above_orb_dist"), ((11.0,), "matched" if orb_dist > 121 else "above_orb_dist")):
            c, d = fr.site(), code(7100 + len(qs))
            fr.kp(c[0] + 0.7, c[1] + 0.7, k, d)
            qs.append(query(fr, c, k, near(d, *delta), name))
    T = translation()
    p = _shuffle(_pack(qs, _rigid_inverse(T), lambda n: n), fr.rng)
    kps, desc, taken = fr.arrays()
    return dict(fn="reloc", name="reloc_orb_%g" % orb_dist, kps=kps, desc=desc, bounds=fr.bounds, T=T, K=fr.K, th=TH["reloc"],
                orb_dist=orb_dist, check_ori=False, occupied=taken.astype(np.uint8), **p)


ORI_CASES = {"ori_at": (3, 3, 2), "ori_below": (2, 2, 1), "ori_third_below": (3, 2, 1)}


@functools.lru_cache(None)
def reloc_ori(case):
    """30 matches in bin 5 and n2 / n3 / n4 in bins 0 (through bin 30), 9 and 2: with (3, 3, 2) the second and third bin hold
    exactly a tenth of the first and stay, with (2, 2, 1) both go, with (3, 2, 1) the third goes; bin 2 always goes"""
    n2, n3, n4 = ORI_CASES[case]
    fr = _Frame(K_DYADIC, BOUNDS_KITTI, 8400)
    qs = []
    for n, angle, name in ((30, 200.0, "matched"), (n2, 950.0, "matched" if n2 >= 3 else "removed_by_orientation"),
                           (n3, 320.0, "matched" if n3 >= 3 else "removed_by_orientation"), (n4, 110.0, "removed_by_orientation")):
        for k in range(n):
            c, d = fr.site(), code(7200 + len(qs))
            fr.kp(c[0] + 0.7, c[1] + 0.7, k % 3, d)
            qs.append(query(fr, c, k % 3, near(d, 0.25), name, angle=angle))
    T = translation()
    p = _shuffle(_pack(qs, _rigid_inverse(T), lambda n: n), fr.rng)
    kps, desc, taken = fr.arrays()
    return dict(fn="reloc", name="reloc_" + case, kps=kps, desc=desc, bounds=fr.bounds, T=T, K=fr.K, th=TH["reloc"], orb_dist=1.0,
                check_ori=True, occupied=taken.astype(np.uint8), **p)


def _sim3_transforms(s12, identity=False):
    T1, T2 = pose_T((0.01, -0.02, 0.005), (0.1, -0.05, 0.3)), pose_T((0.02, 0.01, -0.01), (-0.3, 0.1, 0.2))
    T12 = pose_T((0.004, -0.01, 0.002), (0.15, -0.02, 0.05))
    if identity:
        T1, T2, T12 = translation(), translation((0.25, 0.5, -1.0)), np.eye(4, dtype=F32)
    R12, t12 = T12[:3, :3].copy(), T12[:3, 3].copy()
    s = float(F32(s12))
    R12d, t12d = R12.astype(np.float64), t12.astype(np.float64)
    inv1, inv2 = _rigid_inverse(T1), _rigid_inverse(T2)
    t21 = -(1 / s) * R12d.T @ t12d
    to_world_1 = lambda p2: inv1(s * R12d @ (np.asarray(p2) - t21))            # p2 = sR21 (R1w X + t1w) + t21
    to_world_2 = lambda p1: inv2((1 / s) * R12d.T @ (np.asarray(p1) - t12d))   # p1 = sR12 (R2w X + t2w) + t12
    return T1, T2, R12, t12, to_world_1, to_world_2


def _sim3_set(name, f1, f2, s12, identity=False):
    """f1 / f2: _Frame objects whose keypoints may carry a query aimed into the other frame"""
    T1, T2, R12, t12, w1, w2 = _sim3_transforms(s12, identity)
    out = dict(fn="sim3", name=name, s12=float(s12), R12=R12, t12=t12, T1=T1, T2=T2, K=f1.K, th=TH["sim3"])
    blank = query(f1, None, 0, code(0), "no_point", pc=(0.0, 0.0, 5.0), valid=0)
    for tag, fr, w in (("1", f1, w1), ("2", f2, w2)):
        kps, desc, _ = fr.arrays()
        p = _pack([r["query"] or blank for r in fr.rows], w, lambda n: n)
        out.update({"kps" + tag: kps, "desc" + tag: desc, "bounds" + tag: fr.bounds, "has" + tag: p["valid"], "Xw" + tag: p["Xw"],
                    "mind" + tag: p["mind"], "maxd" + tag: p["maxd"], "mp_desc" + tag: p["mp_desc"], "crafted" + tag: p["crafted"],
                    "exact" + tag: p["exact"]})
    return out


def _holders(fr, other, x0, y0, j0):
    """-> the function that gives a query its own keypoint in `fr`: one of a row 3 px apart at height y0, which no window of the
    crafted rows reaches.  Every keypoint that the row has put into `other` since the last call gets a point aimed back at
    that keypoint, so that a match of the row is mutual and shows in match12."""
    state = dict(n=0, mark=0)

    def add(q):
        state["n"] += 1
        x, d = x0 + 3.0 * state["n"], code(j0 + state["n"])
        fr.kp(x, y0, 0, d, query=q)
        for row in other.rows[state["mark"]:]:
            if row["query"] is None:
                row["query"] = query(fr, np.array([x + 0.3, y0 + 0.2]), 0, near(d, 0.25))
        state["mark"] = len(other.rows)
    return add


@functools.lru_cache(None)
def sim3_exits():
    """both directions get the common rows, each of whose keypoints names the row's own keypoint back; then pairs that name each
    other at, and 2^-20 beyond, TH_HIGH, and pairs of which one names a third keypoint"""
    f1, f2 = _Frame(K_DYADIC, BOUNDS_KITTI, 8500), _Frame(K_DYADIC, BOUNDS_KITTI, 8501)
    _common_rows(f2, _holders(f1, f2, 8.0, 6.0, 3000), "sim3", EQ_HIGH)
    _common_rows(f1, _holders(f2, f1, 8.0, 6.0, 3200), "sim3", EQ_HIGH)
    for k in range(12):
        c1, c2 = f1.site(), f2.site()
        da, db = code(4000 + 2 * k), code(4001 + 2 * k)
        d12 = (EQ_HIGH, EQ_HIGH + (NEIGHBOUR,), (0.25,))[k % 3]            # k % 3 == 1: a's point is 2^-20 too far from b
        a_q = query(f2, c2, k % 3, near(db, *d12), "one_way" if k % 3 != 1 else "above_th_high")
        b_q = query(f1, c1, k % 3, near(da, 0.25), "one_way")
        f1.kp(c1[0] + 0.7, c1[1] + 0.7, k % 3, da, query=a_q)
        f2.kp(c2[0] + 0.7, c2[1] + 0.7, k % 3, db, query=b_q)
        if k >= 8:                                          # a third keypoint in image 1 that b's point prefers
            f1.kp(c1[0] - 1.2, c1[1] + 1.0, k % 3, near(da, 0.125))
    return _sim3_set("sim3_exits", f1, f2, S12)


@functools.lru_cache(None)
def sim3_bounds():
    """the bound rows in both directions with s12 = 2, R12 = I, t12 = 0 and translated cameras: the pixel is exact"""
    f1, f2 = _Frame(K_DYADIC, BOUNDS_KITTI, 8600), _Frame(K_DYADIC, BOUNDS_KITTI, 8601)
    _bound_rows(f2, _holders(f1, f2, 100.0, 150.0, 3500), "sim3")
    _bound_rows(f1, _holders(f2, f1, 100.0, 150.0, 3600), "sim3")
    return _sim3_set("sim3_bounds", f1, f2, 2.0, identity=True)


_QUERY_KEYS = ("valid", "Xw", "normal", "mind", "maxd", "mp_desc", "angle", "crafted", "exact")


# ====================================================================================== shape sets
def _shape_frame(th, seed):
    """-> (_Frame, the first queries in the order the prefixes of 1, 7, 8 and 9 take them, the level-7 queries over the field)"""
    c = float(th) * float(SCALE[7]) / 16
    bounds = (0.0, 64 * c, 0.0, 48 * c)
    fr = _Frame(np.array([2.0 ** np.ceil(np.log2(40 * c))] * 2 + [32 * c, 24 * c], F32), bounds, seed)
    rng = fr.rng
    def rand_desc(n):
        d = rng.standard_normal((n, 128)).astype(F32)
        return d / np.linalg.norm(d, axis=1, keepdims=True)

    def target(i_desc, sigma=0.04):
        return perturbed_descriptors(i_desc[None], sigma, int(rng.integers(1 << 30)))[0]
    r1 = float(th) * float(SCALE[1])
    first, field_q = [], []
    # the clump: 100 keypoints in one cell
    cl = np.array([6.0 * c, 6.0 * c])
    dcl = rand_desc(100)
    for k in range(100):
        fr.kp(cl[0] + 0.3 * c * ((k % 10) / 10 - 0.45), cl[1] + 0.3 * c * ((k // 10) / 10 - 0.45), 1, dcl[k], taken=k % 9 == 0)
    # the lattice: 16 x 8 keypoints within 0.85 r1 of its centre, one more at 1.1 r1
    la = np.array([14.0 * c, 30.0 * c])
    dla = rand_desc(129)
    for k in range(128):
        fr.kp(la[0] + 0.85 * r1 * ((k % 16) / 7.5 - 1), la[1] + 0.85 * r1 * ((k // 16) / 3.5 - 1), 1, dla[k])
    fr.kp(la[0] + 1.1 * r1, la[1] + 0.1, 1, dla[128])
    # the field: 1400 keypoints over 28 x 26 cells, nine in ten at the two top octaves
    nf = 1400
    dfi = rand_desc(nf)
    fx_, fy_ = rng.uniform(34 * c, 62 * c, nf), rng.uniform(20 * c, 46 * c, nf)
    fo = np.where(rng.uniform(size=nf) < 0.9, rng.integers(6, 8, nf), rng.integers(0, 6, nf))
    for k in range(nf):
        fr.kp(fx_[k], fy_[k], int(fo[k]), dfi[k], taken=rng.uniform() < 0.1)
    # keypoints beside the borders and in two corners, and one alone
    edge = [(0.4 * c, 14 * c), (62.9 * c, 8 * c), (26 * c, 0.4 * c), (22 * c, 46.9 * c), (0.5 * c, 0.5 * c), (62.8 * c, 46.8 * c), (24 * c, 12 * c)]
    ded = rand_desc(len(edge))
    for k, (x, y) in enumerate(edge):
        fr.kp(x, y, 3, ded[k])
    off = np.array([0.21 * c, -0.17 * c])
    first.append(query(fr, np.array(edge[-1]) + off, 3, target(ded[-1]), "lone"))
    first.append(query(fr, la + 0.05, 1, target(dla[5]), "list128"))
    first.append(query(fr, la + 0.05, 2, target(dla[77]), "list129"))
    first.append(query(fr, cl + 0.02, 1, target(dcl[31]), "column_over_64"))
    first.append(query(fr, np.array([48 * c, 33 * c]), 8, target(dfi[np.nonzero(fo == 7)[0][0]]), "field"))
    for k in range(6):
        first.append(query(fr, np.array(edge[k]) + off * (1 if k % 2 else -1) + (0.6 * c if k in (0, 2, 4) else -0.6 * c), 3, target(ded[k]),
                           "clipped"))
    top = np.nonzero(fo == 7)[0]
    for k in range(8):
        i = top[1 + k]
        field_q.append(query(fr, np.array([(44 + k) * c + 0.13, (31 + 0.5 * k) * c + 0.07]), 8, target(dfi[i]), "field"))
    return fr, first, field_q


@functools.lru_cache(None)
def shapes(kind, n_first=None, tail=False):
    """kind's shape set: the first n_first queries (None: all of them and the field queries); tail: the field queries alone"""
    fr, first, field_q = _shape_frame(TH[kind], 8700)
    qs = field_q if tail else (first + field_q if n_first is None else first[:n_first])
    name = "%s_shapes_%s" % (kind, "tail" if tail else ("all" if n_first is None else n_first))
    kps, desc, taken = fr.arrays()
    if kind == "sim3":
        # keyframe 1 holds the queries' own keypoints, 1.5 px apart beside its upper border; the keypoint of the shape frame that
        # the reference finds for a query carries a point aimed back at it, so that the pair is mutual and match12 shows it
        f1 = _Frame(fr.K, fr.bounds, 8701)
        for k, q in enumerate(qs):
            f1.kp(2.0 + 1.5 * k, 3.0, 0, code(k), query=q)
        found = run_ref(_sim3_set(name, f1, fr, S12))["d12"]["match"]
        for k in np.nonzero(found >= 0)[0]:
            fr.rows[found[k]]["query"] = query(f1, np.array([2.3 + 1.5 * k, 3.2]), 0, near(code(k), 0.25))
        return _sim3_set(name, f1, fr, S12)
    T = translation()
    p = _pack(qs, _rigid_inverse(T), lambda n: n)
    s = dict(fn=kind, name=name, kps=kps, desc=desc, bounds=fr.bounds, T=T, K=fr.K, th=TH[kind], **p)
    if kind == "reloc":
        s.update(orb_dist=1.0, check_ori=True, occupied=taken.astype(np.uint8))
        s["angle"] = (s["angle"] + fr.rng.uniform(-100, 100, len(qs))).astype(F32)
    else:
        s.update(scale=1.0, matched_kp=np.where(taken, -2, -1).astype(np.int32))
    if n_first is None:                                    # a field keypoint within the tolerance of a window's edge: the query goes
        clear = run_ref(s)["margin"] > 2
        for k in _QUERY_KEYS:
            s[k] = s[k][clear]
    return s


@functools.lru_cache(None)
def fuse_grow():
    """2000 keypoints within 8 cells of the centre and 200 level-7 windows over all of them: 400000 candidates, more than the
    2^18 a fresh context has room for"""
    th = TH["fuse"]
    c = float(th) * float(SCALE[7]) / 16
    fr = _Frame(np.array([2.0 ** np.ceil(np.log2(40 * c))] * 2 + [32 * c, 24 * c], F32), (0.0, 64 * c, 0.0, 48 * c), 8800)
    rng = fr.rng
    d = rng.standard_normal((2000, 128)).astype(F32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x, y, o = rng.uniform(24 * c, 40 * c, 2000), rng.uniform(16 * c, 32 * c, 2000), rng.integers(6, 8, 2000)
    for k in range(2000):
        fr.kp(x[k], y[k], int(o[k]), d[k])
    qs = [query(fr, np.array([32 * c, 24 * c]) + rng.uniform(-3 * c, 3 * c, 2), 8, perturbed_descriptors(d[k][None], 0.04, 8801 + k)[0], "field")
          for k in np.nonzero(o == 7)[0][:200]]
    T = translation()
    kps, desc, _ = fr.arrays()
    return dict(fn="fuse", name="fuse_grow", kps=kps, desc=desc, bounds=fr.bounds, T=T, K=fr.K, th=th, scale=1.0,
                **_pack(qs, _rigid_inverse(T), lambda n: n))


# ====================================================================================== crowded sets
T_CROWD = pose_T((0.01, -0.02, 0.005), (0.4, -0.3, 1.5))


def _rescaled_frame(n, seed, bounds, width=None):
    """make_frame's keypoints inside a region `width` px wide around the centre of the image (None: the whole image)"""
    kps, desc = make_frame(n, seed)
    w = bounds[1] if width is None else width
    h = w * bounds[3] / bounds[1]
    kps["x"] = ((bounds[1] - w) / 2 + kps["x"] * F32(w / 1241.0)).astype(F32)
    kps["y"] = ((bounds[3] - h) / 2 + kps["y"] * F32(h / 376.0)).astype(F32)
    return kps, desc


@functools.lru_cache(None)
def crowded(kind, euroc=False):
    """600 keypoints in the middle of the image (a window holds a few), `per` map points aimed at each within 1.5 px, the level predicted at the keypoint's octave or one above;
    the points kept are the ones run_ref finds clear of every threshold"""
    K, bounds = (K_EUROC, BOUNDS_EUROC) if euroc else (K_KITTI, BOUNDS_KITTI)
    seed = dict(reloc=9100, scw=9200, fuse=9300)[kind]
    rng = np.random.default_rng(seed)
    n_kp, per = 600, (3 if kind in ("reloc", "scw") else 2)
    kps, desc = _rescaled_frame(n_kp, seed + 1, bounds, dict(reloc=600.0, scw=300.0, fuse=200.0)[kind])
    src = rng.permutation(np.repeat(np.arange(n_kp), per))
    n = len(src)
    uv = np.stack([kps["x"][src], kps["y"][src]], 1).astype(np.float64) + rng.uniform(-1.5, 1.5, (n, 2))
    uv[: n // 12] += 3000
    depth = rng.uniform(3, 60, n)
    Kd = K.astype(np.float64)
    pc = np.stack([(uv[:, 0] - Kd[2]) / Kd[0] * depth, (uv[:, 1] - Kd[3]) / Kd[1] * depth, depth], 1)
    pc[n // 12: n // 8] *= -1
    R = T_CROWD[:3, :3].astype(np.float64)
    inv = _rigid_inverse(T_CROWD)
    dist = np.linalg.norm(pc, axis=1)
    level = kps["octave"][src] + rng.integers(0, 2, n) + rng.uniform(-0.8, -0.2, n)
    maxd = (dist * 1.2 ** level).astype(F32)
    nrm = pc / dist[:, None] + rng.normal(0, 0.3, pc.shape)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    taken = rng.uniform(size=n_kp) < 0.1
    s = dict(fn=kind, name="%s_crowded%s" % (kind, "_euroc" if euroc else ""), kps=kps, desc=desc, bounds=bounds, T=T_CROWD, K=K,
             th=TH[kind], valid=(rng.uniform(size=n) < 0.95).astype(np.uint8), Xw=inv(pc).astype(F32), normal=(nrm @ R).astype(F32),
             mind=(maxd / SCALE[7]).astype(F32), maxd=maxd, mp_desc=perturbed_descriptors(desc[src], 0.04, seed + 2),
             angle=((kps["angle"][src] + rng.normal(0, 8, n)) % 360).astype(F32), crafted=np.full(n, ""), exact=np.zeros(n, bool))
    if kind == "reloc":
        s.update(orb_dist=1.0, check_ori=True, occupied=taken.astype(np.uint8))
    else:
        s.update(scale=2.5 if kind == "scw" else 0.37, matched_kp=np.where(taken, -2, -1).astype(np.int32))
    clear = run_ref(s)["margin"] > 2
    for k in _QUERY_KEYS:
        s[k] = s[k][clear]
    return s


@functools.lru_cache(None)
def sim3_crowded():
    """two keyframes of one scene whose maps differ by a similarity (EuRoC camera): 700 keypoints each, the second frame's in
    another order, 0.3 px of noise; points within the tolerances of a gate lose their flag"""
    rng = np.random.default_rng(9400)
    n, K, bounds = 700, K_EUROC, BOUNDS_EUROC
    Kd = K.astype(np.float64)
    T1, T2, R12, t12, w1, w2 = _sim3_transforms(S12)
    k1, d1 = _rescaled_frame(n, 9401, bounds, 400.0)
    depth = rng.uniform(4, 50, n)
    p1 = np.stack([(k1["x"] - Kd[2]) / Kd[0] * depth, (k1["y"] - Kd[3]) / Kd[1] * depth, depth], 1)
    s = float(S12)
    R12d, t12d = R12.astype(np.float64), t12.astype(np.float64)
    p2 = (p1 - t12d) @ R12d / s                              # p2 = (1 / s) R12^T (p1 - t12)
    uv2 = np.stack([Kd[0] * p2[:, 0] / p2[:, 2] + Kd[2], Kd[1] * p2[:, 1] / p2[:, 2] + Kd[3]], 1)
    vis = (p2[:, 2] > 0.5) & (uv2[:, 0] > 20) & (uv2[:, 0] < bounds[1] - 20) & (uv2[:, 1] > 20) & (uv2[:, 1] < bounds[3] - 20)
    perm = rng.permutation(n)
    k2 = k1[perm].copy()
    k2["x"] = (uv2[perm, 0] + rng.normal(0, 0.3, n)).astype(F32)
    k2["y"] = (uv2[perm, 1] + rng.normal(0, 0.3, n)).astype(F32)
    bad = ~vis[perm]
    k2["x"][bad] = rng.uniform(20, bounds[1] - 20, bad.sum()).astype(F32)
    k2["y"][bad] = rng.uniform(20, bounds[3] - 20, bad.sum()).astype(F32)
    d2 = perturbed_descriptors(d1[perm], 0.03, 9402)
    g1, g2 = rng.uniform(-0.8, -0.2, n), rng.uniform(-0.8, -0.2, n)
    maxd1 = (np.linalg.norm(p2, axis=1) * 1.2 ** (k1["octave"] + g1)).astype(F32)
    maxd2 = (np.linalg.norm(p1[perm], axis=1) * 1.2 ** (k2["octave"] + g2)).astype(F32)
    out = dict(fn="sim3", name="sim3_crowded", s12=s, R12=R12, t12=t12, T1=T1, T2=T2, K=K, th=TH["sim3"], kps1=k1, kps2=k2,
               desc1=d1, desc2=d2, bounds1=bounds, bounds2=bounds, has1=(rng.uniform(size=n) < 0.9).astype(np.uint8),
               has2=((rng.uniform(size=n) < 0.9) & ~bad).astype(np.uint8), Xw1=np.array([w1(p) for p in p2]).astype(F32),
               Xw2=np.array([w2(p) for p in p1[perm]]).astype(F32), maxd1=maxd1, mind1=(maxd1 / SCALE[7]).astype(F32), maxd2=maxd2,
               mind2=(maxd2 / SCALE[7]).astype(F32), mp_desc1=perturbed_descriptors(d1, 0.02, 9403), mp_desc2=perturbed_descriptors(d2, 0.02, 9404),
               crafted1=np.full(n, ""), crafted2=np.full(n, ""), exact1=np.zeros(n, bool), exact2=np.zeros(n, bool))
    r = run_ref(out)
    out["has1"] = (out["has1"] & (r["d12"]["margin"] > 2)).astype(np.uint8)
    out["has2"] = (out["has2"] & (r["d21"]["margin"] > 2)).astype(np.uint8)
    return out


# ====================================================================================== drivers
def _scw(s):
    return sim3_of(s["T"], s["scale"])


def with_scale(s, scale):
    """the same set seen through Scw = scale * Tcw.  The rows on a bound are exact at scale 1 alone (Rcw = sRcw * (1 / scw) is not
    the identity to the bit for other scales): the other scales go without them"""
    s = dict(s, scale=scale, name="%s@%g" % (s["name"], scale))
    if scale != 1.0:
        keep = ~s["exact"]
        for k in _QUERY_KEYS:
            s[k] = s[k][keep]
    return s


_FRAMES = {}


def _frame(kps, desc, bounds):
    key = (id(kps), id(desc))
    if key not in _FRAMES:
        _FRAMES[key] = (ref.Frame(kps, desc, bounds), kps, desc)          # (the arrays are kept alive: ids stay unique)
    return _FRAMES[key][0]


def run_ref(s, **mutant):
    fn = s["fn"]
    if fn == "sim3":
        return ref.search_by_sim3(_frame(s["kps1"], s["desc1"], s["bounds1"]), _frame(s["kps2"], s["desc2"], s["bounds2"]), s["has1"], s["has2"],
                                  s["Xw1"], s["Xw2"], s["mind1"], s["maxd1"], s["mind2"], s["maxd2"], s["mp_desc1"], s["mp_desc2"], s["T1"],
                                  s["T2"], s["s12"], s["R12"], s["t12"], s["K"], s["th"], **mutant)
    fr = _frame(s["kps"], s["desc"], s["bounds"])
    if fn == "reloc":
        return ref.search_by_projection_reloc(fr, s["valid"], s["Xw"], s["mind"], s["maxd"], s["mp_desc"], s["angle"], s["occupied"], s["T"],
                                              s["K"], s["th"], s["orb_dist"], s["check_ori"], **mutant)
    if fn == "scw":
        return ref.search_by_projection_scw(fr, _scw(s), s["valid"], s["Xw"], s["normal"], s["mind"], s["maxd"], s["mp_desc"], s["K"], s["th"],
                                            s["matched_kp"], **mutant)
    return ref.fuse_scw(fr, _scw(s), s["valid"], s["Xw"], s["normal"], s["mind"], s["maxd"], s["mp_desc"], s["K"], s["th"], **mutant)


def run_lib(lib, s, slots=(8, 9)):
    """lib: the oracle or the HIP context -> the call's outputs as a tuple"""
    hip = hasattr(lib, "frame_set")

    def frame(slot, kps, desc, bounds):
        if hip:
            lib.frame_set(slot, kps, desc, bounds)
            return slot
        return lib.frame(kps, desc, bounds)
    fn = s["fn"]
    if fn == "sim3":
        a, b = frame(slots[0], s["kps1"], s["desc1"], s["bounds1"]), frame(slots[1], s["kps2"], s["desc2"], s["bounds2"])
        args = (s["has1"], s["has2"], s["Xw1"], s["Xw2"], s["mind1"], s["maxd1"], s["mind2"], s["maxd2"], s["mp_desc1"], s["mp_desc2"], s["T1"],
                s["T2"], s["s12"], s["R12"], s["t12"], s["K"], s["th"])
        return lib.match_sim3(a, b, len(s["kps1"]), *args) if hip else lib.match_sim3(a, b, *args)
    f = frame(slots[0], s["kps"], s["desc"], s["bounds"])
    if fn == "reloc":
        args = (s["valid"], s["Xw"], s["mind"], s["maxd"], s["mp_desc"], s["angle"], s["occupied"], s["T"], s["K"], s["th"], s["orb_dist"],
                s["check_ori"])
        return lib.match_project_keyframe(f, len(s["kps"]), *args) if hip else lib.match_project_keyframe(f, *args)
    args = (_scw(s), s["valid"], s["Xw"], s["normal"], s["mind"], s["maxd"], s["mp_desc"], s["K"], s["th"])
    if fn == "scw":
        return lib.match_project_sim3(f, *args, s["matched_kp"])
    return lib.fuse_search_sim3(f, *args)


def outputs(s, r):
    """the reference's result in the shape of the call's outputs"""
    fn = s["fn"]
    if fn == "reloc":
        return r["match_cur"], r["n_matches"]
    if fn == "scw":
        return r["matched_kp"], r["n_matches"]
    if fn == "fuse":
        return r["best_idx"], r["best_dist"]
    return r["match12"], r["n_matches"]


def decided(s, r):
    """per query: decidable, or on a bound by construction"""
    if s["fn"] == "sim3":
        dec, ok21 = r["d12"]["decidable"] | s["exact1"], r["d21"]["decidable"] | s["exact2"]
        m = r["d12"]["match"]
        dec[m >= 0] &= ok21[m[m >= 0]]
        return dec
    return r["decidable"] | s["exact"]


def check(s, r, got):
    """the call's outputs equal the reference's on every decided element -> the number of elements compared"""
    fn, dec = s["fn"], decided(s, r)
    exp = outputs(s, r)
    if fn in ("reloc", "scw"):                               # claim-coupled: one undecided row may change every later one
        assert dec.all(), (s["name"], np.nonzero(~dec)[0][:10])
        np.testing.assert_array_equal(got[0], exp[0], err_msg=s["name"])
        assert got[1] == exp[1] == ((got[0] >= 0) & (True if fn == "reloc" else s["matched_kp"] == -1)).sum()
        if fn == "scw":
            keep = s["matched_kp"] != -1
            np.testing.assert_array_equal(got[0][keep], s["matched_kp"][keep])
        return int(dec.sum())
    if fn == "fuse":
        np.testing.assert_array_equal(np.asarray(got[0])[dec], exp[0][dec], err_msg=s["name"])
        m = dec & (exp[0] >= 0)
        np.testing.assert_array_equal(np.asarray(got[1])[m].view(np.int32), exp[1][m].view(np.int32), err_msg=s["name"])
        return int(dec.sum())
    np.testing.assert_array_equal(np.asarray(got[0])[dec], exp[0][dec], err_msg=s["name"])
    assert got[1] == (np.asarray(got[0]) >= 0).sum()
    if dec.all():
        assert got[1] == exp[1]
    return int(dec.sum())


def n_candidates(s, r):
    """what k_window_search writes for the call: the keypoints inside every query's window (behind the level gate where the area
    query has one)"""
    if s["fn"] == "sim3":
        return int(r["d12"]["n_list"].sum()), int(r["d21"]["n_list"].sum())
    return int(r["n_list"].sum())
