"""ctypes binding of libasdhip's C ABI (include/asd_slam.h).

Plumbing for tests and bench only -- the same entry points a C++ adapter in the reference's
catkin workspace would call.  There is no fallback: if the shared library
is missing or no HIP device is usable, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    # ASDHIP_LIB: tuning aid to A/B differently built libraries; the default is the in-tree build
    return os.environ.get("ASDHIP_LIB") or os.path.join(_HERE, "libasdhip.so")


class AsdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libasdhip error {code}: {msg}")
        self.code = code


class asd_config(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("scale_factor", C.c_float), ("n_levels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("max_width", C.c_int32),
                ("max_height", C.c_int32), ("max_patches", C.c_int32), ("device", C.c_int32)]


BANK_MAX_ROWS = 1 << 22   # ASD_BANK_MAX_ROWS (include/asd_slam.h): rows of the descriptor and attribute banks

KP_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("size", np.float32), ("angle", np.float32),
                     ("response", np.float32), ("octave", np.int32)])


class asd_feature_vector(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("node_id", C.c_void_p), ("start", C.c_void_p), ("idx", C.c_void_p)]


def make_fv(node_of_kp):
    """node id per keypoint (-1 = none) -> (struct, keep-alive arrays) in DBoW2::FeatureVector order"""
    node_of_kp = np.asarray(node_of_kp)
    ids = np.unique(node_of_kp[node_of_kp >= 0]).astype(np.int32)
    start = np.zeros(len(ids) + 1, np.int32)
    idx = []
    for k, nid in enumerate(ids):
        members = np.nonzero(node_of_kp == nid)[0]
        idx.append(members)
        start[k + 1] = start[k] + len(members)
    idx = (np.concatenate(idx) if idx else np.zeros(0)).astype(np.int32)
    fv = asd_feature_vector(len(ids), ids.ctypes.data, start.ctypes.data, idx.ctypes.data)
    return fv, (ids, start, idx)


class asd_kf_neighbor(C.Structure):
    _fields_ = [("slot", C.c_int32), ("has_mp", C.c_void_p), ("F12", C.c_float * 9), ("ex", C.c_float), ("ey", C.c_float),
                ("Tcw", C.c_float * 16), ("K", C.c_float * 4)]


class asd_fuse_call(C.Structure):
    _fields_ = [("slot_kf", C.c_int32), ("first", C.c_int32), ("n", C.c_int32), ("Tcw", C.c_float * 16), ("K", C.c_float * 4)]


class asd_track_frame_args(C.Structure):
    _fields_ = [("slot_cur", C.c_int32), ("slot_last", C.c_int32), ("has_mp", C.c_void_p), ("Xw_last", C.c_void_p), ("last_rows", C.c_void_p),
                ("last_cand", C.c_void_p), ("last_obs_positive", C.c_void_p), ("Tcw", C.c_void_p), ("th", C.c_float), ("check_orientation", C.c_int32),
                ("n_cand", C.c_int32), ("cand_rows", C.c_void_p), ("cand_obs_positive", C.c_void_p), ("viewing_cos_limit", C.c_float),
                ("th_local", C.c_float), ("nn_ratio", C.c_float), ("K", C.c_void_p), ("pose7", C.c_void_p), ("pose1", C.c_void_p),
                ("match1", C.c_void_p), ("n_matches1", C.c_void_p), ("outlier1", C.c_void_p), ("n_inliers1", C.c_void_p),
                ("match2", C.c_void_p), ("n_matches2", C.c_void_p), ("outlier2", C.c_void_p), ("n_inliers2", C.c_void_p)]


class asd_local_map_args(C.Structure):
    _fields_ = [("n_cur", C.c_int32), ("cur_rows", C.c_void_p), ("n_seen", C.c_int32), ("seen_rows", C.c_void_p), ("n_prev", C.c_int32),
                ("prev_kfs", C.c_void_p), ("max_kfs", C.c_int32), ("kf_capacity", C.c_int32), ("local_kfs", C.c_void_p),
                ("n_local_kfs", C.c_int32), ("ref_kf", C.c_int32), ("row_capacity", C.c_int32), ("local_rows", C.c_void_p),
                ("n_local", C.c_int32), ("search_capacity", C.c_int32), ("search_rows", C.c_void_p), ("n_search", C.c_int32)]


class asd_kf_culling_args(C.Structure):
    _fields_ = [("n_cand", C.c_int32), ("cand", C.c_void_p), ("cand_flags", C.c_void_p), ("apply", C.c_int32), ("decision", C.c_void_p),
                ("n_mps", C.c_void_p), ("n_redundant", C.c_void_p), ("bad_capacity", C.c_int32), ("bad_rows", C.c_void_p), ("n_bad", C.c_int32)]


class asd_normal_depth_args(C.Structure):
    _fields_ = [("n", C.c_int32), ("rows", C.c_void_p), ("ref_kf", C.c_void_p), ("Xw", C.c_void_p), ("normal", C.c_void_p),
                ("min_dist", C.c_void_p), ("max_dist", C.c_void_p), ("status", C.c_void_p)]


class asd_ba_graph_args(C.Structure):
    _fields_ = [("kf", C.c_int32), ("n_neigh", C.c_int32), ("neigh", C.c_void_p), ("kf_capacity", C.c_int32), ("local_kfs", C.c_void_p),
                ("n_local_kfs", C.c_int32), ("point_capacity", C.c_int32), ("local_rows", C.c_void_p), ("point_rank", C.c_void_p),
                ("n_points", C.c_int32), ("fixed_capacity", C.c_int32), ("fixed_kfs", C.c_void_p), ("n_fixed", C.c_int32),
                ("pose_capacity", C.c_int32), ("pose_kfs", C.c_void_p), ("pose_fixed", C.c_void_p), ("n_poses", C.c_int32),
                ("edge_capacity", C.c_int32), ("e_point", C.c_void_p), ("e_pose", C.c_void_p), ("e_kf", C.c_void_p), ("e_idx", C.c_void_p),
                ("e_octave", C.c_void_p), ("n_edges", C.c_int32), ("Xw", C.c_void_p)]


class asd_ba_apply_args(C.Structure):
    _fields_ = [("n_edges", C.c_int32), ("erase", C.c_void_p), ("apply", C.c_int32), ("n_erased", C.c_int32), ("bad_capacity", C.c_int32),
                ("bad_rows", C.c_void_p), ("n_bad", C.c_int32), ("n_points", C.c_int32), ("new_ref", C.c_void_p)]


class asd_fuse_apply_args(C.Structure):
    _fields_ = [("kf", C.c_int32), ("mode", C.c_int32), ("n", C.c_int32), ("cand", C.c_void_p), ("best_idx", C.c_void_p), ("apply", C.c_int32),
                ("action", C.c_void_p), ("other", C.c_void_p), ("obs_cand", C.c_void_p), ("obs_other", C.c_void_p), ("n_moved", C.c_void_p),
                ("n_dropped", C.c_void_p), ("n_fused", C.c_int32)]


class asd_ba_problem(C.Structure):
    _fields_ = [("n_poses", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32),
                ("poses", C.c_void_p), ("fixed", C.c_void_p), ("points", C.c_void_p),
                ("e_point", C.c_void_p), ("e_pose", C.c_void_p), ("e_obs", C.c_void_p), ("e_info", C.c_void_p),
                ("K", C.c_double * 4), ("its_first", C.c_int32), ("its_second", C.c_int32)]


class asd_ba_result(C.Structure):
    _fields_ = [("edge_chi2", C.c_void_p), ("edge_depth_pos", C.c_void_p), ("edge_outlier1", C.c_void_p),
                ("chi2_first", C.c_double), ("chi2_second", C.c_double),
                ("iters_first", C.c_int32), ("iters_second", C.c_int32)]


class asd_gba_problem(C.Structure):
    _fields_ = [("n_poses", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32),
                ("poses", C.c_void_p), ("fixed", C.c_void_p), ("points", C.c_void_p),
                ("e_point", C.c_void_p), ("e_pose", C.c_void_p), ("e_obs", C.c_void_p), ("e_info", C.c_void_p),
                ("K", C.c_double * 4), ("n_iterations", C.c_int32), ("robust", C.c_int32), ("stop", C.c_void_p)]


class asd_gba_result(C.Structure):
    _fields_ = [("edge_chi2", C.c_void_p), ("chi2", C.c_double), ("iterations", C.c_int32), ("trials", C.c_int32)]


class asd_essgraph_problem(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_edges", C.c_int32), ("sim3", C.c_void_p), ("fixed", C.c_void_p), ("e_i", C.c_void_p),
                ("e_j", C.c_void_p), ("e_meas", C.c_void_p), ("fix_scale", C.c_int32), ("n_iterations", C.c_int32),
                ("Tcw_out", C.c_void_p), ("n_mp", C.c_int32), ("mp_ref", C.c_void_p), ("mp_Xw", C.c_void_p)]


class asd_essgraph_result(C.Structure):
    _fields_ = [("edge_chi2", C.c_void_p), ("chi2", C.c_double), ("iterations", C.c_int32), ("trials", C.c_int32)]


class asd_sim3_ransac_problem(C.Structure):
    _fields_ = [("n", C.c_int32), ("X1c", C.c_void_p), ("X2c", C.c_void_p), ("max_err1", C.c_void_p), ("max_err2", C.c_void_p),
                ("K1", C.c_float * 4), ("K2", C.c_float * 4), ("fix_scale", C.c_int32), ("min_inliers", C.c_int32), ("n_iter", C.c_int32),
                ("draws", C.c_void_p), ("best_inliers", C.c_int32), ("best_updated", C.c_int32), ("R12", C.c_float * 9), ("t12", C.c_float * 3),
                ("s12", C.c_float), ("T12", C.c_float * 16), ("found", C.c_int32), ("iterations_done", C.c_int32), ("n_inliers", C.c_int32),
                ("inliers", C.c_void_p)]


class asd_sim3_ransac_debug(C.Structure):
    _fields_ = [("idx", C.c_int32 * 3), ("count", C.c_int32), ("T12", C.c_float * 16), ("T21", C.c_float * 16), ("s", C.c_float),
                ("q", C.c_double * 4)]


class asd_pnp_ransac_problem(C.Structure):
    _fields_ = [("n", C.c_int32), ("P3Dw", C.c_void_p), ("P2D", C.c_void_p), ("max_err", C.c_void_p), ("K", C.c_float * 4),
                ("min_inliers", C.c_int32), ("n_iter", C.c_int32), ("draws", C.c_void_p), ("best_inliers", C.c_int32),
                ("best_updated", C.c_int32), ("best_Tcw", C.c_float * 16), ("best_mask", C.c_void_p), ("found", C.c_int32),
                ("iterations_done", C.c_int32), ("n_inliers", C.c_int32), ("Tcw", C.c_float * 16), ("inliers", C.c_void_p)]


class asd_pnp_ransac_debug(C.Structure):
    _fields_ = [("idx", C.c_int32 * 4), ("count", C.c_int32), ("n_refines", C.c_int32), ("N", C.c_int32), ("hypothesis", C.c_int32),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("cws", C.c_double * 12), ("v", C.c_double * 48), ("eig", C.c_double * 4),
                ("rep_errors", C.c_double * 3), ("betas", C.c_double * 4)]


class asd_initializer_problem(C.Structure):
    _fields_ = [("n1", C.c_int32), ("keys1", C.c_void_p), ("n2", C.c_int32), ("keys2", C.c_void_p), ("matches12", C.c_void_p),
                ("K", C.c_float * 4), ("sigma", C.c_float), ("n_iter", C.c_int32), ("draws", C.c_void_p), ("min_parallax", C.c_float),
                ("min_triangulated", C.c_int32), ("n_matches", C.c_int32), ("SH", C.c_float), ("SF", C.c_float), ("model", C.c_int32),
                ("ok", C.c_int32), ("R21", C.c_float * 9), ("t21", C.c_float * 3), ("P3D", C.c_void_p), ("triangulated", C.c_void_p),
                ("H21", C.c_float * 9), ("F21", C.c_float * 9), ("inliers_H", C.c_void_p), ("inliers_F", C.c_void_p)]


class asd_initializer_debug(C.Structure):
    _fields_ = [("idx", C.c_int32 * 8), ("nullv", C.c_double * 9), ("U", C.c_double * 9), ("w", C.c_double * 3), ("Vt", C.c_double * 9),
                ("M1", C.c_float * 9), ("M2", C.c_float * 9), ("score", C.c_float), ("best_H", C.c_int32), ("best_F", C.c_int32),
                ("n_inliers", C.c_int32), ("n_hyp", C.c_int32), ("winner", C.c_int32), ("second_good", C.c_int32),
                ("R", C.c_float * 72), ("t", C.c_float * 24), ("parallax", C.c_float * 8), ("cos_sel", C.c_float * 8),
                ("n_good", C.c_int32 * 8), ("mask", C.c_void_p), ("points", C.c_void_p), ("flags", C.c_void_p)]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def load_library():
    path = lib_path()
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    return C.CDLL(path)


def undistort_map(K, dist, w, h):
    """asd_undistort_map: the map pair cv::undistort builds (host only, no context) -> (xy int16 [h, w, 2], frac uint16 [h, w]).
    K = (fx, fy, cx, cy), dist = (k1, k2, p1, p2) or None, both passed as float32 like the reference's CV_32F mK / mDistCoef."""
    lib = load_library()
    Kf = _c(K, np.float32)
    df = None if dist is None else _c(dist, np.float32)
    xy = np.empty((h, w, 2), np.int16)
    frac = np.empty((h, w), np.uint16)
    rc = lib.asd_undistort_map(_p(Kf), _p(df), int(w), int(h), _p(xy), _p(frac))
    if rc != 0:
        raise AsdError(rc, "asd_undistort_map: invalid arguments")
    return xy, frac


def bow_score(scoring, v1, v2):
    """asd_bow_score: TemplatedVocabulary::score(v1, v2) for scoring 0 L1 / 1 L2 / 5 DOT_PRODUCT (host only, no context) -> float.
    v1, v2 = (word ids strictly ascending, values)."""
    lib = load_library()
    lib.asd_last_error.restype = C.c_char_p
    i1, x1, i2, x2 = _c(v1[0], np.int32), _c(v1[1], np.float64), _c(v2[0], np.int32), _c(v2[1], np.float64)
    out = C.c_double(0.0)
    rc = lib.asd_bow_score(int(scoring), len(i1), _p(i1), _p(x1), len(i2), _p(i2), _p(x2), C.byref(out))
    if rc != 0:
        raise AsdError(rc, lib.asd_last_error(None).decode())
    return out.value


def sim3_ransac_max_iterations(n, probability, min_inliers, max_iterations):
    """asd_sim3_ransac_max_iterations: Sim3Solver::SetRansacParameters' mRansacMaxIts (Sim3Solver.cc:114-138; host only, no context)"""
    lib = load_library()
    lib.asd_sim3_ransac_max_iterations.restype = C.c_int32
    return int(lib.asd_sim3_ransac_max_iterations(C.c_int32(n), C.c_double(probability), C.c_int32(min_inliers), C.c_int32(max_iterations)))


def pnp_ransac_parameters(n, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """asd_pnp_ransac_parameters: PnPsolver::SetRansacParameters (PnPsolver.cc:121-152; host only, no context) ->
    (mRansacMinInliers, mRansacMaxIts)"""
    lib = load_library()
    a, b = C.c_int32(0), C.c_int32(0)
    rc = lib.asd_pnp_ransac_parameters(C.c_int32(n), C.c_double(probability), C.c_int32(min_inliers), C.c_int32(max_iterations),
                                       C.c_int32(min_set), C.c_float(epsilon), C.byref(a), C.byref(b))
    if rc != 0:
        raise AsdError(rc, "asd_pnp_ransac_parameters: invalid arguments")
    return int(a.value), int(b.value)


def initializer_normalize(keys):
    """asd_initializer_normalize: Initializer::Normalize (Initializer.cc:791-837; host only, no context) over ALL keys [n][2] ->
    (vNormalizedPoints [n][2] f32, T [3][3] f32)"""
    lib = load_library()
    k = _c(keys, np.float32).reshape(-1, 2)
    pts = np.empty_like(k)
    T = np.empty(9, np.float32)
    rc = lib.asd_initializer_normalize(C.c_int32(len(k)), _p(k), _p(pts), _p(T))
    if rc != 0:
        raise AsdError(rc, "asd_initializer_normalize: invalid arguments")
    return pts, T.reshape(3, 3)


def normal_and_depth_point(Ow, ref, Pos, scale_level, scale_top):
    """asd_normal_and_depth_point: the rule of asd_update_normal_and_depth for one point (host only, no context).  Ow [n_obs][3] = the
    observers' centres in walk order, ref = the reference keyframe's index among them -> (normal [3] f32, min_dist, max_dist as np.float32)"""
    lib = load_library()
    Ow, Pos = _c(Ow, np.float32).reshape(-1, 3), _c(Pos, np.float32)
    normal = np.empty(3, np.float32)
    mn, mx = C.c_float(0.0), C.c_float(0.0)
    rc = lib.asd_normal_and_depth_point(C.c_int32(len(Ow)), _p(Ow), C.c_int32(ref), _p(Pos), C.c_float(scale_level), C.c_float(scale_top), _p(normal),
                                        C.byref(mn), C.byref(mx))
    if rc != 0:
        raise AsdError(rc, "asd_normal_and_depth_point: invalid arguments")
    return normal, np.float32(mn.value), np.float32(mx.value)


# asd_debug_prim: op -> (name, doubles in, doubles out), in the order of the enum in include/asd_slam.h
PRIM_OPS = [("asd_rsqrt", 1, 1), ("quat_normalize", 4, 4), ("quat_rotate", 7, 3), ("pose_map", 10, 3), ("pose_oplus", 13, 7),
            ("rot_to_quat_eigen", 9, 4), ("huber", 2, 2), ("jac_pose", 5, 12), ("s3_exp", 7, 8), ("s3_exp_eigen", 7, 8), ("s3_log", 8, 7),
            ("s3_mul", 16, 8), ("s3_mul_eigen", 16, 8), ("s3_inverse", 8, 8), ("s3_map", 11, 3), ("s3_oplus", 16, 8),
            ("s3_oplus_eigen", 16, 8), ("s3_quat_of_rot", 9, 4), ("s3_quat_of_rot_eigen", 9, 4), ("s3_rot_of_quat", 8, 9),
            ("s3_lu_solve3", 12, 3), ("s3_edge_error", 24, 7), ("s3_project_error", 17, 2), ("s3_chi2", 3, 1), ("s3_solve7", 57, 8)]
PRIM_OP = {name: k for k, (name, _i, _o) in enumerate(PRIM_OPS)}
PRIM_SE3_OPS = 8   # ops below this exist in the contracted build too (fused=True)


def debug_prim(op, x, host=False, fused=False, ctx=None):
    """asd_debug_prim: one primitive of csrc/se3.h / csrc/sim3_math.h per row of x [n, width in] -> [n, width out] f64.  op: a name
    of PRIM_OPS or its number.  host: through the same header functions on the host (needs no context and no device); fused: the
    instantiation built with contraction allowed, as ba.o and gba.o (the se3.h ops only)."""
    k = PRIM_OP[op] if isinstance(op, str) else int(op)
    _name, w_in, w_out = PRIM_OPS[k]
    x = _c(x, np.float64).reshape(-1, w_in)
    out = np.full((len(x), w_out), np.nan)
    lib = ctx.lib if ctx is not None else load_library()
    lib.asd_debug_prim.restype = C.c_int32
    lib.asd_debug_prim.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    rc = lib.asd_debug_prim(ctx.ctx if ctx is not None else None, k, (1 if host else 0) | (2 if fused else 0), len(x), _p(x), _p(out))
    if rc != 0:
        raise AsdError(rc, ctx.last_error() if ctx is not None else "asd_debug_prim: invalid arguments")
    return out


class AsdHip:
    """One asd_ctx (= one HIP device + stream)."""

    def __init__(self, n_features=2000, scale_factor=1.2, n_levels=8, ini_th=20, min_th=7,
                 max_width=1241, max_height=376, max_patches=None, device=0):
        self.lib = load_library()
        L = self.lib
        L.asd_last_error.restype = C.c_char_p
        L.asd_version.restype = C.c_char_p
        L.asd_ctx_stream.restype = C.c_void_p
        self.cfg = asd_config(n_features, scale_factor, n_levels, ini_th, min_th, max_width, max_height,
                              max_patches if max_patches is not None else 2 * n_features, device)
        self.ctx = C.c_void_p()
        rc = L.asd_ctx_create(C.byref(self.cfg), C.byref(self.ctx))
        if rc != 0:
            raise AsdError(rc, "asd_ctx_create failed (no usable HIP device? there is no CPU fallback)")
        self.n_levels = n_levels

    def close(self):
        if getattr(self, "ctx", None) is not None and self.ctx:
            self.lib.asd_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise AsdError(rc, self.lib.asd_last_error(self.ctx).decode())

    def last_error(self):
        return self.lib.asd_last_error(self.ctx).decode()

    def calibration_note(self):
        self.lib.asd_calibration_note.restype = C.c_char_p
        return self.lib.asd_calibration_note(self.ctx).decode()

    # ---- tables
    def scale_tables(self):
        n = self.n_levels
        s, i, g, ig = (np.zeros(n, np.float32) for _ in range(4))
        f = np.zeros(n, np.int32)
        self._chk(self.lib.asd_get_scale_tables(self.ctx, _p(s), _p(i), _p(g), _p(ig), _p(f)))
        return dict(scale=s, inv_scale=i, sigma2=g, inv_sigma2=ig, features_per_level=f)

    # ---- ASDNet
    def load_weights(self, layers, eps=1e-5):
        ws = [_c(w, np.float32) for w, _, _ in layers]
        ms = [_c(m, np.float32) for _, m, _ in layers]
        vs = [_c(v, np.float32) for _, _, v in layers]
        arr = lambda xs: (C.c_void_p * 7)(*[x.ctypes.data for x in xs])
        self._keep = (ws, ms, vs)
        self._chk(self.lib.asd_load_weights(self.ctx, arr(ws), arr(ms), arr(vs), C.c_float(eps)))

    def describe(self, patches):
        patches = _c(patches, np.uint8).reshape(-1, 32, 32)
        n = patches.shape[0]
        out = np.empty((n, 128), np.float32)
        self._chk(self.lib.asd_describe(self.ctx, _p(patches), n, _p(out)))
        return out

    # ---- device utilities
    def device_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.lib.asd_device_alloc(self.ctx, C.c_uint64(nbytes), C.byref(p)))
        return p

    def host_alloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.lib.asd_host_alloc(self.ctx, C.c_uint64(nbytes), C.byref(p)))
        return p

    def device_free(self, p):
        self._chk(self.lib.asd_device_free(self.ctx, p))

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self.lib.asd_memcpy_h2d(self.ctx, dptr, _p(arr), C.c_uint64(arr.nbytes)))

    def d2h(self, arr, dptr):
        self._chk(self.lib.asd_memcpy_d2h(self.ctx, _p(arr), dptr, C.c_uint64(arr.nbytes)))

    def sync(self):
        self._chk(self.lib.asd_sync(self.ctx))

    def describe_timed(self, d_patches, n, d_desc, reps):
        ms = C.c_float()
        self._chk(self.lib.asd_describe_timed(self.ctx, d_patches, n, d_desc, reps, C.byref(ms)))
        return ms.value

    def debug_act6(self, n):
        """test aid: conv6's output of the most recent forward, first n patches, f32 [n, 64, 128]"""
        out = np.empty((n, 64, 128), np.float32)
        self.lib.asd_debug_act6.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self._chk(self.lib.asd_debug_act6(self.ctx, n, _p(out)))
        return out

    def describe_device(self, d_patches, n, d_desc):
        self._chk(self.lib.asd_describe_device(self.ctx, d_patches, n, d_desc))

    def last_stage_ms(self, stage):
        ms = C.c_float()
        self._chk(self.lib.asd_last_stage_ms(self.ctx, stage.encode(), C.byref(ms)))
        return ms.value

    # ---- extractor
    def extract(self, image, n_features_override=0):
        image = np.asarray(image, np.uint8)
        if image.strides[1] != 1 or image.strides[0] < image.shape[1]:   # rows of adjacent bytes with any stride >= width go as they are
            image = _c(image, np.uint8)
        h, w = image.shape
        cap = self.cfg.max_patches
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.empty((cap, 128), np.float32)
        n = C.c_int32()
        self._chk(self.lib.asd_extract(self.ctx, _p(image), w, h, image.strides[0], n_features_override,
                                       _p(kps), _p(desc), C.byref(n)))
        return kps[:n.value].copy(), desc[:n.value].copy()

    def extract_device(self, d_image, w, h, stride, n_features_override=0):
        cap = self.cfg.max_patches
        if not hasattr(self, "_kps_buf"):
            self._kps_buf = np.zeros(cap, KP_DTYPE)
            self._desc_buf = np.empty((cap, 128), np.float32)
        n = C.c_int32()
        self._chk(self.lib.asd_extract_device(self.ctx, d_image, w, h, stride, n_features_override,
                                              _p(self._kps_buf), _p(self._desc_buf), C.byref(n)))
        return self._kps_buf[:n.value], self._desc_buf[:n.value]

    def extract_submit(self, image, w, h, stride, device_resident=True, n_features_override=0):
        self._chk(self.lib.asd_extract_submit(self.ctx, image, int(device_resident), w, h, stride, n_features_override))

    def extract_wait(self, view=False):
        """view=True: zero-copy numpy views of the library's result buffers (valid for two further submissions)"""
        n = C.c_int32()
        if view:
            pk, pd = C.c_void_p(), C.c_void_p()
            self._chk(self.lib.asd_extract_wait_view(self.ctx, C.byref(pk), C.byref(pd), C.byref(n)))
            if n.value == 0:
                return np.zeros(0, KP_DTYPE), np.zeros((0, 128), np.float32)
            kb = (C.c_char * (n.value * KP_DTYPE.itemsize)).from_address(pk.value)
            db = (C.c_float * (n.value * 128)).from_address(pd.value)
            return np.frombuffer(kb, dtype=KP_DTYPE, count=n.value), np.frombuffer(db, dtype=np.float32).reshape(n.value, 128)
        cap = self.cfg.max_patches
        if not hasattr(self, "_kps_buf"):
            self._kps_buf = np.zeros(cap, KP_DTYPE)
            self._desc_buf = np.empty((cap, 128), np.float32)
        self._chk(self.lib.asd_extract_wait(self.ctx, _p(self._kps_buf), _p(self._desc_buf), C.byref(n)))
        return self._kps_buf[:n.value], self._desc_buf[:n.value]

    def extract_last_view(self):
        self.lib.asd_extract_last_view.restype = C.c_uint64
        return int(self.lib.asd_extract_last_view(self.ctx))

    def extract_view_valid(self, view_id):
        self.lib.asd_extract_view_valid.restype = C.c_int32
        return bool(self.lib.asd_extract_view_valid(self.ctx, C.c_uint64(view_id)))

    def extract_hold(self, on=True):
        """asd_extract_hold: no further ASDNet forward of the read-ahead extractor is enqueued while on (a wait on a held submission ends it)"""
        self._chk(self.lib.asd_extract_hold(self.ctx, int(on)))

    def set_undistortion(self, K, dist, w, h):
        """asd_set_undistortion: every extraction from now on runs on cv::undistort(image, K, dist); dist None / zeros clears it"""
        Kf = None if K is None else _c(K, np.float32)
        df = None if dist is None else _c(dist, np.float32)
        self._chk(self.lib.asd_set_undistortion(self.ctx, _p(Kf), _p(df), int(w), int(h)))

    def undistort(self, image, device_resident=False, w=None, h=None, stride=None):
        """asd_undistort on the context's map: a host array (or, device_resident=True, a device pointer with w, h, stride) -> u8 [h, w]"""
        if device_resident:
            src = image
        else:
            image = np.asarray(image)
            assert image.dtype == np.uint8 and image.ndim == 2 and image.strides[1] == 1
            h, w = image.shape
            stride = image.strides[0]
            src = C.c_void_p(image.ctypes.data)
        out = np.empty((h, w), np.uint8)
        self._chk(self.lib.asd_undistort(self.ctx, src, int(device_resident), int(w), int(h), int(stride), _p(out), int(w)))
        return out

    def profile_enable(self, on=True):
        self._chk(self.lib.asd_profile_enable(self.ctx, int(on)))

    def profile_get(self, layer):
        ms, calls, patches = C.c_double(), C.c_int32(), C.c_int64()
        self._chk(self.lib.asd_profile_get(self.ctx, layer, C.byref(ms), C.byref(calls), C.byref(patches)))
        return ms.value, calls.value, patches.value

    def asdnet_split_mask(self):
        """Bit l = conv(l+2) runs on the split-operand kernel; 0 = every layer on the f32 MFMA kernels."""
        self.lib.asd_asdnet_split_mask.restype = C.c_int32
        return int(self.lib.asd_asdnet_split_mask(self.ctx))

    def asdnet_pieces(self):
        """2 = operands as two fp16 terms, three products (default); 3 = three bf16 terms, six products (ASD_ASDNET_MATH=bf16x3)."""
        self.lib.asd_asdnet_pieces.restype = C.c_int32
        return int(self.lib.asd_asdnet_pieces(self.ctx))

    def level_size(self, level):
        w, h = C.c_int32(), C.c_int32()
        self._chk(self.lib.asd_get_level_size(self.ctx, level, C.byref(w), C.byref(h)))
        return w.value, h.value

    def level_image(self, level, blurred=False):
        w, h = self.level_size(level)
        out = np.empty((h, w), np.uint8)
        self._chk(self.lib.asd_get_level_image(self.ctx, level, int(blurred), _p(out)))
        return out

    def raw_corners(self, level, cap=200000):
        x, y, r = (np.empty(cap, np.float32) for _ in range(3))
        n = C.c_int32()
        self._chk(self.lib.asd_get_raw_corners(self.ctx, level, cap, _p(x), _p(y), _p(r), C.byref(n)))
        return x[:n.value].copy(), y[:n.value].copy(), r[:n.value].copy()

    def patches(self):
        """asd_get_patches: the 32x32 patches of the last synchronous extraction, u8 [n, 32, 32] in keypoint order"""
        cap = self.cfg.max_patches
        out = np.empty((cap, 32, 32), np.uint8)
        n = C.c_int32()
        self._chk(self.lib.asd_get_patches(self.ctx, cap, _p(out), C.byref(n)))
        return out[:n.value].copy()

    # ---- frames / matchers
    def frame_set(self, slot, kps, desc, bounds):
        kps = _c(kps, KP_DTYPE)
        d = None if desc is None else _c(desc, np.float32)
        self._chk(self.lib.asd_frame_set(self.ctx, slot, _p(kps), _p(d), len(kps), C.c_float(bounds[0]),
                                         C.c_float(bounds[1]), C.c_float(bounds[2]), C.c_float(bounds[3])))

    def frame_set_from_ctx(self, slot, kps, bounds, src):
        """asd_frame_set_from_ctx: asd_frame_set(desc == NULL) with the descriptors of `src`'s last extraction (the right frame of a stereo pair)"""
        kps = _c(kps, KP_DTYPE)
        self._chk(self.lib.asd_frame_set_from_ctx(self.ctx, slot, _p(kps), len(kps), C.c_float(bounds[0]), C.c_float(bounds[1]),
                                                  C.c_float(bounds[2]), C.c_float(bounds[3]), src.ctx))

    def extract_keep_pyramid(self, on=True):
        """asd_extract_keep_pyramid: every submission keeps its own copy of its pyramid for asd_stereo_match"""
        self._chk(self.lib.asd_extract_keep_pyramid(self.ctx, int(on)))

    def features_in_area(self, slot, x, y, r, min_level=-1, max_level=-1, cap=8192):
        out = np.empty(cap, np.int32)
        n = C.c_int32()
        self._chk(self.lib.asd_frame_features_in_area(self.ctx, slot, C.c_float(x), C.c_float(y), C.c_float(r),
                                                      min_level, max_level, cap, _p(out), C.byref(n)))
        return out[:n.value].copy()

    def dist_matrix(self, a, b):
        a, b = _c(a, np.float32), _c(b, np.float32)
        out = np.empty((a.shape[0], b.shape[0]), np.float32)
        self._chk(self.lib.asd_dist_matrix(self.ctx, _p(a), a.shape[0], _p(b), b.shape[0], _p(out)))
        return out

    def distinctive_descriptor(self, desc):
        desc = _c(desc, np.float32)
        best = C.c_int32()
        self._chk(self.lib.asd_distinctive_descriptor(self.ctx, _p(desc), desc.shape[0], C.byref(best)))
        return best.value

    def match_project_frame(self, slot_cur, slot_last, n_cur, has_mp, Xw, mp_desc, Tcw, K, th, check_ori=True, obs_positive=None):
        has_mp, Xw, mp_desc = _c(has_mp, np.uint8), _c(Xw, np.float32), _c(mp_desc, np.float32)
        Tcw, K = _c(Tcw, np.float32), _c(K, np.float32)
        out = np.empty(n_cur, np.int32)
        n = C.c_int32()
        self._chk(self.lib.asd_match_project_frame(self.ctx, slot_cur, slot_last, _p(has_mp), _p(Xw), _p(mp_desc),
                                                   _p(Tcw), _p(K), C.c_float(th), int(check_ori), _p(out),
                                                   C.byref(n), _p(None if obs_positive is None else _c(obs_positive, np.uint8))))
        return out, n.value

    def match_project_points(self, slot_cur, n_cur, in_view, proj, level, view_cos, desc, occupied, th, nn_ratio, obs_positive=None):
        in_view, proj, level = _c(in_view, np.uint8), _c(proj, np.float32), _c(level, np.int32)
        view_cos, desc, occupied = _c(view_cos, np.float32), _c(desc, np.float32), _c(occupied, np.uint8)
        out = np.empty(n_cur, np.int32)
        n = C.c_int32()
        self._chk(self.lib.asd_match_project_points(self.ctx, slot_cur, len(in_view), _p(in_view), _p(proj),
                                                    _p(level), _p(view_cos), _p(desc), _p(occupied), C.c_float(th),
                                                    C.c_float(nn_ratio), _p(out), C.byref(n),
                                                    _p(None if obs_positive is None else _c(obs_positive, np.uint8))))
        return out, n.value

    # ---- fused tracking chains (search + claim replay + PoseOptimization, one synchronisation)
    def track_motion_model(self, slot_cur, slot_last, n_cur, has_mp, Xw, mp_desc_or_rows, Tcw, K, th, pose7, check_ori=True, obs_positive=None, split=False):
        """mp_desc_or_rows: float [n][128] descriptors or int32 bank rows.  -> (match_cur, n_matches, pose7, outlier, n_inliers);
        split=True: asd_track_async + the call (returns None once the work is enqueued), track_finish() returns the tuple"""
        has_mp, Xw, Tcw, K = _c(has_mp, np.uint8), _c(Xw, np.float32), _c(Tcw, np.float32), _c(K, np.float32)
        d = np.asarray(mp_desc_or_rows)
        bank = d.dtype.kind in "iu"
        d = _c(d, np.int32 if bank else np.float32)
        match, outl = np.empty(n_cur, np.int32), np.empty(max(n_cur, 1), np.uint8)
        pose = _c(pose7, np.float64).copy()
        n, ninl = C.c_int32(), C.c_int32()
        fn = self.lib.asd_track_motion_model_bank if bank else self.lib.asd_track_motion_model
        if split:
            self._chk(self.lib.asd_track_async(self.ctx))
        self._chk(fn(self.ctx, slot_cur, slot_last, _p(has_mp), _p(Xw), _p(d), _p(Tcw), _p(K), C.c_float(th), int(check_ori),
                     _p(None if obs_positive is None else _c(obs_positive, np.uint8)), _p(pose), _p(match), C.byref(n), _p(outl), C.byref(ninl)))
        if split:
            self._track_job = (match, n, pose, outl, ninl, n_cur)   # the library writes these at track_finish
            return None
        return match, n.value, pose, outl[:n_cur], ninl.value

    def track_local_map(self, slot_cur, n_cur, in_view, proj, level, view_cos, desc_or_rows, mp_Xw, occupied, cur_Xw, th, nn_ratio, K, pose7,
                        obs_positive=None, split=False):
        in_view, proj, level = _c(in_view, np.uint8), _c(proj, np.float32), _c(level, np.int32)
        view_cos, mp_Xw, occupied, cur_Xw, K = _c(view_cos, np.float32), _c(mp_Xw, np.float32), _c(occupied, np.uint8), _c(cur_Xw, np.float32), _c(K, np.float32)
        d = np.asarray(desc_or_rows)
        bank = d.dtype.kind in "iu"
        d = _c(d, np.int32 if bank else np.float32)
        match, outl = np.empty(n_cur, np.int32), np.empty(max(n_cur, 1), np.uint8)
        pose = _c(pose7, np.float64).copy()
        n, ninl = C.c_int32(), C.c_int32()
        fn = self.lib.asd_track_local_map_bank if bank else self.lib.asd_track_local_map
        if split:
            self._chk(self.lib.asd_track_async(self.ctx))
        self._chk(fn(self.ctx, slot_cur, len(in_view), _p(in_view), _p(proj), _p(level), _p(view_cos), _p(d), _p(mp_Xw), _p(occupied), _p(cur_Xw),
                     C.c_float(th), C.c_float(nn_ratio), _p(None if obs_positive is None else _c(obs_positive, np.uint8)), _p(K), _p(pose),
                     _p(match), C.byref(n), _p(outl), C.byref(ninl)))
        if split:
            self._track_job = (match, n, pose, outl, ninl, n_cur)   # the library writes these at track_finish
            return None
        return match, n.value, pose, outl[:n_cur], ninl.value

    def track_local_points(self, slot_cur, n_cur, Xw, normal, min_dist, max_dist, desc_or_rows, Tcw, K, occupied, cur_Xw, th, nn_ratio, pose7,
                           cos_limit=0.5, obs_positive=None, split=False):
        """frustum test + windows + search + claims + PoseOptimization in one submission"""
        Xw, normal, min_dist, max_dist = (_c(a, np.float32) for a in (Xw, normal, min_dist, max_dist))
        Tcw, K, occupied, cur_Xw = _c(Tcw, np.float32), _c(K, np.float32), _c(occupied, np.uint8), _c(cur_Xw, np.float32)
        d = np.asarray(desc_or_rows)
        bank = d.dtype.kind in "iu"
        d = _c(d, np.int32 if bank else np.float32)
        match, outl = np.empty(n_cur, np.int32), np.empty(max(n_cur, 1), np.uint8)
        pose = _c(pose7, np.float64).copy()
        n, ninl = C.c_int32(), C.c_int32()
        fn = self.lib.asd_track_local_points_bank if bank else self.lib.asd_track_local_points
        if split:
            self._chk(self.lib.asd_track_async(self.ctx))
        self._chk(fn(self.ctx, slot_cur, len(min_dist), _p(Xw), _p(normal), _p(min_dist), _p(max_dist), _p(d), _p(Tcw), _p(K), C.c_float(cos_limit),
                     _p(occupied), _p(cur_Xw), C.c_float(th), C.c_float(nn_ratio), _p(None if obs_positive is None else _c(obs_positive, np.uint8)),
                     _p(pose), _p(match), C.byref(n), _p(outl), C.byref(ninl)))
        if split:
            self._track_job = (match, n, pose, outl, ninl, n_cur)   # the library writes these at track_finish
            return None
        return match, n.value, pose, outl[:n_cur], ninl.value

    def track_local_points_rows(self, slot_cur, n_cur, rows, Tcw, K, occupied, cur_Xw, th, nn_ratio, pose7, cos_limit=0.5, obs_positive=None, split=False):
        """asd_track_local_points_rows: the map points by row of the descriptor + attribute banks"""
        rows = _c(rows, np.int32)
        Tcw, K, occupied, cur_Xw = _c(Tcw, np.float32), _c(K, np.float32), _c(occupied, np.uint8), _c(cur_Xw, np.float32)
        match, outl = np.empty(n_cur, np.int32), np.empty(max(n_cur, 1), np.uint8)
        pose = _c(pose7, np.float64).copy()
        n, ninl = C.c_int32(), C.c_int32()
        if split:
            self._chk(self.lib.asd_track_async(self.ctx))
        self._chk(self.lib.asd_track_local_points_rows(self.ctx, slot_cur, len(rows), _p(rows), _p(Tcw), _p(K), C.c_float(cos_limit), _p(occupied), _p(cur_Xw),
                                                       C.c_float(th), C.c_float(nn_ratio), _p(None if obs_positive is None else _c(obs_positive, np.uint8)),
                                                       _p(pose), _p(match), C.byref(n), _p(outl), C.byref(ninl)))
        if split:
            self._track_job = (match, n, pose, outl, ninl, n_cur)
            return None
        return match, n.value, pose, outl[:n_cur], ninl.value

    def mpbank_put(self, first_row, Xw, normal, min_dist, max_dist):
        Xw, normal, min_dist, max_dist = (_c(a, np.float32) for a in (Xw, normal, min_dist, max_dist))
        self._chk(self.lib.asd_mpbank_put(self.ctx, first_row, len(min_dist), _p(Xw), _p(normal), _p(min_dist), _p(max_dist)))

    def prep_async(self, on):
        self._chk(self.lib.asd_prep_async(self.ctx, int(on)))

    def track_frame(self, slot_cur, slot_last, n_cur, has_mp, Xw_last, last_rows, last_cand, Tcw, K, th, pose7, cand_rows, th_local, nn_ratio,
                    cos_limit=0.5, check_ori=True, last_obs_positive=None, cand_obs_positive=None, split=False):
        """asd_track_frame: both tracking stages as one submission -> dict(match1, n1, pose1, outlier1, n_inl1, match2, n2, pose, outlier2, n_inl2);
        split=True: returns None once enqueued, track_frame_finish() returns the dict"""
        a = asd_track_frame_args()
        keep = dict(has=_c(has_mp, np.uint8), Xw=_c(Xw_last, np.float32), rows=_c(last_rows, np.int32),
                    lc=None if last_cand is None else _c(last_cand, np.int32),
                    o1=None if last_obs_positive is None else _c(last_obs_positive, np.uint8), T=_c(Tcw, np.float32),
                    cr=_c(cand_rows, np.int32), o2=None if cand_obs_positive is None else _c(cand_obs_positive, np.uint8), K=_c(K, np.float32),
                    pose=_c(pose7, np.float64).copy(), pose1=np.zeros(7, np.float64),
                    m1=np.empty(n_cur, np.int32), m2=np.empty(n_cur, np.int32), out1=np.zeros(max(n_cur, 1), np.uint8), out2=np.zeros(max(n_cur, 1), np.uint8),
                    n1=C.c_int32(), n2=C.c_int32(), i1=C.c_int32(), i2=C.c_int32())
        adr = lambda x: None if x is None else x.ctypes.data
        a.slot_cur, a.slot_last = slot_cur, slot_last
        a.has_mp, a.Xw_last, a.last_rows, a.last_cand, a.last_obs_positive = adr(keep["has"]), adr(keep["Xw"]), adr(keep["rows"]), adr(keep["lc"]), adr(keep["o1"])
        a.Tcw, a.th, a.check_orientation = adr(keep["T"]), th, int(check_ori)
        a.n_cand, a.cand_rows, a.cand_obs_positive = len(keep["cr"]), adr(keep["cr"]), adr(keep["o2"])
        a.viewing_cos_limit, a.th_local, a.nn_ratio, a.K = cos_limit, th_local, nn_ratio, adr(keep["K"])
        a.pose7, a.pose1 = adr(keep["pose"]), adr(keep["pose1"])
        a.match1, a.n_matches1, a.outlier1, a.n_inliers1 = adr(keep["m1"]), C.addressof(keep["n1"]), adr(keep["out1"]), C.addressof(keep["i1"])
        a.match2, a.n_matches2, a.outlier2, a.n_inliers2 = adr(keep["m2"]), C.addressof(keep["n2"]), adr(keep["out2"]), C.addressof(keep["i2"])
        if split:
            self._chk(self.lib.asd_track_async(self.ctx))
        self._chk(self.lib.asd_track_frame(self.ctx, C.byref(a)))
        self._frame_job = (keep, n_cur)
        return None if split else self._frame_result()

    def _frame_result(self):
        k, n_cur = self._frame_job
        self._frame_job = None
        return dict(match1=k["m1"], n1=k["n1"].value, pose1=k["pose1"], outlier1=k["out1"][:n_cur], n_inl1=k["i1"].value,
                    match2=k["m2"], n2=k["n2"].value, pose=k["pose"], outlier2=k["out2"][:n_cur], n_inl2=k["i2"].value)

    def track_frame_finish(self):
        self._chk(self.lib.asd_track_finish(self.ctx))
        return self._frame_result()

    def track_finish(self):
        """completes the asd_track_* call started with split=True -> (match_cur, n_matches, pose7, outlier, n_inliers)"""
        rc = self.lib.asd_track_finish(self.ctx)
        job, self._track_job = getattr(self, "_track_job", None), None
        self._chk(rc)
        match, n, pose, outl, ninl, n_cur = job
        return match, n.value, pose, outl[:n_cur], ninl.value

    def debug_level_sweep(self, lo, hi):
        n = C.c_int64()
        self.lib.asd_debug_level_sweep.restype = C.c_int32
        bad = self.lib.asd_debug_level_sweep(self.ctx, C.c_float(lo), C.c_float(hi), C.byref(n))
        return bad, n.value

    def local_ba_forms(self):
        """[2, 5] int32 per round of the last LocalBA: (dense solve 0 solve_lds / 1 chol_lds / 2 chol / -1 none,
        structure 0 device / 1 host, nPf, nLa, Ea) -- asd_debug_local_ba_forms"""
        out = np.empty((2, 5), np.int32)
        self._chk(self.lib.asd_debug_local_ba_forms(self.ctx, _p(out)))
        return out

    def local_ba_lm(self):
        """[2, 4] int32 per round of the last LocalBA: (iterations, trials, trial blocks enqueued, first chunk) --
        asd_debug_local_ba_lm"""
        out = np.empty((2, 4), np.int32)
        self._chk(self.lib.asd_debug_local_ba_lm(self.ctx, _p(out)))
        return out

    def pose_opt_debug(self):
        """(store, rounds [4, 10] int32) of the last pose_optimize: store 2 compact LDS / 1 full LDS / 0 global; per round (state 0 ran /
        1 not run as a repeat / -1 not reached, active edges, iterations, trials, passes, phase-2 passes, trials not positive
        definite, nBad, ended on a rejected trial, iterations with a rejected trial followed by another) -- asd_debug_pose_opt"""
        out = np.empty(41, np.int32)
        self.lib.asd_debug_pose_opt.restype = C.c_int32
        self._chk(self.lib.asd_debug_pose_opt(self.ctx, _p(out)))
        return int(out[0]), out[1:].reshape(4, 10).copy()

    def match_project_keyframe(self, slot_cur, n_cur, valid, Xw, min_dist, max_dist, desc, kf_angle, occupied, Tcw, K, th, orb_dist,
                               check_ori=True):
        a = [_c(valid, np.uint8), _c(Xw, np.float32), _c(min_dist, np.float32), _c(max_dist, np.float32), _c(desc, np.float32),
             _c(kf_angle, np.float32), _c(occupied, np.uint8), _c(Tcw, np.float32), _c(K, np.float32)]
        out = np.empty(n_cur, np.int32)
        n = C.c_int32()
        self._chk(self.lib.asd_match_project_keyframe(self.ctx, slot_cur, len(a[0]), *[_p(x) for x in a], C.c_float(th), C.c_float(orb_dist),
                                                      int(check_ori), _p(out), C.byref(n)))
        return out, n.value

    def match_project_sim3(self, slot_kf, Scw, valid, Xw, normal, min_dist, max_dist, desc, K, th, matched_kp):
        a = [_c(valid, np.uint8), _c(Xw, np.float32), _c(normal, np.float32), _c(min_dist, np.float32), _c(max_dist, np.float32),
             _c(desc, np.float32), _c(K, np.float32)]
        Scw = _c(Scw, np.float32)
        mk = _c(matched_kp, np.int32).copy()
        n = C.c_int32()
        self._chk(self.lib.asd_match_project_sim3(self.ctx, slot_kf, _p(Scw), len(a[0]), *[_p(x) for x in a], int(th), _p(mk), C.byref(n)))
        return mk, n.value

    def fuse_search_sim3(self, slot_kf, Scw, valid, Xw, normal, min_dist, max_dist, desc, K, th=3.0):
        a = [_c(valid, np.uint8), _c(Xw, np.float32), _c(normal, np.float32), _c(min_dist, np.float32), _c(max_dist, np.float32),
             _c(desc, np.float32), _c(K, np.float32)]
        Scw = _c(Scw, np.float32)
        bi, bd = np.empty(len(a[0]), np.int32), np.empty(len(a[0]), np.float32)
        self._chk(self.lib.asd_fuse_search_sim3(self.ctx, slot_kf, _p(Scw), len(a[0]), *[_p(x) for x in a], C.c_float(th), _p(bi), _p(bd)))
        return bi, bd

    def match_sim3(self, slot1, slot2, n1, has1, has2, Xw1, Xw2, mind1, maxd1, mind2, maxd2, desc1, desc2, T1w, T2w, s12, R12, t12, K, th):
        a = [_c(has1, np.uint8), _c(has2, np.uint8)] + [_c(x, np.float32) for x in (Xw1, Xw2, mind1, maxd1, mind2, maxd2, desc1, desc2, T1w, T2w)]
        R12, t12, K = _c(R12, np.float32), _c(t12, np.float32), _c(K, np.float32)
        out = np.empty(n1, np.int32)
        n = C.c_int32()
        self._chk(self.lib.asd_match_sim3(self.ctx, slot1, slot2, *[_p(x) for x in a], C.c_float(s12), _p(R12), _p(t12), _p(K), C.c_float(th),
                                          _p(out), C.byref(n)))
        return out, n.value

    def stereo_match(self, right_ctx, slot_left, slot_right, n_left, mb, mbf):
        u, d = np.empty(n_left, np.float32), np.empty(n_left, np.float32)
        n = C.c_int32()
        self._chk(self.lib.asd_stereo_match(self.ctx, right_ctx.ctx, slot_left, slot_right, C.c_float(mb), C.c_float(mbf), _p(u), _p(d),
                                            C.byref(n)))
        return u, d, n.value

    def distinctive_descriptor_batch(self, set_start, desc):
        set_start, desc = _c(set_start, np.int32), _c(desc, np.float32)
        out = np.empty(len(set_start) - 1, np.int32)
        self._chk(self.lib.asd_distinctive_descriptor_batch(self.ctx, len(out), _p(set_start), _p(desc), _p(out)))
        return out

    def fuse_search(self, slot_kf, valid, Xw, normal, min_dist, max_dist, desc, Tcw, K, th=3.0):
        valid, Xw, normal = _c(valid, np.uint8), _c(Xw, np.float32), _c(normal, np.float32)
        min_dist, max_dist, desc = _c(min_dist, np.float32), _c(max_dist, np.float32), _c(desc, np.float32)
        Tcw, K = _c(Tcw, np.float32), _c(K, np.float32)
        n = len(valid)
        bi = np.empty(n, np.int32)
        bd = np.empty(n, np.float32)
        self._chk(self.lib.asd_fuse_search(self.ctx, slot_kf, n, _p(valid), _p(Xw), _p(normal), _p(min_dist), _p(max_dist),
                                           _p(desc), _p(Tcw), _p(K), C.c_float(th), _p(bi), _p(bd)))
        return bi, bd

    # ---- the per-keyframe stage, batched
    def frame_set_bow(self, slot, nodes):
        fv, keep = make_fv(nodes)
        self._chk(self.lib.asd_frame_set_bow(self.ctx, slot, C.byref(fv)))

    def create_map_points_batch(self, slot_cur, n_cur, has_cur, Tcw_cur, K_cur, neighbours):
        """neighbours: list of dict(slot, has_mp, F12, ex, ey, Tcw, K) -> matches [nb][n_cur], n_matches [nb], x3D [nb][n_cur][3], ok [nb][n_cur]"""
        nb = (asd_kf_neighbor * len(neighbours))()
        keep = []
        for b, d in enumerate(neighbours):
            h = _c(d["has_mp"], np.uint8); keep.append(h)
            nb[b].slot, nb[b].has_mp = d["slot"], h.ctypes.data
            nb[b].F12 = (C.c_float * 9)(*[float(v) for v in np.asarray(d["F12"], np.float32).ravel()])
            nb[b].ex, nb[b].ey = float(d["ex"]), float(d["ey"])
            nb[b].Tcw = (C.c_float * 16)(*[float(v) for v in np.asarray(d["Tcw"], np.float32).ravel()])
            nb[b].K = (C.c_float * 4)(*[float(v) for v in np.asarray(d["K"], np.float32).ravel()])
        has_cur, Tcw_cur, K_cur = _c(has_cur, np.uint8), _c(Tcw_cur, np.float32), _c(K_cur, np.float32)
        B = len(neighbours)
        m = np.empty((B, n_cur), np.int32); nm = np.zeros(B, np.int32)
        x = np.empty((B, n_cur, 3), np.float32); ok = np.empty((B, n_cur), np.uint8)
        self._chk(self.lib.asd_create_map_points_batch(self.ctx, slot_cur, _p(has_cur), _p(Tcw_cur), _p(K_cur), B, nb, _p(m), _p(nm), _p(x), _p(ok)))
        return m, nm, x, ok

    def fuse_search_batch(self, calls, valid, Xw, normal, min_dist, max_dist, desc, th=3.0):
        """calls: list of dict(slot_kf, first, n, Tcw, K) over the shared map-point tables -> best_idx, best_dist [n_total];
        desc: float [n][128] descriptors or int32 rows of the descriptor bank"""
        cs = (asd_fuse_call * len(calls))()
        for c, d in enumerate(calls):
            cs[c].slot_kf, cs[c].first, cs[c].n = d["slot_kf"], d["first"], d["n"]
            cs[c].Tcw = (C.c_float * 16)(*[float(v) for v in np.asarray(d["Tcw"], np.float32).ravel()])
            cs[c].K = (C.c_float * 4)(*[float(v) for v in np.asarray(d["K"], np.float32).ravel()])
        valid, Xw, normal = _c(valid, np.uint8), _c(Xw, np.float32), _c(normal, np.float32)
        min_dist, max_dist = _c(min_dist, np.float32), _c(max_dist, np.float32)
        d = np.asarray(desc)
        rows = d.dtype.kind in "iu"
        d = _c(d, np.int32 if rows else np.float32)
        n = len(valid)
        bi, bd = np.empty(n, np.int32), np.empty(n, np.float32)
        self._chk(self.lib.asd_fuse_search_batch(self.ctx, len(calls), cs, n, _p(valid), _p(Xw), _p(normal), _p(min_dist), _p(max_dist),
                                                 _p(None if rows else d), _p(d if rows else None), C.c_float(th), _p(bi), _p(bd)))
        return bi, bd

    def triangulate_pairs(self, slot1, slot2, idx1, idx2, Tcw1, Tcw2, K1, K2):
        idx1, idx2 = _c(idx1, np.int32), _c(idx2, np.int32)
        Tcw1, Tcw2, K1, K2 = _c(Tcw1, np.float32), _c(Tcw2, np.float32), _c(K1, np.float32), _c(K2, np.float32)
        n = len(idx1)
        x = np.empty((n, 3), np.float32)
        ok = np.empty(n, np.uint8)
        nok = C.c_int32(0)
        self._chk(self.lib.asd_triangulate_pairs(self.ctx, slot1, slot2, n, _p(idx1), _p(idx2), _p(Tcw1), _p(Tcw2), _p(K1), _p(K2),
                                                 _p(x), _p(ok), C.byref(nok)))
        return x, ok, nok.value

    def svd4_null(self, A):
        A = _c(A, np.float32).reshape(-1, 16)
        v = np.empty((len(A), 4), np.float32)
        self._chk(self.lib.asd_svd4_null(self.ctx, len(A), _p(A), _p(v)))
        return v

    # ---- vocabulary / BoW
    def voc_load(self, voc, weighting=0, scoring=0):
        cs, ci = _c(voc["child_start"], np.int32), _c(voc["child_ids"], np.int32)
        w, wid, d = _c(voc["weight"], np.float64), _c(voc["word_id"], np.int32), _c(voc["desc"], np.float32)
        self._chk(self.lib.asd_voc_load(self.ctx, int(voc["n_nodes"]), int(voc["k"]), int(voc["L"]), weighting, scoring,
                                        _p(cs), _p(ci), _p(w), _p(wid), _p(d)))

    def bow_descend(self, desc=None, slot=-1, n=None, levelsup=4):
        if desc is not None:
            desc = _c(desc, np.float32)
            n = len(desc)
        word, node, weight = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.float64)
        self._chk(self.lib.asd_bow_descend(self.ctx, slot, _p(desc) if desc is not None else None, n, levelsup,
                                           _p(word), _p(node), _p(weight)))
        return word, node, weight

    def compute_bow(self, desc=None, slot=-1, n=None, levelsup=4):
        """-> (bow_id, bow_val), (fv_node, fv_start, fv_idx)"""
        if desc is not None:
            desc = _c(desc, np.float32)
            n = len(desc)
        bid, bval = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.float64)
        fnode, fstart, fidx = np.empty(max(n, 1), np.int32), np.empty(n + 1, np.int32), np.empty(max(n, 1), np.int32)
        nw, nn = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.asd_compute_bow(self.ctx, slot, _p(desc) if desc is not None else None, n, levelsup, _p(bid), _p(bval),
                                           C.byref(nw), _p(fnode), _p(fstart), _p(fidx), C.byref(nn)))
        return (bid[:nw.value].copy(), bval[:nw.value].copy()), \
               (fnode[:nn.value].copy(), fstart[:nn.value + 1].copy(), fidx[:fstart[nn.value]].copy())

    # ---- keyframe database (KeyFrameDatabase.cc)
    def kfdb_clear(self, scoring=-1):
        self._chk(self.lib.asd_kfdb_clear(self.ctx, int(scoring)))

    def kfdb_add(self, kf, bow, global_map=True):
        ids, vals = _c(bow[0], np.int32), _c(bow[1], np.float64)
        self._chk(self.lib.asd_kfdb_add(self.ctx, int(kf), len(ids), _p(ids), _p(vals), int(bool(global_map))))

    def kfdb_erase(self, kf):
        self._chk(self.lib.asd_kfdb_erase(self.ctx, int(kf)))

    def kfdb_score(self, bow, kfs):
        """f64 score of the query BowVector against the named entries"""
        ids, vals, kfs = _c(bow[0], np.int32), _c(bow[1], np.float64), _c(kfs, np.int32)
        out = np.empty(len(kfs), np.float64)
        self._chk(self.lib.asd_kfdb_score(self.ctx, len(ids), _p(ids), _p(vals), len(kfs), _p(kfs), _p(out)))
        return out

    def _kfdb_query(self, call):
        cap = int(self.kfdb_debug()[0])
        kf, sc, n = np.empty(max(cap, 1), np.int32), np.empty(max(cap, 1), np.float32), C.c_int32(0)
        self._chk(call(cap, _p(kf), _p(sc), C.byref(n)))
        return kf[:n.value].copy(), sc[:n.value].copy()

    def kfdb_query_loop(self, bow, connected, min_score, only_global_map=False):
        """-> lScoreAndMatch as (keyframe ids, float32 scores) in the reference's list order"""
        ids, vals, con = _c(bow[0], np.int32), _c(bow[1], np.float64), _c(connected, np.int32)
        return self._kfdb_query(lambda cap, kf, sc, n: self.lib.asd_kfdb_query_loop(
            self.ctx, len(ids), _p(ids), _p(vals), len(con), _p(con), C.c_float(min_score), int(bool(only_global_map)), cap, kf, sc, n))

    def kfdb_query_reloc(self, bow, only_global_map=False):
        ids, vals = _c(bow[0], np.int32), _c(bow[1], np.float64)
        return self._kfdb_query(lambda cap, kf, sc, n: self.lib.asd_kfdb_query_reloc(
            self.ctx, len(ids), _p(ids), _p(vals), int(bool(only_global_map)), cap, kf, sc, n))

    def kfdb_select(self, mode, neigh):
        """mode 0 loop / 1 reloc; neigh = one list of up to 10 neighbour ids per scored keyframe -> candidate ids"""
        nb = np.full((len(neigh), 10), -1, np.int32)
        for i, row in enumerate(neigh):
            row = list(row)[:10]
            nb[i, :len(row)] = row
        cand, n = np.empty(max(len(neigh), 1), np.int32), C.c_int32(0)
        self._chk(self.lib.asd_kfdb_select(self.ctx, int(mode), len(neigh), _p(nb), len(neigh), _p(cand), C.byref(n)))
        return cand[:n.value].copy()

    def kfdb_debug(self, kf=None):
        """kf None -> (live entries, live words, entry capacity, word capacity, growths); else dict of the entry's query fields"""
        if kf is None:
            out = np.zeros(5, np.int64)
            self._chk(self.lib.asd_debug_kfdb(self.ctx, _p(out)))
            return tuple(int(x) for x in out)
        out, sc = np.zeros(4, np.int32), np.zeros(2, np.float32)
        self._chk(self.lib.asd_debug_kfdb_entry(self.ctx, int(kf), _p(out), _p(sc)))
        return dict(loop_stamped=bool(out[0]), loop_words=int(out[1]), reloc_stamped=bool(out[2]), reloc_words=int(out[3]),
                    loop_score=np.float32(sc[0]), reloc_score=np.float32(sc[1]))

    # ---- observation table and the local map (localmap.hip)
    def map_clear(self):
        self._chk(self.lib.asd_map_clear(self.ctx))

    def map_put(self, kf, rows):
        rows = _c(rows, np.int32)
        self._chk(self.lib.asd_map_put(self.ctx, int(kf), len(rows), _p(rows)))

    def map_set(self, kf, idx, rows):
        idx, rows = _c(idx, np.int32), _c(rows, np.int32)
        self._chk(self.lib.asd_map_set(self.ctx, int(kf), len(idx), _p(idx), _p(rows)))

    def map_erase(self, kf):
        self._chk(self.lib.asd_map_erase(self.ctx, int(kf)))

    def map_kf_links(self, kf, cov, children, parent):
        cov, children = _c(cov, np.int32), _c(children, np.int32)
        self._chk(self.lib.asd_map_kf_links(self.ctx, int(kf), len(cov), _p(cov), len(children), _p(children), int(parent)))

    def map_kf_bad(self, kf, flag=True):
        self._chk(self.lib.asd_map_kf_bad(self.ctx, int(kf), int(bool(flag))))

    def map_point_bad(self, rows, flag=True):
        rows = _c(rows, np.int32)
        self._chk(self.lib.asd_map_point_bad(self.ctx, len(rows), _p(rows), int(bool(flag))))

    def update_local_map_raw(self, cur_rows, seen_rows, prev_kfs, max_kfs, kf_capacity, row_capacity, search_capacity):
        """asd_update_local_map with the caller's capacities -> (rc, dict); the dict's lists are cut to the counts only when rc == 0"""
        cur, seen, prev = _c(cur_rows, np.int32), _c(seen_rows, np.int32), _c(prev_kfs, np.int32)
        kfs, rows, srch = (np.full(max(c, 1), -7, np.int32) for c in (kf_capacity, row_capacity, search_capacity))
        a = asd_local_map_args()
        a.n_cur, a.cur_rows, a.n_seen, a.seen_rows, a.n_prev, a.prev_kfs = len(cur), cur.ctypes.data, len(seen), seen.ctypes.data, len(prev), prev.ctypes.data
        a.max_kfs = int(max_kfs)
        a.kf_capacity, a.local_kfs, a.row_capacity, a.local_rows = int(kf_capacity), kfs.ctypes.data, int(row_capacity), rows.ctypes.data
        a.search_capacity, a.search_rows = int(search_capacity), srch.ctypes.data
        rc = self.lib.asd_update_local_map(self.ctx, C.byref(a))
        out = dict(n_local_kfs=a.n_local_kfs, ref_kf=a.ref_kf, n_local=a.n_local, n_search=a.n_search)
        if rc == 0:
            out.update(local_kfs=kfs[:a.n_local_kfs].copy(), local_rows=rows[:a.n_local].copy(), search_rows=srch[:a.n_search].copy())
        return rc, out

    def update_local_map(self, cur_rows, seen_rows=(), prev_kfs=(), max_kfs=80):
        """Tracking::UpdateLocalMap + SearchLocalPoints' skip loop -> dict(local_kfs, ref_kf, local_rows, search_rows); repeats once with the
        counts the library asked for (the ASD_ERR_CAPACITY rule of the call)"""
        rc, out = self.update_local_map_raw(cur_rows, seen_rows, prev_kfs, max_kfs, 256, 65536, 65536)
        if rc == -5:   # ASD_ERR_CAPACITY
            rc, out = self.update_local_map_raw(cur_rows, seen_rows, prev_kfs, max_kfs, out["n_local_kfs"], out["n_local"], out["n_search"])
        self._chk(rc)
        return out

    def map_shared_counts(self, kf, capacity=None):
        """KFcounter of KeyFrame::UpdateConnections -> (keyframe ids ascending, counts)"""
        cap = int(self.map_debug()[0]) if capacity is None else int(capacity)
        kfs, cnt, n = np.empty(max(cap, 1), np.int32), np.empty(max(cap, 1), np.int32), C.c_int32(0)
        rc = self.lib.asd_map_shared_counts(self.ctx, int(kf), cap, _p(kfs), _p(cnt), C.byref(n))
        if rc != 0:
            raise AsdError(rc, f"{self.last_error()} [n = {n.value}]")
        return kfs[:n.value].copy(), cnt[:n.value].copy()

    def map_put_octaves(self, kf, octaves):
        octaves = _c(octaves, np.uint8)
        self._chk(self.lib.asd_map_put_octaves(self.ctx, int(kf), len(octaves), _p(octaves)))

    def keyframe_culling_raw(self, cand, flags, apply, bad_capacity):
        """asd_keyframe_culling with the caller's bad_capacity -> (rc, dict); the outputs are in the dict only when rc == 0"""
        cand, flags = _c(cand, np.int32), _c(flags, np.uint8)
        n = len(cand)
        dec, nm, nr = np.full(max(n, 1), 9, np.uint8), np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), -7, np.int32)
        bad = np.full(max(int(bad_capacity), 1), -7, np.int32)
        a = asd_kf_culling_args()
        a.n_cand, a.cand, a.cand_flags, a.apply = n, cand.ctypes.data, flags.ctypes.data, int(bool(apply))
        a.decision, a.n_mps, a.n_redundant = dec.ctypes.data, nm.ctypes.data, nr.ctypes.data
        a.bad_capacity, a.bad_rows, a.n_bad = int(bad_capacity), bad.ctypes.data, -1
        rc = self.lib.asd_keyframe_culling(self.ctx, C.byref(a))
        out = dict(n_bad=a.n_bad)
        if rc == 0:
            out.update(decision=dec[:n].copy(), n_mps=nm[:n].copy(), n_redundant=nr[:n].copy(), bad_rows=bad[:a.n_bad].copy())
        return rc, out

    def keyframe_culling(self, cand, flags=None, apply=False, bad_capacity=256):
        """LocalMapping::KeyFrameCulling -> dict(decision, n_mps, n_redundant, bad_rows); repeats once with the capacity the library asked for"""
        flags = np.zeros(len(cand), np.uint8) if flags is None else flags
        rc, out = self.keyframe_culling_raw(cand, flags, apply, bad_capacity)
        if rc == -5 and out["n_bad"] > bad_capacity:   # ASD_ERR_CAPACITY
            rc, out = self.keyframe_culling_raw(cand, flags, apply, out["n_bad"])
        self._chk(rc)
        return out

    def map_observations(self, rows):
        """MapPoint::Observations() for bank rows"""
        rows = _c(rows, np.int32)
        counts = np.full(max(len(rows), 1), -7, np.int32)
        self._chk(self.lib.asd_map_observations(self.ctx, len(rows), _p(rows), _p(counts)))
        return counts[:len(rows)].copy()

    def map_kf_centers(self, kfs, Ow):
        """KeyFrame::GetCameraCenter() of keyframes in the table (Ow [n][3] f32)"""
        kfs, Ow = _c(kfs, np.int32), _c(Ow, np.float32).reshape(-1, 3)
        assert len(kfs) == len(Ow)
        self._chk(self.lib.asd_map_kf_centers(self.ctx, len(kfs), _p(kfs), _p(Ow)))

    def update_normal_and_depth_raw(self, rows, ref_kf, Xw=None):
        """asd_update_normal_and_depth -> (rc, dict(normal, min_dist, max_dist, status)); the dict is filled only when rc == 0"""
        rows, ref_kf = _c(rows, np.int32), _c(ref_kf, np.int32)
        n = len(rows)
        assert len(ref_kf) == n
        xw = None if Xw is None else _c(Xw, np.float32).reshape(n, 3)
        normal, mn, mx = np.full((max(n, 1), 3), -7, np.float32), np.full(max(n, 1), -7, np.float32), np.full(max(n, 1), -7, np.float32)
        status = np.full(max(n, 1), 9, np.uint8)
        a = asd_normal_depth_args()
        a.n, a.rows, a.ref_kf, a.Xw = n, rows.ctypes.data, ref_kf.ctypes.data, None if xw is None else xw.ctypes.data
        a.normal, a.min_dist, a.max_dist, a.status = normal.ctypes.data, mn.ctypes.data, mx.ctypes.data, status.ctypes.data
        rc = self.lib.asd_update_normal_and_depth(self.ctx, C.byref(a))
        out = {}
        if rc == 0:
            out.update(normal=normal[:n].copy(), min_dist=mn[:n].copy(), max_dist=mx[:n].copy(), status=status[:n].copy())
        return rc, out

    def update_normal_and_depth(self, rows, ref_kf, Xw=None):
        """MapPoint::UpdateNormalAndDepth over the tables (with Xw: SetWorldPos first) -> dict(normal, min_dist, max_dist, status)"""
        rc, out = self.update_normal_and_depth_raw(rows, ref_kf, Xw)
        self._chk(rc)
        return out

    def local_ba_graph_raw(self, kf, neigh, caps, want_Xw=False):
        """asd_local_ba_graph with the caller's capacities caps = (kfs, points, fixed, poses, edges) -> (rc, dict); the dict always holds
        the five counts, the lists (cut to the counts) only when rc == 0"""
        neigh = _c(neigh, np.int32)
        ck, cp, cf, cq, ce = (int(c) for c in caps)
        i32 = lambda c: np.full(max(c, 1), -7, np.int32)
        kfs, rows, rank, fixed, pose = i32(ck), i32(cp), i32(cp), i32(cf), i32(cq)
        pfix, e_point, e_pose, e_kf, e_idx = np.full(max(cq, 1), 9, np.uint8), i32(ce), i32(ce), i32(ce), i32(ce)
        e_oct = np.full(max(ce, 1), 99, np.uint8)
        xw = np.full((max(cp, 1), 3), np.nan) if want_Xw else None
        a = asd_ba_graph_args()
        a.kf, a.n_neigh, a.neigh = int(kf), len(neigh), neigh.ctypes.data
        a.kf_capacity, a.local_kfs = ck, kfs.ctypes.data
        a.point_capacity, a.local_rows, a.point_rank = cp, rows.ctypes.data, rank.ctypes.data
        a.fixed_capacity, a.fixed_kfs = cf, fixed.ctypes.data
        a.pose_capacity, a.pose_kfs, a.pose_fixed = cq, pose.ctypes.data, pfix.ctypes.data
        a.edge_capacity, a.e_point, a.e_pose, a.e_kf, a.e_idx, a.e_octave = ce, e_point.ctypes.data, e_pose.ctypes.data, e_kf.ctypes.data, e_idx.ctypes.data, e_oct.ctypes.data
        a.Xw = None if xw is None else xw.ctypes.data
        a.n_local_kfs = a.n_points = a.n_fixed = a.n_poses = a.n_edges = -1
        rc = self.lib.asd_local_ba_graph(self.ctx, C.byref(a))
        out = dict(n_local_kfs=a.n_local_kfs, n_points=a.n_points, n_fixed=a.n_fixed, n_poses=a.n_poses, n_edges=a.n_edges)
        if rc == 0:
            out.update(local_kfs=kfs[:a.n_local_kfs].copy(), local_rows=rows[:a.n_points].copy(), point_rank=rank[:a.n_points].copy(),
                       fixed_kfs=fixed[:a.n_fixed].copy(), pose_kfs=pose[:a.n_poses].copy(), pose_fixed=pfix[:a.n_poses].copy(),
                       e_point=e_point[:a.n_edges].copy(), e_pose=e_pose[:a.n_edges].copy(), e_kf=e_kf[:a.n_edges].copy(),
                       e_idx=e_idx[:a.n_edges].copy(), e_octave=e_oct[:a.n_edges].copy())
            if want_Xw:
                out["Xw"] = xw[:a.n_points].copy()
        return rc, out

    def local_ba_graph(self, kf, neigh, want_Xw=False, caps=(64, 4096, 64, 128, 16384)):
        """Optimizer::LocalBundleAdjustment's lists and edges over the table; repeats once with the counts the library asked for"""
        rc, out = self.local_ba_graph_raw(kf, neigh, caps, want_Xw)
        if rc == -5 and out["n_local_kfs"] > 0:   # ASD_ERR_CAPACITY with the counts set
            rc, out = self.local_ba_graph_raw(kf, neigh, (out["n_local_kfs"], out["n_points"], out["n_fixed"], out["n_poses"], out["n_edges"]), want_Xw)
        self._chk(rc)
        return out

    def local_ba_apply_raw(self, erase, n_points, apply, bad_capacity):
        """asd_local_ba_apply -> (rc, dict(n_erased, n_bad[, bad_rows, new_ref]))"""
        erase = _c(erase, np.uint8)
        bad, ref = np.full(max(int(bad_capacity), 1), -7, np.int32), np.full(max(int(n_points), 1), -7, np.int32)
        a = asd_ba_apply_args()
        a.n_edges, a.erase, a.apply, a.n_erased = len(erase), erase.ctypes.data, int(bool(apply)), -1
        a.bad_capacity, a.bad_rows, a.n_bad, a.n_points, a.new_ref = int(bad_capacity), bad.ctypes.data, -1, int(n_points), ref.ctypes.data
        rc = self.lib.asd_local_ba_apply(self.ctx, C.byref(a))
        out = dict(n_erased=a.n_erased, n_bad=a.n_bad)
        if rc == 0:
            out.update(bad_rows=bad[:a.n_bad].copy(), new_ref=ref[:int(n_points)].copy())
        return rc, out

    def local_ba_apply(self, erase, n_points, apply=False, bad_capacity=64):
        """the erase policy of Optimizer.cc:652-697 over the resident graph; repeats once with the capacity the library asked for"""
        rc, out = self.local_ba_apply_raw(erase, n_points, apply, bad_capacity)
        if rc == -5 and out["n_bad"] > bad_capacity:
            rc, out = self.local_ba_apply_raw(erase, n_points, apply, out["n_bad"])
        self._chk(rc)
        return out

    def fuse_apply_raw(self, kf, cand, best_idx, mode=0, apply=False):
        """asd_fuse_apply -> (rc, dict(action, other, obs_cand, obs_other, n_moved, n_dropped, n_fused)); the dict is filled only when rc == 0"""
        cand, best = _c(cand, np.int32), _c(best_idx, np.int32)
        n = len(cand)
        assert len(best) == n
        act = np.full(max(n, 1), 99, np.uint8)
        oth, oc, oo, mv, dr = (np.full(max(n, 1), -7, np.int32) for _ in range(5))
        a = asd_fuse_apply_args()
        a.kf, a.mode, a.n, a.cand, a.best_idx, a.apply = int(kf), int(mode), n, cand.ctypes.data, best.ctypes.data, int(bool(apply))
        a.action, a.other, a.obs_cand, a.obs_other = act.ctypes.data, oth.ctypes.data, oc.ctypes.data, oo.ctypes.data
        a.n_moved, a.n_dropped, a.n_fused = mv.ctypes.data, dr.ctypes.data, -1
        rc = self.lib.asd_fuse_apply(self.ctx, C.byref(a))
        out = {}
        if rc == 0:
            out.update(action=act[:n].copy(), other=oth[:n].copy(), obs_cand=oc[:n].copy(), obs_other=oo[:n].copy(), n_moved=mv[:n].copy(),
                       n_dropped=dr[:n].copy(), n_fused=int(a.n_fused))
        return rc, out

    def fuse_apply(self, kf, cand, best_idx, mode=0, apply=False):
        """the side effects of ORBmatcher::Fuse (mode 0), Fuse with Scw + SearchAndFuse's loop (1), CorrectLoop's loop fusion (2) over the table"""
        rc, out = self.fuse_apply_raw(kf, cand, best_idx, mode, apply)
        self._chk(rc)
        return out

    def map_get_raw(self, kf, capacity):
        rows, n = np.full(max(int(capacity), 1), -7, np.int32), C.c_int32(-1)
        rc = self.lib.asd_map_get(self.ctx, int(kf), int(capacity), _p(rows), C.byref(n))
        return rc, n.value, (rows[:n.value].copy() if rc == 0 else None)

    def map_get(self, kf, capacity=2048):
        """KeyFrame::GetMapPointMatches(): the keyframe's row as it stands; repeats once with the length the library asked for"""
        rc, n, rows = self.map_get_raw(kf, capacity)
        if rc == -5:   # ASD_ERR_CAPACITY
            rc, n, rows = self.map_get_raw(kf, n)
        self._chk(rc)
        return rows

    def map_points_raw(self, kfs, capacity):
        kfs = _c(kfs, np.int32)
        rows, n = np.full(max(int(capacity), 1), -7, np.int32), C.c_int32(-1)
        rc = self.lib.asd_map_points(self.ctx, len(kfs), _p(kfs), int(capacity), _p(rows), C.byref(n))
        return rc, n.value, (rows[:n.value].copy() if rc == 0 else None)

    def map_points(self, kfs, capacity=65536):
        """the distinct not-bad points of the keyframes' rows in order (UpdateLocalPoints' rule); repeats once with the count asked for"""
        rc, n, rows = self.map_points_raw(kfs, capacity)
        if rc == -5:   # ASD_ERR_CAPACITY
            rc, n, rows = self.map_points_raw(kfs, n)
        self._chk(rc)
        return rows

    def map_debug(self):
        """(live keyframes, live entries, slot capacity, arena capacity, row-table capacity, slot / arena / row-table growths)"""
        out = np.zeros(8, np.int64)
        self._chk(self.lib.asd_debug_map(self.ctx, _p(out)))
        return tuple(int(x) for x in out)

    def track_local_points_map(self, slot_cur, n_cur, Tcw, K, occupied, cur_Xw, th, nn_ratio, pose7, cos_limit=0.5, obs_positive=None, split=False):
        """asd_track_local_points_map: asd_track_local_points_rows over the search list the last update_local_map left on the device"""
        Tcw, K, occupied, cur_Xw = _c(Tcw, np.float32), _c(K, np.float32), _c(occupied, np.uint8), _c(cur_Xw, np.float32)
        match, outl = np.empty(n_cur, np.int32), np.empty(max(n_cur, 1), np.uint8)
        pose = _c(pose7, np.float64).copy()
        n, ninl = C.c_int32(), C.c_int32()
        if split:
            self._chk(self.lib.asd_track_async(self.ctx))
        self._chk(self.lib.asd_track_local_points_map(self.ctx, slot_cur, _p(Tcw), _p(K), C.c_float(cos_limit), _p(occupied), _p(cur_Xw), C.c_float(th),
                                                      C.c_float(nn_ratio), _p(None if obs_positive is None else _c(obs_positive, np.uint8)), _p(pose),
                                                      _p(match), C.byref(n), _p(outl), C.byref(ninl)))
        if split:
            self._track_job = (match, n, pose, outl, ninl, n_cur)
            return None
        return match, n.value, pose, outl[:n_cur], ninl.value

    def bank_put(self, first_row, desc):
        desc = _c(desc, np.float32)
        self._chk(self.lib.asd_bank_put(self.ctx, first_row, desc.shape[0], _p(desc)))

    def bank_put_from_frame(self, slot, first_row, n):
        self._chk(self.lib.asd_bank_put_from_frame(self.ctx, slot, first_row, n))

    def bank_get(self, first_row, n, desc=True, attr=True):
        """asd_debug_bank_get: rows [first_row, first_row + n) of the banks as a consumer reads them (the context's stream only) ->
        (descriptors [n, 128] f32 or None, attributes [n, 8] f32 = Xw, normal, min_dist, max_dist or None)"""
        d = np.empty((max(n, 0), 128), np.float32) if desc else None
        a = np.empty((max(n, 0), 8), np.float32) if attr else None
        self.lib.asd_debug_bank_get.restype = C.c_int32
        self._chk(self.lib.asd_debug_bank_get(self.ctx, C.c_int32(first_row), C.c_int32(n), _p(d), _p(a)))
        return d, a

    def match_project_frame_bank(self, slot_cur, slot_last, n_cur, has_mp, Xw, mp_rows, Tcw, K, th, check_ori=True, obs_positive=None):
        has_mp, Xw, mp_rows = _c(has_mp, np.uint8), _c(Xw, np.float32), _c(mp_rows, np.int32)
        Tcw, K = _c(Tcw, np.float32), _c(K, np.float32)
        out = np.empty(n_cur, np.int32)
        n = C.c_int32()
        self._chk(self.lib.asd_match_project_frame_bank(self.ctx, slot_cur, slot_last, _p(has_mp), _p(Xw), _p(mp_rows),
                                                        _p(Tcw), _p(K), C.c_float(th), int(check_ori), _p(out), C.byref(n),
                                                        _p(None if obs_positive is None else _c(obs_positive, np.uint8))))
        return out, n.value

    def match_project_points_bank(self, slot_cur, n_cur, in_view, proj, level, view_cos, rows, occupied, th, nn_ratio, obs_positive=None):
        in_view, proj, level = _c(in_view, np.uint8), _c(proj, np.float32), _c(level, np.int32)
        view_cos, rows, occupied = _c(view_cos, np.float32), _c(rows, np.int32), _c(occupied, np.uint8)
        out = np.empty(n_cur, np.int32)
        n = C.c_int32()
        self._chk(self.lib.asd_match_project_points_bank(self.ctx, slot_cur, len(in_view), _p(in_view), _p(proj), _p(level),
                                                         _p(view_cos), _p(rows), _p(occupied), C.c_float(th),
                                                         C.c_float(nn_ratio), _p(out), C.byref(n),
                                                         _p(None if obs_positive is None else _c(obs_positive, np.uint8))))
        return out, n.value

    def frustum(self, slot_cur, Xw, normal, min_dist, max_dist, Tcw, K, cos_limit=0.5):
        Xw, normal = _c(Xw, np.float32), _c(normal, np.float32)
        min_dist, max_dist = _c(min_dist, np.float32), _c(max_dist, np.float32)
        Tcw, K = _c(Tcw, np.float32), _c(K, np.float32)
        n = Xw.shape[0]
        in_view = np.zeros(n, np.uint8)
        proj = np.zeros((n, 2), np.float32)
        level = np.zeros(n, np.int32)
        vc = np.zeros(n, np.float32)
        self._chk(self.lib.asd_frustum(self.ctx, slot_cur, n, _p(Xw), _p(normal), _p(min_dist), _p(max_dist),
                                       _p(Tcw), _p(K), C.c_float(cos_limit), _p(in_view), _p(proj), _p(level),
                                       _p(vc)))
        return in_view, proj, level, vc

    def match_init(self, slot1, slot2, prev_matched, window=100, nn_ratio=0.9, check_ori=True):
        pm = _c(prev_matched, np.float32).copy()
        out = np.empty(pm.shape[0], np.int32)
        n = C.c_int32()
        self._chk(self.lib.asd_match_init(self.ctx, slot1, slot2, _p(pm), window, C.c_float(nn_ratio),
                                          int(check_ori), _p(out), C.byref(n)))
        return out, n.value, pm

    def match_bow(self, slot_kf, slot_f, n_f, nodes_kf, nodes_f, has_mp_kf, nn_ratio=0.7, check_ori=True):
        fa, ka = make_fv(nodes_kf)
        fb, kb = make_fv(nodes_f)
        has = _c(has_mp_kf, np.uint8)
        out = np.empty(n_f, np.int32)
        n = C.c_int32()
        self._chk(self.lib.asd_match_bow(self.ctx, slot_kf, slot_f, C.byref(fa), C.byref(fb), _p(has), C.c_float(nn_ratio),
                                         int(check_ori), _p(out), C.byref(n)))
        return out, n.value

    def match_bow_kf(self, slot1, slot2, n1, nodes1, nodes2, has_mp1, has_mp2, nn_ratio=0.85, check_ori=True):
        """ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (ORBmatcher.cc:533-666; LoopClosing.cc:277 builds the matcher
        with nnratio 0.85 and the orientation check): (match12[n1] = keypoint of keyframe 2 or -1, number of matches)"""
        fa, ka = make_fv(nodes1)
        fb, kb = make_fv(nodes2)
        h1, h2 = _c(has_mp1, np.uint8), _c(has_mp2, np.uint8)
        out = np.empty(n1, np.int32)
        n = C.c_int32()
        self._chk(self.lib.asd_match_bow_kf(self.ctx, slot1, slot2, C.byref(fa), C.byref(fb), _p(h1), _p(h2), C.c_float(nn_ratio),
                                            int(check_ori), _p(out), C.byref(n)))
        return out, n.value

    def match_triangulate(self, slot1, slot2, n1, nodes1, nodes2, has_mp1, has_mp2, F12, ex, ey, check_ori=False):
        fa, ka = make_fv(nodes1)
        fb, kb = make_fv(nodes2)
        h1, h2, F = _c(has_mp1, np.uint8), _c(has_mp2, np.uint8), _c(F12, np.float32)
        out = np.empty(n1, np.int32)
        n = C.c_int32()
        self._chk(self.lib.asd_match_triangulate(self.ctx, slot1, slot2, C.byref(fa), C.byref(fb), _p(h1), _p(h2), _p(F),
                                                 C.c_float(ex), C.c_float(ey), int(check_ori), _p(out), C.byref(n)))
        return out, n.value

    # ---- optimizer
    def pose_optimize(self, pose7, Xw, obs, inv_sigma2, K):
        pose = _c(pose7, np.float64).copy()
        Xw, obs, inv_sigma2, K = (_c(a, np.float64) for a in (Xw, obs, inv_sigma2, K))
        n = Xw.shape[0]
        outlier = np.zeros(n, np.uint8)
        ninl = C.c_int32()
        self._chk(self.lib.asd_pose_optimize(self.ctx, _p(pose), n, _p(Xw), _p(obs), _p(inv_sigma2), _p(K),
                                             _p(outlier), C.byref(ninl)))
        return pose, outlier, ninl.value

    def optimize_sim3(self, sim3, P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K1, K2, th2=10.0, fix_scale=False):
        """Optimizer::OptimizeSim3 (Optimizer.cc:1002-1194) over n correspondences: (sim3[8] = qx qy qz qw tx ty tz s, keep[n], nIn).
        On the early return (fewer than 10 pairs left after the first round) sim3 comes back as it went in and nIn is 0."""
        S = _c(sim3, np.float64).copy()
        a = [_c(x, np.float64) for x in (P1c, P2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2, K1, K2)]
        n = len(a[4])
        keep = np.zeros(n, np.uint8)
        n_in = C.c_int32()
        self._chk(self.lib.asd_optimize_sim3(self.ctx, _p(S), n, *[_p(x) for x in a], C.c_float(th2), int(bool(fix_scale)),
                                             _p(keep), C.byref(n_in)))
        return S, keep, n_in.value

    def debug_optimize_sim3(self):
        """what the last optimize_sim3 did: dict(rounds=[dict(active, iterations, trials, ends_rejected)] for the rounds that ran,
        n_bad, cap (the second round's iteration limit, 5 or 10), early, n) -- asd_debug_optimize_sim3"""
        out = np.full(12, -1, np.int32)
        self.lib.asd_debug_optimize_sim3.restype = C.c_int32
        self._chk(self.lib.asd_debug_optimize_sim3(self.ctx, _p(out)))
        rounds = [dict(active=int(out[4 * r]), iterations=int(out[4 * r + 1]), trials=int(out[4 * r + 2]), ends_rejected=int(out[4 * r + 3]))
                  for r in range(2) if out[4 * r] >= 0]
        return dict(rounds=rounds, n_bad=int(out[8]), cap=int(out[9]), early=int(out[10]), n=int(out[11]))

    def sim3_ransac(self, problems):
        """asd_sim3_ransac: Sim3Solver::iterate (Sim3Solver.cc:140-207) for a batch of solvers.  problems = dicts with n, X1c, X2c,
        max_err1, max_err2, K1, K2, fix_scale, min_inliers, n_iter, draws [n_iter][3], best_inliers (further keys are ignored) -> one dict
        per problem: best_inliers, best_updated, R12, t12, s12, T12 (as they went in -- NaN-filled here -- unless best_updated), found,
        iterations_done, n_inliers, inliers [n] uint8."""
        arr = (asd_sim3_ransac_problem * max(len(problems), 1))()
        keep = []
        for j, q in enumerate(problems):
            n = int(q["n"])
            a = [_c(q["X1c"], np.float32), _c(q["X2c"], np.float32), _c(q["max_err1"], np.float32), _c(q["max_err2"], np.float32),
                 _c(q["draws"], np.int32), np.zeros(max(n, 1), np.uint8)]
            keep.append(a)
            P = arr[j]
            P.n = n
            P.X1c, P.X2c, P.max_err1, P.max_err2, P.draws, P.inliers = (x.ctypes.data for x in a)
            P.K1 = (C.c_float * 4)(*[float(k) for k in q["K1"]])
            P.K2 = (C.c_float * 4)(*[float(k) for k in q["K2"]])
            P.fix_scale, P.min_inliers, P.n_iter, P.best_inliers = int(q["fix_scale"]), int(q["min_inliers"]), int(q["n_iter"]), int(q["best_inliers"])
            P.best_updated, P.found, P.iterations_done, P.n_inliers = -1, -1, -1, -1
            nan = float("nan")
            P.R12 = (C.c_float * 9)(*[nan] * 9)
            P.t12 = (C.c_float * 3)(*[nan] * 3)
            P.T12 = (C.c_float * 16)(*[nan] * 16)
            P.s12 = nan
        self._chk(self.lib.asd_sim3_ransac(self.ctx, len(problems), arr))
        out = []
        for j, q in enumerate(problems):
            P = arr[j]
            out.append(dict(best_inliers=int(P.best_inliers), best_updated=int(P.best_updated), R12=np.array(P.R12, np.float32).reshape(3, 3),
                            t12=np.array(P.t12, np.float32), s12=np.float32(P.s12), T12=np.array(P.T12, np.float32).reshape(4, 4),
                            found=int(P.found), iterations_done=int(P.iterations_done), n_inliers=int(P.n_inliers),
                            inliers=keep[j][5][:int(q["n"])].copy()))
        return out

    def debug_sim3_ransac(self, problem, hypothesis):
        """one iteration of the last sim3_ransac: dict(idx [3], count, T12, T21 (4x4 f32), s (f32), q (w x y z, f64)) -- asd_debug_sim3_ransac"""
        d = asd_sim3_ransac_debug()
        self.lib.asd_debug_sim3_ransac.restype = C.c_int32
        rc = self.lib.asd_debug_sim3_ransac(self.ctx, int(problem), int(hypothesis), C.byref(d))
        if rc != 0:
            raise AsdError(rc, f"asd_debug_sim3_ransac: the last call ran no hypothesis {hypothesis} of problem {problem}")
        return dict(idx=[int(i) for i in d.idx], count=int(d.count), T12=np.array(d.T12, np.float32).reshape(4, 4),
                    T21=np.array(d.T21, np.float32).reshape(4, 4), s=np.float32(d.s), q=np.array(d.q, np.float64))

    def pnp_ransac(self, problems, null=None):
        """asd_pnp_ransac: PnPsolver::iterate (PnPsolver.cc:165-258) for a batch of solvers.  problems = dicts with n, P3Dw, P2D, max_err,
        K, min_inliers, n_iter, draws [n_iter][4], best_inliers (further keys are ignored) -> one dict per problem: best_inliers,
        best_updated, best_Tcw, best_mask (as they went in -- NaN / 0xff here -- unless best_updated), found, iterations_done, n_inliers,
        Tcw (NaN unless found), inliers [n] uint8 (0xff-filled going in).  null = (problem, field): that pointer is passed as NULL."""
        arr = (asd_pnp_ransac_problem * max(len(problems), 1))()
        keep = []
        nan = float("nan")
        for j, q in enumerate(problems):
            n = int(q["n"])
            a = [_c(q["P3Dw"], np.float32), _c(q["P2D"], np.float32), _c(q["max_err"], np.float32), _c(q["draws"], np.int32),
                 np.full(max(n, 1), 0xff, np.uint8), np.full(max(n, 1), 0xff, np.uint8)]
            keep.append(a)
            P = arr[j]
            P.n = n
            P.P3Dw, P.P2D, P.max_err, P.draws, P.best_mask, P.inliers = (x.ctypes.data for x in a)
            if null is not None and null[0] == j:
                setattr(P, null[1], None)
            P.K = (C.c_float * 4)(*[float(k) for k in q["K"]])
            P.min_inliers, P.n_iter, P.best_inliers = int(q["min_inliers"]), int(q["n_iter"]), int(q["best_inliers"])
            P.best_updated, P.found, P.iterations_done, P.n_inliers = -1, -1, -1, -1
            P.best_Tcw = (C.c_float * 16)(*[nan] * 16)
            P.Tcw = (C.c_float * 16)(*[nan] * 16)
        self._chk(self.lib.asd_pnp_ransac(self.ctx, len(problems), arr))
        out = []
        for j, q in enumerate(problems):
            P = arr[j]
            n = int(q["n"])
            out.append(dict(best_inliers=int(P.best_inliers), best_updated=int(P.best_updated),
                            best_Tcw=np.array(P.best_Tcw, np.float32).reshape(4, 4), best_mask=keep[j][4][:n].copy(), found=int(P.found),
                            iterations_done=int(P.iterations_done), n_inliers=int(P.n_inliers), Tcw=np.array(P.Tcw, np.float32).reshape(4, 4),
                            inliers=keep[j][5][:n].copy()))
        return out

    def debug_pnp_ransac(self, problem, which):
        """one compute_pose of the last pnp_ransac (which >= 0: that iteration; -1 - r: the r-th Refine): dict(idx [4], count, n_refines, N,
        hypothesis, R (3x3), t, cws (4x3), v (4x12), eig [4], rep_errors [3], betas [4], all f64) -- asd_debug_pnp_ransac"""
        d = asd_pnp_ransac_debug()
        self.lib.asd_debug_pnp_ransac.restype = C.c_int32
        rc = self.lib.asd_debug_pnp_ransac(self.ctx, int(problem), int(which), C.byref(d))
        if rc != 0:
            raise AsdError(rc, f"asd_debug_pnp_ransac: the last call ran no compute_pose {which} of problem {problem}")
        f = lambda a, *shape: np.array(a, np.float64).reshape(*shape)
        return dict(idx=[int(i) for i in d.idx], count=int(d.count), n_refines=int(d.n_refines), N=int(d.N), hypothesis=int(d.hypothesis),
                    R=f(d.R, 3, 3), t=f(d.t, 3), cws=f(d.cws, 4, 3), v=f(d.v, 4, 12), eig=f(d.eig, 4), rep_errors=f(d.rep_errors, 3),
                    betas=f(d.betas, 4))

    def initialize(self, problems, null=None):
        """asd_initialize: Initializer::Initialize (Initializer.cc:43-120) for a batch of frame pairs.  problems = dicts with keys1 [n1][2],
        keys2 [n2][2], matches12 [n1], K, sigma, n_iter, draws [n_iter][8], min_parallax, min_triangulated (further keys are ignored; n1 /
        n2 override the array lengths) -> one dict per problem: n_matches, SH, SF, model, ok, R21, t21, P3D [n1][3], triangulated [n1], H21,
        F21, inliers_H, inliers_F [n_matches].  What the call does not write stays as it went in: NaN in R21 / t21 / P3D / H21 / F21, 0xff
        in triangulated.  null = (problem, field): that pointer is passed as NULL."""
        arr = (asd_initializer_problem * max(len(problems), 1))()
        keep = []
        nan = float("nan")
        for j, q in enumerate(problems):
            k1, k2 = _c(q["keys1"], np.float32).reshape(-1, 2), _c(q["keys2"], np.float32).reshape(-1, 2)
            n1, n2 = int(q.get("n1", len(k1))), int(q.get("n2", len(k2)))
            a = [k1, k2, _c(q["matches12"], np.int32), _c(q["draws"], np.int32), np.full((max(n1, 1), 3), nan, np.float32),
                 np.full(max(n1, 1), 0xff, np.uint8), np.full(max(n1, 1), 0xff, np.uint8), np.full(max(n1, 1), 0xff, np.uint8)]
            keep.append(a)
            P = arr[j]
            P.n1, P.n2 = n1, n2
            P.keys1, P.keys2, P.matches12, P.draws, P.P3D, P.triangulated, P.inliers_H, P.inliers_F = (x.ctypes.data for x in a)
            if null is not None and null[0] == j:
                setattr(P, null[1], None)
            P.K = (C.c_float * 4)(*[float(k) for k in q["K"]])
            P.sigma, P.n_iter = float(q["sigma"]), int(q["n_iter"])
            P.min_parallax, P.min_triangulated = float(q["min_parallax"]), int(q["min_triangulated"])
            P.n_matches, P.model, P.ok = -1, -1, -1
            P.SH = P.SF = nan
            P.R21 = (C.c_float * 9)(*[nan] * 9)
            P.t21 = (C.c_float * 3)(*[nan] * 3)
            P.H21 = (C.c_float * 9)(*[nan] * 9)
            P.F21 = (C.c_float * 9)(*[nan] * 9)
        self._chk(self.lib.asd_initialize(self.ctx, len(problems), arr))
        out = []
        for j, q in enumerate(problems):
            P = arr[j]
            a = keep[j]
            n1, N = int(P.n1), int(P.n_matches)
            f = lambda x, *shape: np.array(x, np.float32).reshape(*shape)
            out.append(dict(n_matches=N, SH=np.float32(P.SH), SF=np.float32(P.SF), model=int(P.model), ok=int(P.ok), R21=f(P.R21, 3, 3),
                            t21=f(P.t21, 3), P3D=a[4][:n1].copy(), triangulated=a[5][:n1].copy(), H21=f(P.H21, 3, 3), F21=f(P.F21, 3, 3),
                            inliers_H=a[6][:N].copy(), inliers_F=a[7][:N].copy()))
        return out

    def debug_initialize(self, problem, which, n_matches=0):
        """asd_debug_initialize of the last initialize.  which = 2 k + m (m = 0 H, 1 F): dict(idx [8], nullv [9] f64, U, w, Vt f64 (F: the
        rank-2 step), M1 = H21i / F21i, M2 = H12i, score, mask [n_matches]); which = -1: the reconstruction: dict(U, w, Vt f64, best_H,
        best_F, n_inliers, n_hyp, winner, second_good, R [8][3][3], t [8][3], parallax [8], cos_sel [8], n_good [8]); which = -2 - h: the
        same plus points [n_matches][3] and flags [n_matches] of hypothesis h.  n_matches sizes the per-match arrays (0: not asked for)."""
        d = asd_initializer_debug()
        n = int(n_matches)
        mask = np.zeros(max(n, 1), np.uint8)
        pts = np.zeros((max(n, 1), 3), np.float32)
        flags = np.zeros(max(n, 1), np.uint8)
        if n > 0:
            d.mask, d.points, d.flags = mask.ctypes.data, pts.ctypes.data, flags.ctypes.data
        self.lib.asd_debug_initialize.restype = C.c_int32
        rc = self.lib.asd_debug_initialize(self.ctx, int(problem), int(which), C.byref(d))
        if rc != 0:
            raise AsdError(rc, f"asd_debug_initialize: the last call has no record {which} of problem {problem}")
        f8 = lambda a, *shape: np.array(a, np.float64).reshape(*shape)
        f4 = lambda a, *shape: np.array(a, np.float32).reshape(*shape)
        out = dict(U=f8(d.U, 3, 3), w=f8(d.w, 3), Vt=f8(d.Vt, 3, 3), best_H=int(d.best_H), best_F=int(d.best_F), n_inliers=int(d.n_inliers),
                   n_hyp=int(d.n_hyp), winner=int(d.winner), second_good=int(d.second_good))
        if which >= 0:
            out.update(idx=[int(i) for i in d.idx], nullv=f8(d.nullv, 9), M1=f4(d.M1, 3, 3), M2=f4(d.M2, 3, 3), score=np.float32(d.score),
                       mask=mask[:n].copy())
        else:
            out.update(R=f4(d.R, 8, 3, 3), t=f4(d.t, 8, 3), parallax=f4(d.parallax, 8), cos_sel=f4(d.cos_sel, 8),
                       n_good=np.array(d.n_good, np.int32))
            if which < -1:
                out.update(points=pts[:n].copy(), flags=flags[:n].copy())
        return out

    def _ba_pack(self, prob, its_first, its_second):
        poses = _c(prob["poses"], np.float64).copy()
        points = _c(prob["points"], np.float64).copy()
        fixed = _c(prob["fixed"], np.uint8)
        e_point, e_pose = _c(prob["e_point"], np.int32), _c(prob["e_pose"], np.int32)
        e_obs, e_info = _c(prob["e_obs"], np.float64), _c(prob["e_info"], np.float64)
        E = len(e_point)
        chi2 = np.zeros(E, np.float64)
        dpos = np.zeros(E, np.uint8)
        out1 = np.zeros(E, np.uint8)
        p = asd_ba_problem(len(poses), len(points), E, poses.ctypes.data, fixed.ctypes.data, points.ctypes.data,
                           e_point.ctypes.data, e_pose.ctypes.data, e_obs.ctypes.data, e_info.ctypes.data,
                           (C.c_double * 4)(*[float(k) for k in prob["K"]]), its_first, its_second)
        r = asd_ba_result(chi2.ctypes.data, dpos.ctypes.data, out1.ctypes.data, 0.0, 0.0, 0, 0)
        keep = (poses, points, fixed, e_point, e_pose, e_obs, e_info, chi2, dpos, out1)   # the structs hold raw addresses
        return p, r, keep

    @staticmethod
    def _ba_unpack(r, keep):
        poses, points, _f, _ep, _es, _eo, _ei, chi2, dpos, out1 = keep
        return dict(poses=poses, points=points, edge_chi2=chi2, edge_depth_pos=dpos, edge_outlier1=out1,
                    chi2_first=r.chi2_first, chi2_second=r.chi2_second, iters_first=r.iters_first,
                    iters_second=r.iters_second)

    def local_ba(self, prob, its_first=5, its_second=10):
        p, r, keep = self._ba_pack(prob, its_first, its_second)
        self._chk(self.lib.asd_local_ba(self.ctx, C.byref(p), C.byref(r)))
        return self._ba_unpack(r, keep)

    def bundle_adjustment(self, prob, n_iterations=20, robust=True, stop=None):
        """Optimizer::BundleAdjustment (Optimizer.cc:51-237) -- asd_bundle_adjustment.  prob: the flat arrays of synth.gba_map /
        synth.ba_problem; stop: None or an int32 array of one element (pbStopFlag).  Returns dict(poses, points, edge_chi2, chi2,
        iterations, trials)."""
        poses = _c(prob["poses"], np.float64).reshape(-1, 7).copy()
        points = _c(prob["points"], np.float64).reshape(-1, 3).copy()
        fixed = _c(prob["fixed"], np.uint8)
        e_point, e_pose = _c(prob["e_point"], np.int32), _c(prob["e_pose"], np.int32)
        e_obs, e_info = _c(prob["e_obs"], np.float64), _c(prob["e_info"], np.float64)
        E = len(e_point)
        chi2 = np.zeros(max(E, 1), np.float64)
        if stop is not None:
            assert stop.dtype == np.int32 and stop.size == 1
        p = asd_gba_problem(len(poses), len(points), E, poses.ctypes.data, fixed.ctypes.data, points.ctypes.data,
                            e_point.ctypes.data, e_pose.ctypes.data, e_obs.ctypes.data, e_info.ctypes.data,
                            (C.c_double * 4)(*[float(k) for k in prob["K"]]), int(n_iterations), int(bool(robust)),
                            stop.ctypes.data if stop is not None else None)
        r = asd_gba_result(chi2.ctypes.data, 0.0, 0, 0)
        self._chk(self.lib.asd_bundle_adjustment(self.ctx, C.byref(p), C.byref(r)))
        return dict(poses=poses, points=points, edge_chi2=chi2[:E], chi2=r.chi2, iterations=int(r.iterations), trials=int(r.trials))

    def optimize_essential_graph(self, prob, n_iterations=None, tail=True):
        """Optimizer::OptimizeEssentialGraph (Optimizer.cc:737-1000) -- asd_optimize_essential_graph.  prob: the flat arrays of
        asd_essgraph_problem (sim3 [K][8], fixed, e_i, e_j, e_meas [E][8], fix_scale, n_iterations, optionally mp_ref, mp_Xw).
        Returns dict(sim3, Tcw, points, edge_chi2, chi2, iterations, trials)."""
        sim3 = _c(prob["sim3"], np.float64).reshape(-1, 8).copy()
        fixed = _c(prob["fixed"], np.uint8)
        e_i, e_j = _c(prob["e_i"], np.int32), _c(prob["e_j"], np.int32)
        e_meas = _c(prob["e_meas"], np.float64).reshape(-1, 8)
        K, E = len(sim3), len(e_i)
        mp_ref = _c(prob.get("mp_ref", np.zeros(0, np.int32)), np.int32)
        mp_Xw = _c(prob.get("mp_Xw", np.zeros((0, 3), np.float32)), np.float32).reshape(-1, 3).copy()
        M = len(mp_ref) if tail else 0
        Tcw = np.zeros((K, 16), np.float32)
        chi2 = np.zeros(max(E, 1), np.float64)
        its = int(prob["n_iterations"] if n_iterations is None else n_iterations)
        p = asd_essgraph_problem(K, E, sim3.ctypes.data, fixed.ctypes.data, e_i.ctypes.data, e_j.ctypes.data, e_meas.ctypes.data,
                                 int(prob["fix_scale"]), its, Tcw.ctypes.data if tail else None, M, mp_ref.ctypes.data, mp_Xw.ctypes.data)
        r = asd_essgraph_result(chi2.ctypes.data, 0.0, 0, 0)
        self._chk(self.lib.asd_optimize_essential_graph(self.ctx, C.byref(p), C.byref(r)))
        return dict(sim3=sim3, Tcw=Tcw, points=mp_Xw, edge_chi2=chi2[:E], chi2=r.chi2, iterations=int(r.iterations), trials=int(r.trials))

    def essgraph_forms(self):
        """[active vertices, free active vertices, active edges, tiles per side] -- asd_debug_essgraph_forms"""
        out = np.zeros(4, np.int32)
        self.lib.asd_debug_essgraph_forms.restype = C.c_int32
        self._chk(self.lib.asd_debug_essgraph_forms(self.ctx, _p(out)))
        return [int(v) for v in out]

    def essgraph_trials(self, cap=256):
        """trials per iteration of the last optimize_essential_graph -- asd_debug_essgraph_trials"""
        out = np.zeros(cap, np.int32)
        self.lib.asd_debug_essgraph_trials.restype = C.c_int32
        n = int(self.lib.asd_debug_essgraph_trials(self.ctx, _p(out), C.c_int32(cap)))
        return [int(v) for v in out[:min(n, cap)]]

    def gba_forms(self):
        """[dense solve 0 solve_lds / 1 chol_lds / 2 chol / 3 tiled / -1 none, nPf, nLa, Ea, tiles] -- asd_debug_gba_forms"""
        out = np.zeros(5, np.int32)
        self.lib.asd_debug_gba_forms.restype = C.c_int32
        self._chk(self.lib.asd_debug_gba_forms(self.ctx, _p(out)))
        return [int(v) for v in out]

    def gba_trials(self, cap=256):
        """trials per iteration of the last bundle_adjustment -- asd_debug_gba_trials"""
        out = np.zeros(cap, np.int32)
        self.lib.asd_debug_gba_trials.restype = C.c_int32
        n = int(self.lib.asd_debug_gba_trials(self.ctx, _p(out), C.c_int32(cap)))
        return [int(v) for v in out[:min(n, cap)]]

    def dense_solve(self, A, b, form, done=0, chol_ok_in=1, x0=None):
        """One dense SPD solve by the kernel of `form` (0 k_ba_solve_lds, 1 k_ba_chol_lds, 2 k_ba_chol, 3 tiled on MFMA, 4 tiled on
        plain FMA) -- asd_debug_dense_solve.  A: n x n f64, the lower triangle is the matrix; x0: what x holds on entry (default NaN).
        Returns dict(x, chol_ok, L): L = the matrix as the kernel left it for forms 2 .. 4, else None."""
        A = _c(A, np.float64)
        b = _c(b, np.float64).reshape(-1)
        n = int(A.shape[0]) if A.ndim == 2 else -1
        if A.ndim != 2 or A.shape[1] != n or len(b) != n:
            raise ValueError("dense_solve: A must be n x n and b of length n")
        x = np.full(max(n, 1), np.nan) if x0 is None else _c(x0, np.float64).reshape(-1).copy()
        if x0 is not None and len(x) != n:
            raise ValueError("dense_solve: x0 must have length n")
        L = np.empty((n, n), np.float64) if int(form) >= 2 else None
        ok = C.c_int32(-1)
        self.lib.asd_debug_dense_solve.restype = C.c_int32
        self._chk(self.lib.asd_debug_dense_solve(self.ctx, C.c_int32(int(form)), C.c_int32(n), _p(A), _p(b), C.c_int32(int(done)),
                                                 C.c_int32(int(chol_ok_in)), _p(L), _p(x), C.byref(ok)))
        return dict(x=x[:n], chol_ok=int(ok.value), L=L)

    def debug_prim(self, op, x, host=False, fused=False):
        """one primitive of se3.h / sim3_math.h on every row of x (see debug_prim below) -- asd_debug_prim"""
        return debug_prim(op, x, host=host, fused=fused, ctx=self)

    def local_ba_submit(self, prob, its_first=5, its_second=10):
        """LocalBundleAdjustment on the library's OPTIONAL lane: returns at once; local_ba_wait() returns the result dict.  One run
        at a time.  Not the reference's order -- Tracking.cc:797 -> LocalMapping.cc:89 runs it in line (local_ba above); frames tracked
        while a run is out read the pre-BA map."""
        p, r, keep = self._ba_pack(prob, its_first, its_second)
        self._chk(self.lib.asd_local_ba_submit(self.ctx, C.byref(p), C.byref(r)))
        self._ba_job = (p, r, keep)   # the library owns these until wait

    def local_ba_wait(self):
        rc = self.lib.asd_local_ba_wait(self.ctx)
        job, self._ba_job = getattr(self, "_ba_job", None), None
        self._chk(rc)
        p, r, keep = job
        return self._ba_unpack(r, keep)

    def local_ba_poll(self):
        return int(self.lib.asd_local_ba_poll(self.ctx))

    def tcw_to_pose7(self, T):
        T = _c(T, np.float32)
        p = np.zeros(7, np.float64)
        self.lib.asd_tcw_to_pose7(_p(T), _p(p))
        return p

    def pose7_to_tcw(self, p):
        p = _c(p, np.float64)
        T = np.zeros((4, 4), np.float32)
        self.lib.asd_pose7_to_tcw(_p(p), _p(T))
        return T
