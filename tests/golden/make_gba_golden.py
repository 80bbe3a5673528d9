#!/usr/bin/env python3
"""Generate tests/golden/gba_golden.npz: what the REFERENCE's own vendored g2o returns for Optimizer::BundleAdjustment
(Optimizer.cc:51-237) on the problems of CASES, for tests/test_gba_golden.py and tests/test_gba.py.

main() runs only in the build container (it needs the reference's sources).  It compiles the reference's 28 g2o sources plus
tests/golden/gba_ref_driver.cpp (ours) with the flags of oracle/ref_g2o/Makefile into a temporary directory outside the tree, TWICE:
as that Makefile does (-O2), and with -O2 -mfma -ffp-contract=fast.  Every case goes through three reference runs:
  (a) -O2, BlockSolverX + LinearSolverEigen -- the reference's own solver, the run the device is compared with;
  (b) the fma build, the same solver: another rounding of the same program;
  (c) -O2, BlockSolver_6_3 + LinearSolverDense: the same normal equations factored densely, as the device factors them.
S is the largest distance between the three runs over all cases, separately for quaternion, translation, points, chi2 (relative)
and the edges' chi2 (relative to max(chi2, 1)); the device is held to 4 x S against run (a).

Everything else in this module -- CASES, problem(), the digest -- is imported by the tests and needs nothing but numpy.

The generator fails if the three runs disagree on optimize()'s return or on the trials of any iteration, if g2o is not
deterministic (run (a) twice), if a case does not show the paths it names (PATHS), or if 4 x S exceeds 1e-6 (POINT_ATOL of
tests/test_optimizer.py, the loosest absolute BA tolerance of the suite).  A candidate that breaks a condition goes to DROPPED (at
most two); the conditions stay.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gba_golden.npz")

T = 16                 # pose blocks per tile of the tiled Cholesky (csrc/gba.h: kGbaTilePoses)
TOL_CAP = 1e-6         # 4 x S must not exceed POINT_ATOL
# Huber delta^2 as g2o holds it: delta = (float)sqrt(5.99) (Optimizer.cc:91), its square rounded to float (robust_kernel_impl.h:84)
DELTA2 = float(np.float32(float(np.float32(np.sqrt(5.99))) ** 2))
HUBER_MARGIN = 1e-3    # every stored chi2 of the Huber case is at least this far from delta^2, relative
BUILDS = (("O2", []), ("O2_fma", ["-mfma", "-ffp-contract=fast"]))
TRIALS_CAP = 64


def C(name, kw, its=20, robust=1, edit=None, paths=()):
    return dict(name=name, kw=kw, its=its, robust=robust, edit=edit, paths=list(paths))


INIT = dict(n_kf=2, n_free_points=120, seed=41)


def BAND(n_free, seed, **kw):
    return dict(dict(n_kf=n_free + 1, pts_per_kf=40, seed=seed), **kw)


# name, synth.gba_map kwargs, iterations, bRobust, post-edit, the paths g2o's own run must show (PATHS)
CASES = [
    C("init2_robust", INIT, paths=("iterates", "free1")),
    C("init2_plain", INIT, robust=0, paths=("iterates", "free1")),
    C("zero_edges", INIT, edit="no_edges", paths=("no_active",)),
    C("point_no_edges", INIT, edit="lone_point", paths=("iterates", "vertex_removed")),
    C("pose_no_edges", BAND(4, 42), edit="lone_pose", paths=("iterates",)),
    C("its0", BAND(4, 44), its=0, paths=("zero_iterations",)),
    C("far_start", BAND(6, 49, pose_sigma=0.3, point_sigma=1.5), paths=("iterates", "rejected")),
    C("outliers", BAND(8, 54, outlier_frac=0.3, outlier_px=(2.0, 9.0)), paths=("iterates", "huber_both")),
    C("duplicate", BAND(4, 47), edit="duplicate", paths=("iterates",)),
    C(f"band_{T - 1}", BAND(T - 1, 48), its=6, paths=("iterates",)),
    C(f"band_{T}", BAND(T, 49), its=6, paths=("iterates",)),
    C(f"band_{T + 1}", BAND(T + 1, 50), its=6, paths=("iterates",)),
    C(f"band_{2 * T + 1}", BAND(2 * T + 1, 51), its=6, paths=("iterates",)),
    C(f"band_{3 * T + 5}", BAND(3 * T + 5, 52), its=6, paths=("iterates",)),
    C("loop_20", BAND(20, 53, loop_points=30), its=6, paths=("iterates", "corner")),
    C("loop_40_plain", BAND(40, 54, loop_points=30), its=6, robust=0, paths=("iterates", "corner")),
]
# the problems whose time DESIGN.md quotes: tools/gba_times.py runs them on the device, `make_gba_golden.py --times` through the -O2
# build of g2o with the reference's solver
TIMING_CASES = [
    C("t_init2", INIT),
    C("t_kf128", dict(n_kf=128, pts_per_kf=100, seed=61, loop_points=60), its=10),
    C("t_kf1024", dict(n_kf=1024, pts_per_kf=100, seed=62, loop_points=60), its=10),
]
# candidates dropped because they broke a condition of the generator (at most two): (name, what broke)
DROPPED = [("all_fixed", "edges but no free pose: the reference's g2o does not return -1, it aborts on the assertion `_sizePoses > 0` of "
            "BlockSolver::resize (block_solver.hpp:75); the device refuses such a problem with ASD_ERR_INVALID (tests/test_gba.py)")]


def problem(case, synth):
    """synth.gba_map(**kw) and the case's post-edit: the flat arrays of asd_gba_problem"""
    pp = synth.gba_map(**case["kw"])
    edit = case["edit"]
    if edit == "no_edges":
        pp["e_point"], pp["e_pose"] = pp["e_point"][:0], pp["e_pose"][:0]
        pp["e_obs"], pp["e_info"] = pp["e_obs"][:0], pp["e_info"][:0]
    elif edit == "lone_point":      # one more point, in the middle of the id range, that nobody observes
        l = len(pp["points"]) // 2
        pp["points"] = np.insert(pp["points"], l, [0.3, -0.2, 7.0], axis=0)
        pp["e_point"] = (pp["e_point"] + (pp["e_point"] >= l)).astype(np.int32)
    elif edit == "lone_pose":       # one more free keyframe, in the middle of the id range, that observes nothing
        p = 2
        pp["poses"] = np.insert(pp["poses"], p, [0.0, 0.0, 0.0, 1.0, -0.9, 0.05, 0.02], axis=0)
        pp["fixed"] = np.insert(pp["fixed"], p, 0).astype(np.uint8)
        pp["e_pose"] = (pp["e_pose"] + (pp["e_pose"] >= p)).astype(np.int32)
    elif edit == "all_fixed":
        pp["fixed"] = np.ones_like(pp["fixed"])
    elif edit == "duplicate":       # the first observation of point 3 once more, one pixel off, next to the original
        k = int(np.flatnonzero(pp["e_point"] == 3)[0])
        for key in ("e_point", "e_pose", "e_obs", "e_info"):
            pp[key] = np.insert(pp[key], k + 1, pp[key][k], axis=0)
        pp["e_obs"][k + 1] += np.float32(1.0)
    else:
        assert edit is None, edit
    pp["n_iterations"] = np.int32(case["its"])
    pp["robust"] = np.int32(case["robust"])
    return pp


def problem_digest(pp):
    return hashlib.sha256(b"".join(np.ascontiguousarray(pp[k]).tobytes() for k in sorted(pp))).hexdigest()


def distances(a, b):
    """[quaternion, translation, points, chi2 (relative), edge chi2 (relative to max(chi2, 1): an edge's chi2 moves linearly with the
    estimates, the sum -- at a minimum -- does not)] between two runs' outputs; quaternions compared up to sign"""
    qa, qb = a["poses"][:, :4], b["poses"][:, :4]
    sgn = np.where((qa * qb).sum(1, keepdims=True) < 0, -1.0, 1.0)
    dq = float(np.abs(qa * sgn - qb).max()) if len(qa) else 0.0
    dt = float(np.abs(a["poses"][:, 4:] - b["poses"][:, 4:]).max()) if len(qa) else 0.0
    dp = float(np.abs(a["points"] - b["points"]).max()) if len(a["points"]) else 0.0
    dc = abs(a["chi2"] - b["chi2"]) / max(abs(b["chi2"]), 1e-300) if b["chi2"] != 0 or a["chi2"] != 0 else 0.0
    de = float((np.abs(a["edge_chi2"] - b["edge_chi2"]) / np.maximum(np.abs(b["edge_chi2"]), 1.0)).max()) if len(b["edge_chi2"]) else 0.0
    return np.array([dq, dt, dp, dc, de])


def trials_of(o):
    return [int(t) for t in o["trials"] if t >= 0]


def corner_pairs(pp):
    """points that connect one of the first two free poses with one of the last two"""
    free = np.flatnonzero(pp["fixed"] == 0)
    lo, hi = set(free[:2].tolist()), set(free[-2:].tolist())
    n = 0
    for l in np.unique(pp["e_point"]):
        ps = set(pp["e_pose"][pp["e_point"] == l].tolist())
        n += bool(ps & lo) and bool(ps & hi)
    return n


# what g2o's own run must show for a path; o = one run's outputs (dict of run()), pp = the problem
PATHS = {
    "iterates": lambda o, pp: o["info"][0] >= 1 and o["info"][0] == o["info"][1],
    "free1": lambda o, pp: int((pp["fixed"] == 0).sum()) == 1,
    "no_active": lambda o, pp: o["info"][0] == -1 and o["info"][1] == 0,   # "0 vertices to optimize" (sparse_optimizer.cpp:356-359)
    "vertex_removed": lambda o, pp: o["info"][3] == len(pp["poses"]) + len(pp["points"]) - 1,
    "no_free_pose": lambda o, pp: int((pp["fixed"] == 0).sum()) == 0,
    "zero_iterations": lambda o, pp: o["info"][0] == 0 and o["info"][1] == 0,
    "rejected": lambda o, pp: any(t > 1 for t in trials_of(o)),
    "huber_both": lambda o, pp: (o["edge_chi2"] > DELTA2).sum() >= 5 and (o["edge_chi2"] < DELTA2).sum() >= 5
    and float(np.abs(o["edge_chi2"] / DELTA2 - 1).min()) >= HUBER_MARGIN,
    "corner": lambda o, pp: corner_pairs(pp) >= 10,
}


def build_reference(tmp, extra):
    """the reference's g2o (the 28 sources and flags of oracle/ref_g2o/Makefile) + our driver -> tmp/libgba_ref.so"""
    ref = "/root/reference"
    g2o = f"{ref}/src/g2o_catkin"
    eigen = f"{ref}/src/3rd_party/eigen_catkin/eigen-eigen-b9cd8366d4e8"
    mk = open(os.path.join(ROOT, "oracle", "ref_g2o", "Makefile")).read()
    srcs = mk.split("SRCS_CPP =")[1].split("OBJS =")[0].replace("\\", " ").split()
    assert len(srcs) == 28, srcs   # the C++ sources of the reference's CMakeLists.txt (+ stuff/os_specific.c below)
    flags = ["-O2", *extra, "-fPIC", "-w"]
    inc = [f"-I{g2o}/include", f"-I{g2o}/include/g2o/core", f"-I{g2o}/include/g2o/types", f"-I{g2o}/include/g2o/stuff",
           f"-I{g2o}/include/g2o/solvers", f"-I{eigen}"]
    drv = os.path.join(ROOT, "tests", "golden", "gba_ref_driver.cpp")
    jobs = [(["g++", *flags, "-std=c++11", *inc, "-c", f"{g2o}/src/{s}", "-o", os.path.join(tmp, f"o{k}.o")]) for k, s in enumerate(srcs)]
    jobs.append(["gcc", *flags, f"-I{g2o}/include/g2o/stuff", "-c", f"{g2o}/src/stuff/os_specific.c", "-o", os.path.join(tmp, "os.o")])
    jobs.append(["g++", *flags, "-std=c++11", *inc, "-c", drv, "-o", os.path.join(tmp, "drv.o")])
    lib = os.path.join(tmp, "libgba_ref.so")
    if os.path.exists(lib) and os.path.getmtime(lib) > os.path.getmtime(drv):
        return ctypes.CDLL(lib)   # --build-dir: a build kept from an earlier run
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(subprocess.check_call, jobs))
    subprocess.check_call(["g++", "-shared", "-o", lib, *[j[-1] for j in jobs]])
    return ctypes.CDLL(lib)


def run(lib, pp, dense=False):
    dp, ip, bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)
    P, L, E = len(pp["poses"]), len(pp["points"]), len(pp["e_point"])
    poses = np.ascontiguousarray(pp["poses"], np.float64).reshape(-1, 7).copy()
    points = np.ascontiguousarray(pp["points"], np.float64).reshape(-1, 3).copy()
    fixed = np.ascontiguousarray(pp["fixed"], np.uint8)
    e_point, e_pose = np.ascontiguousarray(pp["e_point"], np.int32), np.ascontiguousarray(pp["e_pose"], np.int32)
    e_obs, e_info = np.ascontiguousarray(pp["e_obs"], np.float64), np.ascontiguousarray(pp["e_info"], np.float64)
    K = np.ascontiguousarray(pp["K"], np.float64)
    edge_chi2 = np.zeros(max(E, 1))
    info, trials, dout = np.zeros(4, np.int32), np.zeros(TRIALS_CAP, np.int32), np.zeros(2)
    fn = lib.gba_ref_dense if dense else lib.gba_ref_sparse
    fn.restype = ctypes.c_int
    rc = fn(ctypes.c_int(P), ctypes.c_int(L), ctypes.c_int(E), poses.ctypes.data_as(dp), fixed.ctypes.data_as(bp),
            points.ctypes.data_as(dp), e_point.ctypes.data_as(ip), e_pose.ctypes.data_as(ip), e_obs.ctypes.data_as(dp),
            e_info.ctypes.data_as(dp), K.ctypes.data_as(dp), ctypes.c_int(int(pp["n_iterations"])), ctypes.c_int(int(pp["robust"])),
            edge_chi2.ctypes.data_as(dp), info.ctypes.data_as(ip), trials.ctypes.data_as(ip), ctypes.c_int(TRIALS_CAP), dout.ctypes.data_as(dp))
    assert rc == 0
    return dict(poses=poses, points=points, edge_chi2=edge_chi2[:E], info=info, trials=trials, chi2=float(dout[0]), seconds=float(dout[1]))


def load_synth():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.load_package().synth


def main():
    assert os.path.isdir("/root/reference/src/g2o_catkin"), "the generator needs the reference's sources"
    assert len(DROPPED) <= 2
    synth = load_synth()
    # --build-dir DIR (outside the tree): keep the two builds there between runs while a case list is being searched
    keep_dir = sys.argv[sys.argv.index("--build-dir") + 1] if "--build-dir" in sys.argv else None
    assert keep_dir is None or not os.path.abspath(keep_dir).startswith(ROOT + os.sep), "the builds stay outside the tree"
    with tempfile.TemporaryDirectory() as tmp:
        tmp = keep_dir or tmp
        libs = []
        for tag, extra in BUILDS:
            d = os.path.join(tmp, tag)
            os.makedirs(d, exist_ok=True)
            libs.append(build_reference(d, extra))
        if "--times" in sys.argv:   # g2o -O2, the reference's solver, on TIMING_CASES: median and minimum; writes nothing
            for case in TIMING_CASES:
                pp = problem(case, synth)
                reps = 3 if len(pp["poses"]) > 500 else 9
                t = sorted(run(libs[0], pp)["seconds"] for _ in range(reps))
                o = run(libs[0], pp)
                print(f"g2o -O2 {case['name']}: poses {len(pp['poses'])} points {len(pp['points'])} edges {len(pp['e_point'])} | median "
                      f"{t[reps // 2] * 1e3:.2f} ms min {t[0] * 1e3:.2f} ms | iterations {o['info'][0]} trials {o['info'][2]}")
            return
        out = {"cases": np.array(json.dumps(CASES)), "dropped": np.array(json.dumps(DROPPED)), "builds": np.array(json.dumps(BUILDS)),
               "tile_poses": np.int32(T)}
        S = np.zeros(5)
        for i, case in enumerate(CASES):
            pp = problem(case, synth)
            a, b, c = run(libs[0], pp), run(libs[1], pp), run(libs[0], pp, dense=True)
            again = run(libs[0], pp)
            for k in ("poses", "points", "edge_chi2", "info", "trials"):
                assert np.array_equal(again[k], a[k]), f"{case['name']}: g2o is not deterministic ({k})"
            for tag, o in (("fma", b), ("dense", c)):
                assert o["info"][0] == a["info"][0] and np.array_equal(o["trials"], a["trials"]), \
                    f"{case['name']}: run ({tag}) disagrees on iterations / trials: {o['info']} {trials_of(o)} vs {a['info']} {trials_of(a)}"
            for tag, o in (("O2", a), ("fma", b), ("dense", c)):
                for path in case["paths"]:
                    assert PATHS[path](o, pp), f"{case['name']} ({tag}): g2o's run does not show {path}"
            dist = np.maximum(distances(b, a), distances(c, a))
            S = np.maximum(S, dist)
            out[f"c{i}_in_sha256"] = np.array(problem_digest(pp))
            for k in ("poses", "points", "edge_chi2", "info", "trials"):
                out[f"c{i}_{k}"] = a[k]
            out[f"c{i}_chi2"] = np.float64(a["chi2"])
            print(f"{case['name']:16s} P {len(pp['poses']):3d} L {len(pp['points']):4d} E {len(pp['e_point']):5d} ret {a['info'][0]:3d} "
                  f"trials {trials_of(a)} chi2 {a['chi2']:.6e} dist q {dist[0]:.1e} t {dist[1]:.1e} X {dist[2]:.1e} chi2 {dist[3]:.1e} edge {dist[4]:.1e} "
                  f"g2o {a['seconds'] * 1e3:.2f} ms")
        out["S"] = S
        print("S (quaternion, translation, points, chi2 relative, edge chi2):", " ".join(f"{v:.2e}" for v in S))
        assert 4 * S.max() <= TOL_CAP, f"4 x S = {4 * S.max():.2e} exceeds {TOL_CAP}"
        np.savez_compressed(GOLDEN, **out)
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
