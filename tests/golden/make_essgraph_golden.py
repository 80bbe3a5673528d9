#!/usr/bin/env python3
"""Generate tests/golden/essgraph_golden.npz: what the REFERENCE's own vendored g2o returns for Optimizer::OptimizeEssentialGraph
(Optimizer.cc:737-1000) on the problems of CASES, for tests/test_essgraph_golden.py, tests/test_essgraph_host.py and
tests/test_essgraph.py.

main() runs only in the build container (it needs the reference's sources).  It compiles the reference's 28 g2o sources plus
tests/golden/essgraph_ref_driver.cpp (ours) with the flags of oracle/ref_g2o/Makefile into a temporary directory outside the tree,
once per entry of make_gba_golden.BUILDS: as that Makefile does (-O2), and with -O2 -mfma -ffp-contract=fast.  Every case goes
through three reference runs:
  (a) -O2, BlockSolver_7_3 + LinearSolverEigen -- the reference's own solver, the run the device is compared with;
  (b) the fma build, the same solver: another rounding of the same program;
  (c) -O2, BlockSolver_7_3 + LinearSolverDense: the same normal equations factored densely, as the device factors them.
S is the largest distance between the three runs over all cases, separately for quaternion, translation, scale (relative), points,
chi2 (relative) and the edges' chi2 (relative to max(chi2, 1)); the device is held to 4 x S against run (a).

Everything else in this module -- CASES, problem(), edges_of(), abi_problem(), the digest -- is imported by the tests and needs
nothing but numpy.

Conditions (fixed, not measured): the three runs agree on optimize()'s return and on the trials of every iteration, and every
accept / reject of run (a) compares two chi2 that lie further apart than 4 x what either differs by between the runs (decided():
three runs can agree on a coin toss; the fourth arithmetic, the device's, then need not); run (a) twice is bit-identical; every case shows the paths it names (PATHS); S <= S_CAP = 2.5e-7, the cap of make_sim3_golden.py for the same
numeric Jacobians (4 x S <= 1e-6).  The Jacobians carry ~1e-7 of noise, so late iterations can be decided by rounding: a candidate
whose runs disagree on trials at 20 iterations, or agree without deciding, stands at the largest iteration count where they agree (`--search` prints it; the
count is the case's `its`), at least three cases stand at the full 20.  A candidate that breaks a condition at every count goes
to DROPPED (at most two); the conditions stay.
"""
import ctypes
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden", "essgraph_golden.npz")

TILE = 96              # rows per tile of the tiled Cholesky (csrc/gba.h: kGbaTile)
S_CAP = 2.5e-7         # S_CAP of make_sim3_golden.py: the device tolerance 4 x S stays <= 1e-6
TRIALS_CAP = 64
EVALS_CAP = 256        # chi2 evaluations of a run: one per iteration and one per trial, 20 x 11 at the most
MIN_FEAT = 100
FULL = 20              # the reference's iteration count (:943)
S_NAMES = ("quaternion", "translation", "scale", "points", "chi2", "edge_chi2")


def C(name, kw, its=FULL, edit=None, paths=()):
    return dict(name=name, kw=kw, its=its, edit=edit, paths=list(paths))


# name, synth.essential_graph kwargs, iterations, post-edit, the paths g2o's own run must show (PATHS)
CASES = [
    C("chain_3", dict(n_kf=3, seed=71, loop=False), edit="exact_poses", paths=("rho_zero",)),
    C("loop_8", dict(n_kf=8, seed=313, fix_scale=0), paths=("iterates", "rejected", "scale_moves")),
    C("loop_8_fix_scale", dict(n_kf=8, seed=201, fix_scale=1), its=3, paths=("iterates", "scale_kept")),
    C("drift_far", dict(n_kf=10, seed=216, drift=0.1), paths=("iterates", "rejected")),
    C("dup_pair", dict(n_kf=8, seed=215), edit="dup_pair", paths=("iterates", "duplicate")),
    C("lone_kf", dict(n_kf=9, seed=205), edit="lone_kf", paths=("iterates", "lone")),
    C("its0", dict(n_kf=8, seed=200), its=0, paths=("zero_iterations",)),
    C("no_edges", dict(n_kf=3, seed=77, loop=False), edit="no_edges", paths=("no_active",)),
    C("fixed_mid", dict(n_kf=8, seed=204), edit="fixed_mid", paths=("iterates", "fixed_mid")),
    C("tile_13", dict(n_kf=14, seed=208), paths=("iterates", "rejected", "tiles_1")),
    C("tile_14", dict(n_kf=15, seed=318), paths=("iterates", "rejected", "tiles_2")),
    C("tile_28", dict(n_kf=29, seed=218), paths=("iterates", "rejected", "tiles_3")),
    C("covis_40", dict(n_kf=40, seed=223, covis=4), paths=("iterates", "covis_rules")),
]
# the problems whose time DESIGN.md quotes: tools/essgraph_times.py runs them on the device, `make_essgraph_golden.py --times` through
# the -O2 build of g2o with the reference's solver
TIMING_CASES = [
    C("t_kf128", dict(n_kf=128, seed=91, covis=4)),
    C("t_kf1024", dict(n_kf=1024, seed=92, covis=4)),
]
# candidates dropped because they broke a condition of the generator at every iteration count (at most two): (name, what broke)
DROPPED = []

LIST_KEYS = (("child_start", "child"), ("loop_start", "loop"), ("cov_start", "cov"))


def _lists(start, flat):
    return [list(map(int, flat[start[i]:start[i + 1]])) for i in range(len(start) - 1)]


def _csr(lists):
    start = np.zeros(len(lists) + 1, np.int32)
    for i, l in enumerate(lists):
        start[i + 1] = start[i] + len(l)
    return start, np.array([v for l in lists for v in l], np.int32)


def problem(case, synth):
    """synth.essential_graph(**kw) and the case's post-edit: the flat keyframe views"""
    pp = synth.essential_graph(**case["kw"])
    K = len(pp["mnId"])
    edit = case["edit"]
    cur = int(pp["cur_kf"])
    if edit == "dup_pair":          # LoopConnections of pCurKF also names its parent (a strong covisible): the spanning-tree edge once more
        lc = _lists(pp["lc_start"], pp["lc"])
        m = list(pp["lc_kf"]).index(cur)
        lc[m].append(int(pp["parent"][cur]))
        pp["lc_start"], pp["lc"] = _csr(lc)
    elif edit == "exact_poses":     # no rotation, translations that are sums of a few powers of two: every Sji, and every error at the
        T = np.tile(np.eye(4, dtype=np.float32), (K, 1, 1))   # start, is exact -- chi2 is 0 in any arithmetic, not rounding noise
        for k in range(K):
            T[k, :3, 3] = (-0.25 * k, 0.125 * k, 0.5 * k)
        pp["Tcw"] = T.reshape(K, 16)
    elif edit == "lone_kf":         # the keyframe in the middle of the id range loses every link: its child goes to its parent
        r = K // 2
        parent = pp["parent"].copy()
        for c in range(K):
            if parent[c] == r:
                parent[c] = parent[r]
        parent[r] = -1
        pp["parent"] = parent
        pp["child_start"], pp["child"] = _csr([[c for c in range(K) if parent[c] == k] for k in range(K)])
        cov, cw = _lists(pp["cov_start"], pp["cov"]), _lists(pp["cov_start"], pp["cov_w"])
        for k in range(K):
            keep = [q for q, o in enumerate(cov[k]) if o != r and k != r]
            cov[k], cw[k] = [cov[k][q] for q in keep], [cw[k][q] for q in keep]
        pp["cov_start"], pp["cov"] = _csr(cov)
        pp["cov_w"] = _csr(cw)[1]
        # its child and its parent become covisibles of each other through the new tree edge
        assert r not in pp["loop"] and r not in pp["lc"] and r not in pp["lc_kf"]
    elif edit == "no_edges":
        pp["parent"] = np.full(K, -1, np.int32)
        for a, b in LIST_KEYS:
            pp[a], pp[b] = np.zeros(K + 1, np.int32), np.zeros(0, np.int32)
        pp["cov_w"] = np.zeros(0, np.int32)
    elif edit == "fixed_mid":       # pLoopKF is row 3: the fixed vertex is not the first one
        pp["loop_kf"] = np.int32(3)
        lc = pp["lc"].copy()
        lc[lc == 0] = 3
        pp["lc"] = lc
    else:
        assert edit is None, edit
    pp["n_iterations"] = np.int32(case["its"])
    return pp


def problem_digest(pp):
    return hashlib.sha256(b"".join(np.ascontiguousarray(pp[k]).tobytes() for k in sorted(pp))).hexdigest()


def edges_of(pp):
    """The edge list of Optimizer.cc:808-939 from the views, restated: [(row i, row j, kind)], and how often each rule dropped a
    candidate.  kind: 0 LoopConnections, 1 spanning tree, 2 loop edge, 3 covisibility."""
    K = len(pp["mnId"])
    mn = pp["mnId"]
    cov, cw = _lists(pp["cov_start"], pp["cov"]), _lists(pp["cov_start"], pp["cov_w"])
    child, loops = _lists(pp["child_start"], pp["child"]), _lists(pp["loop_start"], pp["loop"])
    lc = _lists(pp["lc_start"], pp["lc"])
    cur, lp = int(pp["cur_kf"]), int(pp["loop_kf"])
    hits = dict(lc_weak=0, lc_exempt=0, min_feat=0, parent=0, has_child=0, loop_edge=0, inserted=0, later_id=0)
    edges, inserted = [], set()
    for m, i in enumerate(map(int, pp["lc_kf"])):
        for j in lc[m]:
            w = dict(zip(cov[i], cw[i])).get(j, 0)
            if (i != cur or j != lp) and w < MIN_FEAT:
                hits["lc_weak"] += 1
                continue
            hits["lc_exempt"] += int(i == cur and j == lp and w < MIN_FEAT)
            edges.append((i, j, 0))
            inserted.add((min(mn[i], mn[j]), max(mn[i], mn[j])))
    for i in range(K):
        pa = int(pp["parent"][i])
        if pa >= 0:
            edges.append((i, pa, 1))
        for l in loops[i]:
            if mn[l] < mn[i]:
                edges.append((i, l, 2))
        for o, w in zip(cov[i], cw[i]):
            if w < MIN_FEAT:
                hits["min_feat"] += 1
                continue
            if o == pa:
                hits["parent"] += 1
            elif o in child[i]:
                hits["has_child"] += 1
            elif o in loops[i]:
                hits["loop_edge"] += 1
            elif not mn[o] < mn[i]:
                hits["later_id"] += 1
            elif (min(mn[i], mn[o]), max(mn[i], mn[o])) in inserted:
                hits["inserted"] += 1
            else:
                edges.append((i, o, 3))
    return edges, hits


def mp_rows(pp):
    """the row of the keyframe each map point is corrected through (the mnCorrectedByKF rule of :976-985)"""
    row_of = {int(v): r for r, v in enumerate(pp["mnId"])}
    by_cur = pp["mp_corrected_by"] == pp["mnId"][int(pp["cur_kf"])]
    return np.array([row_of[int(c)] if b else int(r) for b, c, r in zip(by_cur, pp["mp_corrected_ref"], pp["mp_ref"])], np.int32)


def abi_problem(pp, sim3_in, e_i, e_j, e_meas):
    """the flat arrays of asd_essgraph_problem from the views and an edge list with measurements"""
    K = len(pp["mnId"])
    fixed = np.zeros(K, np.uint8)
    fixed[int(pp["loop_kf"])] = 1
    return dict(sim3=np.array(sim3_in, np.float64).reshape(K, 8).copy(), fixed=fixed, e_i=np.array(e_i, np.int32), e_j=np.array(e_j, np.int32),
                e_meas=np.array(e_meas, np.float64).reshape(-1, 8).copy(), fix_scale=int(pp["fix_scale"]), n_iterations=int(pp["n_iterations"]),
                mp_ref=mp_rows(pp), mp_Xw=np.array(pp["mp_Xw"], np.float32).reshape(-1, 3).copy())


def free_active(pp, e_i, e_j):
    act = set(map(int, e_i)) | set(map(int, e_j))
    return len(act - {int(pp["loop_kf"])})


def distances(a, b):
    """[quaternion, translation, scale (relative), points, chi2 (relative), edge chi2 (relative to max(chi2, 1))] between two runs'
    outputs; quaternions compared up to sign"""
    if not len(a["sim3"]):
        return np.zeros(6)
    qa, qb = a["sim3"][:, :4], b["sim3"][:, :4]
    sgn = np.where((qa * qb).sum(1, keepdims=True) < 0, -1.0, 1.0)
    dq = float(np.abs(qa * sgn - qb).max())
    dt = float(np.abs(a["sim3"][:, 4:7] - b["sim3"][:, 4:7]).max())
    ds = float(np.abs(a["sim3"][:, 7] / b["sim3"][:, 7] - 1).max())
    dp = float(np.abs(a["points"].astype(np.float64) - b["points"].astype(np.float64)).max()) if len(a["points"]) else 0.0
    dc = abs(a["chi2"] - b["chi2"]) / max(abs(b["chi2"]), 1e-300) if b["chi2"] != 0 or a["chi2"] != 0 else 0.0
    de = float((np.abs(a["edge_chi2"] - b["edge_chi2"]) / np.maximum(np.abs(b["edge_chi2"]), 1.0)).max()) if len(b["edge_chi2"]) else 0.0
    return np.array([dq, dt, ds, dp, dc, de])


def decisions(o):
    """[(currentChi, tempChi)] of every Levenberg trial of a run, from the chi2 behind each computeActiveErrors"""
    ev, p, out = o["evals"], 0, []
    for q in trials_of(o):
        cur = ev[p]
        p += 1
        for _ in range(q):
            out.append((cur, ev[p]))
            if ev[p] < cur:
                cur = ev[p]
            p += 1
    assert p == int(o["info"][4]), (p, o["info"])
    return out


def decided(a, b, c):
    """every accept / reject of run (a) is decided by more than rounding: |currentChi - tempChi| is at least 4 x the largest
    difference of either value between the three runs (the device is held to 4 x S; a comparison closer than that is a coin)"""
    da, db, dc = decisions(a), decisions(b), decisions(c)
    return all(abs(cur - tmp) >= 4 * max(abs(x[k][j] - da[k][j]) for x in (db, dc) for j in (0, 1)) for k, (cur, tmp) in enumerate(da))


def trials_of(o):
    return [int(t) for t in o["trials"] if t >= 0]


def _tiles(o, pp):
    return (7 * free_active(pp, o["e_i"], o["e_j"]) + TILE - 1) // TILE


def _covis_rules(o, pp):
    edges, hits = edges_of(pp)
    return (sum(k == 3 for _, _, k in edges) >= 5 and sum(k == 2 for _, _, k in edges) >= 1 and
            all(hits[k] >= 1 for k in ("lc_weak", "lc_exempt", "min_feat", "parent", "has_child", "loop_edge", "inserted", "later_id")))


# what g2o's own run must show for a path; o = one run's outputs (dict of run()), pp = the views
PATHS = {
    "iterates": lambda o, pp: o["info"][0] >= 1 and o["info"][0] == o["info"][1],
    # the start is the optimum, exactly: the first trial leaves chi2 where it was, rho == 0, Terminate (levenberg.cpp:151-152)
    "rho_zero": lambda o, pp: o["info"][0] == 1 and trials_of(o) == [1] and o["chi2"] == 0.0 and np.array_equal(o["sim3"], o["sim3_in"]),
    "rejected": lambda o, pp: any(t > 1 for t in trials_of(o)),
    "scale_moves": lambda o, pp: float(np.abs(o["sim3"][:, 7] - o["sim3_in"][:, 7]).max()) > 1e-6,
    "scale_kept": lambda o, pp: np.array_equal(o["sim3"][:, 7], o["sim3_in"][:, 7]),
    "duplicate": lambda o, pp: len(set(zip(o["e_i"].tolist(), o["e_j"].tolist()))) < len(o["e_i"]),
    "lone": lambda o, pp: 0 < len(pp["mnId"]) // 2 < len(pp["mnId"]) - 1 and len(pp["mnId"]) // 2 not in set(o["e_i"].tolist()) | set(o["e_j"].tolist()),
    "zero_iterations": lambda o, pp: o["info"][0] == 0 and o["info"][1] == 0 and len(o["e_i"]) > 0,
    "no_active": lambda o, pp: o["info"][0] == -1 and o["info"][1] == 0 and len(o["e_i"]) == 0,
    "fixed_mid": lambda o, pp: int(pp["loop_kf"]) == 3 and np.array_equal(o["sim3"][3], o["sim3_in"][3]),
    "tiles_1": lambda o, pp: _tiles(o, pp) == 1 and 7 * free_active(pp, o["e_i"], o["e_j"]) == 91,
    "tiles_2": lambda o, pp: _tiles(o, pp) == 2 and 7 * free_active(pp, o["e_i"], o["e_j"]) == 98,
    "tiles_3": lambda o, pp: _tiles(o, pp) == 3 and 7 * free_active(pp, o["e_i"], o["e_j"]) == 196,
    "covis_rules": _covis_rules,
}


def build_reference(tmp, extra):
    """the reference's g2o (the 28 sources and flags of oracle/ref_g2o/Makefile) + our driver -> tmp/libessgraph_ref.so, as
    make_gba_golden.build_reference does"""
    import subprocess
    from concurrent.futures import ThreadPoolExecutor
    ref = "/root/reference"
    g2o = f"{ref}/src/g2o_catkin"
    eigen = f"{ref}/src/3rd_party/eigen_catkin/eigen-eigen-b9cd8366d4e8"
    mk = open(os.path.join(ROOT, "oracle", "ref_g2o", "Makefile")).read()
    srcs = mk.split("SRCS_CPP =")[1].split("OBJS =")[0].replace("\\", " ").split()
    assert len(srcs) == 28, srcs
    flags = ["-O2", *extra, "-fPIC", "-w"]
    inc = [f"-I{g2o}/include", f"-I{g2o}/include/g2o/core", f"-I{g2o}/include/g2o/types", f"-I{g2o}/include/g2o/stuff",
           f"-I{g2o}/include/g2o/solvers", f"-I{eigen}"]
    drv = os.path.join(ROOT, "tests", "golden", "essgraph_ref_driver.cpp")
    jobs = [(["g++", *flags, "-std=c++11", *inc, "-c", f"{g2o}/src/{s}", "-o", os.path.join(tmp, f"o{k}.o")]) for k, s in enumerate(srcs)]
    jobs.append(["gcc", *flags, f"-I{g2o}/include/g2o/stuff", "-c", f"{g2o}/src/stuff/os_specific.c", "-o", os.path.join(tmp, "os.o")])
    lib = os.path.join(tmp, "libessgraph_ref.so")
    if os.path.exists(lib) and os.path.getmtime(lib) > os.path.getmtime(drv):
        return ctypes.CDLL(lib)   # --build-dir: a build kept from an earlier run
    if all(os.path.exists(j[-1]) for j in jobs):
        jobs = []                 # --build-dir: only the driver changed
    jobs.append(["g++", *flags, "-std=c++11", *inc, "-c", drv, "-o", os.path.join(tmp, "drv.o")])
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(subprocess.check_call, jobs))
    objs = [os.path.join(tmp, f"o{k}.o") for k in range(len(srcs))] + [os.path.join(tmp, "os.o"), os.path.join(tmp, "drv.o")]
    subprocess.check_call(["g++", "-shared", "-o", lib, *objs])
    return ctypes.CDLL(lib)


def run(lib, pp, dense=False, its=None):
    K, M = len(pp["mnId"]), len(pp["mp_ref"])
    hdr = np.array([K, M, len(pp["lc_kf"]), int(pp["loop_kf"]), int(pp["cur_kf"]), int(pp["fix_scale"]),
                    int(pp["n_iterations"]) if its is None else its, int(dense)], np.int32)
    cap = 64 * max(K, 1)
    out = dict(e_i=np.zeros(cap, np.int32), e_j=np.zeros(cap, np.int32), e_meas=np.zeros((cap, 8)), sim3_in=np.zeros((K, 8)), sim3=np.zeros((K, 8)),
               Tiw=np.zeros((K, 16), np.float32), points=np.zeros((M, 3), np.float32), edge_chi2=np.zeros(cap), info=np.zeros(5, np.int32),
               trials=np.zeros(TRIALS_CAP, np.int32), dout=np.zeros(2), evals=np.zeros(EVALS_CAP))
    keys = ("mnId", "Tcw", "parent", "child_start", "child", "loop_start", "loop", "cov_start", "cov", "cov_w", "corrected", "corrected_sim3",
            "noncorrected", "noncorrected_sim3", "lc_kf", "lc_start", "lc", "mp_Xw", "mp_ref", "mp_corrected_by", "mp_corrected_ref")
    hold = [np.ascontiguousarray(pp[k]) for k in keys]
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    lib.essgraph_ref.restype = ctypes.c_int
    rc = lib.essgraph_ref(ptr(hdr), *[ptr(a) for a in hold], ctypes.c_int32(cap), ptr(out["e_i"]), ptr(out["e_j"]), ptr(out["e_meas"]),
                          ptr(out["sim3_in"]), ptr(out["sim3"]), ptr(out["Tiw"]), ptr(out["points"]), ptr(out["edge_chi2"]), ptr(out["info"]),
                          ptr(out["trials"]), ctypes.c_int32(TRIALS_CAP), ptr(out["dout"]), ptr(out["evals"]), ctypes.c_int32(EVALS_CAP))
    assert rc == 0, rc
    E = int(out["info"][3])
    for k in ("e_i", "e_j", "e_meas", "edge_chi2"):
        out[k] = out[k][:E].copy()
    out["chi2"], out["seconds"] = float(out["dout"][0]), float(out["dout"][1])
    return out


STORED = ("e_i", "e_j", "e_meas", "sim3_in", "sim3", "Tiw", "points", "edge_chi2", "info", "trials", "evals")


def agree(a, o):
    return o["info"][0] == a["info"][0] and np.array_equal(o["trials"], a["trials"])


def load_synth():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    return g.load_package().synth


def main():
    assert os.path.isdir("/root/reference/src/g2o_catkin"), "the generator needs the reference's sources"
    assert len(DROPPED) <= 2
    assert sum(c["its"] == FULL for c in CASES) >= 3
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from make_gba_golden import BUILDS
    synth = load_synth()
    # --build-dir DIR (outside the tree): keep the two builds there between runs while a case list is being searched
    keep_dir = sys.argv[sys.argv.index("--build-dir") + 1] if "--build-dir" in sys.argv else None
    assert keep_dir is None or not os.path.abspath(keep_dir).startswith(ROOT + os.sep), "the builds stay outside the tree"
    with tempfile.TemporaryDirectory() as tmp:
        tmp = keep_dir or tmp
        libs = []
        for tag, extra in BUILDS:
            d = os.path.join(tmp, "essgraph_" + tag)
            os.makedirs(d, exist_ok=True)
            libs.append(build_reference(d, extra))
        if "--times" in sys.argv:   # g2o -O2, the reference's solver, on TIMING_CASES: median and minimum; writes nothing
            for case in TIMING_CASES:
                pp = problem(case, synth)
                reps = 3 if len(pp["mnId"]) > 500 else 9
                t = sorted(run(libs[0], pp)["seconds"] for _ in range(reps))
                o = run(libs[0], pp)
                print(f"g2o -O2 {case['name']}: keyframes {len(pp['mnId'])} edges {len(o['e_i'])} | median {t[reps // 2] * 1e3:.2f} ms "
                      f"min {t[0] * 1e3:.2f} ms | iterations {o['info'][0]} trials {o['info'][2]}")
            return
        if "--search" in sys.argv:  # per case: the largest iteration count at which the three runs agree on return and trials
            for case in CASES:
                pp = problem(case, synth)
                best = None
                for its in range(FULL, -1, -1):
                    a, b, c = run(libs[0], pp, its=its), run(libs[1], pp, its=its), run(libs[0], pp, dense=True, its=its)
                    if agree(a, b) and agree(a, c) and decided(a, b, c):
                        best = its
                        break
                print(f"{case['name']:18s} its {case['its']:2d} largest agreeing count {best} trials {trials_of(a)}")
            return
        out = {"cases": np.array(json.dumps(CASES)), "dropped": np.array(json.dumps(DROPPED)), "builds": np.array(json.dumps(BUILDS)),
               "tile": np.int32(TILE), "s_names": np.array(json.dumps(S_NAMES))}
        S = np.zeros(6)
        for i, case in enumerate(CASES):
            pp = problem(case, synth)
            a, b, c = run(libs[0], pp), run(libs[1], pp), run(libs[0], pp, dense=True)
            again = run(libs[0], pp)
            for k in STORED:
                assert np.array_equal(again[k], a[k]), f"{case['name']}: g2o is not deterministic ({k})"
            for tag, o in (("fma", b), ("dense", c)):
                assert agree(a, o), f"{case['name']}: run ({tag}) disagrees on iterations / trials: {o['info']} {trials_of(o)} vs {a['info']} {trials_of(a)}"
                assert np.array_equal(o["e_i"], a["e_i"]) and np.array_equal(o["e_j"], a["e_j"])
            assert decided(a, b, c), f"{case['name']}: a trial of g2o's run is decided by rounding (see decided())"
            for tag, o in (("O2", a), ("fma", b), ("dense", c)):
                for path in case["paths"]:
                    assert PATHS[path](o, pp), f"{case['name']} ({tag}): g2o's run does not show {path}"
            assert [(i_, j_) for i_, j_, _ in edges_of(pp)[0]] == list(zip(a["e_i"].tolist(), a["e_j"].tolist())), case["name"]
            dist = np.maximum(distances(b, a), distances(c, a))
            S = np.maximum(S, dist)
            out[f"c{i}_in_sha256"] = np.array(problem_digest(pp))
            for k in STORED:
                out[f"c{i}_{k}"] = a[k]
            out[f"c{i}_chi2"] = np.float64(a["chi2"])
            print(f"{case['name']:18s} K {len(pp['mnId']):3d} E {len(a['e_i']):4d} ret {a['info'][0]:3d} trials {trials_of(a)} chi2 {a['chi2']:.6e} dist "
                  + " ".join(f"{n[:5]} {v:.1e}" for n, v in zip(S_NAMES, dist)) + f" g2o {a['seconds'] * 1e3:.2f} ms")
        out["S"] = S
        print("S:", " ".join(f"{n} {v:.2e}" for n, v in zip(S_NAMES, S)))
        assert S.max() <= S_CAP, f"S = {S.max():.2e} exceeds the cap {S_CAP}"
        np.savez_compressed(GOLDEN, **out)
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
