#!/usr/bin/env python3
"""Generate tests/golden/sim3_golden.npz: what the REFERENCE's own vendored g2o returns for Optimizer::OptimizeSim3
(Optimizer.cc:1002-1194) on the problems of CASES, for tests/test_sim3_golden.py and tests/test_sim3_opt.py.

main() runs only in the build container (it needs the reference's sources).  It compiles the reference's 28 g2o sources plus
tests/golden/sim3_ref_driver.cpp (ours) with the flags of oracle/ref_g2o/Makefile into a temporary directory outside the tree, TWICE:
as that Makefile does (-O2), and with -O2 -mfma -ffp-contract=fast.  The edge classes of OptimizeSim3 have no analytic Jacobian, so
g2o differentiates numerically with delta = 1e-9 and the second round ends at the differencing noise floor: two roundings of the same
program differ by far more than the 1e-8 of the pose solvers.  The distance between the two builds, S (largest over the cases, per
Sim3 component, scale relative), is what the device is held to: 4 x S against the -O2 build (tests/test_sim3_opt.py).

Everything else in this module -- CASES, problem(), the digest -- is imported by the tests and needs nothing but numpy.

The generator fails if a case does not take the path it names in g2o's own run (PATHS), if the two builds disagree on keep / nIn /
nBad / the early return, if a chi2 that a re-classification read lies within GATE_MARGIN of th2 in either build, or if S exceeds
S_CAP.
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "sim3_golden.npz")

TH2 = 10.0            # LoopClosing.cc:362
GATE_MARGIN = 1e-3    # relative distance of every re-classified chi2 from th2, in both builds
S_CAP = 2.5e-7        # two-build distance: the device tolerance 4 x S stays <= 1e-6
BUILDS = (("O2", []), ("O2_fma", ["-mfma", "-ffp-contract=fast"]))
WORKGROUP = 256       # threads of k_sim3_opt (csrc/sim3.hip): the sizes 255 / 256 / 257 are one pass, one full pass, one pass + 1


def C(name, n, seed, outlier_frac=0.1, start_sigma=0.02, fix_scale=0, edit=None, paths=()):
    return dict(name=name, n=n, seed=seed, outlier_frac=outlier_frac, start_sigma=start_sigma, fix_scale=fix_scale, edit=edit,
                paths=list(paths))


# name, size, seed, outlier fraction, start distance, fix_scale, post-edit, the paths g2o's own run must show (PATHS)
CASES = [
    C("n0", 0, 300, 0.0, paths=("empty",)),
    C("n9", 9, 301, 0.0, paths=("early", "no_drop")),
    C("n10", 10, 302, 0.0, paths=("round2", "no_drop", "cap5")),
    C("n11", 11, 303, 0.0, paths=("round2", "no_drop", "cap5")),
    C("n11_fix", 11, 304, 0.0, fix_scale=1, paths=("round2",)),
    C("drop_to_9", 12, 305, 0.25, paths=("early", "drop")),
    C("n63", 63, 306, paths=("round2", "drop", "cap10")),
    C("n64", 64, 307, paths=("round2", "drop", "cap10")),
    C("n64_fix", 64, 308, fix_scale=1, paths=("round2", "drop", "cap10")),
    C("n65", 65, 309, paths=("round2", "drop", "cap10")),
    C("n255", 255, 310, paths=("round2", "drop", "cap10")),
    C("n256", 256, 311, paths=("round2", "drop", "cap10")),
    C("n257", 257, 312, paths=("round2", "drop", "cap10")),
    C("n257_fix", 257, 313, fix_scale=1, paths=("round2", "drop", "cap10")),
    C("n600", 600, 314, paths=("round2", "drop", "cap10")),
    C("n600_fix", 600, 315, fix_scale=1, paths=("round2", "drop", "cap10")),
    C("n2000", 2000, 316, paths=("round2", "drop", "cap10")),
    C("clean_300", 300, 317, 0.0, paths=("round2", "no_drop", "cap5")),
    C("all_outliers", 50, 318, 1.0, paths=("early", "all_dropped")),
    C("far_start", 300, 319, 0.1, 0.4, paths=("round2", "rejected_r1")),
    C("far_start_fix", 300, 320, 0.1, 0.4, fix_scale=1, paths=("round2", "drop")),
    C("hard_40", 40, 504, 0.5, 0.8, paths=("round2", "drop", "cap10", "rejected_r1", "its_gt5")),
    # outliers only 3-6 px off: their chi2 lands on both sides of th2, within a few percent of it (still >= GATE_MARGIN away)
    C("near_gate_200", 200, 341, 0.5, edit="near", paths=("round2", "drop", "near_gate")),
    C("near_gate_65_fix", 65, 342, 0.5, fix_scale=1, edit="near", paths=("round2", "drop", "near_gate")),
    C("K1_ne_K2", 200, 321, edit="K2", paths=("round2", "drop")),
    C("behind_100", 100, 322, 0.0, edit="behind", paths=("round2", "drop")),
]
# the two problems whose time DESIGN.md section 4 quotes: tools/sim3_times.py runs them on the device, `make_sim3_golden.py --times`
# through the -O2 build of g2o
TIMING_CASES = [C("t100", 100, 331), C("t2000", 2000, 316)]
# candidates dropped because a chi2 sits within GATE_MARGIN of th2 in one of the builds (at most two): (name, seed, margin)
DROPPED = []


# ---- Sim3 as (q xyzw, t, s), plain numpy (problem construction only: no test compares against these)
def q_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def q_rot(q, X):
    u = 2 * np.cross(q[:3], X)
    return X + q[3] * u + np.cross(q[:3], u)


def q_from_rotvec(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([np.sin(th / 2) * w / th, [np.cos(th / 2)]])


def sim3_map(S, X):
    return S[7] * q_rot(S[:4], X) + S[4:7]


def sim3_inv(S):
    qc = S[:4] * np.array([-1.0, -1.0, -1.0, 1.0])
    return np.concatenate([qc, q_rot(qc, -S[4:7] / S[7]), [1.0 / S[7]]])


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def project(K, X):
    return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)


def problem(case):
    """the flat arrays of asd_optimize_sim3 for a case; every draw comes from the case's own seeded stream"""
    rng = np.random.default_rng(case["seed"])
    n, fix = case["n"], case["fix_scale"]
    K1 = f32([718.856, 718.856, 607.1928, 185.2157])
    K2 = f32([707.0912, 709.5, 601.8873, 183.1104]) if case["edit"] == "K2" else K1.copy()
    s_true = 1.0 if fix else float(np.exp(rng.normal(0, 0.1)))
    truth = np.concatenate([q_from_rotvec(rng.normal(0, 0.08, 3)), rng.normal(0, 0.3, 3), [s_true]])
    X1 = np.stack([rng.uniform(-3, 3, n), rng.uniform(-1.2, 1.2, n), rng.uniform(4, 12, n)], 1)
    inv = sim3_inv(truth)
    X2 = np.array([sim3_map(inv, x) for x in X1]).reshape(n, 3)
    obs1 = project(K1, X1) + rng.normal(0, 0.7, (n, 2))
    obs2 = project(K2, X2) + rng.normal(0, 0.7, (n, 2))
    n_out = int(round(case["outlier_frac"] * n))
    bad = rng.permutation(n)[:n_out]
    lo, hi = (3, 6) if case["edit"] == "near" else (15, 60)
    shift = rng.uniform(lo, hi, (n_out, 2)) * rng.choice([-1.0, 1.0], (n_out, 2))
    side = rng.integers(0, 2, n_out).astype(bool)     # which image carries the wrong observation
    obs1[bad[side]] += shift[side]
    obs2[bad[~side]] += shift[~side]
    levels = 1.2 ** -(2.0 * np.arange(8))            # eight information values, as mvInvLevelSigma2 of an 8-level pyramid
    is1 = f32(levels)[rng.integers(0, 8, n)]
    is2 = f32(levels)[rng.integers(0, 8, n)]
    P1c, P2c = f32(X1), f32(X2)
    if case["edit"] == "behind":                      # three points behind camera 1 (z < 0, not 0) through S12
        P2c[:3] = -P2c[:3]
    d = rng.normal(0, case["start_sigma"], 7)
    if fix:
        d[6] = 0.0
    start = np.concatenate([q_mul(q_from_rotvec(d[:3]), truth[:4]), truth[4:7] + d[3:6], [truth[7] * np.exp(d[6])]])
    return dict(sim3=start, P1c=P1c, P2c=P2c, obs1=f32(obs1), obs2=f32(obs2), inv_sigma2_1=is1, inv_sigma2_2=is2, K1=K1, K2=K2,
                th2=np.float32(TH2), fix_scale=np.int32(fix))


def problem_digest(pp):
    return hashlib.sha256(b"".join(np.ascontiguousarray(pp[k]).tobytes() for k in sorted(pp))).hexdigest()


def sim3_distance(a, b):
    """per component, the scale relative to b's"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    d[7] /= abs(b[7])
    return d


def rounds_of(info, trials):
    """[(active edges, optimize()'s return, ended on a rejected trial, trials per iteration)] of the rounds that ran"""
    out = []
    for r in range(2):
        if info[2 + 3 * r] >= 0:
            out.append(dict(active=int(info[2 + 3 * r]), ret=int(info[3 + 3 * r]), ends_rejected=int(info[4 + 3 * r]),
                            trials=[int(t) for t in trials[r] if t >= 0]))
    return out


# what g2o's own run must show for a path; o = one build's outputs (dict of run())
PATHS = {
    "empty": lambda o, n: o["n_in"] == 0 and o["info"][1] == 1 and o["info"][3] == -1,
    "early": lambda o, n: o["info"][1] == 1 and o["info"][5] == -1,
    "round2": lambda o, n: o["info"][1] == 0 and o["info"][6] > 0,
    "no_drop": lambda o, n: o["info"][0] == 0,
    "drop": lambda o, n: o["info"][0] > 0,
    "all_dropped": lambda o, n: o["info"][0] == n,
    "cap5": lambda o, n: o["info"][0] == 0 and o["info"][6] <= 5,
    "cap10": lambda o, n: o["info"][0] > 0 and o["info"][6] <= 10,
    "rejected_r1": lambda o, n: any(t > 1 for t in o["trials"][0] if t >= 0),
    "near_gate": lambda o, n: o["margin"] <= 0.05,   # some chi2 a re-classification read is within 5 % of th2
    "its_gt5": lambda o, n: o["info"][6] > 5,      # the cap of 10 is not only chosen but used
}
# Reported, not required.  A round ends on a rejected trial only through ten rejections in a row (or rho == 0), and by the tenth the
# damping has grown by 2^45: the rejected estimate is then, bit for bit, the one it is popped back to.  No problem tried here (the
# case list and some six hundred seeded variants of it) left stored errors that differ from the errors at the final estimate, so the
# fixture makes no claim about that path; "trials_10" lists the cases whose last iteration took all ten trials.
AXES = {
    "ends_rejected_r1": lambda o, n: o["info"][4] == 1,
    "ends_rejected_r2": lambda o, n: o["info"][7] == 1,
    "trials_10": lambda o, n: 10 in list(o["trials"][0]) + list(o["trials"][1]),
}


def build_reference(tmp, extra):
    """the reference's g2o (the 28 sources and flags of oracle/ref_g2o/Makefile) + our driver -> tmp/libsim3_ref.so"""
    ref = "/root/reference"
    g2o = f"{ref}/src/g2o_catkin"
    eigen = f"{ref}/src/3rd_party/eigen_catkin/eigen-eigen-b9cd8366d4e8"
    mk = open(os.path.join(ROOT, "oracle", "ref_g2o", "Makefile")).read()
    srcs = mk.split("SRCS_CPP =")[1].split("OBJS =")[0].replace("\\", " ").split()
    assert len(srcs) == 28, srcs   # the C++ sources of the reference's CMakeLists.txt (+ stuff/os_specific.c below)
    flags = ["-O2", *extra, "-fPIC", "-w"]
    inc = [f"-I{g2o}/include", f"-I{g2o}/include/g2o/core", f"-I{g2o}/include/g2o/types", f"-I{g2o}/include/g2o/stuff",
           f"-I{g2o}/include/g2o/solvers", f"-I{eigen}"]
    jobs = [(["g++", *flags, "-std=c++11", *inc, "-c", f"{g2o}/src/{s}", "-o", os.path.join(tmp, f"o{k}.o")]) for k, s in enumerate(srcs)]
    jobs.append(["gcc", *flags, f"-I{g2o}/include/g2o/stuff", "-c", f"{g2o}/src/stuff/os_specific.c", "-o", os.path.join(tmp, "os.o")])
    jobs.append(["g++", *flags, "-std=c++11", *inc, "-c", os.path.join(ROOT, "tests", "golden", "sim3_ref_driver.cpp"), "-o", os.path.join(tmp, "drv.o")])
    lib = os.path.join(tmp, "libsim3_ref.so")
    if os.path.exists(lib) and os.path.getmtime(lib) > os.path.getmtime(os.path.join(ROOT, "tests", "golden", "sim3_ref_driver.cpp")):
        return ctypes.CDLL(lib)   # --build-dir: a build kept from an earlier run
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(subprocess.check_call, jobs))
    subprocess.check_call(["g++", "-shared", "-o", lib, *[j[-1] for j in jobs]])
    return ctypes.CDLL(lib)


def run(lib, pp):
    n = len(pp["P1c"])
    dp = ctypes.POINTER(ctypes.c_double)
    arr = lambda k: np.ascontiguousarray(pp[k], np.float64)
    sim3 = arr("sim3").copy()
    keep = np.zeros(max(n, 1), np.uint8)
    info, trials, dinfo = np.zeros(8, np.int32), np.zeros((2, 10), np.int32), np.zeros(2)
    ins = [arr(k) for k in ("P1c", "P2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "K1", "K2")]
    lib.sim3_ref_optimize.restype = ctypes.c_int
    n_in = lib.sim3_ref_optimize(sim3.ctypes.data_as(dp), ctypes.c_int(n), *[a.ctypes.data_as(dp) for a in ins],
                                 ctypes.c_float(float(pp["th2"])), ctypes.c_int(int(pp["fix_scale"])),
                                 keep.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), info.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                 trials.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), dinfo.ctypes.data_as(dp))
    return dict(sim3=sim3, keep=keep[:n], n_in=int(n_in), info=info, trials=trials, margin=float(dinfo[0]), seconds=float(dinfo[1]))


def main():
    assert os.path.isdir("/root/reference/src/g2o_catkin"), "the generator needs the reference's sources"
    assert len(DROPPED) <= 2
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
        if "--times" in sys.argv:   # g2o -O2 on TIMING_CASES: median and minimum of 15 runs; writes nothing
            for case in TIMING_CASES:
                pp = problem(case)
                t = sorted(run(libs[0], pp)["seconds"] for _ in range(15))
                o = run(libs[0], pp)
                print(f"g2o -O2 n={case['n']}: median {t[7] * 1e3:.2f} ms min {t[0] * 1e3:.2f} ms | n_in {o['n_in']} nBad {o['info'][0]} "
                      f"iterations {[r['ret'] for r in rounds_of(o['info'], o['trials'])]}")
            return
        out = {"cases": np.array(json.dumps(CASES)), "dropped": np.array(json.dumps(DROPPED)), "builds": np.array(json.dumps(BUILDS))}
        S = np.zeros(8)
        met = {a: [] for a in AXES}
        for i, case in enumerate(CASES):
            pp = problem(case)
            res = [run(lib, pp) for lib in libs]
            again = run(libs[0], pp)
            assert np.array_equal(again["sim3"], res[0]["sim3"]) and np.array_equal(again["keep"], res[0]["keep"]), f"{case['name']}: g2o is not deterministic"
            a, b = res
            for k in ("keep",):
                assert np.array_equal(a[k], b[k]), f"{case['name']}: the builds disagree on {k}"
            assert a["n_in"] == b["n_in"] and a["info"][0] == b["info"][0] and a["info"][1] == b["info"][1], f"{case['name']}: the builds disagree"
            for tag, o in zip(("O2", "O2_fma"), res):
                assert o["margin"] >= GATE_MARGIN, f"{case['name']} ({tag}): a chi2 is {o['margin']:.2e} from the gate"
                for path in case["paths"]:
                    assert PATHS[path](o, case["n"]), f"{case['name']} ({tag}): g2o's run does not show {path}"
            if case["fix_scale"] and not a["info"][1]:
                assert a["sim3"][7] == pp["sim3"][7] and b["sim3"][7] == pp["sim3"][7], f"{case['name']}: g2o moved a fixed scale"
            dist = sim3_distance(b["sim3"], a["sim3"])
            S = np.maximum(S, dist)
            for ax, f in AXES.items():
                if f(a, case["n"]) and f(b, case["n"]):
                    met[ax].append(case["name"])
            out[f"c{i}_in_sha256"] = np.array(problem_digest(pp))
            for tag, o in zip(("a", "b"), res):
                for k in ("sim3", "keep", "info", "trials"):
                    out[f"c{i}_{tag}_{k}"] = o[k]
                out[f"c{i}_{tag}_n_in"] = np.int32(o["n_in"])
                out[f"c{i}_{tag}_margin"] = np.float64(o["margin"])
            seconds = min(run(libs[0], pp)["seconds"] for _ in range(3))   # printed, not stored: the fixture holds no wall-clock value
            print(f"{case['name']:14s} n {case['n']:5d} nIn {a['n_in']:5d} nBad {a['info'][0]:4d} early {a['info'][1]} margin {min(a['margin'], b['margin']):.1e} "
                  f"two-build {dist.max():.1e} g2o {seconds * 1e3:.2f} ms | " +
                  " | ".join(f"{ra['active']} it {ra['ret']}/{rb['ret']} tr {ra['trials']}{' END-REJ' if ra['ends_rejected'] else ''}"
                             for ra, rb in zip(rounds_of(a["info"], a["trials"]), rounds_of(b["info"], b["trials"]))))
        for ax in AXES:
            print(f"axis {ax}: {met[ax]}")
        out["axes"] = np.array(json.dumps(met))
        out["S"] = np.float64(S.max())
        out["S_comp"] = S
        print("S per component:", " ".join(f"{v:.2e}" for v in S))
        assert S.max() <= S_CAP, f"two-build distance {S.max():.2e} exceeds the cap"
        np.savez_compressed(GOLDEN, **out)
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
