#!/usr/bin/env python3
"""Generate tests/golden/pose_paths_golden.npz: what the REFERENCE's own vendored g2o (compiled in place by oracle/ref_g2o/Makefile,
output in oracle/_ref/, never committed) returns on PoseOptimization problems shaped to take every edge-store form and every
round / Levenberg path of asd_pose_optimize (tests/test_pose_paths.py).

Runs only in the build container.  Each problem is synth.pose_problem(**kw) followed by the named post-edit of problem() below,
which the tests share.  The fixture stores the case list, a digest of every problem's inputs, g2o's pose, flags and inlier count,
g2o's per-round trace (oracle/ref_g2o/driver.cpp, ref_pose_optimize_trace) and the oracle-to-g2o pose distance measured here.

The generator checks from g2o's own trace that every case takes the paths it names (PATHS) and has the shape that selects its
store (store_of restates the host's rule), that no edge chi2 read by a re-classification lies within GATE_MARGIN of 5.991, and
that oracle and g2o agree (flags, inlier count, pose within ORACLE_TOL).  It fails otherwise.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402
from tests.golden.make_live_golden import problem_digest  # noqa: E402

GATE_MARGIN = 1e-6    # relative distance of every re-classified chi2 from 5.991
ORACLE_TOL = 1e-9     # a case on which two fp64 implementations differ by more is not admitted
TRIAL_MARGIN = 1e-8   # an accept / reject that changes the robust chi2 by less (relative) is decided by rounding
NBAD_MARGIN = 1e-6    # the same for (iniChi - currentChi) * 1e3 < iniChi
LDS_BYTES = 150 * 1024


def P(n, seed, outlier_frac=0.1, pose_sigma=0.02):
    return dict(n=n, seed=seed, outlier_frac=outlier_frac, pose_sigma=pose_sigma)


# name, synth.pose_problem kwargs, post-edit, the store the case must take (2 compact LDS / 1 full f64 LDS / 0 global), the paths
# g2o's trace must show (PATHS)
CASES = [
    # ---- store: last LDS size and first global size of each form, and the largest frame
    dict(name="compact_4388", kw=P(4388, 201), edit=None, store=2, paths=()),
    dict(name="compact_4389", kw=P(4389, 202), edit=None, store=0, paths=()),
    dict(name="f64obs_3071", kw=P(3071, 203), edit="f64obs", store=1, paths=()),
    dict(name="f64obs_3072", kw=P(3072, 204), edit="f64obs", store=0, paths=()),
    dict(name="info17_1500", kw=P(1500, 205), edit="info17", store=1, paths=()),
    dict(name="info17_3500", kw=P(3500, 206), edit="info17", store=0, paths=()),
    dict(name="big_9000", kw=P(9000, 207), edit=None, store=0, paths=()),
    # ---- pass geometry: one pass of the 512 threads, the wave early exit, the tail iteration; n % 8 != 0 in every store
    dict(name="n511", kw=P(511, 211), edit=None, store=2, paths=()),
    dict(name="n512", kw=P(512, 212), edit=None, store=2, paths=()),
    dict(name="n513", kw=P(513, 213), edit=None, store=2, paths=()),
    dict(name="n575", kw=P(575, 214), edit=None, store=2, paths=()),
    dict(name="n576", kw=P(576, 215), edit=None, store=2, paths=()),
    dict(name="n577", kw=P(577, 216), edit=None, store=2, paths=()),
    dict(name="n1023", kw=P(1023, 217), edit=None, store=2, paths=()),
    dict(name="n1025", kw=P(1025, 218), edit=None, store=2, paths=()),
    dict(name="n1025_f64obs", kw=P(1025, 219), edit="f64obs", store=1, paths=()),
    # ---- round structure
    dict(name="clean", kw=P(300, 62, 0.0, 0.0), edit=None, store=2, paths=("skip_both",)),
    dict(name="steady", kw=P(300, 2, 0.1, 0.02), edit=None, store=2, paths=("skip_r2",)),
    dict(name="far_start", kw=P(500, 63, 0.1, 0.3), edit=None, store=2,
         paths=("no_skip", "changed_r2", "reinlier", "its10", "rejected_mid", "active4")),
    dict(name="all_outliers", kw=P(300, 60, 1.0, 0.02), edit=None, store=2, paths=()),
    # ---- Levenberg exits: ten rejected trials / a round that ends on a rejected trial (n = 400, 20 % outliers, sigma 0.25)
    *[dict(name=f"reject_{s}", kw=P(400, s, 0.2, 0.25), edit=None, store=2, paths=()) for s in (71, 72, 73, 77, 80, 86, 88, 89)],
    *[dict(name=f"reject_mid_{s}", kw=P(400, s, 0.2, 0.25), edit=None, store=2, paths=()) for s in (74, 76, 79)],
    # ---- empty / tiny
    dict(name="gated_all", kw=P(500, 63, 0.1, 0.4), edit=None, store=2, paths=("no_active",)),
    dict(name="same_point", kw=P(300, 64), edit="same_point", store=2, paths=("no_active",)),
    dict(name="n2", kw=P(2, 221), edit=None, store=-1, paths=("none",)),
    dict(name="n3", kw=P(3, 222), edit=None, store=2, paths=("one_round",)),
    dict(name="n9", kw=P(9, 223), edit=None, store=2, paths=("one_round",)),
    dict(name="n10", kw=P(10, 224), edit=None, store=2, paths=("four_rounds",)),
    dict(name="n11", kw=P(11, 225), edit=None, store=2, paths=("four_rounds",)),
    # ---- conditioning
    dict(name="collinear", kw=P(300, 231, 0.0, 0.0), edit="collinear", store=2, paths=()),
    dict(name="zero_info5", kw=P(300, 232), edit="zero_info5", store=2, paths=()),
    dict(name="info_1e-6", kw=P(300, 233), edit="info_1e-6", store=2, paths=("skip_both",)),
    dict(name="behind", kw=P(300, 33), edit="behind", store=2, paths=()),
    dict(name="sigma_0.1", kw=P(300, 234, 0.1, 0.1), edit=None, store=2, paths=()),
    dict(name="sigma_0.2", kw=P(300, 235, 0.1, 0.2), edit=None, store=2, paths=()),
    dict(name="sigma_0.3", kw=P(300, 236, 0.1, 0.3), edit=None, store=2, paths=()),
]
# candidates dropped because oracle and g2o differ by more than ORACLE_TOL on them (at most two): (name, kw, edit, distance)
DROPPED = []


def quat_rotate(q, X):
    u = 2 * np.cross(q[:3], X)
    return X + q[3] * u + np.cross(q[:3], u)


def problem(case, synth):
    """synth.pose_problem(**kw) and the case's post-edit (every draw comes from a seeded stream of the case's own)"""
    pp = synth.pose_problem(**case["kw"])
    edit = case["edit"]
    rng = np.random.default_rng(2000 + case["kw"]["seed"])
    if edit == "f64obs":       # observations no longer exact in f32: the compact store cannot hold them
        pp["obs"] = pp["obs"] + rng.uniform(-1e-9, 1e-9, pp["obs"].shape)
    elif edit == "info17":     # more than 16 distinct information values
        pp["info"] = pp["info"] * (1.0 + 1e-3 * rng.integers(0, 40, pp["info"].shape))
    elif edit == "same_point":
        pp["Xw"][:] = pp["Xw"][0]
    elif edit == "collinear":  # every point on one line through the scene, observed where the input pose projects it (+- 0.5 px)
        s = np.linspace(0.0, 1.0, len(pp["Xw"]))[:, None]
        pp["Xw"] = (pp["Xw"][0] + s * (pp["Xw"][1] - pp["Xw"][0])).astype(np.float32).astype(np.float64)
        Xc = np.array([quat_rotate(pp["pose"][:4], X) for X in pp["Xw"]]) + pp["pose"][4:]
        fx, fy, cx, cy = pp["K"]
        uv = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1) + rng.uniform(-0.5, 0.5, (len(Xc), 2))
        pp["obs"] = uv.astype(np.float32).astype(np.float64)
    elif edit == "zero_info5":
        pp["info"][:5] = 0.0
    elif edit == "info_1e-6":
        pp["info"] = pp["info"] * 1e-6
    elif edit == "behind":     # negative depth: large residuals, gated as outliers
        pp["Xw"][:20] *= -1.0
    else:
        assert edit is None, edit
    return pp


def store_of(pp):
    """the host's rule (asd_pose_optimize): compact LDS for f32-exact observations and <= 16 information bit patterns while 35 n + 16
    bytes fit, else full f64 LDS while 50 n + 16 fit, else global memory; no solver runs on fewer than 3 edges (-1)"""
    n = len(pp["Xw"])
    if n < 3:
        return -1
    obs = np.ascontiguousarray(pp["obs"], np.float64)
    info = np.ascontiguousarray(pp["info"], np.float64)
    compact = bool((obs.astype(np.float32).astype(np.float64) == obs).all()) and len(np.unique(info.view(np.uint64))) <= 16
    if compact and 35 * n + 16 <= LDS_BYTES:
        return 2
    return 1 if 50 * n + 16 <= LDS_BYTES else 0


def replay(rnd):
    """Levenberg control of one round (levenberg.cpp:95-147) restated from the trace: per iteration a dict with ini (chi2 at its
    start), temps (chi2 of each trial), acc (accepted?), cur (chi2 at its end), decisive (no accept / reject moved the chi2 by less
    than TRIAL_MARGIN relative and the nBad test is NBAD_MARGIN away from equality).  A trial is accepted when it lowered the chi2."""
    calls, out, j = list(rnd["calls"]), [], 0
    for n_tr in rnd["trials"]:
        ini = cur = calls[j]
        temps = calls[j + 1:j + 1 + n_tr]
        j += 1 + n_tr
        acc, decisive = [], True
        for t in temps:
            decisive &= abs(t - cur) >= TRIAL_MARGIN * abs(cur)
            acc.append(t < cur)
            if t < cur:
                cur = t
        ended = not acc[-1]   # ten rejections or rho == 0: the round stops without the nBad test
        if not ended:
            decisive &= abs((ini - cur) * 1e3 - ini) >= NBAD_MARGIN * abs(ini)
        out.append(dict(ini=ini, temps=temps, acc=acc, cur=cur, decisive=bool(decisive)))
    assert j == len(calls), (j, len(calls))
    return out


def decisive_prefix(rnd):
    """number of leading iterations of the round on which g2o's counts can be compared with another implementation's"""
    k = 0
    for it in replay(rnd):
        if not it["decisive"]:
            break
        k += 1
    return k


def expected_skips(trace):
    """rounds asd_pose_optimize does not run: 1 and 2, where the re-classification before them changed no flag in g2o's run"""
    return [r for r in (1, 2) if r < len(trace) and trace[r - 1]["changed"] == 0]


def rejected_mid(trace, decisive_only=False):
    """iterations that rejected a trial and were followed by another iteration"""
    k = 0
    for rnd in trace:
        rep, pre = replay(rnd), decisive_prefix(rnd)
        for i, it in enumerate(rep[:-1]):
            if not all(it["acc"]) and (not decisive_only or i < pre):
                k += 1
    return k


def ends_rejected(rnd):
    rep = replay(rnd)
    return bool(rep) and not rep[-1]["acc"][-1]


PATHS = {
    "skip_both": lambda tr: len(tr) == 4 and tr[0]["changed"] == 0 and tr[1]["changed"] == 0,
    "skip_r2": lambda tr: len(tr) == 4 and tr[0]["changed"] > 0 and tr[1]["changed"] == 0,
    "no_skip": lambda tr: len(tr) == 4 and tr[0]["changed"] > 0 and tr[1]["changed"] > 0,
    "changed_r2": lambda tr: len(tr) == 4 and tr[2]["changed"] > 0 and tr[3]["active"] != tr[2]["active"],
    "reinlier": lambda tr: any(r["reinlier"] > 0 for r in tr),
    "its10": lambda tr: any(r["ret"] == 10 for r in tr),
    "nbad": lambda tr: any(3 <= r["ret"] < 10 and r["trials"][-1] < 10 and not ends_rejected(r) for r in tr),
    "qmax10": lambda tr: any(10 in r["trials"] for r in tr),
    "rejected_mid": lambda tr: rejected_mid(tr, decisive_only=True) > 0,
    "ends_rejected": lambda tr: any(ends_rejected(r) for r in tr),
    "no_active": lambda tr: len(tr) == 4 and all(r["active"] == 0 and r["ret"] == -1 for r in tr[1:]),
    "active4": lambda tr: any(r["active"] == 4 for r in tr),
    "one_round": lambda tr: len(tr) == 1,
    "four_rounds": lambda tr: len(tr) == 4,
    "none": lambda tr: len(tr) == 0,
}
# every axis of the Levenberg exits must be met by SOME case (found from the trace, not promised per case: whether a round ends on ten
# rejections is decided at the rounding floor, see tests/test_pose_paths.py)
AXES = ("its10", "nbad", "qmax10", "rejected_mid", "ends_rejected", "active4", "reinlier", "changed_r2")


def pack_trace(trace):
    hdr = np.array([[r["active"], r["ret"], r["n_bad"], r["changed"], r["reinlier"], r["gate_edge"]] for r in trace], np.int32).reshape(-1, 6)
    misc = np.array([list(r["pose"]) + [r["gate_margin"]] for r in trace], np.float64).reshape(-1, 8)
    trials = np.full((len(trace), 10), -1, np.int32)
    for k, r in enumerate(trace):
        trials[k, :len(r["trials"])] = r["trials"]
    ncalls = np.array([len(r["calls"]) for r in trace], np.int32)
    calls = np.concatenate([r["calls"] for r in trace]) if trace else np.zeros(0)
    return dict(hdr=hdr, misc=misc, trials=trials, ncalls=ncalls, calls=calls)


def unpack_trace(G, i):
    hdr, misc, trials, ncalls, calls = (G[f"c{i}_{k}"] for k in ("hdr", "misc", "trials", "ncalls", "calls"))
    out, j = [], 0
    for k in range(len(hdr)):
        out.append(dict(active=int(hdr[k, 0]), ret=int(hdr[k, 1]), n_bad=int(hdr[k, 2]), changed=int(hdr[k, 3]), reinlier=int(hdr[k, 4]),
                        gate_edge=int(hdr[k, 5]), pose=misc[k, :7], gate_margin=float(misc[k, 7]),
                        trials=[int(t) for t in trials[k] if t >= 0], calls=calls[j:j + ncalls[k]]))
        j += int(ncalls[k])
    return out


def main():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "oracle", "ref_g2o")])
    synth = g.load_package().synth
    po = g.load_oracle()
    po.build()
    ref, orc = po.RefG2O(), po.Oracle()
    assert ref.abi >= 3, "oracle/_ref/libg2o_ref.so predates the traced driver: rebuild it (__graft_entry__.build())"
    assert len(DROPPED) <= 2
    out = {"cases": np.array(json.dumps(CASES)), "dropped": np.array(json.dumps(DROPPED))}
    met = {a: [] for a in AXES}
    for i, case in enumerate(CASES):
        pp = problem(case, synth)
        args = (pp["pose"], pp["Xw"], pp["obs"], pp["info"], pp["K"])
        pose, flags, ninl = ref.pose_optimize(*args)
        trace = ref.pose_optimize_trace()
        pose2, flags2, ninl2 = ref.pose_optimize(*args)
        assert np.array_equal(pose, pose2) and np.array_equal(flags, flags2) and ninl == ninl2, f"{case['name']}: g2o is not deterministic"
        opose, oflags, oninl = orc.pose_optimize(*args)
        dist = float(np.abs(opose - pose).max())
        assert np.array_equal(oflags, flags) and oninl == ninl, f"{case['name']}: oracle and g2o disagree on the flags"
        assert dist <= ORACLE_TOL, f"{case['name']}: oracle-to-g2o pose distance {dist:.2e}"
        assert store_of(pp) == case["store"], f"{case['name']}: shape selects store {store_of(pp)}"
        for path in case["paths"]:
            assert PATHS[path](trace), f"{case['name']}: g2o's trace does not show {path}"
        for r, rnd in enumerate(trace):
            assert rnd["gate_margin"] >= GATE_MARGIN, f"{case['name']} round {r}: edge {rnd['gate_edge']} is {rnd['gate_margin']:.2e} from the gate"
        for a in AXES:
            if PATHS[a](trace):
                met[a].append(case["name"])
        out[f"c{i}_in_sha256"] = np.array(problem_digest(pp))
        out[f"c{i}_out_pose"], out[f"c{i}_out_outlier"], out[f"c{i}_out_ninl"] = pose, flags, np.int32(ninl)
        out[f"c{i}_orc_dist"] = np.float64(dist)
        for k, v in pack_trace(trace).items():
            out[f"c{i}_{k}"] = v
        print(f"{case['name']:14s} n {len(pp['Xw']):5d} inl {ninl:5d} orc-g2o {dist:.1e} skip {expected_skips(trace)} | " +
              " | ".join(f"{r['active']} it {r['ret']} tr {r['trials']} pre {decisive_prefix(r)} bad {r['n_bad']} chg {r['changed']}"
                         f"{' END-REJ' if ends_rejected(r) else ''}" for r in trace))
    for a in AXES:
        print(f"axis {a}: {met[a]}")
        assert met[a], f"no case takes the path {a}"
    out["axes"] = np.array(json.dumps(met))
    path = os.path.join(ROOT, "tests", "golden", "pose_paths_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
