"""asd::PnPsolver and asd::Tracking::RelocalizationRound (asd-slam_amd/host/asd_adapters.hpp) through host/test_pnp_solver.

Without a device: --params against the restated SetRansacParameters, --draws against the reference's loop (PnPsolver.cc:182-201), which
calls rand() four times per iteration as the iterations run and, with the OR of :182, runs max(nIterations, mRansacMaxIts - mnIterations)
iterations in a call that returns no refined model.  On the device (marked gpu): the solver and the passes of the relocalisation loop
against a Python loop over single pnp_ransac calls that consumes the same raw rand() values with the reference's sequential semantics
(Tracking.cc:1156-1249: candidate by candidate, iterate(5) each)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from tests import pnpsolver_cases as C
from tests import pnpsolver_ref as R
from tests.conftest import ROOT

PROBE = os.path.join(ROOT, "asd-slam_amd", "host", "test_pnp_solver")
N_RAW = 4000
# (seed of the raw stream, the scripted tail's matching call): with 1 the first pose is turned down and the second matches while a
# candidate is live behind it; with -1 no pose is ever accepted and every solver runs into bNoMore
SCRIPTS = ((3, 1), (10, -1))


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(PROBE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "asd-slam_amd", "csrc"), "../host/test_pnp_solver"])
    return lambda *a: subprocess.run([PROBE, *map(str, a)], capture_output=True, text=True, timeout=120)


def _libc_rand(seed, count):
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(ctypes.c_uint(seed))
    libc.rand.restype = ctypes.c_int
    return [libc.rand() for _ in range(count)]


# ------------------------------------------------------------------------------------------------------------------------ no device
def test_params_mode_equals_the_restatement(probe):
    for row in [(15, 0.99, 10, 300, 4, 0.5), (64, 0.99, 10, 300, 4, 0.5), (10, 0.99, 10, 300, 4, 0.5), (20, 0.99, 15, 300, 4, 0.4),
                (1000, 0.99, 10, 300, 4, 0.05), (150, 0.5, 8, 35, 4, 0.4), (8, 0.99, 10, 300, 4, 0.5)]:
        r = probe("--params", *row)
        assert r.returncode == 0, r.stderr
        mi, its = R.parameters(*row)
        assert r.stdout.split() == ["min_inliers", str(mi), "max_its", str(its)], (row, r.stdout)


def test_draw_stream_consumes_the_reference_sequence(probe):
    """iterate(5) calls with early returns and without, stepped through Begin / End: the raw rand() values the solver consumes and the
    RandomInt results it hands to the device are those of the reference's loop, and the numbers handed back reappear in order"""
    seed, n = 7, 40
    min_inliers, max_its = R.parameters(n, *C.RANSAC)
    assert max_its == 35
    script = [2, 0, -1, 3, -1, 4, -1]
    raw = _libc_rand(seed, 4 * (max_its + 5 * len(script)))
    at, iterations, exp = 0, 0, []
    for early in script:                                   # the reference: one rand() per draw, at the moment of the draw
        cur, draws, used, returned = 0, [], [], False
        while iterations < max_its or cur < 5:             # :182, OR
            cur += 1
            iterations += 1
            for i in range(4):
                used.append(raw[at])
                draws.append(R.random_int(raw[at], 0, n - 1 - i))
                at += 1
            if early == cur - 1:
                returned = True
                break
        exp.append((cur if returned else None, draws, used, iterations, int(iterations >= max_its and not returned)))
    r = probe("--draws", seed, n, *script)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"min_inliers {min_inliers} max_its {max_its}" and len(lines) == 1 + len(script)
    n_iters = []
    for line, (_cur, draws, used, its, no_more) in zip(lines[1:], exp):
        w = line.split()
        i_d, i_r, i_i = w.index("draws"), w.index("raw"), w.index("iterations")
        n_iters.append(int(w[w.index("n_iter") + 1]))
        assert [int(x) for x in w[i_d + 1:i_r]] == draws, line
        assert [int(x) for x in w[i_r + 1:i_i]] == used, line
        assert int(w[i_i + 1]) == its and int(w[w.index("no_more") + 1]) == no_more, line
        assert int(w[w.index("pending") + 1]) == 4 * n_iters[-1] - len(used), line
    # the n_iter rule: max(nIterations, mRansacMaxIts - mnIterations) with mnIterations as the calls before left it
    done = [0] + [e[3] for e in exp[:-1]]
    assert n_iters == [R.n_iter_rule(5, max_its, d) for d in done] and n_iters[0] == 35 and n_iters[-1] == 5
    assert any(e[4] for e in exp), "a call without a refined model always ends with bNoMore"


# -------------------------------------------------------------------------------------------------------------------- on the device
def candidates():
    """four candidates in the order of the relocalisation loop: 80 exact correspondences, 8 (fewer than mRansacMinInliers: discarded at
    once), 70 exact, 60 of which 40 % are gross outliers; the keypoint index of correspondence i (mvKeyPointIndices) is a seeded
    increasing map into twice as many keypoints"""
    out = []
    for ci, (n, frac, noise) in enumerate([(80, 0.0, 0.0), (8, 0.0, 0.0), (70, 0.0, 0.0), (60, 0.4, 0.0)]):
        rng = np.random.default_rng(700 + ci)
        S = C._scene(rng, n, frac, noise)
        idx = np.sort(rng.permutation(2 * n)[:n])
        sigma2 = C.SIGMA2[rng.integers(0, 8, n)]
        mi, its = R.parameters(n, *C.RANSAC)
        out.append(dict(NF=2 * n, n=n, K=S["K"], idx=idx, P3Dw=S["P3Dw"], P2D=S["P2D"], sigma2=sigma2,
                        max_err=(sigma2 * C.TH2).astype(np.float32), min_inliers=mi, max_its=its))
    return out


def raw_values(seed):
    return [int(v) for v in np.random.default_rng(seed).integers(0, 2 ** 31, N_RAW)]


def write_problem_file(path, cands, raw, match_at):
    hx = lambda a: " ".join(float(x).hex() for x in np.asarray(a, np.float32).reshape(-1))
    with open(path, "w") as f:
        f.write(f"{len(raw)}\n" + " ".join(map(str, raw)) + f"\n{match_at} {len(cands)}\n")
        for c in cands:
            f.write(f"{c['NF']} {c['n']}\n")
            f.write(" ".join(repr(float(k)) for k in c["K"]) + "\n")
            f.write(" ".join(str(int(i)) for i in c["idx"]) + "\n")
            for k in ("P3Dw", "P2D", "sigma2"):
                f.write(hx(c[k]) + "\n")


class Stream:
    def __init__(self, raw):
        self.raw, self.at = raw, 0


def new_state():
    return dict(iterations=0, best=0, best_mask=None, best_Tcw=None, refined=None)


def iterate(solve, c, st, stream, n_iterations=5):
    """PnPsolver::iterate(nIterations) of candidate c (state st) as one single-problem call: the draws are the next raw values, and
    only those of the iterations that ran are consumed"""
    if c["n"] < c["min_inliers"]:
        return dict(pose=0, no_more=1, raw=[], inliers=[], n_inliers=0, Tcw=None)
    n_iter = R.n_iter_rule(n_iterations, c["max_its"], st["iterations"])
    raw = stream.raw[stream.at:stream.at + 4 * n_iter]
    assert len(raw) == 4 * n_iter, "the raw stream of the test is too short"
    draws = np.array([R.random_int(r, 0, c["n"] - 1 - (k % 4)) for k, r in enumerate(raw)], np.int32).reshape(n_iter, 4)
    res = solve(dict(c, n_iter=n_iter, draws=draws, best_inliers=st["best"]))
    done = res["iterations_done"]
    if st["refined"] is not None:
        # iterated again after its refined model came back: the reference calls Refine() at the next iteration that passes :209, and on an
        # unchanged best set it succeeds again -- the same refined model returns there
        for k in range(done):
            cnt = solve.count(k)
            if cnt < c["min_inliers"]:
                continue
            if cnt <= st["best"]:
                stream.at += 4 * (k + 1)
                st["iterations"] += k + 1
                return dict(st["refined"], raw=raw[:4 * (k + 1)])
            break
    used = 4 * done
    stream.at += used
    st["iterations"] += done
    st["best"] = res["best_inliers"]
    if res["best_updated"]:
        st["best_mask"], st["best_Tcw"] = res["best_mask"].copy(), res["best_Tcw"].copy()
        st["refined"] = None
    out = dict(pose=0, no_more=0, raw=raw[:used], inliers=[], n_inliers=0, Tcw=None)
    if res["found"]:
        out.update(pose=1, inliers=[int(c["idx"][i]) for i in np.nonzero(res["inliers"])[0]], n_inliers=res["n_inliers"], Tcw=res["Tcw"])
        st["refined"] = dict(out)
    elif st["iterations"] >= c["max_its"]:
        out["no_more"] = 1
        if st["best"] >= c["min_inliers"] and st["best_mask"] is not None:
            out.update(pose=1, inliers=[int(c["idx"][i]) for i in np.nonzero(st["best_mask"])[0]], n_inliers=st["best"], Tcw=st["best_Tcw"])
    return out


class Solve:
    """one single-problem call, and the count of an iteration of the call just made"""
    def __init__(self, hip):
        self.hip = hip

    def __call__(self, p):
        return self.hip.pnp_ransac([p])[0]

    def count(self, k):
        return self.hip.debug_pnp_ransac(0, k)["count"]


def run_single(solve, c, raw):
    stream, st, calls = Stream(raw), new_state(), []
    while True:
        r = iterate(solve, c, st, stream)
        calls.append((r, dict(st)))
        if r["pose"] or r["no_more"]:
            return calls, stream.at


def run_passes(solve, cands, raw, match_at):
    """Tracking.cc:1156-1249 with the scripted tail"""
    stream = Stream(raw)
    states = [new_state() for _ in cands]
    discarded = [False] * len(cands)
    tails, matched, passes = [], -1, 0
    while not all(discarded) and matched < 0:
        passes += 1
        for i, c in enumerate(cands):
            if discarded[i]:
                continue
            r = iterate(solve, c, states[i], stream)
            if r["no_more"]:
                discarded[i] = True
            if r["pose"]:
                tails.append((i, passes, r, dict(states[i])))
                if len(tails) - 1 == match_at:
                    matched = i
                    break
    return dict(tails=tails, matched=matched, passes=passes, states=states, discarded=discarded, at=stream.at)


def same_call(js, r, st):
    assert js["pose"] == r["pose"] and js["no_more"] == r["no_more"], (js, r)
    assert js["iterations"] == st["iterations"] and js["best_inliers"] == st["best"]
    assert js["raw"] == r["raw"]
    assert js["inliers"] == r["inliers"] and js["n_inliers"] == r["n_inliers"]
    if r["pose"]:
        assert [float.fromhex(x) for x in js["Tcw"]] == [float(x) for x in np.asarray(r["Tcw"]).reshape(-1)]


@pytest.fixture(scope="module", params=SCRIPTS)
def probe_output(request, tmp_path_factory, probe):
    seed, match_at = request.param
    path = tmp_path_factory.mktemp("pnp") / "problem.txt"
    write_problem_file(path, candidates(), raw_values(seed), match_at)
    r = probe(str(path))
    assert r.returncode == 0, r.stderr
    return seed, match_at, json.loads(r.stdout)


@pytest.mark.gpu
def test_single_solver_iterates_like_single_calls(hip, probe_output):
    solve = Solve(hip)
    seed, _match_at, out = probe_output
    for ci, c in enumerate(candidates()):
        js = out["single"][ci]
        calls, at = run_single(solve, c, raw_values(seed))
        assert js["min_inliers"] == c["min_inliers"] and js["max_its"] == c["max_its"] and js["ran_out"] == 0
        assert len(js["calls"]) == len(calls)
        for a, (r, st) in zip(js["calls"], calls):
            if c["n"] < c["min_inliers"]:
                assert a["pose"] == 0 and a["no_more"] == 1 and a["raw"] == []
            else:
                same_call(a, r, st)
        assert js["source_at"] - js["pending"] == at, "the raw values consumed are exactly the reference's"
    first, _ = run_single(solve, candidates()[0], raw_values(seed))
    assert first[-1][0]["pose"] and first[-1][1]["iterations"] < candidates()[0]["max_its"], \
        "the exact candidate returns its refined model before the last supplied iteration"


@pytest.mark.gpu
def test_relocalization_round_is_the_sequential_loop(hip, probe_output):
    solve = Solve(hip)
    cands = candidates()
    seed, match_at, out = probe_output
    exp = run_passes(solve, cands, raw_values(seed), match_at)
    js = out["round"]
    assert js["ran_out"] == 0
    assert js["matched"] == exp["matched"] and js["passes"] == exp["passes"]
    assert len(js["tails"]) == len(exp["tails"])
    for a, (i, p, r, st) in zip(js["tails"], exp["tails"]):
        assert a["candidate"] == i and a["pass"] == p
        same_call(a["call"], dict(r, no_more=0), st)      # (the probe prints the tail's arguments: bNoMore is not one of them)
    assert js["iterations"] == [s["iterations"] for s in exp["states"]]
    assert js["best_inliers"] == [s["best"] for s in exp["states"]]
    assert js["discarded"] == [int(d) for d in exp["discarded"]]
    assert js["source_at"] - js["pending"] == exp["at"], "the raw values consumed are exactly the reference's"
    assert exp["discarded"][1], "the candidate with N < mRansacMinInliers is discarded without a draw"
    if match_at >= 0:
        # the scenario: a pose was turned down in a pass in which candidates were live behind it, the match came with a live candidate
        # behind it -- the batched pass had drawn for that one and had to hand its numbers back and leave its state alone
        assert exp["matched"] >= 0 and len(exp["tails"]) == match_at + 1
        assert exp["states"][3]["iterations"] == 0 and not exp["discarded"][3] and js["pending"] > 0
    else:
        assert exp["matched"] == -1 and all(exp["discarded"])
