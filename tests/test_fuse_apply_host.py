"""asd_fuse_apply's rule over flat host tables (asd-slam_amd/host/fuse_apply.hpp) through host/test_fuse_apply_rule, a program without
device code that is also the one to build under AddressSanitizer / UBSan, against tests/fuse_apply_ref.py on the hand-worked and the
random cases, in all modes; and asd::LocalMapping::SearchInNeighbors, asd::LoopClosing::SearchAndFuse and asd::LoopClosing::FuseMatchedPoints
(asd-slam_amd/host/asd_adapters.hpp) through host/test_fuse_apply, against the restatement fed with the existing oracle's search results."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import fuse_apply_ref as ref
from tests.conftest import ROOT
from tests.culling_ref import CullingMap
from tests.fuse_apply_cases import KEYS, hand_cases, problem_text, random_cases
from tests.test_matcher import BOUNDS, SCALES, backproject, perturbed_descriptors, pose_T

HOST = os.path.join(ROOT, "asd-slam_amd", "host")
CSRC = os.path.join(ROOT, "asd-slam_amd", "csrc")


def _built(name):
    path = os.path.join(HOST, name)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", CSRC, f"../host/{name}"])
    return path


def _run(tmp_path, m, calls):
    """-> (the program's output, the restatement's outcomes); m is left as the restatement's calls leave it"""
    path = tmp_path / "fuse.txt"
    path.write_text(problem_text(m, calls))
    r = subprocess.run([_built("test_fuse_apply_rule"), str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout), [ref.fuse_apply(m, kf, cand, best, mode, apply) for kf, mode, cand, best, apply in calls]


def _compare(out, expected, m):
    assert len(out["calls"]) == len(expected)
    for got, exp in zip(out["calls"], expected):
        for k in KEYS:
            assert got[k] == [int(x) for x in exp[k]], k
        assert got["n_fused"] == exp["n_fused"]
    assert {kf: r["row"] for kf, r in out["rows"]} == m.kf_points           # the whole table at the end
    assert set(out["bad"]) == set(m.pt_bad)


def test_rule_on_the_hand_worked_maps(tmp_path):
    for name, m, calls, (rows_after, bad_after) in hand_cases():
        dry_then_apply = [(kf, mode, cand, best, a) for kf, mode, cand, best, _ in calls for a in (0, 1)]
        out, expected = _run(tmp_path, m, dry_then_apply)
        _compare(out, expected, m)
        for (_kf, _mode, _cand, _best, want), got in zip(calls, out["calls"][1::2]):
            assert all(got[k] == want[k] for k in KEYS) and got["n_fused"] == want["n_fused"], name
        assert m.kf_points == rows_after and m.pt_bad == bad_after, name


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_rule_on_the_random_maps(tmp_path, mode):
    for m, kf, cand, best in random_cases(mode):
        kfs = sorted(m.kf_points)
        calls = [(kf, mode, cand, best, 0), (kf, mode, cand, best, 1), (kf, mode, cand, best, 1), (kfs[0], mode, cand[:len(m.kf_points[kfs[0]])], best[:len(m.kf_points[kfs[0]])], 1)]
        if mode == 2:                                                # (another keyframe, the same convention: best_idx[i] = i or -1)
            calls[3] = (kfs[0], 2, cand, best, 1)
        out, expected = _run(tmp_path, m, calls)
        assert any(a in (1, 2, 3) for a in expected[1]["action"])
        _compare(out, expected, m)


def _winners(cand, out, mode):
    w = []
    for c, a, o in zip(cand, out["action"], out["other"]):
        if a == 2:
            w.append(int(o))
        elif a == 3 or (a == 1 and mode == 2):
            w.append(int(c))
    return w


class _World:
    """12 keyframes on a short track over 260 world points.  Every world point has three map points (bank rows 3 w .. 3 w + 2: the
    duplicates Fuse is there to merge); keyframe k's keypoints are the projections of the points it sees, with the frames' structure of
    tests/test_matcher.make_frame (sorted by octave, unit descriptors), and about half of them hold the duplicate k % 3."""

    def __init__(self, pkg, seed=5, n_kf=12, n_world=260):
        rng = np.random.default_rng(seed)
        self.K = np.array(pkg.synth.KITTI_K, np.float32)
        self.ids = [3 + 2 * k for k in range(n_kf)]
        self.T = {kf: pose_T((0.01 + 0.002 * k, -0.02 + 0.003 * k, 0.005), (0.1 - 0.06 * k, -0.05, 0.3 + 0.02 * k)) for k, kf in enumerate(self.ids)}
        Tm = self.T[self.ids[n_kf // 2]]
        uv = np.stack([rng.uniform(60, 1180, n_world), rng.uniform(40, 330, n_world)], 1).astype(np.float32)
        Xw = backproject(Tm, self.K, uv, rng.uniform(6, 40, n_world))
        octave = rng.choice(8, n_world, p=np.array([434, 362, 302, 251, 209, 175, 145, 122]) / 2000.0)
        dw = rng.standard_normal((n_world, 128)).astype(np.float32)
        dw /= np.linalg.norm(dw, axis=1, keepdims=True)
        Ow = -(Tm[:3, :3].astype(np.float64).T @ Tm[:3, 3].astype(np.float64))
        n_pts = 3 * n_world
        w_of = np.repeat(np.arange(n_world), 3)
        X = (Xw[w_of] + rng.normal(0, 0.004, (n_pts, 3))).astype(np.float32)
        nrm = X.astype(np.float64) - Ow
        dist = np.linalg.norm(nrm, axis=1)
        maxd = (dist * SCALES[octave[w_of]] * 1.2).astype(np.float32)
        self.attr = np.concatenate([X, (nrm / dist[:, None]).astype(np.float32), (maxd / np.float32(SCALES[7]) * 0.8)[:, None].astype(np.float32), maxd[:, None]], 1).astype(np.float32)
        self.desc = perturbed_descriptors(dw[w_of], 0.03, seed + 1)
        self.desc2 = perturbed_descriptors(dw[w_of], 0.05, seed + 2)
        self.refreshed = np.zeros(n_pts, bool)
        self.m = CullingMap()
        self.kps, self.kdesc, self.world_of = {}, {}, {}
        KP = pkg.capi.KP_DTYPE
        assert KP.itemsize == 24
        for k, kf in enumerate(self.ids):
            T = self.T[kf].astype(np.float64)
            Xc = Xw.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
            px = np.stack([self.K[0] * Xc[:, 0] / Xc[:, 2] + self.K[2], self.K[1] * Xc[:, 1] / Xc[:, 2] + self.K[3]], 1)
            vis = np.nonzero((Xc[:, 2] > 0.5) & (px[:, 0] > 25) & (px[:, 0] < 1215) & (px[:, 1] > 25) & (px[:, 1] < 350))[0]
            vis = vis[np.argsort(octave[vis], kind="stable")]
            kp = np.zeros(len(vis), KP)
            kp["x"] = (px[vis, 0] + rng.normal(0, 0.4, len(vis))).astype(np.float32)
            kp["y"] = (px[vis, 1] + rng.normal(0, 0.4, len(vis))).astype(np.float32)
            kp["octave"], kp["size"] = octave[vis], 31
            kp["angle"] = rng.uniform(0, 360, len(vis)).astype(np.float32)
            kp["response"] = rng.integers(7, 200, len(vis))
            self.kps[kf], self.kdesc[kf], self.world_of[kf] = kp, perturbed_descriptors(dw[vis], 0.04, seed + 10 + k), vis
            self.m.put_keyframe(kf, [int(3 * w + k % 3) if rng.uniform() < 0.55 else -1 for w in vis])

    def problem(self, cur, targets, loop_kf, loop_kfs, matched_kf, matched):
        i32 = lambda *v: np.array(v, "<i4").tobytes()
        out = [i32(len(self.ids), len(self.attr)), self.K.astype("<f4").tobytes()]
        for kf in self.ids:
            out += [i32(kf, len(self.kps[kf])), self.T[kf].astype("<f4").tobytes(), self.kps[kf].tobytes(), self.kdesc[kf].astype("<f4").tobytes(),
                    np.array(self.m.kf_points[kf], "<i4").tobytes()]
        out += [self.attr.tobytes(), self.desc.tobytes(), self.desc2.tobytes(), i32(0)]
        out += [i32(cur, len(targets), *targets), i32(loop_kf, len(loop_kfs), *loop_kfs), i32(matched_kf, len(matched), *matched)]
        return b"".join(out)

    def search(self, oracle, frames, kf, rows, sim3=False):
        """the adapters' search half through the existing oracle: valid = a point the keyframe's row does not hold"""
        in_kf = set(p for p in self.m.kf_points[kf] if p >= 0)
        rows = np.asarray(rows, np.int64)
        valid = np.array([r >= 0 and int(r) not in in_kf for r in rows], np.uint8)
        if len(rows) == 0:
            return []
        idx = np.maximum(rows, 0)
        a = self.attr[idx] * valid[:, None]
        d = np.where(self.refreshed[idx][:, None], self.desc2[idx], self.desc[idx]) * valid[:, None]
        if sim3:
            bi, _ = oracle.fuse_search_sim3(frames[kf], self.T[kf], valid, a[:, :3], a[:, 3:6], a[:, 6], a[:, 7], d, self.K, 4.0)
        else:
            bi, _ = oracle.fuse_search(frames[kf], valid, a[:, :3], a[:, 3:6], a[:, 6], a[:, 7], d, self.T[kf], self.K, 3.0)
        return [int(x) for x in bi]


def _same_outcome(got, exp, cand, best, mode):
    assert got["rc"] == 0
    if best is not None:
        assert got["best_idx"] == best
    for k in KEYS:
        assert got[k] == [int(x) for x in exp[k]], k
    assert got["n_fused"] == exp["n_fused"] and got["winners"] == _winners(cand, exp, mode)


@pytest.mark.gpu
def test_adapters_equal_the_restatement(tmp_path, oracle):
    """SearchInNeighbors of 3 targets over a 12-keyframe map whose frames sit in the context's slots, so that the searches really hit, then
    one SearchAndFuse keyframe and one FuseMatchedPoints on the same table -- against the restatement fed with the existing oracle's
    search result for every call: best_idx, outcomes, the onReplaced lists in order (a named point reads another descriptor from then
    on, on both sides) and every row of the table at the end"""
    from tests.conftest import load_package
    w = _World(load_package())
    m, ids = w.m, w.ids
    cur, targets, loop_kf, loop_kfs, matched_kf = ids[6], [ids[5], ids[7], ids[4]], ids[1], [ids[9], ids[10], ids[11]], ids[11]
    rng = np.random.default_rng(8)
    k11 = 11
    matched = [int(3 * wd + (k11 + 1) % 3) if rng.uniform() < 0.5 else -1 for wd in w.world_of[matched_kf]]
    path = tmp_path / "fuse_adapters.bin"
    path.write_bytes(w.problem(cur, targets, loop_kf, loop_kfs, matched_kf, matched))
    r = subprocess.run([_built("test_fuse_apply"), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    frames = {kf: oracle.frame(w.kps[kf], w.kdesc[kf], BOUNDS) for kf in ids}
    # the restatement through the same steps (LocalMapping.cc:587-617, LoopClosing.cc:603-629, :540-555)
    matches = ref.map_get(m, cur)
    assert out["neighbors"]["rc"] == 0 and out["neighbors"]["matches"] == matches
    on_replaced, acts, stale = [], [], 0

    def fuse(kf, rows, got, mode=0):
        nonlocal stale
        stale += int(any(r >= 0 and w.refreshed[r] for r in rows))     # a search that reads a descriptor an earlier onReplaced changed
        best = w.search(oracle, frames, kf, rows, sim3=mode == 1)
        exp = ref.fuse_apply(m, kf, rows, best, mode, True)
        _same_outcome(got, exp, rows, best, mode)
        acts.extend(exp["action"])
        return _winners(rows, exp, mode)

    for t, got in zip(targets, out["neighbors"]["targets"]):
        win = fuse(t, matches, got)
        if win:
            on_replaced.append(win)
            w.refreshed[win] = True
    cands = ref.map_points(m, targets)
    assert out["neighbors"]["candidates"] == cands
    win = fuse(cur, cands, out["neighbors"]["current"])
    if win:
        on_replaced.append(win)
        w.refreshed[win] = True
    assert [x["rows"] for x in out["on_replaced"]] == on_replaced and len(on_replaced) == 4 and stale >= 2
    assert acts.count(1) >= 10 and acts.count(2) + acts.count(3) >= 10 and acts.count(7) >= 1     # the searches really hit
    loop_points = ref.map_points(m, loop_kfs)
    assert out["loop_points"] == loop_points
    n0 = len(acts)
    fuse(loop_kf, loop_points, out["search_and_fuse"], mode=1)
    assert acts[n0:].count(3) >= 3
    exp = ref.fuse_apply(m, matched_kf, matched, [i if p >= 0 else -1 for i, p in enumerate(matched)], 2, True)
    assert exp["action"].count(3) >= 5
    _same_outcome(out["fuse_matched"], exp, matched, None, 2)
    assert {kf: r["row"] for kf, r in out["rows"]} == m.kf_points
