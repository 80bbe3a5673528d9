"""asd_fuse_apply, asd_map_get and asd_map_points on the device against tests/fuse_apply_ref.py (which tests/test_fuse_apply_ref.py pins by
hand): every outcome array and n_fused equal, exactly, and after an apply every row of every keyframe read back through asd_map_get, plus
everything the existing queries read from the table."""
import numpy as np
import pytest

from tests import fuse_apply_ref as ref
from tests.culling_cases import RANDOM_SHAPES, load, mk, random_case
from tests.fuse_apply_cases import assert_same, hand_cases, random_fuse_case
from tests.local_map_cases import assert_same as assert_same_local_map
from tests.local_map_cases import load as load_rows_only
from tests.local_map_cases import random_frame
from tests.test_matcher import BOUNDS, SCALES, backproject, make_frame, perturbed_descriptors, pose_T
from tests.test_track_chain import _pose7

ASD_ERR_INVALID, ASD_ERR_CAPACITY = -1, -5


def _fuse(hip, m, kf, cand, best, mode, apply):
    exp = ref.fuse_apply(m, kf, cand, best, mode, apply)
    assert_same(hip.fuse_apply(kf, cand, best, mode, apply), exp)
    return exp


def _all_points(m):
    return sorted({p for row in m.kf_points.values() for p in row if p >= 0} | set(m.pt_bad) | set(m.obs))


def _rows(hip, m):
    return {kf: [int(x) for x in hip.map_get(kf, len(m.kf_points[kf]))] for kf in sorted(m.kf_points)}


def _check_table(hip, m, frames=()):
    """the whole table row by row, the bad bytes (through asd_map_points) and what the counting queries read, against the restatement's map"""
    assert _rows(hip, m) == {kf: list(r) for kf, r in m.kf_points.items()}
    kfs = sorted(m.kf_points)
    assert [int(x) for x in hip.map_points(kfs)] == ref.map_points(m, kfs)
    pts = _all_points(m)
    assert list(hip.map_observations(pts)) == m.observations(pts)
    for kf in (kfs[0], kfs[len(kfs) // 2], kfs[-1]):
        gk, gc = hip.map_shared_counts(kf)
        assert [(int(a), int(b)) for a, b in zip(gk, gc)] == m.shared_counts(kf)
    for cur, seen in frames:
        assert_same_local_map(hip.update_local_map(cur, seen, kfs[:3]), m.update_local_map(cur, seen, kfs[:3]))


def _list_state(hip):
    """what asd_track_local_points_map says about the resident search list, asked with a frame slot that does not exist: 'changed' when a
    table change has invalidated the list, another refusal when the list is still good (the probe of tests/test_culling.py)"""
    z = np.zeros(16, np.float32)
    with pytest.raises(Exception):                                  # (a refusal without a message of its own leaves the last one: make that one known)
        hip.map_observations([-2])
    with pytest.raises(Exception) as e:
        hip.track_local_points_map(1000, 4, z, z[:4], np.zeros(4, np.uint8), np.zeros((4, 3), np.float32), 1.0, 0.8, np.zeros(7))
    assert e.value.code == ASD_ERR_INVALID
    return "changed" if "changed" in str(e.value) else "kept"


def _stepped(exp):
    return any(a in (1, 2, 3) for a in exp["action"])


@pytest.mark.gpu
def test_hand_worked_maps(hip):
    for name, m, calls, (rows_after, bad_after) in hand_cases():
        load(hip, m)
        for kf, mode, cand, best, want in calls:
            assert_same(_fuse(hip, m, kf, cand, best, mode, apply=False), want)
            assert _rows(hip, m) == m.kf_points, name
            assert_same(_fuse(hip, m, kf, cand, best, mode, apply=True), want)
        assert _rows(hip, m) == rows_after and m.pt_bad == bad_after, name
        _check_table(hip, m)
    hip.map_clear()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (0, 1, 2))
@pytest.mark.parametrize("case", range(len(RANDOM_SHAPES)))
def test_random_maps_equal_the_restatement(hip, case, mode):
    for seed in (1, 2):
        m, kf, cand, best = random_fuse_case(RANDOM_SHAPES[case], seed, mode)
        load(hip, m)
        kfs = sorted(m.kf_points)
        frames = [random_frame(m, 40, 10 * case + q) for q in range(2)]
        _check_table(hip, m, frames)                                # (leaves a search list behind)
        d0, v0 = hip.map_debug(), _rows(hip, m)
        # apply = 0: twice the same, no row moved, the search list still good
        exp = ref.fuse_apply(m, kf, cand, best, mode, False)
        got = hip.fuse_apply(kf, cand, best, mode, False)
        assert_same(got, exp)
        again = hip.fuse_apply(kf, cand, best, mode, False)
        for k in got:
            np.testing.assert_array_equal(got[k], again[k])
        assert _rows(hip, m) == v0 and hip.map_debug()[:7] == d0[:7] and _list_state(hip) == "kept"
        # apply = 1
        assert_same(_fuse(hip, m, kf, cand, best, mode, True), exp)
        assert _stepped(exp) and _list_state(hip) == "changed"
        _check_table(hip, m, frames)
        # the second call on the mutated map, another target, and a cull after it
        _fuse(hip, m, kf, cand, best, mode, True)
        other_kf = kfs[0] if kfs[0] != kf else kfs[1]
        rng = np.random.default_rng(300 + case)
        n_kp = len(m.kf_points[other_kf])
        cand2 = [int(x) for x in rng.permutation(_all_points(m))[:2 * n_kp]]
        best2 = [int(x) for x in rng.integers(-1, n_kp, len(cand2))]
        if mode == 2:
            cand2, best2 = cand2[:n_kp], [i if b >= 0 else -1 for i, b in enumerate(best2[:n_kp])]
        _fuse(hip, m, other_kf, cand2, best2, mode, True)
        _check_table(hip, m, frames)
        cull = [int(k) for k in rng.permutation(kfs)[:10]]
        exp_c = m.keyframe_culling(cull, [0] * len(cull), True)
        got_c = hip.keyframe_culling(cull, apply=True)
        for k in ("decision", "n_mps", "n_redundant", "bad_rows"):
            assert [int(x) for x in got_c[k]] == [int(x) for x in exp_c[k]], k
        _check_table(hip, m)
    hip.map_clear()


def _long_loser(n_obs, n_shared=10):
    """keyframes 1 .. n_obs hold point 7 (keyframe 1 is the target), n_shared of them point 8 too, n_obs more hold only 8: 8 has
    n_shared + n_obs >= n_obs observations, so 7 goes -- n_obs - n_shared observations move, n_shared are erased"""
    kfs = {k: [7, 8 if 2 <= k < 2 + n_shared else -1] for k in range(1, n_obs + 1)}
    kfs.update({k: [8, -1] for k in range(n_obs + 1, 2 * n_obs + 1)})
    return mk(kfs)


@pytest.mark.gpu
def test_shapes_the_kernels_can_get_wrong(hip):
    # a loser with more observers than a wave, than the workgroup, and no multiple of either
    for n_obs in (65, 257, 300):
        for mode in (0, 2):
            m = _long_loser(n_obs)
            load_rows_only(hip, m)                                  # (neither octaves nor centres are needed)
            exp = _fuse(hip, m, 1, [8], [0], mode, True)
            assert (exp["action"], exp["n_moved"], exp["n_dropped"]) == ([3], [n_obs - 10], [10])
            _check_table(hip, m)
    # the other way round: the candidate is the long loser (its observers outnumbered by one)
    m = _long_loser(300, 0)
    m.put_keyframe(700, [7])
    load_rows_only(hip, m)
    exp = _fuse(hip, m, 1, [8], [0], 0, True)                       # 7 sits in keyframe 1 with 301 observations, 8 has 300: 8 goes
    assert (exp["action"], exp["n_moved"], exp["n_dropped"]) == ([2], [300], [0])
    _check_table(hip, m)
    # a winner whose chain has absorbed 3 segments before it is tested for membership: the hand chain, with the last loser seen by a
    # keyframe that the winner reached through an absorbed segment
    chain = {1: [100, -1], 2: [101, 103], 3: [101, -1], 4: [102, -1], 5: [102, -1], 6: [102, -1], 7: [102, -1], 8: [103, -1]}
    m = mk(chain)
    load(hip, m)
    exp = _fuse(hip, m, 1, [101, 102, 103], [0, 0, 0], 0, True)
    assert (exp["action"], exp["n_moved"], exp["n_dropped"]) == ([3, 3, 2], [1, 3, 1], [0, 0, 1])
    _check_table(hip, m)
    # 257 hits in one call, then 1 hit among 5000 candidates
    m = mk({1: [-1] * 300, 2: [5, 6]})
    load(hip, m)
    exp = _fuse(hip, m, 1, list(range(1000, 1257)), list(range(257)), 0, True)
    assert exp["action"] == [1] * 257 and exp["n_fused"] == 257
    cand, best = list(range(2000, 7000)), [-1] * 5000
    best[4321] = 299
    exp = _fuse(hip, m, 1, cand, best, 0, True)
    assert exp["n_fused"] == 1 and exp["action"][4321] == 1
    _check_table(hip, m)
    # a table of one keyframe with a one-entry row
    m = mk({5: [-1]})
    load(hip, m)
    assert _fuse(hip, m, 5, [3], [0], 0, True)["action"] == [1]
    assert _fuse(hip, m, 5, [4], [0], 0, True)["action"] == [2]     # Observations(3) = 1 > 0
    assert _fuse(hip, m, 5, [9], [0], 2, True)["action"] == [3]
    _check_table(hip, m)
    # a target put directly after an arena growth, candidates beyond the row tables (growth inside the call), ids that are not dense
    ids = [5000, 6000, 2 ** 30, 2 ** 30 + 7] + list(range(7000, 7036))
    m, _ = random_case(40, 48, 200, 14, 0.8, ids=ids)
    load(hip, m)
    d0 = hip.map_debug()
    rng = np.random.default_rng(15)
    long_row = np.full(20000, -1, np.int64)
    long_row[rng.choice(20000, 100, replace=False)] = rng.choice(200, 100, replace=False)
    m.put_keyframe(2 ** 30 + 9, long_row)
    hip.map_put(2 ** 30 + 9, long_row)
    assert hip.map_debug()[6] > d0[6]
    pts = [p for p in _all_points(m) if 2 ** 30 + 9 not in m.obs.get(p, {})]
    assert len(pts) >= 60
    cand = [int(x) for x in rng.permutation(pts)[:60]] + list(range(d0[4] + 100000, d0[4] + 100040))
    best = [int(x) for x in rng.integers(0, 20000, 60)] + [int(x) for x in np.nonzero(long_row >= 0)[0][:40]]
    exp = _fuse(hip, m, 2 ** 30 + 9, cand, best, 0, True)
    assert hip.map_debug()[7] > d0[7] and exp["action"].count(1) >= 30 and exp["action"].count(2) >= 30
    _check_table(hip, m)
    for mode, kf in ((0, 5000), (1, 2 ** 30), (2, 2 ** 30 + 7)):
        row = m.kf_points[kf]
        cand = [int(x) for x in rng.permutation(_all_points(m))[:len(row)]]
        best = list(range(len(row))) if mode == 2 else [int(x) for x in rng.integers(0, len(row), len(cand))]
        _fuse(hip, m, kf, cand, best, mode, True)
    _check_table(hip, m)
    hip.map_clear()


@pytest.mark.gpu
def test_map_get_and_map_points(hip):
    for case, shape in enumerate(RANDOM_SHAPES):
        m, cand = random_case(*shape[:3], 40 + case, shape[3])
        load(hip, m)
        kfs = sorted(m.kf_points)
        for kf in kfs:
            assert [int(x) for x in hip.map_get(kf)] == ref.map_get(m, kf)
        lists = [kfs, kfs[::-1], cand, [kfs[3], 10 ** 6, kfs[1]], [10 ** 6], []]
        for lst in lists:
            got = [int(x) for x in hip.map_points(lst)]
            assert got == ref.map_points(m, lst)
            # UpdateLocalPoints with nobody voting: the caller's list is taken as it is
            assert got == [int(x) for x in hip.update_local_map([], [], lst, max_kfs=len(lst))["local_rows"]]
        hip.update_local_map(*random_frame(m, 40, case))
        assert _list_state(hip) == "kept"
        hip.map_get(kfs[0]); hip.map_points(kfs)
        assert _list_state(hip) == "kept"                            # neither changes the version
        # the capacity round trips
        n_row, n_pts = len(m.kf_points[kfs[0]]), len(ref.map_points(m, kfs))
        rc, n, _ = hip.map_get_raw(kfs[0], n_row - 1)
        assert (rc, n) == (ASD_ERR_CAPACITY, n_row)
        rc, n, rows = hip.map_get_raw(kfs[0], n)
        assert rc == 0 and [int(x) for x in rows] == ref.map_get(m, kfs[0])
        rc, n, _ = hip.map_points_raw(kfs, n_pts - 1)
        assert (rc, n) == (ASD_ERR_CAPACITY, n_pts)
        rc, n, rows = hip.map_points_raw(kfs, n)
        assert rc == 0 and [int(x) for x in rows] == ref.map_points(m, kfs)
        rc, n, _ = hip.map_points_raw(kfs, 0)
        assert (rc, n) == (ASD_ERR_CAPACITY, n_pts)
        for call in (lambda: hip.map_get(10 ** 6), lambda: hip.map_points([kfs[0], kfs[1], kfs[0]])):
            with pytest.raises(Exception) as e:
                call()
            assert e.value.code == ASD_ERR_INVALID
    # a row longer than a tile of the compaction
    m, _ = random_case(8, 1500, 1400, 12, 0.8, ids=range(1, 9))
    load(hip, m)
    assert [int(x) for x in hip.map_points([3, 1, 8])] == ref.map_points(m, [3, 1, 8])
    assert [int(x) for x in hip.map_get(8)] == ref.map_get(m, 8)
    hip.map_clear()
    assert len(hip.map_points([1, 2])) == 0


@pytest.mark.gpu
def test_errors_and_the_armed_call_rule(hip, synth):
    m, kf, cand, best = random_fuse_case(RANDOM_SHAPES[1], 3, 0)
    load(hip, m)
    hip.update_local_map(*random_frame(m, 40, 1))
    n_kp = len(m.kf_points[kf])
    before = (_rows(hip, m), hip.map_debug(), list(hip.map_observations(_all_points(m))), [int(x) for x in hip.map_points(sorted(m.kf_points))])
    big = np.arange(2 ** 20 + 1, dtype=np.int32)
    bad_calls = [(lambda: hip.fuse_apply(10 ** 6, cand, best, 0, True), ASD_ERR_INVALID, "keyframe 1000000"),
                 (lambda: hip.fuse_apply(kf, cand[:3], [0, n_kp, 1], 0, True), ASD_ERR_INVALID, f"best_idx {n_kp}"),
                 (lambda: hip.fuse_apply(kf, cand[:3], [0, -2, 1], 0, True), ASD_ERR_INVALID, "best_idx -2"),
                 (lambda: hip.fuse_apply(kf, [cand[0], cand[1], cand[0]], [0, 1, -1], 0, True), ASD_ERR_INVALID, f"row {cand[0]} occurs twice"),
                 (lambda: hip.fuse_apply(kf, [cand[0], 2 ** 28], [0, 1], 0, True), ASD_ERR_INVALID, f"row {2 ** 28}"),
                 (lambda: hip.fuse_apply(kf, [cand[0], -2], [0, 1], 0, True), ASD_ERR_INVALID, "row -2"),
                 (lambda: hip.fuse_apply(kf, cand, best, 3, True), ASD_ERR_INVALID, "mode 3"),
                 (lambda: hip.fuse_apply(kf, cand, best, -1, True), ASD_ERR_INVALID, "mode -1"),
                 (lambda: hip.fuse_apply(kf, big, np.full(len(big), -1, np.int32), 0, True), ASD_ERR_CAPACITY, "candidates")]
    for call, code, words in bad_calls:
        with pytest.raises(Exception) as e:
            call()
        assert e.value.code == code and words in str(e.value), str(e.value)
        assert (_rows(hip, m), hip.map_debug(), list(hip.map_observations(_all_points(m))), [int(x) for x in hip.map_points(sorted(m.kf_points))]) == before
    assert _list_state(hip) == "kept"
    _fuse(hip, m, kf, cand, best, 0, False)
    # while an armed asd_track_* call is unfinished every new entry is refused like every call of the section
    n_mp = 300
    kc, dc = make_frame(2000, 290)
    K = np.array(synth.KITTI_K, np.float32)
    T = pose_T()
    rng = np.random.default_rng(41)
    src = rng.integers(0, 2000, n_mp)
    uv = np.stack([kc["x"][src], kc["y"][src]], 1) + rng.uniform(-1.5, 1.5, (n_mp, 2)).astype(np.float32)
    Xw = backproject(T, K, uv, rng.uniform(3, 60, n_mp))
    Ow = -(T[:3, :3].astype(np.float64).T @ T[:3, 3].astype(np.float64))
    normal = Xw.astype(np.float64) - Ow
    dist = np.linalg.norm(normal, axis=1)
    normal = (normal / dist[:, None]).astype(np.float32)
    maxd = (dist * SCALES[kc["octave"][src]] * 1.2).astype(np.float32)
    mind = (maxd / np.float32(SCALES[7]) * 0.8).astype(np.float32)
    hip.frame_set(0, kc, dc, BOUNDS)
    base = 12000
    hip.bank_put(base, perturbed_descriptors(dc[src], 0.05, 42))
    hip.mpbank_put(base, Xw, normal, mind, maxd)
    occupied = np.zeros(2000, np.uint8)
    cur_Xw = np.zeros((2000, 3), np.float32)
    pose0 = _pose7(pose_T(rv=(0.011, -0.021, 0.004), t=(0.09, -0.06, 0.31)))
    rows = np.arange(base, base + n_mp, dtype=np.int32)
    assert hip.track_local_points_rows(0, 2000, rows, T, K, occupied, cur_Xw, 1.0, 0.8, pose0, split=True) is None
    for call in (lambda: hip.fuse_apply(kf, cand, best, 0, True), lambda: hip.map_get(kf), lambda: hip.map_points([kf])):
        with pytest.raises(Exception) as e:
            call()
        assert e.value.code == ASD_ERR_INVALID and "asd_track_finish" in str(e.value)
    hip.track_finish()
    _fuse(hip, m, kf, cand, best, 0, True)
    _check_table(hip, m)
    hip.map_clear()
