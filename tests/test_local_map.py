"""asd_update_local_map, asd_map_shared_counts and asd_track_local_points_map on the device against tests/local_map_ref.py (which
tests/test_local_map_ref.py pins by hand): every output is a list of integers and must be equal, exactly."""
import numpy as np
import pytest

from tests.local_map_cases import assert_same, load, random_frame, random_map
from tests.local_map_ref import RefMap
from tests.test_matcher import BOUNDS, SCALES, backproject, make_frame, perturbed_descriptors, pose_T
from tests.test_track_chain import _pose7

ASD_ERR_INVALID, ASD_ERR_CAPACITY = -1, -5


def _query(hip, m, cur, seen=(), prev=(), max_kfs=80):
    exp = m.update_local_map(cur, seen, prev, max_kfs)
    got = hip.update_local_map(cur, seen, prev, max_kfs)
    assert_same(got, exp)
    return exp


def _hand_maps():
    """the maps of tests/test_local_map_ref.py: (map, cur, seen, prev, max_kfs)"""
    out = []

    def mk(kfs):
        m = RefMap()
        for kf, pts in kfs.items():
            m.put_keyframe(kf, pts)
        return m
    m = mk({1: [100, -1], 2: [-1, 100], 10: [101], 20: [102]})                      # the parent break
    m.set_links(1, [], [], 10)
    m.set_links(2, [20], [], -1)
    out.append((m, [100], [], [], 80))
    m = mk({1: [100], 5: [100, 103], 6: [104], 7: [105], 8: [106], 9: [107, 100]})    # a bad covisible skipped, the parent without a bad test
    m.kf_bad |= {7, 9}
    m.set_links(1, [7, 8, 6], [6, 5], 9)
    out.append((m, [100], [], [], 80))
    for n in (80, 81):                                                               # the more-than-80 stop
        m = mk({k: [5] for k in range(n)})
        for k in range(n):
            m.set_links(k, [1000 + k], [], -1)
            m.put_keyframe(1000 + k, [6 + k])
        out.append((m, [5], [], [], 80))
    m = mk({5: [100, 101], 3: [101, 100], 9: [-1, 100], 4: [100, 101, 102]})         # the lowest-id maximum; a bad maximum
    out.append((m, [100, 101, -1], [], [], 80))
    m = mk({5: [100, 101], 3: [101, 100], 9: [-1, 100], 4: [100, 101, 102]})
    m.kf_bad.add(4)
    out.append((m, [100, 101, 102], [], [], 80))
    m = mk({5: [100, 101], 3: [101, 100]})                                           # every voted keyframe bad
    m.kf_bad |= {3, 5}
    out.append((m, [100], [], [3, 5], 80))
    m = mk({1: [100, 101], 2: [101, 102], 3: [103]})                                 # nobody votes
    m.kf_bad.add(2)
    m.pt_bad.add(100)
    out.append((m, [-1, 100, -1], [102], [2, 77, 1, 2], 80))
    m = mk({1: [101], 2: [100]})                                                     # a point held twice votes twice
    out.append((m, [100, 101, 100], [], [], 80))
    m = mk({1: [5], 2: [5], 3: [5], 11: [], 12: [], 13: []})                         # the bound as a parameter
    for k in (1, 2, 3):
        m.set_links(k, [10 + k], [], -1)
    out.append((m, [5], [], [], 3))
    return out


@pytest.mark.gpu
def test_hand_worked_maps(hip):
    for m, cur, seen, prev, max_kfs in _hand_maps():
        load(hip, m)
        _query(hip, m, cur, seen, prev, max_kfs)
    # an empty table: the caller's list comes back, no points
    hip.map_clear()
    got = hip.update_local_map([3, -1, 4], [], [9, 8])
    assert list(got["local_kfs"]) == [9, 8] and got["ref_kf"] == -1 and len(got["local_rows"]) == 0 and len(got["search_rows"]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n_kf,n_kp,seed,sparse", [(6, 8, 1, False), (23, 33, 2, True), (64, 64, 3, False), (120, 47, 4, True), (97, 64, 5, False)])
def test_random_maps_equal_the_restatement(hip, n_kf, n_kp, seed, sparse):
    """votes, list, expansion, points, search list and KFcounter on maps of 6-120 keyframes x 8-64 keypoints: sparse and large keyframe
    ids, rows far beyond the initial row tables, links that name absent ids, bad keyframes and points, stage-1 outliers in seen_rows"""
    rng = np.random.default_rng(100 + seed)
    ids = np.sort(rng.choice(2 ** 31 - 1, n_kf, replace=False)) if sparse else None
    m = random_map(n_kf, n_kp, seed, ids=ids, row0=250000 if sparse else 0)
    load(hip, m)
    kfs = sorted(m.kf_points)
    for q in range(4):
        cur, seen = random_frame(m, 40 + 7 * q, 10 * seed + q)
        exp = _query(hip, m, cur, seen, prev=kfs[:3])
        assert exp["ref_kf"] >= 0 and len(exp["local_rows"]) > len(exp["search_rows"])
    _query(hip, m, np.full(9, -1, np.int32), [], prev=[kfs[-1], 5, kfs[0]])          # nobody votes
    for kf in (kfs[0], kfs[len(kfs) // 2], kfs[-1]):
        gk, gc = hip.map_shared_counts(kf)
        exp = m.shared_counts(kf)
        assert [(int(a), int(b)) for a, b in zip(gk, gc)] == exp
    # both capacity returns and the repeat
    cur, seen = random_frame(m, 64, 99 + seed)
    exp = m.update_local_map(cur, seen)
    rc, out = hip.update_local_map_raw(cur, seen, [], 80, 1, 2, 3)
    assert rc == ASD_ERR_CAPACITY
    assert (out["n_local_kfs"], out["n_local"], out["n_search"]) == (len(exp["local_kfs"]), len(exp["local_rows"]), len(exp["search_rows"]))
    rc, out = hip.update_local_map_raw(cur, seen, [], 80, out["n_local_kfs"], out["n_local"], out["n_search"])
    assert rc == 0
    assert_same(out, exp)
    exp_c = m.shared_counts(kfs[1])
    if len(exp_c) > 1:
        with pytest.raises(Exception) as e:
            hip.map_shared_counts(kfs[1], capacity=len(exp_c) - 1)
        assert e.value.code == ASD_ERR_CAPACITY and f"[n = {len(exp_c)}]" in str(e.value)
    gk, gc = hip.map_shared_counts(kfs[1], capacity=len(exp_c))
    assert [(int(a), int(b)) for a, b in zip(gk, gc)] == exp_c


@pytest.mark.gpu
def test_table_changes_and_growth(hip):
    """erase / put again / set / flags followed by repeated queries, with more keyframes than the initial slot table (64) and a row longer
    than the initial arena (16384 entries) arriving mid-test"""
    m = random_map(40, 48, 21, n_points=900)
    load(hip, m)
    d0 = hip.map_debug()
    cur, seen = random_frame(m, 60, 5)
    _query(hip, m, cur, seen)
    rng = np.random.default_rng(22)
    more = random_map(90, 48, 23, ids=range(1000, 1090), n_points=900)
    for kf in sorted(more.kf_points):                         # 130 keyframes: the slot table grows
        m.put_keyframe(kf, more.kf_points[kf])
        hip.map_put(kf, more.kf_points[kf])
        m.set_links(kf, more.cov[kf], more.children[kf], more.parent[kf])
        hip.map_kf_links(kf, more.cov[kf], more.children[kf], more.parent[kf])
    _query(hip, m, cur, seen)
    long_row = np.full(20000, -1, np.int64)                   # the arena grows (and moves every row)
    long_row[rng.choice(20000, 700, replace=False)] = rng.choice(900, 700, replace=False)
    m.put_keyframe(5000, long_row)
    hip.map_put(5000, long_row)
    d1 = hip.map_debug()
    assert d1[0] == 131 and d1[5] > d0[5] and d1[6] > d0[6] and d1[2] >= 131 and d1[3] >= d1[1]
    _query(hip, m, cur, seen)
    gk, gc = hip.map_shared_counts(5000)
    assert [(int(a), int(b)) for a, b in zip(gk, gc)] == m.shared_counts(5000)
    # erase (an unknown id is fine), put again under the same id with a shorter and a longer row, single entries
    for kf in (3, 1007, 424242):
        m.erase_keyframe(kf)
        hip.map_erase(kf)
    _query(hip, m, cur, seen)
    m.put_keyframe(3, long_row[:30])
    hip.map_put(3, long_row[:30])
    m.put_keyframe(4, np.concatenate([np.asarray(m.kf_points[4]), [-1, -1, -1]]))
    hip.map_put(4, m.kf_points[4])
    free = [p for p in range(900) if 9 not in m.obs.get(p, {})][:4]
    idx = [i for i, p in enumerate(m.kf_points[9]) if p < 0][:2] + [i for i, p in enumerate(m.kf_points[9]) if p >= 0][:2]
    vals = [free[0], free[1], -1, free[2]]                    # AddObservation x2, EraseObservation, Replace
    for i, v in zip(idx, vals):
        m.set_entry(9, i, v)
    hip.map_set(9, idx, vals)
    m.kf_bad.add(12)
    hip.map_kf_bad(12, True)
    m.kf_bad.discard(next(iter(sorted(m.kf_bad))))
    for kf in sorted(m.kf_points):
        hip.map_kf_bad(kf, kf in m.kf_bad)
    flip = [int(p) for p in cur if p >= 0][:3]
    m.pt_bad |= set(flip)
    hip.map_point_bad(flip, True)
    some = sorted(m.pt_bad)[:2]
    m.pt_bad -= set(some)
    hip.map_point_bad(some, False)
    for q in range(3):
        c2, s2 = random_frame(m, 50, 30 + q)
        _query(hip, m, c2, s2, prev=[3, 4, 9])
    _query(hip, m, cur, seen)
    # errors leave the table as it was
    for call in (lambda: hip.map_set(424242, [0], [1]), lambda: hip.map_set(9, [48], [1]), lambda: hip.map_kf_bad(424242),
                 lambda: hip.map_kf_links(424242, [], [], -1), lambda: hip.map_kf_links(9, list(range(11)), [], -1),
                 lambda: hip.map_kf_links(9, [], [5, 5], -1), lambda: hip.map_put(-1, [0]), lambda: hip.map_put(7, [-2])):
        with pytest.raises(Exception) as e:
            call()
        assert e.value.code == ASD_ERR_INVALID
    with pytest.raises(Exception) as e:
        hip.map_put(7, np.zeros(70000, np.int32))
    assert e.value.code == ASD_ERR_CAPACITY and "65536" in str(e.value)
    _query(hip, m, cur, seen)
    hip.map_clear()
    assert hip.map_debug()[:2] == (0, 0)


@pytest.fixture(scope="module")
def large_case():
    """about 300 keyframes x 2000 keypoints; most keyframes are voted, so the compaction runs over some 600 tiles of 1024 entries (2000 is
    no multiple of the 256-thread rounds, and the tile scan needs more than one block of 256)"""
    m = random_map(300, 2000, 77, n_points=30000, fill=0.7, bad_kf=0.03)
    rng = np.random.default_rng(78)
    cur = np.full(2000, -1, np.int32)
    cur[rng.choice(2000, 1500, replace=False)] = rng.choice(30000, 1500, replace=False)
    cur[:5] = cur[cur >= 0][:5]
    seen = rng.choice(30000, 40, replace=False).astype(np.int32)
    return m, cur, seen, m.update_local_map(cur, seen)


@pytest.mark.gpu
def test_large_map_and_repeated_call(hip, large_case):
    m, cur, seen, exp = large_case
    assert len(exp["local_kfs"]) > 256 and len(exp["local_rows"]) > 20000
    load(hip, m)
    got = hip.update_local_map(cur, seen)
    assert_same(got, exp)
    again = hip.update_local_map(cur, seen)
    for k in ("local_kfs", "local_rows", "search_rows"):
        np.testing.assert_array_equal(got[k], again[k])
    kf = exp["ref_kf"]
    gk, gc = hip.map_shared_counts(kf)
    assert [(int(a), int(b)) for a, b in zip(gk, gc)] == m.shared_counts(kf)
    hip.map_clear()


@pytest.mark.gpu
@pytest.mark.parametrize("n_mp,th", [(4000, 1.0), (900, 3.0)])
def test_track_local_points_map_equals_rows(hip, synth, n_mp, th):
    """asd_track_local_points_map (the search list resident on the device) against asd_track_local_points_rows given the returned list:
    every output bit-equal, synchronous and split in two; the refusals of the call and the armed-call rule of the table"""
    kc, dc = make_frame(2000, 290)
    K = np.array(synth.KITTI_K, np.float32)
    T = pose_T()
    rng = np.random.default_rng(291 + n_mp)
    src = rng.integers(0, 2000, n_mp)
    uv = np.stack([kc["x"][src], kc["y"][src]], 1) + rng.uniform(-1.5, 1.5, (n_mp, 2)).astype(np.float32)
    uv[: n_mp // 12] += 2500
    depth = rng.uniform(3, 60, n_mp)
    depth[n_mp // 12: n_mp // 8] *= -1
    Xw = backproject(T, K, uv, depth)
    Ow = -(T[:3, :3].astype(np.float64).T @ T[:3, 3].astype(np.float64))
    normal = Xw.astype(np.float64) - Ow
    dist = np.linalg.norm(normal, axis=1)
    normal = normal / dist[:, None] + rng.normal(0, 0.45, normal.shape)
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
    maxd = (dist * SCALES[kc["octave"][src]] * rng.uniform(0.7, 1.4, n_mp)).astype(np.float32)
    mind = (maxd / np.float32(SCALES[7]) * rng.uniform(0.8, 1.3, n_mp)).astype(np.float32)
    hip.frame_set(0, kc, dc, BOUNDS)
    base = 12000
    hip.bank_put(base, perturbed_descriptors(dc[src], 0.05, 292))
    hip.mpbank_put(base, Xw, normal, mind, maxd)
    occupied = (rng.uniform(size=2000) < 0.3).astype(np.uint8)
    cur_Xw = backproject(T, K, np.stack([kc["x"], kc["y"]], 1) + rng.uniform(-0.7, 0.7, (2000, 2)).astype(np.float32), rng.uniform(4, 50, 2000))
    pose0 = _pose7(pose_T(rv=(0.011, -0.021, 0.004), t=(0.09, -0.06, 0.31)))
    # eight keyframes whose rows cover the bank's points in a shuffled order, with overlap
    m = RefMap()
    n_kp = n_mp // 4
    for kf in range(8):
        row = np.full(n_kp + 11, -1, np.int64)
        row[rng.choice(n_kp + 11, n_kp, replace=False)] = base + rng.choice(n_mp, n_kp, replace=False)
        m.put_keyframe(kf, row)
    load(hip, m)
    cur_rows = np.full(2000, -1, np.int32)
    cur_rows[np.nonzero(occupied)[0][:40]] = base + rng.choice(n_mp, 40, replace=False)
    seen_rows = (base + rng.choice(n_mp, 9, replace=False)).astype(np.int32)
    exp = _query(hip, m, cur_rows, seen_rows)
    rows = np.asarray(exp["search_rows"], np.int32)
    assert 0.6 * n_mp < len(rows) < n_mp
    want = hip.track_local_points_rows(0, 2000, rows, T, K, occupied, cur_Xw, th, 0.8, pose0)
    assert want[1] > 0 and want[4] > 0
    got = hip.track_local_points_map(0, 2000, T, K, occupied, cur_Xw, th, 0.8, pose0)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    # split in two; while the call is armed and unfinished every call of the table is refused
    assert hip.track_local_points_map(0, 2000, T, K, occupied, cur_Xw, th, 0.8, pose0, split=True) is None
    for call in (lambda: hip.map_put(99, [base]), lambda: hip.map_set(0, [0], [-1]), lambda: hip.map_erase(0), lambda: hip.map_clear(),
                 lambda: hip.map_kf_bad(0), lambda: hip.map_kf_links(0, [], [], -1), lambda: hip.map_point_bad([base]),
                 lambda: hip.update_local_map(cur_rows), lambda: hip.map_shared_counts(0)):
        with pytest.raises(Exception) as e:
            call()
        assert e.value.code == ASD_ERR_INVALID and "asd_track_finish" in str(e.value)
    got = hip.track_finish()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    # the list is the last query's: a table change, an empty list and a cleared table are refused
    hip.map_kf_bad(3, False)
    with pytest.raises(Exception) as e:
        hip.track_local_points_map(0, 2000, T, K, occupied, cur_Xw, th, 0.8, pose0)
    assert e.value.code == ASD_ERR_INVALID and "changed" in str(e.value)
    _query(hip, m, cur_rows, seen_rows)
    got = hip.track_local_points_map(0, 2000, T, K, occupied, cur_Xw, th, 0.8, pose0)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    everything = np.unique(np.concatenate([np.asarray(r)[np.asarray(r) >= 0] for r in m.kf_points.values()])).astype(np.int32)
    exp = _query(hip, m, everything[:5], everything)
    assert len(exp["search_rows"]) == 0 and len(exp["local_rows"]) > 0
    with pytest.raises(Exception) as e:
        hip.track_local_points_map(0, 2000, T, K, occupied, cur_Xw, th, 0.8, pose0)
    assert e.value.code == ASD_ERR_INVALID and "empty" in str(e.value)
    hip.map_clear()
    with pytest.raises(Exception) as e:
        hip.track_local_points_map(0, 2000, T, K, occupied, cur_Xw, th, 0.8, pose0)
    assert e.value.code == ASD_ERR_INVALID
