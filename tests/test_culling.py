"""asd_keyframe_culling, asd_map_observations and asd_map_put_octaves on the device against tests/culling_ref.py (which
tests/test_culling_ref.py pins by hand): decisions, nMPs, nRedundantObservations and bad_rows in order must be equal, exactly, and so
must everything the existing queries read from the table after a cull was applied."""
import numpy as np
import pytest

from tests.culling_cases import RANDOM_SHAPES, assert_same, hand_cases, load, mk, random_case, without_erasure
from tests.local_map_cases import assert_same as assert_same_local_map
from tests.local_map_cases import random_frame
from tests.test_matcher import BOUNDS, SCALES, backproject, make_frame, perturbed_descriptors, pose_T
from tests.test_track_chain import _pose7

ASD_ERR_INVALID, ASD_ERR_CAPACITY = -1, -5
SEED = 1


def _cull(hip, m, cand, flags=None, apply=False):
    flags = [0] * len(cand) if flags is None else flags
    exp = m.keyframe_culling(cand, flags, apply)
    got = hip.keyframe_culling(cand, flags, apply)
    assert_same(got, exp)
    return exp


def _all_points(m):
    return sorted({p for row in m.kf_points.values() for p in row if p >= 0} | set(m.pt_bad) | set(m.obs))


def _check_table(hip, m, frames=()):
    """everything the existing calls read from the table, against the restatement's map"""
    pts = _all_points(m)
    assert list(hip.map_observations(pts)) == m.observations(pts)
    kfs = sorted(m.kf_points)
    for kf in (kfs[0], kfs[len(kfs) // 2], kfs[-1]):
        gk, gc = hip.map_shared_counts(kf)
        assert [(int(a), int(b)) for a, b in zip(gk, gc)] == m.shared_counts(kf)
    for cur, seen in frames:
        assert_same_local_map(hip.update_local_map(cur, seen, kfs[:3]), m.update_local_map(cur, seen, kfs[:3]))


def _list_state(hip):
    """what asd_track_local_points_map says about the resident search list, asked with a frame slot that does not exist: 'changed' when a
    table change has invalidated the list, another refusal when the list is still good"""
    z = np.zeros(16, np.float32)
    with pytest.raises(Exception):                                  # (a refusal without a message of its own leaves the last one: make that one known)
        hip.map_observations([-2])
    with pytest.raises(Exception) as e:
        hip.track_local_points_map(1000, 4, z, z[:4], np.zeros(4, np.uint8), np.zeros((4, 3), np.float32), 1.0, 0.8, np.zeros(7))
    assert e.value.code == ASD_ERR_INVALID
    return "changed" if "changed" in str(e.value) else "kept"


@pytest.fixture(scope="module")
def random_cases():
    """the random maps at the shapes of the issue, each with the restatement's answer for its candidates (computed once)"""
    out = []
    for n_kf, n_kp, n_points, fill in RANDOM_SHAPES:
        m, cand = random_case(n_kf, n_kp, n_points, SEED, fill)
        out.append((m, cand, m.keyframe_culling(cand, [0] * len(cand), False)))
    return out


def test_random_cases_are_not_degenerate(random_cases):
    """asserted on the restatement's output: >= 2 culls in every case, a cascaded bad point and an outcome that depends on the in-loop
    erasure in at least one"""
    cascades = order_dependent = 0
    for m, cand, exp in random_cases:
        culled = [int(d == 1) for d in exp["decision"]]
        assert sum(culled) >= 2
        cascades += len(exp["bad_rows"]) > 0
        order_dependent += culled != without_erasure(m, cand)
    assert cascades >= 1 and order_dependent >= 1


@pytest.mark.gpu
def test_hand_worked_maps(hip):
    for name, m, cand, flags, want in hand_cases():
        load(hip, m)
        exp = _cull(hip, m, cand, flags, apply=False)
        assert (exp["decision"], exp["n_mps"], exp["n_redundant"], exp["bad_rows"]) == want, name
        _cull(hip, m, cand, flags, apply=True)
        _check_table(hip, m)
        _cull(hip, m, sorted(m.kf_points), apply=False)            # and what every keyframe looks like now
    hip.map_clear()
    got = hip.keyframe_culling([], [])
    assert len(got["decision"]) == 0 and len(got["bad_rows"]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(RANDOM_SHAPES)))
def test_random_maps_equal_the_restatement(hip, random_cases, case):
    m, cand, exp = random_cases[case]
    m = m._copy()
    load(hip, m)
    kfs = sorted(m.kf_points)
    frames = [random_frame(m, 40, 10 * case + q) for q in range(2)]
    _check_table(hip, m, frames)
    d0 = hip.map_debug()
    # apply = 0: twice the same, nothing moved, the search list still good
    got = hip.keyframe_culling(cand)
    assert_same(got, exp)
    again = hip.keyframe_culling(cand)
    for k in ("decision", "n_mps", "n_redundant", "bad_rows"):
        np.testing.assert_array_equal(got[k], again[k])
    assert hip.map_debug() == d0 and _list_state(hip) == "kept"
    _check_table(hip, m, frames[-1:])
    # flags: some candidates skipped, some held by mbNotErase
    rng = np.random.default_rng(70 + case)
    flags = rng.choice([0, 0, 0, 1, 2, 3], len(cand)).astype(np.uint8)
    _cull(hip, m, cand, flags)
    _cull(hip, m, cand[:1])
    _cull(hip, m, kfs)                                              # every live keyframe
    # the bad_capacity round trip leaves the table alone, whatever apply says
    if len(exp["bad_rows"]) > 0:
        rc, out = hip.keyframe_culling_raw(cand, np.zeros(len(cand), np.uint8), True, len(exp["bad_rows"]) - 1)
        assert rc == ASD_ERR_CAPACITY and out["n_bad"] == len(exp["bad_rows"])
        assert _list_state(hip) == "kept"
        _check_table(hip, m)
    # apply = 1
    assert_same(_cull(hip, m, cand, apply=True), exp)
    assert _list_state(hip) == "changed"
    _check_table(hip, m, frames)
    _cull(hip, m, cand, apply=True)                                 # the second run, on the mutated map
    _cull(hip, m, kfs, flags=rng.choice([0, 2], len(kfs)).astype(np.uint8), apply=True)
    _check_table(hip, m, frames)


@pytest.mark.gpu
def test_shapes_the_kernels_can_get_wrong(hip):
    # rows of 33 entries (47 is among the random shapes): no multiple of the wave
    m, cand = random_case(23, 33, 80, 11, 0.8)
    load(hip, m)
    assert sum(d == 1 for d in _cull(hip, m, cand)["decision"]) >= 2
    # rows of 1500 entries, longer than the workgroup of the walk and than a tile of the compaction
    m, cand = random_case(8, 1500, 1400, 12, 0.8, ids=range(1, 9))
    load(hip, m)
    exp = _cull(hip, m, cand, apply=True)
    assert sum(d == 1 for d in exp["decision"]) >= 2 and len(exp["bad_rows"]) > 20
    _check_table(hip, m)
    # 300 keyframes x 4 keypoints that observe the same 3 points: every count lands on three addresses
    rng = np.random.default_rng(13)
    m = mk({kf: [int(x) for x in rng.permutation([7, 8, 9, -1])] for kf in range(1, 301)},
           {kf: [int(x) for x in rng.integers(0, 3, 4)] for kf in range(1, 301)})
    load(hip, m)
    assert list(hip.map_observations([7, 8, 9, 10])) == [300, 300, 300, 0]
    kfs = sorted(m.kf_points)
    exp = _cull(hip, m, kfs)
    assert sum(d == 1 for d in exp["decision"]) > 250
    _cull(hip, m, kfs, apply=True)
    _check_table(hip, m)
    # sparse ids up to 2^31 - 2, rows beyond the initial row tables
    ids = np.sort(np.concatenate([np.random.default_rng(14).choice(2 ** 31 - 2, 39, replace=False), [2 ** 31 - 2]]))
    m, cand = random_case(40, 48, 200, 14, 0.8, ids=ids, row0=250000)
    load(hip, m)
    exp = _cull(hip, m, cand)
    assert sum(d == 1 for d in exp["decision"]) >= 2
    _cull(hip, m, [int(ids[-1])])
    _cull(hip, m, [int(i) for i in ids], apply=True)
    _check_table(hip, m)
    hip.map_clear()


@pytest.mark.gpu
def test_observations(hip):
    m, _ = random_case(64, 64, 300, 21, 0.7)
    load(hip, m)
    rows = list(range(0, 300)) + [5, 5, 299, 300, 4095, 4096, 70000] + sorted(m.pt_bad)   # twice, never named, beyond the row tables, bad
    exp = m.observations(rows)
    assert max(exp) > 3 and 0 in exp and any(m.observations([p])[0] > 0 for p in m.pt_bad)
    d0 = hip.map_debug()
    assert list(hip.map_observations(rows)) == exp
    assert list(hip.map_observations(rows)) == exp
    assert hip.map_debug() == d0                                    # not even the row tables grow for a row nobody names
    assert len(hip.map_observations([])) == 0
    with pytest.raises(Exception) as e:
        hip.map_observations([3, -1])
    assert e.value.code == ASD_ERR_INVALID
    hip.map_clear()
    assert list(hip.map_observations([0, 9])) == [0, 0]


@pytest.mark.gpu
def test_octave_lifetime_and_growth(hip):
    m, cand = random_case(40, 48, 900, 31, 0.8)
    load(hip, m)
    cur, seen = random_frame(m, 40, 3)
    hip.update_local_map(cur, seen)
    assert _list_state(hip) == "kept"
    kf = cand[0]
    hip.map_put_octaves(kf, m.octave[kf])                           # setting octaves leaves the search list alone
    assert _list_state(hip) == "kept"
    _cull(hip, m, cand)
    # a put with the same n keeps them
    row = list(m.kf_points[kf])
    row[0], row[1] = row[1], row[0]
    m.put_keyframe(kf, row)
    hip.map_put(kf, row)
    _cull(hip, m, cand)
    # another n drops them: culling is refused and names the keyframe
    m.put_keyframe(kf, row[:-1])
    hip.map_put(kf, row[:-1])
    assert kf not in m.octave
    with pytest.raises(Exception) as e:
        hip.keyframe_culling(cand)
    assert e.value.code == ASD_ERR_INVALID and f"keyframe {kf} " in str(e.value)
    m.put_octaves(kf, [3] * (len(row) - 1))
    hip.map_put_octaves(kf, m.octave[kf])
    _cull(hip, m, cand)
    # erase drops them with the row: the id put again has none
    other = cand[1]
    old = m.octave[other]
    m.erase_keyframe(other)
    hip.map_erase(other)
    _cull(hip, m, [c for c in cand if c != other])
    m.put_keyframe(other, [5, 6])
    hip.map_put(other, [5, 6])
    with pytest.raises(Exception) as e:
        hip.keyframe_culling(cand)
    assert e.value.code == ASD_ERR_INVALID and f"keyframe {other} " in str(e.value)
    with pytest.raises(Exception) as e:
        hip.map_put_octaves(other, old)                             # the old octaves no longer fit
    assert e.value.code == ASD_ERR_INVALID
    m.put_octaves(other, [0, 1])
    hip.map_put_octaves(other, [0, 1])
    # map_set does not touch them
    free = [p for p in range(900) if kf not in m.obs.get(p, {})][0]
    m.set_entry(kf, 2, free)
    hip.map_set(kf, [2], [free])
    _cull(hip, m, cand)
    # a row longer than the arena arrives: every row moves, the octaves with it
    d0 = hip.map_debug()
    rng = np.random.default_rng(32)
    long_row = np.full(20000, -1, np.int64)
    long_row[rng.choice(20000, 700, replace=False)] = rng.choice(900, 700, replace=False)
    m.put_keyframe(5000, long_row)
    hip.map_put(5000, long_row)
    m.put_octaves(5000, rng.integers(0, 8, 20000))
    hip.map_put_octaves(5000, m.octave[5000])
    assert hip.map_debug()[6] > d0[6]
    _cull(hip, m, cand + [5000])
    _cull(hip, m, [5000] + cand, apply=True)
    _check_table(hip, m, [(cur, seen)])
    hip.map_clear()
    hip.map_put(3, [1, 2])
    with pytest.raises(Exception) as e:                             # clear dropped everything
        hip.keyframe_culling([3])
    assert e.value.code == ASD_ERR_INVALID and "keyframe 3 " in str(e.value)
    hip.map_clear()


@pytest.mark.gpu
def test_errors_and_the_armed_call_rule(hip, synth):
    name, m, cand, flags, want = [c for c in hand_cases() if c[0] == "cascade"][0]
    load(hip, m)
    for call in (lambda: hip.map_put_octaves(10, [0] * 10 + [16]), lambda: hip.map_put_octaves(10, [0] * 10), lambda: hip.map_put_octaves(999, [0]),
                 lambda: hip.keyframe_culling([10, 11, 10]), lambda: hip.keyframe_culling([10, 999]), lambda: hip.map_observations([-2])):
        with pytest.raises(Exception) as e:
            call()
        assert e.value.code == ASD_ERR_INVALID
    with pytest.raises(Exception) as e:
        hip.keyframe_culling(list(range(4097)))
    assert e.value.code == ASD_ERR_CAPACITY
    # the capacity answer, the table untouched in between, the repeat
    pts = _all_points(m)
    obs = list(hip.map_observations(pts))
    rc, out = hip.keyframe_culling_raw(cand, flags, True, 0)
    assert rc == ASD_ERR_CAPACITY and out["n_bad"] == 1
    assert list(hip.map_observations(pts)) == obs == m.observations(pts)
    rc, out = hip.keyframe_culling_raw(cand, flags, True, out["n_bad"])
    assert rc == 0
    assert ([int(x) for x in out["decision"]], [int(x) for x in out["n_mps"]], [int(x) for x in out["n_redundant"]], [int(x) for x in out["bad_rows"]]) == want
    m.keyframe_culling(cand, flags, True)
    _check_table(hip, m)
    # while an armed asd_track_* call is unfinished the three calls are refused like every call of the section
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
    for call in (lambda: hip.map_put_octaves(12, [0]), lambda: hip.keyframe_culling([12]), lambda: hip.map_observations([200])):
        with pytest.raises(Exception) as e:
            call()
        assert e.value.code == ASD_ERR_INVALID and "asd_track_finish" in str(e.value)
    hip.track_finish()
    _cull(hip, m, [12, 20])
    hip.map_clear()
