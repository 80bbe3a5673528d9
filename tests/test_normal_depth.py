"""asd_map_kf_centers and asd_update_normal_and_depth on the device against tests/normal_depth_ref.py (which
tests/test_normal_depth_ref.py pins by hand): normals, ranges, statuses and the attribute bank as it stands afterwards, bit for bit."""
import numpy as np
import pytest

from tests import normal_depth_ref as ref
from tests.culling_cases import RANDOM_SHAPES, load, mk, random_case
from tests.local_map_cases import random_frame
from tests.normal_depth_cases import hand_cases, load_all, ref_kfs
from tests.test_matcher import BOUNDS, backproject, make_frame, perturbed_descriptors, pose_T
from tests.test_track_chain import _pose7

ASD_ERR_INVALID, ASD_ERR_CAPACITY = -1, -5


def _bank(hip, n):
    return hip.bank_get(0, n, desc=False)[1]


def _same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _update(hip, m, centres, bank, rows, ref_kf, Xw=None):
    """one call on the device and on the restatement (which changes `bank`): outputs and the whole bank must agree"""
    exp = ref.update_normal_and_depth(m, centres, bank, rows, ref_kf, hip.scale_tables()["scale"], Xw=Xw)
    got = hip.update_normal_and_depth(rows, ref_kf, Xw)
    assert list(got["status"]) == list(exp["status"])
    for k in ("normal", "min_dist", "max_dist"):
        ref.assert_bits(got[k], exp[k], k)
    ref.assert_bits(_bank(hip, len(bank)), bank, "bank")
    return exp


def _list_state(hip):
    """'changed' when a table change has invalidated the resident search list, 'kept' when asd_track_local_points_map refuses only the frame
    slot it is asked with (one that does not exist)"""
    z = np.zeros(16, np.float32)
    with pytest.raises(Exception):                                  # (a refusal without a message of its own leaves the last one: make that one known)
        hip.map_observations([-2])
    with pytest.raises(Exception) as e:
        hip.track_local_points_map(1000, 4, z, z[:4], np.zeros(4, np.uint8), np.zeros((4, 3), np.float32), 1.0, 0.8, np.zeros(7))
    assert e.value.code == ASD_ERR_INVALID
    return "changed" if "changed" in str(e.value) else "kept"


def _not_bad(m, n_points):
    return [p for p in range(n_points) if p not in m.pt_bad]


@pytest.fixture(scope="module")
def random_cases():
    """the random maps of the culling tests with centres in +-50 and a bank of positions in +-50 (built once, copied by the tests)"""
    out = []
    for k, (n_kf, n_kp, n_points, fill) in enumerate(RANDOM_SHAPES):
        m, cand = random_case(n_kf, n_kp, n_points, 1, fill)
        out.append((m, cand, ref.random_centres(m, 100 + k), ref.random_bank(n_points, 200 + k)))
    return out


@pytest.mark.gpu
def test_scale_table_is_the_restatements(hip):
    assert _same_bytes(hip.scale_tables()["scale"], ref.scale_table())


@pytest.mark.gpu
def test_hand_worked_maps(hip):
    for case in hand_cases():
        bank = case["bank"].copy()
        load_all(hip, case["map"], case["centres"], bank)
        exp = _update(hip, case["map"], case["centres"], bank, case["rows"], case["ref_kf"])
        assert list(exp["status"]) == list(case["status"]), case["name"]
        ref.assert_bits(exp["normal"], case["normal"], case["name"])
    assert hip.update_normal_and_depth([], [])["status"].shape == (0,)
    hip.map_clear()


@pytest.mark.gpu
def test_row_lengths_around_the_wave(hip):
    rng = np.random.default_rng(3)
    n_points = 140
    kfs, octs = {}, {}
    for kf, n in ((5, 1), (4, 63), (3, 64), (2, 65), (1, 130), (6, 130)):
        row = rng.permutation(n_points)[:n]
        row[rng.uniform(size=n) < 0.1] = -1
        kfs[kf], octs[kf] = [int(x) for x in row], [int(x) for x in rng.integers(0, 8, n)]
    m = mk(kfs, octs)
    centres, bank = ref.random_centres(m, 31), ref.random_bank(n_points + 2, 32)      # (the last two rows: observed by nobody)
    load_all(hip, m, centres, bank)
    rows = [int(x) for x in rng.permutation(n_points + 2)]
    exp = _update(hip, m, centres, bank, rows, ref_kfs(m, rows, 33))
    assert (exp["status"] == ref.UPDATED).sum() > 100 and (exp["status"] == ref.NO_OBSERVATIONS).sum() >= 2
    # the last entry of every row counts: the point there, asked for alone
    for kf in kfs:
        named = [p for p in kfs[kf] if p >= 0]
        if named:
            _update(hip, m, centres, bank, named[-1:], [kf])
    hip.map_clear()


@pytest.mark.gpu
def test_one_point_observed_by_300_keyframes(hip):
    rng = np.random.default_rng(4)
    ids = [int(x) for x in rng.permutation(np.arange(1, 301) * 7)]
    kfs, octs = {}, {}
    for kf in ids:
        row = [-1, -1, -1, -1]
        row[int(rng.integers(4))] = 7
        kfs[kf], octs[kf] = row, [int(x) for x in rng.integers(0, 8, 4)]
    m = mk(kfs, octs)
    centres = ref.random_centres(m, 41)
    bank = ref.random_bank(16, 42)
    # shuffled insertion order, so the slot order is not the id order; keyframe 5000 takes a slot first and leaves it to ids[150]
    hip.map_clear()
    hip.map_put(5000, [7, 3])
    for kf in ids[:150]:
        hip.map_put(kf, kfs[kf])
    hip.map_erase(5000)
    for kf in ids[150:]:
        hip.map_put(kf, kfs[kf])
    for kf in ids:
        hip.map_put_octaves(kf, octs[kf])
    hip.map_kf_centers(ids, np.array([centres[k] for k in ids], np.float32))
    hip.mpbank_put(0, bank[:, 0:3], bank[:, 3:6], bank[:, 6], bank[:, 7])
    assert list(hip.map_observations([7])) == [300]
    asc = sorted(ids)
    Ow = [centres[k] for k in asc]
    up = ref.point(Ow, 0, bank[7, 0:3], 1.0, 2.0)[0]
    shuffled = ref.point(Ow, 0, bank[7, 0:3], 1.0, 2.0, order=[asc.index(k) for k in ids])[0]
    assert not _same_bytes(up, shuffled)                             # the order is visible in this sum
    exp = _update(hip, m, centres, bank, [7, 3], [asc[-1], asc[0]])
    assert list(exp["status"]) == [ref.UPDATED, ref.NO_OBSERVATIONS]
    again = hip.update_normal_and_depth([3, 7], [asc[0], asc[-1]])
    assert _same_bytes(again["normal"][1], exp["normal"][0])
    hip.map_clear()


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(RANDOM_SHAPES)))
def test_random_maps_equal_the_restatement(hip, random_cases, case):
    m, _cand, centres, bank0 = random_cases[case]
    bank = bank0.copy()
    n_points = len(bank)
    load_all(hip, m, centres, bank)
    rng = np.random.default_rng(300 + case)
    rows = [int(x) for x in rng.permutation(_not_bad(m, n_points))]
    refs = ref_kfs(m, rows, 310 + case)
    d0 = hip.map_debug()
    exp = _update(hip, m, centres, bank, rows, refs)
    assert (exp["status"] == ref.UPDATED).sum() > len(rows) // 2
    first = _bank(hip, n_points)
    again = hip.update_normal_and_depth(rows, refs)
    assert all(_same_bytes(again[k], exp[k]) for k in ("normal", "min_dist", "max_dist")) and _same_bytes(_bank(hip, n_points), first)
    # the write-back form for a subset: positions moved by up to 0.1; only those rows change
    sub = rows[::3]
    Xw = (bank[sub, 0:3] + rng.uniform(-0.1, 0.1, (len(sub), 3))).astype(np.float32)
    sub_refs = refs[::3]
    _update(hip, m, centres, bank, sub, sub_refs, Xw=Xw)
    now = _bank(hip, n_points)
    others = np.setdiff1d(np.arange(n_points), sub)
    assert _same_bytes(now[others], first[others]) and not _same_bytes(now[sub], first[sub])
    assert hip.map_debug() == d0
    hip.map_clear()


@pytest.mark.gpu
def test_statuses_and_set_world_pos(hip):
    m, _ = random_case(40, 48, 200, 5, 0.8)
    centres, bank = ref.random_centres(m, 51), ref.random_bank(6000, 52)
    load_all(hip, m, centres, bank)
    good = [p for p in range(200) if p not in m.pt_bad and m.obs.get(p)]
    bad = [p for p in sorted(m.pt_bad) if m.obs.get(p)][0]
    nobody = 5000                                                    # inside the attribute bank, beyond the row tables
    assert hip.map_debug()[4] <= nobody
    stranger = good[0]
    not_observer = [k for k in sorted(m.kf_points) if k not in m.obs[stranger]][0]
    rows = good[1:9] + [bad, nobody, stranger, good[9]]
    refs = ref_kfs(m, good[1:9], 53) + [sorted(m.obs[bad])[0], 0, not_observer, 99999]
    rng = np.random.default_rng(54)
    for Xw in (None, (bank[rows, 0:3] + rng.uniform(-0.1, 0.1, (len(rows), 3))).astype(np.float32)):
        before = bank.copy()
        exp = _update(hip, m, centres, bank, rows, refs, Xw=Xw)
        assert list(exp["status"]) == [0] * 8 + [ref.BAD, ref.NO_OBSERVATIONS, ref.NO_REFERENCE, ref.NO_REFERENCE]
        assert _same_bytes(bank[rows[8:], 3:8], before[rows[8:], 3:8])
        if Xw is not None:
            assert _same_bytes(_bank(hip, 6000)[rows, 0:3], Xw)
    hip.map_clear()


@pytest.mark.gpu
def test_after_a_keyframe_culling(hip, random_cases):
    m, cand, centres, bank0 = random_cases[2]
    m, bank = m._copy(), bank0.copy()
    load_all(hip, m, centres, bank)
    bad0 = set(m.pt_bad)
    exp = m.keyframe_culling(cand, [0] * len(cand), True)
    got = hip.keyframe_culling(cand, apply=True)
    assert list(got["decision"]) == exp["decision"] and sum(d == 1 for d in exp["decision"]) >= 2 and len(m.pt_bad) > len(bad0)
    rows = _not_bad(m, len(bank))
    out = _update(hip, m, centres, bank, rows, ref_kfs(m, rows, 61))
    assert (out["status"] == ref.UPDATED).sum() > 50
    # the points that just turned bad are status 1 now, and a culled keyframe observes nothing
    turned = sorted(m.pt_bad - bad0)
    assert list(_update(hip, m, centres, bank, turned, [cand[0]] * len(turned))["status"]) == [ref.BAD] * len(turned)
    hip.map_clear()


@pytest.mark.gpu
def test_centres_follow_their_keyframes(hip):
    m, _ = random_case(12, 16, 24, 7, 0.7)
    centres, bank = ref.random_centres(m, 71), ref.random_bank(24, 72)
    load_all(hip, m, centres, bank)
    rows = _not_bad(m, 24)
    refs = ref_kfs(m, rows, 73)
    _update(hip, m, centres, bank, rows, refs)
    # a keyframe named twice takes the last value; an unknown one refuses the whole call
    kf = sorted(m.kf_points)[3]
    centres[kf] = np.array([1.5, -2.5, 3.5], np.float32)
    hip.map_kf_centers([kf, kf], np.array([[9, 9, 9], centres[kf]], np.float32))
    _update(hip, m, centres, bank, rows, refs)
    with pytest.raises(Exception) as e:
        hip.map_kf_centers([kf, 4242], np.zeros((2, 3), np.float32))
    assert e.value.code == ASD_ERR_INVALID and "4242" in str(e.value)
    _update(hip, m, centres, bank, rows, refs)                       # nothing was written
    # slot-table growth (more than 64 keyframes) and arena growth (a row longer than the arena)
    d0 = hip.map_debug()
    rng = np.random.default_rng(74)
    for new in range(1000, 1150):
        m.put_keyframe(new, [int(rng.integers(24)), -1])
        m.put_octaves(new, [int(rng.integers(8)), 0])
        centres[new] = rng.uniform(-50, 50, 3).astype(np.float32)
        hip.map_put(new, m.kf_points[new])
        hip.map_put_octaves(new, m.octave[new])
    long_row = np.full(20000, -1, np.int64)
    long_row[rng.choice(20000, 20, replace=False)] = rng.permutation(24)[:20]
    m.put_keyframe(2000, long_row)
    m.put_octaves(2000, rng.integers(0, 8, 20000))
    centres[2000] = np.array([0.25, 0.5, -0.75], np.float32)
    hip.map_put(2000, long_row)
    hip.map_put_octaves(2000, m.octave[2000])
    d1 = hip.map_debug()
    assert d1[5] > d0[5] and d1[6] > d0[6]
    with pytest.raises(Exception) as e:                              # the new keyframes have no centre yet
        hip.update_normal_and_depth(rows, refs)
    assert e.value.code == ASD_ERR_INVALID and "keyframe 1000 " in str(e.value) and "centre" in str(e.value)
    new = list(range(1000, 1150)) + [2000]
    hip.map_kf_centers(new, np.array([centres[k] for k in new], np.float32))
    _update(hip, m, centres, bank, rows, refs)                       # the old centres came through both growths
    # a replacing put keeps the centre (the octaves go with another n)
    row = m.kf_points[kf][:-1]
    m.put_keyframe(kf, row)
    m.put_octaves(kf, [2] * len(row))
    hip.map_put(kf, row)
    hip.map_put_octaves(kf, m.octave[kf])
    refs = ref_kfs(m, rows, 75)
    _update(hip, m, centres, bank, rows, refs)
    # erase drops it: the id put again has none, and the call names it
    octs = m.octave[kf]
    m.erase_keyframe(kf)
    hip.map_erase(kf)
    m.put_keyframe(kf, row)
    m.put_octaves(kf, octs)
    hip.map_put(kf, row)
    hip.map_put_octaves(kf, octs)
    before = _bank(hip, 24)
    rc, _ = hip.update_normal_and_depth_raw(rows, refs, bank[rows, 0:3] + np.float32(1.0))
    assert rc == ASD_ERR_INVALID and f"keyframe {kf} " in hip.last_error() and "centre" in hip.last_error()
    assert _same_bytes(_bank(hip, 24), before)
    hip.map_kf_centers([kf], centres[kf][None])
    _update(hip, m, centres, bank, rows, refs)
    hip.map_clear()
    hip.map_put(3, [1, 2])
    hip.map_put_octaves(3, [0, 0])
    rc, _ = hip.update_normal_and_depth_raw([1], [3])                # clear dropped every centre
    assert rc == ASD_ERR_INVALID and "keyframe 3 " in hip.last_error()
    hip.map_clear()


def _armed_call(hip, synth):
    """an asd_track_local_points_rows call started with asd_track_async and not finished (bank rows 12000 ..)"""
    n_mp = 300
    kc, dc = make_frame(300, 290)
    K = np.array(synth.KITTI_K, np.float32)
    T = pose_T()
    rng = np.random.default_rng(41)
    src = rng.integers(0, 300, n_mp)
    uv = np.stack([kc["x"][src], kc["y"][src]], 1) + rng.uniform(-1.5, 1.5, (n_mp, 2)).astype(np.float32)
    Xw = backproject(T, K, uv, rng.uniform(3, 60, n_mp))
    hip.frame_set(0, kc, dc, BOUNDS)
    hip.bank_put(12000, perturbed_descriptors(dc[src], 0.05, 42))
    hip.mpbank_put(12000, Xw, np.tile(np.float32([0, 0, 1]), (n_mp, 1)), np.full(n_mp, 0.1, np.float32), np.full(n_mp, 500.0, np.float32))
    pose0 = _pose7(pose_T(rv=(0.011, -0.021, 0.004), t=(0.09, -0.06, 0.31)))
    rows = np.arange(12000, 12000 + n_mp, dtype=np.int32)
    assert hip.track_local_points_rows(0, 300, rows, T, K, np.zeros(300, np.uint8), np.zeros((300, 3), np.float32), 1.0, 0.8, pose0, split=True) is None


@pytest.mark.gpu
def test_refusals_change_nothing(hip, synth):
    m, _ = random_case(12, 16, 24, 8, 0.7)
    centres, bank = ref.random_centres(m, 81), ref.random_bank(24, 82)
    load_all(hip, m, centres, bank)
    rows = _not_bad(m, 24)
    refs = ref_kfs(m, rows, 83)
    _update(hip, m, centres, bank, rows, refs)
    before, d0, obs0 = _bank(hip, 24), hip.map_debug(), list(hip.map_observations(rows))
    Xw = bank[rows, 0:3] + np.float32(1.0)

    def refused(rows_, refs_, xw, *words):
        rc, _ = hip.update_normal_and_depth_raw(rows_, refs_, xw)
        msg = hip.last_error()
        assert rc == ASD_ERR_INVALID and all(w in msg for w in words), msg

    refused(rows + rows[:1], refs + refs[:1], np.concatenate([Xw, Xw[:1]]), f"row {rows[0]} ", "twice")
    refused(rows + [2 ** 22], refs + [0], np.concatenate([Xw, Xw[:1]]), str(2 ** 22), "attribute bank")
    refused(rows + [-1], refs + [0], np.concatenate([Xw, Xw[:1]]), "-1")
    hip.map_put(777, [3, -1])                                        # a live keyframe without octaves (it has a centre)
    hip.map_kf_centers([777], np.zeros((1, 3), np.float32))
    refused(rows, refs, Xw, "keyframe 777 ", "octaves")
    hip.map_erase(777)
    d0 = hip.map_debug()
    hip.prep_async(1)
    refused(rows, refs, Xw, "asd_prep_async")
    hip.prep_async(0)
    _armed_call(hip, synth)
    refused(rows, refs, Xw, "asd_track_finish")
    with pytest.raises(Exception) as e:
        hip.map_kf_centers([sorted(m.kf_points)[0]], np.zeros((1, 3), np.float32))
    assert e.value.code == ASD_ERR_INVALID and "asd_track_finish" in str(e.value)
    hip.track_finish()
    rc, _ = hip.update_normal_and_depth_raw(list(range(2 ** 20 + 1)), [0] * (2 ** 20 + 1))
    assert rc == ASD_ERR_CAPACITY
    assert _same_bytes(_bank(hip, 24), before) and hip.map_debug() == d0 and list(hip.map_observations(rows)) == obs0
    _update(hip, m, centres, bank, rows, refs, Xw=Xw)
    hip.map_clear()


@pytest.mark.gpu
def test_the_search_list_stays(hip, random_cases):
    m, _cand, centres, bank0 = random_cases[1]
    bank = bank0.copy()
    load_all(hip, m, centres, bank)
    cur, seen = random_frame(m, 40, 3)
    hip.update_local_map(cur, seen)
    assert _list_state(hip) == "kept"
    kfs = sorted(m.kf_points)
    hip.map_kf_centers(kfs[:5], np.array([centres[k] for k in kfs[:5]], np.float32))
    assert _list_state(hip) == "kept"
    rows = _not_bad(m, len(bank))
    _update(hip, m, centres, bank, rows, ref_kfs(m, rows, 91), Xw=bank[rows, 0:3] + np.float32(0.01))
    assert _list_state(hip) == "kept"
    hip.map_clear()


@pytest.mark.gpu
def test_tracking_reads_what_the_update_wrote(hip, synth):
    """TrackLocalMap over bank rows whose normals and ranges came from the device update == over rows that got the restatement's values
    through asd_mpbank_put"""
    n_kp, n_mp, n_kf, base = 300, 360, 6, 20000
    kc, dc = make_frame(n_kp, 290)
    K = np.array(synth.KITTI_K, np.float32)
    T = pose_T()
    rng = np.random.default_rng(95)
    src = rng.integers(0, n_kp, n_mp)
    uv = np.stack([kc["x"][src], kc["y"][src]], 1) + rng.uniform(-1.5, 1.5, (n_mp, 2)).astype(np.float32)
    Xw = backproject(T, K, uv, rng.uniform(3, 60, n_mp))
    Ow = -(T[:3, :3].astype(np.float64).T @ T[:3, 3].astype(np.float64))
    # six keyframes near the camera; every point is observed by two to four of them, at the octave of the keypoint it came from
    kfs = {k: [] for k in range(1, n_kf + 1)}
    octs = {k: [] for k in kfs}
    for p in range(n_mp):
        for k in rng.choice(n_kf, int(rng.integers(2, 5)), replace=False) + 1:
            kfs[int(k)].append(base + p)
            octs[int(k)].append(int(kc["octave"][src[p]]))
    m = mk(kfs, octs)
    centres = {k: (Ow + rng.uniform(-0.3, 0.3, 3)).astype(np.float32) for k in kfs}
    rows = np.arange(base, base + n_mp, dtype=np.int32)
    refs = ref_kfs(m, rows, 96)
    bank = np.zeros((base + n_mp, 8), np.float32)
    bank[base:, 0:3] = Xw
    exp = ref.update_normal_and_depth(m, centres, bank, rows, refs, hip.scale_tables()["scale"])
    assert (exp["status"] == ref.UPDATED).all()
    load(hip, m)
    hip.map_kf_centers(sorted(centres), np.array([centres[k] for k in sorted(centres)], np.float32))
    hip.frame_set(0, kc, dc, BOUNDS)
    hip.bank_put(base, perturbed_descriptors(dc[src], 0.05, 97))
    pose0 = _pose7(pose_T(rv=(0.011, -0.021, 0.004), t=(0.09, -0.06, 0.31)))
    occupied, cur_Xw = np.zeros(n_kp, np.uint8), np.zeros((n_kp, 3), np.float32)
    junk = np.zeros(n_mp, np.float32)
    results = []
    for device in (True, False):
        if device:
            hip.mpbank_put(base, Xw, np.zeros((n_mp, 3), np.float32), junk, junk)
            got = hip.update_normal_and_depth(rows, refs)
            ref.assert_bits(got["normal"], exp["normal"], "normal")
        else:
            hip.mpbank_put(base, Xw, exp["normal"], exp["min_dist"], exp["max_dist"])
        results.append(hip.track_local_points_rows(0, n_kp, rows, T, K, occupied, cur_Xw, 1.0, 0.8, pose0))
    (m0, n0, p0, o0, i0), (m1, n1, p1, o1, i1) = results
    assert n0 == n1 and n0 > 100 and i0 == i1
    assert np.array_equal(m0, m1) and np.array_equal(p0, p1) and np.array_equal(o0, o1)
    hip.map_clear()
