"""asd_local_ba_graph and asd_local_ba_apply on the device against tests/local_ba_graph_ref.py (which tests/test_local_ba_graph_ref.py
pins by hand): every list equal exactly, the applied table read back through asd_map_observations and a following graph call."""
import numpy as np
import pytest

from tests import local_ba_graph_ref as ref
from tests import normal_depth_ref as nd_ref
from tests.culling_cases import RANDOM_SHAPES, load, mk, random_case
from tests.local_ba_graph_cases import GRAPH_KEYS, assert_erase, assert_graph, erase_cases, flags_of, graph_cases
from tests.local_map_cases import assert_same as assert_same_local_map
from tests.local_map_cases import random_frame
from tests.test_normal_depth import _armed_call, _list_state

ASD_ERR_INVALID, ASD_ERR_CAPACITY = -1, -5


def _graph(hip, m, kf, neigh, what="", **kw):
    exp = ref.graph(m, kf, neigh)
    got = hip.local_ba_graph(kf, neigh, **kw)
    assert_graph(got, exp, what)
    return got, exp


def _apply(hip, m, g, flags, apply, what=""):
    """the erase policy on the device and on the restatement (which mutates m with apply)"""
    exp = ref.erase(m, g, flags, apply)
    got = hip.local_ba_apply(flags, len(g["local_rows"]), apply=apply)
    assert_erase(got, exp, what)
    return exp


def _table_equals(hip, m, kf, neigh, n_rows):
    """Observations() of every row, and the graph the table now gives (its points are the not-bad ones: the bad bytes show there)"""
    rows = list(range(n_rows))
    assert [int(x) for x in hip.map_observations(rows)] == m.observations(rows)
    _graph(hip, m, kf, neigh, "after apply")
    for k in sorted(m.kf_points)[:3]:                                # and from three other keyframes' point of view
        _graph(hip, m, k, [x for x in sorted(m.kf_points, reverse=True) if x != k][:4], "after apply")


def _load_shuffled(hip, m, seed):
    """the map into a cleared table in a random keyframe order, a slot freed and taken in between: the slot order is not the id order"""
    rng = np.random.default_rng(seed)
    kfs = [int(k) for k in rng.permutation(sorted(m.kf_points))]
    hip.map_clear()
    hip.map_put(2 ** 30, [0, 1])
    for k in kfs[:len(kfs) // 2]:
        hip.map_put(k, m.kf_points[k])
    hip.map_erase(2 ** 30)
    for k in kfs[len(kfs) // 2:]:
        hip.map_put(k, m.kf_points[k])
    for k in kfs:
        hip.map_put_octaves(k, m.octave[k])
        if k in m.kf_bad:
            hip.map_kf_bad(k, True)
    if m.pt_bad:
        hip.map_point_bad(sorted(m.pt_bad), True)


def _random_flags(n, seed, p=0.05):
    return (np.random.default_rng(seed).uniform(size=n) < p).astype(np.uint8)


@pytest.mark.gpu
def test_hand_worked_maps(hip):
    for case in graph_cases():
        load(hip, case["map"])
        got, _ = _graph(hip, case["map"], case["kf"], case["neigh"], case["name"])
        assert_graph(got, case["graph"], case["name"])
    for case in erase_cases():
        for apply in (False, True):
            m = case["map"]._copy()
            load(hip, m)
            got, g = _graph(hip, m, case["kf"], case["neigh"], case["name"])
            assert_graph(got, case["graph"], case["name"])
            exp = _apply(hip, m, g, flags_of(case), apply, case["name"])
            assert_erase(exp, case["result"], case["name"])
            if apply:
                assert m.kf_points == case["after"]
            _table_equals(hip, m, case["kf"], case["neigh"], 210)
    hip.map_clear()


@pytest.fixture(scope="module")
def random_maps():
    out = []
    for k, (n_kf, n_kp, n_points, fill) in enumerate(RANDOM_SHAPES):
        m, cand = random_case(n_kf, n_kp, n_points, 1, fill)
        rng = np.random.default_rng(700 + k)
        for bad in rng.choice(sorted(m.kf_points), 2, replace=False):          # (random_case makes no bad keyframes)
            m.kf_bad.add(int(bad))
        kfs = sorted(m.kf_points)
        kf = [x for x in kfs if x not in m.kf_bad][int(rng.integers(3))]
        neigh = [int(x) for x in rng.permutation([x for x in kfs if x != kf])[:max(3, n_kf // 3)]]
        out.append((m, kf, neigh + [max(kfs) + 77], n_points))                   # (and an id the table does not hold)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(RANDOM_SHAPES)))
def test_random_maps_equal_the_restatement(hip, random_maps, case):
    m0, kf, neigh, n_points = random_maps[case]
    m = m0._copy()
    _load_shuffled(hip, m, 710 + case)
    d0 = hip.map_debug()
    got, g = _graph(hip, m, kf, neigh)
    assert len(g["e_kf"]) > 20 and len(g["fixed_kfs"]) > 0
    flags = _random_flags(len(g["e_kf"]), 720 + case)
    e_point = np.array(g["e_point"])
    for r in np.random.default_rng(730 + case).choice(len(g["local_rows"]), 4, replace=False):   # four points lose every edge (two bad keyframes' entries at most stay): bad
        flags[e_point == r] = 1
    dry = _apply(hip, m, g, flags, False)
    assert len(dry["bad_rows"]) >= 4 and any(x >= 0 for x in dry["new_ref"])
    assert hip.map_debug() == d0
    wet = _apply(hip, m, g, flags, True)
    assert wet == dry and wet["n_erased"] > 0
    _table_equals(hip, m, kf, neigh, n_points)
    hip.map_clear()


def _seam_rows(rng, lengths, n_points, empty=0.1):
    kfs, octs = {}, {}
    for kf, n in lengths.items():
        row = rng.permutation(n_points)[:n]
        row[rng.uniform(size=n) < empty] = -1
        kfs[kf], octs[kf] = [int(x) for x in row], [int(x) for x in rng.integers(0, 8, n)]
    return kfs, octs


@pytest.mark.gpu
def test_row_lengths_around_the_wave_and_the_tile(hip):
    """rows of 1 / 63 / 64 / 65 / 130 entries (the wave strides of the table passes) and local rows whose concatenation crosses 1024 and
    2048 entries, one of them longer than a tile; sparse ids that are not in slot order"""
    rng = np.random.default_rng(3)
    n_points = 2600
    lengths = {50: 1, 4000: 63, 31: 64, 20000: 65, 11: 130, 600: 130, 7: 1500, 800: 700, 90000: 700, 100: 300, 2 ** 30 + 5: 257}
    kfs, octs = _seam_rows(rng, lengths, n_points)
    m = mk(kfs, octs, bad_points=[int(x) for x in rng.choice(n_points, 60, replace=False)])
    m.kf_bad.add(600)
    _load_shuffled(hip, m, 31)
    for kf, neigh in ((11, [50, 4000, 31, 20000, 600, 7, 800]), (7, [800, 90000, 11]), (50, []), (2 ** 30 + 5, [31, 7])):
        got, g = _graph(hip, m, kf, neigh, f"kf {kf}")
        if kf == 11:
            base = np.cumsum([0] + [len(m.kf_points[k]) for k in g["local_kfs"]])
            assert base[-1] > 2048 and any(a < 1024 < b for a, b in zip(base, base[1:]))
    got, g = _graph(hip, m, 7, [800, 90000, 11])
    _apply(hip, m, g, _random_flags(len(g["e_kf"]), 32, 0.2), True)
    _table_equals(hip, m, 7, [800, 90000, 11], n_points)
    hip.map_clear()


@pytest.mark.gpu
def test_segments_beyond_a_wave_and_257_poses(hip):
    """one point with 130 observers, one with 65 (the ordering of a segment beyond a wave), 258 poses (more than 256)"""
    rng = np.random.default_rng(4)
    ids = [int(x) for x in rng.permutation(np.arange(1, 261) * 11)]
    local, rest = ids[0], ids[1:]
    rows = {k: [-1, -1, -1, -1] for k in ids}
    rows[local] = [900, 901, 902, 903]
    for p, ks in ((900, rest[:129]), (901, rest[129:193]), (902, rest[193:259]), (903, rest[100:140])):
        for k in ks:
            free = [i for i, x in enumerate(rows[k]) if x < 0]
            rows[k][free[int(rng.integers(len(free)))]] = p
    m = mk(rows, {k: [int(x) for x in rng.integers(0, 8, 4)] for k in ids})
    m.kf_bad |= {rest[5], rest[150]}
    _load_shuffled(hip, m, 41)
    assert list(hip.map_observations([900, 901, 902, 903])) == [130, 65, 67, 41]
    got, g = _graph(hip, m, local, [])
    assert len(g["pose_kfs"]) == 258 and len(g["fixed_kfs"]) == 257            # (two of the 259 others are bad)
    got, g = _graph(hip, m, local, [rest[5], rest[0], rest[258]])
    flags = _random_flags(len(g["e_kf"]), 42, 0.3)
    flags[:129] = 1                                                             # 900 loses every observation that has an edge
    exp = _apply(hip, m, g, flags, True)
    assert 900 in exp["bad_rows"]
    _table_equals(hip, m, local, [rest[0]], 904)
    hip.map_clear()


@pytest.mark.gpu
def test_more_than_4096_local_points(hip):
    """70 keyframes of 64 keypoints with distinct points: the one-workgroup scan over the points takes a second round"""
    rng = np.random.default_rng(5)
    rows = {10 + 3 * k: [int(x) for x in rng.permutation(np.arange(64 * k, 64 * k + 64))] for k in range(70)}
    for k in range(6):                                                          # six more keyframes that see 200 of those points each
        rows[500 + k] = [int(x) for x in rng.choice(64 * 70, 200, replace=False)]
    m = mk(rows, {k: [int(x) for x in rng.integers(0, 8, len(r))] for k, r in rows.items()})
    _load_shuffled(hip, m, 51)
    kf = 10
    neigh = [int(x) for x in rng.permutation([10 + 3 * k for k in range(1, 70)])]
    got, g = _graph(hip, m, kf, neigh, want_Xw=False, caps=(80, 5000, 16, 80, 8192))
    assert len(g["local_rows"]) == 4480 and g["point_rank"] != sorted(g["point_rank"]) and len(g["fixed_kfs"]) == 6
    _apply(hip, m, g, _random_flags(len(g["e_kf"]), 52), True)
    _table_equals(hip, m, kf, neigh[:10], 64 * 70)
    hip.map_clear()


@pytest.mark.gpu
def test_capacities_one_too_small(hip, random_maps):
    m0, kf, neigh, n_points = random_maps[2]
    m = m0._copy()
    load(hip, m)
    g = ref.graph(m, kf, neigh)
    need = [len(g[k]) for k in ("local_kfs", "local_rows", "fixed_kfs", "pose_kfs", "e_kf")]
    names = ("n_local_kfs", "n_points", "n_fixed", "n_poses", "n_edges")
    obs0, d0 = list(hip.map_observations(list(range(n_points)))), hip.map_debug()
    cur, seen = random_frame(m, 40, 3)
    for short in range(5):
        caps = list(need)
        caps[short] -= 1
        rc, out = hip.local_ba_graph_raw(kf, neigh, caps)
        assert rc == ASD_ERR_CAPACITY and [out[k] for k in names] == need, names[short]
        rc, _ = hip.local_ba_apply_raw(np.zeros(need[4], np.uint8), need[1], False, 8)      # a refused call leaves no graph
        assert rc == ASD_ERR_INVALID
        assert list(hip.map_observations(list(range(n_points)))) == obs0 and hip.map_debug() == d0
        # the marks and claims are as they were: UpdateLocalMap on the same context still equals its restatement
        assert_same_local_map(hip.update_local_map(cur, seen), m.update_local_map(cur, seen))
        rc, out = hip.local_ba_graph_raw(kf, neigh, need)
        assert rc == 0
        assert_graph(out, g, "repeat")
    # the erase policy's capacity
    flags = _random_flags(need[4], 61, 0.4)
    exp = ref.erase(m, g, flags, False)
    assert len(exp["bad_rows"]) >= 2
    rc, out = hip.local_ba_apply_raw(flags, need[1], True, len(exp["bad_rows"]) - 1)
    assert rc == ASD_ERR_CAPACITY and out["n_bad"] == len(exp["bad_rows"]) and out["n_erased"] == exp["n_erased"]
    assert list(hip.map_observations(list(range(n_points)))) == obs0
    assert_same_local_map(hip.update_local_map(cur, seen), m.update_local_map(cur, seen))
    _graph(hip, m, kf, neigh)                                                   # the table is untouched: the same graph again
    rc, out = hip.local_ba_apply_raw(flags, need[1], True, len(exp["bad_rows"]))
    assert rc == 0
    assert_erase(out, ref.erase(m, g, flags, True), "repeat")
    _table_equals(hip, m, kf, neigh, n_points)
    hip.map_clear()


@pytest.mark.gpu
def test_refusals_change_nothing(hip, synth, random_maps):
    m0, kf, neigh, n_points = random_maps[1]
    m = m0._copy()
    load(hip, m)
    caps = (64, 4096, 64, 128, 16384)
    obs0 = list(hip.map_observations(list(range(n_points))))

    def refused(kf_, neigh_, *words, code=ASD_ERR_INVALID, want_Xw=False):
        rc, _ = hip.local_ba_graph_raw(kf_, neigh_, caps, want_Xw)
        msg = hip.last_error()
        assert rc == code and all(w in msg for w in words), msg

    refused(424242, neigh, "424242", "not in the observation table")
    refused(kf, neigh + neigh[:1], f"keyframe {neigh[0]} ", "twice")
    refused(kf, neigh + [kf], f"keyframe {kf} ", "twice")
    refused(kf, neigh + [-3], "-3")
    refused(kf, list(range(10 ** 6, 10 ** 6 + 4097)), "4097", code=ASD_ERR_CAPACITY)
    hip.map_put(777, [3, -1])                                                   # a live keyframe without octaves
    refused(kf, neigh, "keyframe 777 ", "octaves")
    hip.map_erase(777)
    hip.prep_async(1)
    refused(kf, neigh, "asd_prep_async", want_Xw=True)
    hip.prep_async(0)
    hip.mpbank_put(0, np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), np.zeros(4, np.float32), np.zeros(4, np.float32))
    hip.map_put(778, [2 ** 22 + 5])                                             # a point whose row lies outside the attribute bank
    hip.map_put_octaves(778, [0])
    refused(778, [], str(2 ** 22 + 5), "attribute bank", want_Xw=True)
    hip.map_erase(778)
    # asd_local_ba_apply
    def refused_apply(flags, n_points_, *words):
        rc, _ = hip.local_ba_apply_raw(flags, n_points_, True, 64)
        msg = hip.last_error()
        assert rc == ASD_ERR_INVALID and all(w in msg for w in words), msg

    hip.map_clear()
    load(hip, m)
    refused_apply(np.zeros(3, np.uint8), 1, "no asd_local_ba_graph")
    got, g = _graph(hip, m, kf, neigh)
    E, P = len(g["e_kf"]), len(g["local_rows"])
    flags = _random_flags(E, 81, 0.2)
    refused_apply(flags[:-1], P, f"{E - 1} edges")
    refused_apply(flags, P + 1, f"{P + 1} points")
    _armed_call(hip, synth)
    refused_apply(flags, P, "asd_track_finish")
    refused(kf, neigh, "asd_track_finish")
    hip.track_finish()
    hip.map_set(kf, [0], [m.kf_points[kf][0]])                                  # the same value: the table's version moves all the same
    refused_apply(flags, P, "changed")
    assert list(hip.map_observations(list(range(n_points)))) == obs0
    got, g = _graph(hip, m, kf, neigh)
    _apply(hip, m, g, flags, True)
    refused_apply(flags, P, "no asd_local_ba_graph")                            # apply = 1 consumed the graph
    _table_equals(hip, m, kf, neigh, n_points)
    hip.map_clear()


@pytest.mark.gpu
def test_version_and_search_list(hip, random_maps):
    m0, kf, neigh, n_points = random_maps[3]
    m = m0._copy()
    load(hip, m)
    cur, seen = random_frame(m, 40, 3)
    hip.update_local_map(cur, seen)
    assert _list_state(hip) == "kept"
    raw = [hip.local_ba_graph_raw(kf, neigh, (64, 4096, 128, 256, 16384), True) for _ in range(2)]
    assert raw[0][0] == 0 and raw[1][0] == 0
    for k in GRAPH_KEYS + ("Xw",):                                              # two identical calls return identical bytes
        assert raw[0][1][k].tobytes() == raw[1][1][k].tobytes(), k
    assert _list_state(hip) == "kept"
    g = ref.graph(m, kf, neigh)
    assert_graph(raw[0][1], g)
    flags = _random_flags(len(g["e_kf"]), 91)
    first = _apply(hip, m, g, flags, False)
    assert _apply(hip, m, g, flags, False) == first and first["n_erased"] > 0
    assert _list_state(hip) == "kept"
    # apply = 1 without a flagged edge keeps the list (and consumes the graph), with one it invalidates it
    _apply(hip, m, g, np.zeros(len(flags), np.uint8), True)
    assert _list_state(hip) == "kept"
    _graph(hip, m, kf, neigh)
    assert _apply(hip, m, g, flags, True) == first
    assert _list_state(hip) == "changed"
    hip.map_clear()


def _quat_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _centre(pose7):
    """KeyFrame::SetPose's Ow = -Rwc * tcw in f32 (the same numbers go to the device and to the restatement)"""
    R, t = _quat_R(pose7[:4]).astype(np.float32), np.asarray(pose7[4:], np.float32)
    return (-(R.T @ t)).astype(np.float32)


def _synthetic_local_map(synth, inv_sigma2):
    """the project's synthetic LocalBA problem (8 free and 4 fixed poses on a track, 300 points, pixel noise, a few gross outliers) as a map:
    -> (problem, map, keypoints per keyframe, pose7 per keyframe, centres, bank, keyframe, neighbours, first bank row, the generator it drew from)"""
    src = synth.ba_problem(n_free=8, n_fixed=4, n_points=300, obs_per_point=4, seed=7, pix_noise=0.5, outlier_frac=0.03)
    rng = np.random.default_rng(8)
    n_pose, n_pt, row0 = len(src["poses"]), len(src["points"]), 40
    kf_id = [5 + 7 * p for p in range(n_pose)]                                   # sparse ids, fixed ones first as in the synthetic problem
    level = [int(np.argmin(np.abs(inv_sigma2.astype(np.float64) - x))) for x in src["e_info"]]
    rows, octs, keys = {k: [] for k in kf_id}, {k: [] for k in kf_id}, {k: [] for k in kf_id}
    left = np.bincount(src["e_point"], minlength=n_pt)
    for p in range(n_pose):
        mine = [int(e) for e in rng.permutation(np.nonzero(src["e_pose"] == p)[0])]
        for e in mine:
            if left[src["e_point"][e]] > 2 and rng.uniform() < 0.15:             # an observation the map never got: points with 2 .. 4 observers
                left[src["e_point"][e]] -= 1
                continue
            if rng.uniform() < 0.1:                                             # a keypoint without a point in between
                rows[kf_id[p]].append(-1); octs[kf_id[p]].append(0); keys[kf_id[p]].append((0.0, 0.0))
            rows[kf_id[p]].append(row0 + int(src["e_point"][e])); octs[kf_id[p]].append(level[e]); keys[kf_id[p]].append(tuple(src["e_obs"][e]))
    m = mk(rows, octs)
    pose7 = {kf_id[p]: src["poses"][p].copy() for p in range(n_pose)}
    centres = {k: _centre(pose7[k]) for k in kf_id}
    bank = np.zeros((row0 + n_pt, 8), np.float32)
    bank[:, 3:8] = [9.0, 9.0, 9.0, -1.0, -2.0]
    bank[row0:, 0:3] = src["points"]
    kf, neigh = kf_id[-1], [int(x) for x in rng.permutation(kf_id[4:-1])]
    return src, m, keys, pose7, centres, bank, kf, neigh, row0, rng


@pytest.mark.gpu
def test_local_bundle_adjustment_end_to_end(hip, synth):
    """DoMapping's chain over the tables: graph -> asd_ba_problem -> asd_local_ba -> apply -> centres -> UpdateNormalAndDepth(Xw), against the
    same chain over the restatement's lists and map.  Everything compared is integer or the same arithmetic on both sides."""
    inv_sigma2 = hip.scale_tables()["inv_sigma2"]
    src, m, keys, pose7, centres, bank, kf, neigh, row0, rng = _synthetic_local_map(synth, inv_sigma2)
    n_pt = len(src["points"])
    from tests.normal_depth_cases import load_all
    load_all(hip, m, centres, bank)
    got, g = _graph(hip, m, kf, neigh, want_Xw=True)
    assert len(g["local_kfs"]) == 8 and len(g["fixed_kfs"]) >= 3 and len(g["local_rows"]) > 200

    def problem(lists, Xw):
        return dict(poses=np.array([pose7[int(k)] for k in lists["pose_kfs"]]),
                    fixed=np.array([int(f) | int(k == 0) for k, f in zip(lists["pose_kfs"], lists["pose_fixed"])], np.uint8), points=np.asarray(Xw, np.float64),
                    e_point=np.array(lists["e_point"], np.int32), e_pose=np.array(lists["e_pose"], np.int32),
                    e_obs=np.array([keys[int(k)][int(i)] for k, i in zip(lists["e_kf"], lists["e_idx"])], np.float64),
                    e_info=np.array([inv_sigma2[int(o)] for o in lists["e_octave"]], np.float64), K=src["K"])

    rows_sorted = sorted(g["local_rows"])
    p_dev, p_ref = problem(got, got["Xw"]), problem(g, bank[rows_sorted, 0:3].astype(np.float64))
    for k in p_ref:
        assert p_dev[k].dtype == p_ref[k].dtype and p_dev[k].tobytes() == p_ref[k].tobytes(), k
    res = hip.local_ba(p_dev)
    flags = ((res["edge_chi2"] > 5.991) | (res["edge_depth_pos"] == 0)).astype(np.uint8)
    assert 0 < flags.sum() < len(flags)
    seats = {p: min(m.obs[p]) if rng.uniform() < 0.5 else max(m.obs[p]) for p in g["local_rows"]}     # mpRefKF before
    exp_seats = dict(seats)
    exp = ref.erase(m, g, flags, True, ref_kf=exp_seats)
    out = hip.local_ba_apply(flags, len(g["local_rows"]), apply=True)
    assert_erase(out, exp, "end to end")
    erased = {}
    for e in np.nonzero(flags)[0]:
        erased.setdefault(rows_sorted[g["e_point"][e]], set()).add(g["e_kf"][e])
    for i, p in enumerate(g["local_rows"]):                                     # the adapter's rule for mpRefKF
        if out["new_ref"][i] >= 0 and seats[p] in erased.get(p, ()):
            seats[p] = int(out["new_ref"][i])
        if p not in m.pt_bad:
            assert seats[p] == exp_seats[p], p
    # WriteBack: the local keyframes' new centres, then SetWorldPos + UpdateNormalAndDepth for every local point
    local_pose = {int(k): res["poses"][i] for i, k in enumerate(g["pose_kfs"]) if not g["pose_fixed"][i]}
    for k in g["local_kfs"]:
        centres[k] = _centre(local_pose[k])
    hip.map_kf_centers(g["local_kfs"], np.array([centres[k] for k in g["local_kfs"]], np.float32))
    Xw = res["points"][g["point_rank"]].astype(np.float32)
    refs = [seats[p] for p in g["local_rows"]]
    e_nd = nd_ref.update_normal_and_depth(m, centres, bank, g["local_rows"], refs, hip.scale_tables()["scale"], Xw=Xw)
    g_nd = hip.update_normal_and_depth(g["local_rows"], refs, Xw)
    assert list(g_nd["status"]) == list(e_nd["status"]) and set(g_nd["status"]) <= {nd_ref.UPDATED, nd_ref.BAD}
    assert [p for p, s in zip(g["local_rows"], e_nd["status"]) if s == nd_ref.BAD] == exp["bad_rows"]
    for k in ("normal", "min_dist", "max_dist"):
        nd_ref.assert_bits(g_nd[k], e_nd[k], k)
    nd_ref.assert_bits(hip.bank_get(0, len(bank), desc=False)[1], bank, "bank")
    _table_equals(hip, m, kf, neigh, row0 + n_pt)
    hip.map_clear()
