"""tests/normal_depth_ref.py against hand-worked literals, and asd_normal_and_depth_point of the built library (the kernel's own
functions, csrc/normal_depth.h, on the host) against the restatement bit for bit.  No GPU."""
import ctypes

import numpy as np

from tests import normal_depth_ref as ref
from tests.normal_depth_cases import hand_cases

SCALE = ref.scale_table()


def _run(case):
    bank = case["bank"].copy()
    got = ref.update_normal_and_depth(case["map"], case["centres"], bank, case["rows"], case["ref_kf"], SCALE)
    return got, bank


def test_default_scale_table():
    # 1.2f widened to double, the running product stored as float (ORBextractor.cc:459-466)
    want = np.array([0x3f800000, 0x3f99999a, 0x3fb851ec, 0x3fdd2f1c, 0x4004b5de, 0x401f40a4, 0x403f1a5f, 0x406552d9], np.uint32)
    assert np.array_equal(SCALE.view(np.uint32), want)


def test_hand_cases_equal_their_literals():
    for case in hand_cases():
        got, bank = _run(case)
        assert list(got["status"]) == list(case["status"]), case["name"]
        ref.assert_bits(got["normal"], case["normal"], case["name"] + " normal")
        ref.assert_bits(got["min_dist"], case["min_dist"], case["name"] + " min")
        ref.assert_bits(got["max_dist"], case["max_dist"], case["name"] + " max")
        # the positions are nobody's to change without Xw, and the outputs are what the bank holds
        assert np.array_equal(bank[:, 0:3], case["bank"][:, 0:3])
        rows = case["rows"]
        ref.assert_bits(bank[rows, 3:6], case["normal"], case["name"])


def test_axis_case_by_hand():
    case = [c for c in hand_cases() if c["name"] == "axis"][0]
    got, _ = _run(case)
    assert got["normal"].tolist() == [[1.0, 0.0, 0.0]]
    assert got["max_dist"][0] == np.float32(2.0) * np.float32(1.2)
    assert got["min_dist"][0] == np.float32(np.float64(got["max_dist"][0]) / np.float64(SCALE[7]))


def test_the_sum_depends_on_the_order_and_the_walk_is_by_id():
    case = [c for c in hand_cases() if c["name"] == "order"][0]
    Ow = [case["centres"][k] for k in (10, 20, 30)]
    pos = case["bank"][100, 0:3]
    up = ref.point(Ow, 1, pos, SCALE[3], SCALE[7])[0]
    down = ref.point(Ow, 1, pos, SCALE[3], SCALE[7], order=[2, 1, 0])[0]
    assert not np.array_equal(up.view(np.uint32), down.view(np.uint32))           # f32 (a + b) + c != (c + b) + a
    got, _ = _run(case)
    assert np.array_equal(got["normal"][0].view(np.uint32), up.view(np.uint32))
    assert list(case["map"].kf_points) == [30, 10, 20]
    assert np.array_equal(up.view(np.uint32), case["normal"][0].view(np.uint32))


def test_set_world_pos_comes_first_whatever_the_status():
    case = [c for c in hand_cases() if c["name"] == "statuses"][0]
    bank = case["bank"].copy()
    Xw = bank[case["rows"], 0:3] + np.float32(0.5)
    got = ref.update_normal_and_depth(case["map"], case["centres"], bank, case["rows"], case["ref_kf"], SCALE, Xw=Xw)
    assert list(got["status"]) == list(case["status"])
    assert np.array_equal(bank[case["rows"], 0:3], Xw)
    keep = got["status"] != ref.UPDATED
    assert np.array_equal(got["normal"][keep], case["normal"][keep]) and np.array_equal(got["min_dist"][keep], case["min_dist"][keep])
    assert not np.array_equal(got["normal"][~keep], case["normal"][~keep])


def test_a_point_on_a_centre_is_ieee():
    case = [c for c in hand_cases() if c["name"] == "on a centre"][0]
    got, _ = _run(case)
    assert np.isnan(got["normal"]).all()
    assert np.isfinite(got["min_dist"]).all() and np.isfinite(got["max_dist"]).all()
    assert got["max_dist"][1] == 0.0 and got["min_dist"][1] == 0.0


# ---- the built library
def _random_points(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        n_obs = int(rng.integers(1, 13))
        Ow = rng.uniform(-50, 50, (n_obs, 3)).astype(np.float32)
        pos = rng.uniform(-50, 50, 3).astype(np.float32)
        out.append((Ow, int(rng.integers(n_obs)), pos, SCALE[int(rng.integers(len(SCALE)))], SCALE[-1]))
    return out


def _library_equals(pkg, points):
    got, exp = [], []
    for Ow, r, pos, s_level, s_top in points:
        n, mn, mx = pkg.capi.normal_and_depth_point(Ow, r, pos, s_level, s_top)
        got.append(list(n) + [mn, mx])
        n, mn, mx = ref.point(Ow, r, pos, s_level, s_top)
        exp.append(list(n) + [mn, mx])
    ref.assert_bits(np.array(got, np.float32), np.array(exp, np.float32), "asd_normal_and_depth_point")
    return np.array(exp, np.float32)


def test_library_point_equals_the_restatement_on_random_points(pkg):
    points = _random_points(2000, 7)
    assert {len(p[0]) for p in points} == set(range(1, 13)) and {float(p[3]) for p in points} == {float(s) for s in SCALE}
    _library_equals(pkg, points)


def test_library_point_equals_the_restatement_on_the_hand_cases(pkg):
    points = []
    for case in hand_cases():
        m = case["map"]
        for r, kf, st in zip(case["rows"], case["ref_kf"], case["status"]):
            if st != ref.UPDATED:
                continue
            kfs = sorted(m.obs[r])
            points.append((np.array([case["centres"][k] for k in kfs], np.float32), kfs.index(kf), case["bank"][r, 0:3],
                           SCALE[m.octave[kf][m.obs[r][kf]]], SCALE[-1]))
    exp = _library_equals(pkg, points)
    assert np.isnan(exp).any() and len(points) == 5


def test_library_point_refuses_bad_arguments(pkg):
    lib = pkg.capi.load_library()
    z = np.zeros(3, np.float32)
    out, a, b = np.zeros(3, np.float32), ctypes.c_float(), ctypes.c_float()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    for n_obs, r in ((0, 0), (1, 1), (1, -1)):
        rc = lib.asd_normal_and_depth_point(ctypes.c_int32(n_obs), p(z), ctypes.c_int32(r), p(z), ctypes.c_float(1), ctypes.c_float(1), p(out),
                                            ctypes.byref(a), ctypes.byref(b))
        assert rc == -1


def test_library_exports_and_argument_layout(pkg):
    lib = pkg.capi.load_library()
    for name in ("asd_map_kf_centers", "asd_update_normal_and_depth", "asd_normal_and_depth_point"):
        assert hasattr(lib, name), name
    # include/asd_slam.h: int32 n, then seven pointers at their natural alignment
    assert ctypes.sizeof(pkg.capi.asd_normal_depth_args) == 8 + 7 * ctypes.sizeof(ctypes.c_void_p)
    assert pkg.capi.asd_normal_depth_args.rows.offset == 8 and pkg.capi.asd_normal_depth_args.status.offset == 56
