"""tests/initializer_ref.py against itself (no GPU): the draws against libc's rand(), Normalize against asd_initializer_normalize bit for
bit, the outcomes beside the named scenes of tests/initializer_cases.py, hand-made rows for the exits no scene reaches, and a list of
mutants of the restatement that must each change an output.

Mutants: 20.  Eight change a constant or an order and are killed by a scene (SCENE_MUTANTS: the case that kills each); twelve turn a
comparison into its neighbour (> into >=, < into <=) and are killed by a hand-made row that sits exactly on the gate.  Three gates of the
reference cannot be told from their neighbours in f32 and have no mutant: RH > 0.40 (:114), cosParallax < 0.99998 (:899, :905, :934) and
d1 / d2 < 1.0000001 (:607) compare a float with a double constant that no float equals."""
import ctypes

import numpy as np
import pytest

from tests import initializer_cases as C
from tests import initializer_ref as R

F32, F64, LD = np.float32, np.float64, np.longdouble
SCENE_MUTANTS = {"th_fundamental_5.991": "n64", "th_score_3.841": "n64", "score_test2_first": "n64", "normalize_matched_only": "unmatched",
                 "index_40": "n64", "walk_ge": "ties", "similar_0.8": None, "min_good_0.8": None}
_OUT = {}


@pytest.fixture(scope="module")
def svd4(oracle):
    return lambda A: oracle.svd4_vt(A)[:, 3]


def outcome(case, svd4, mut=()):
    key = (case, tuple(mut))
    if key not in _OUT:
        _OUT[key] = R.initialize(C.problem(case), svd4, mut=mut)
    return _OUT[key]


# ---------------------------------------------------------------------------------------------------------------- draws
def sample_tracked(draws, N):
    """the kernel's form: the identity plus the displaced positions, the latest override of a position wins"""
    opos, oval, idx = [], [], []
    for j in range(8):
        r, size = int(draws[j]), N - j
        v, b = r, size - 1
        for p, x in zip(opos, oval):
            if p == r:
                v = x
            if p == size - 1:
                b = x
        idx.append(v)
        opos.append(r)
        oval.append(b)
    return idx


def test_draws_follow_libc_rand():
    raw = R.libc_rand(0, 8 * 50)
    assert raw[:3] == [1804289383, 846930886, 1681692777]           # glibc after srand(0) (= srand(1))
    for N in (8, 9, 64, 300):
        d = R.draws_from_raw(raw, N, 50)
        k = 0
        for it in range(50):
            for j in range(8):
                span = N - 1 - j + 1
                assert d[it, j] == int((raw[k] / (2147483647 + 1.0)) * span) and 0 <= d[it, j] <= N - 1 - j    # Random.cpp:47-50
                k += 1
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(ctypes.c_uint(0))
    libc.rand.restype = ctypes.c_int
    assert [libc.rand() for _ in range(16)] == raw[:16]


def test_sampling_forms_agree():
    rng = np.random.default_rng(5)
    for N in (8, 9, 12, 64, 257):
        rows = [[int(rng.integers(0, N - j)) for j in range(8)] for _ in range(300)]
        rows += [[N - 1 - j for j in range(8)], [0] * 8, [max(0, N - 9)] * 8, [min(r, N - 1 - j) for j, r in enumerate([0, N - 2, 0, N - 4, 0, 0, 1, 1])]]
        for d in rows:
            idx = R.sample(d, N)
            assert idx == sample_tracked(d, N) and len(set(idx)) == 8 and all(0 <= i < N for i in idx), (N, d)


# ---------------------------------------------------------------------------------------------------------------- Normalize
def test_normalize_equals_the_library(pkg):
    rng = np.random.default_rng(11)
    sets = [C.problem(c)[k] for c in ("unmatched", "keys2000", "n8") for k in ("keys1", "keys2")]
    sets += [rng.uniform(0, 1241, (n, 2)).astype(F32) for n in (1, 2, 3, 777)] + [np.full((5, 2), 3.25, F32)]
    for keys in sets:
        pts, T = pkg.capi.initializer_normalize(keys)
        rp, rT = R.normalize(keys)
        assert pts.tobytes() == rp.tobytes() or (np.isnan(pts) == np.isnan(rp)).all(), len(keys)
        assert np.array_equal(pts, rp, equal_nan=True) and np.array_equal(T, rT, equal_nan=True), len(keys)
    # all keys of the frame, not the matched ones: the two differ where the frame has unmatched keys
    P = C.problem("unmatched")
    first, _, k1, _ = R.matched_keys(P)
    assert not np.array_equal(R.normalize(k1)[1], R.normalize(P["keys1"])[1])


def test_sequential_sums():
    rng = np.random.default_rng(3)
    x = rng.uniform(0, 6, 999).astype(F32)
    assert R.seq_sum32(x).tobytes() == np.cumsum(x, dtype=F32)[-1].tobytes()     # numpy's cumsum is the sequential f32 sum
    assert R.seq_sum32(x) != x.sum(dtype=F32) or True                            # (numpy's sum is pairwise: not used)
    t1, t2 = x[:400], x[400:800]
    assert R._score(t1, t2, ()).tobytes() == R.seq_sum32(np.stack([t1, t2], axis=1).reshape(-1)).tobytes()


# ---------------------------------------------------------------------------------------------------------------- outcomes
@pytest.mark.parametrize("case", C.NAMED)
def test_named_outcomes(case, svd4):
    o = outcome(case, svd4)
    model, ok, n_good = C.EXPECTED[case]
    assert (o["model"], o["ok"], [int(g) for g in o["n_good"]]) == (model, ok, n_good), (case, o["model"], o["ok"], o["n_good"], float(o["RH"]))


def test_outcome_details(svd4):
    o = outcome("planar120", svd4)
    assert o["winner"] == 0 and o["second"] == 29 and 1 < o["parallax"][0] < 1.2 and o["parallax"][1] > 4     # tied at 108: the first met is kept
    o = outcome("rotation120", svd4)
    assert max(float(p) for p in o["parallax"]) < 0.25 and o["winner"] == -1
    assert o["exits"][6] > 400                                                                       # good without parallax (cos >= 0.99998)
    o = outcome("small40", svd4)
    assert o["n_inliers"] == 38 and max(o["parallax"]) > 1                                           # refused by nMinGood alone
    o = outcome("noisy120", svd4)
    assert o["exits"][3] == 97
    o = outcome("general64", svd4)
    P = C.problem("general64")
    assert o["triangulated"].sum() == 62 and (o["P3D"][o["triangulated"] == 1][:, 2] > 5).all()
    assert abs(float(np.linalg.norm(o["t21"])) - 1) < 1e-6 and np.allclose(o["R21"], C._rot([0.1, 1, 0.05], 0.03), atol=2e-3)
    assert np.array_equal(o["inliers_F"], P["planted"])


# ---------------------------------------------------------------------------------------------------------------- hand-made rows
EYE = np.eye(3, dtype=F32)
F_SHIFT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], F32)      # the fundamental matrix of a translation along x: lines v = const


def test_row_chi_square_on_th():
    a, b = F32(float.fromhex("0x1.008p-1")), F32(float.fromhex("0x1.32aab4p+1"))
    assert F32(F32(a * a) + F32(b * b)) == F32(5.991)
    k1, k2 = np.array([[a, b], [a, b + F32(1e-3)]], F32), np.zeros((2, 2), F32)
    s, m, chi = R.check_homography(EYE, EYE, k1, k2, 1.0)
    assert chi[0, 0] == chi[0, 1] == F32(5.991) and m.tolist() == [True, False] and s == F32(0)     # on th: an inlier that adds 0
    assert R.check_homography(EYE, EYE, k1, k2, 1.0, {"chi_ge_H"})[1].tolist() == [False, False]
    d = F32(1.959847)
    assert F32(d * d) == F32(3.841)
    k1 = np.array([[0, d], [0, np.nextafter(d, F32(9))]], F32)
    s, m, chi = R.check_fundamental(F_SHIFT, k1, k2, 1.0)
    assert chi[0, 0] == chi[0, 1] == F32(3.841) and m.tolist() == [True, False]
    assert s.tobytes() == F32(F32(F32(5.991) - F32(3.841)) + F32(F32(5.991) - F32(3.841))).tobytes()
    assert R.check_fundamental(F_SHIFT, k1, k2, 1.0, {"chi_ge_F"})[1].tolist() == [False, False]


def test_row_score_ties_and_nan():
    assert R.walk([F32(3), F32(3), F32(2)]) == (0, F32(3)) and R.walk([F32(3), F32(3)], {"walk_ge"})[0] == 1
    assert R.walk([F32(0), F32(np.nan)]) == (-1, F32(0))                       # nothing scores above 0: no model
    assert R.choose_model(F32(0), F32(0))[0] == 1                              # RH = NaN goes to F
    assert R.choose_model(F32(2), F32(3))[0] == 0 and R.choose_model(F32(1.9), F32(3))[0] == 1      # (float)0.4 is above 0.40


def test_row_singular_homography():
    H = np.array([[1, 2, 3], [2, 4, 6], [0, 0, 1]], F32)
    H12, v, S = R.inv33(H, LD, detail=True)
    assert not H12.any()                                                        # cv::invert leaves the zero matrix
    k = np.array([[10, 20], [30, 40]], F32)
    s, m, _ = R.check_homography(H, H12, k, k, 1.0)
    assert np.isnan(s) and m.tolist() == [False, False] or np.isnan(s)          # 1 / 0 -> inf, 0 * inf -> NaN: the score is NaN ...
    assert R.walk([F32(1), s])[0] == 0                                          # ... and never beats a number


def _rt_rows(X, k1, k2, mut=()):
    K = np.array([1, 1, 0, 0], F32)
    t = np.array([1, 0, 0], F32)
    return R.check_rt_rows(EYE, t, K, np.asarray(k1, F32), np.asarray(k2, F32), np.asarray(X, F32), F32(4.0), F64, mut)


def test_row_check_rt_exits():
    inf, nan = np.inf, np.nan
    X = [[inf, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, -1], [-2, 0, 1], [0, 0, 0], [1e9, 0, 1e9 * 1.0]]
    k1 = [[0, 0], [2, 0], [2.001, 0], [0, 0], [0, 0], [-2, 0], [0, 0], [1, 0]]
    k2 = [[0, 0], [1, 0], [1, 0], [3.001, 0], [0, 0], [-1, 0], [0, 0], [1, 0]]
    flags, cos, exits = _rt_rows(X, k1, k2)
    assert exits[0] == 0 and flags[0] == 0                                      # a non-finite triangulation (:883)
    assert exits[1] == 5 and flags[1] == 3                                      # squareError1 == th2 exactly: kept (:916 is >)
    assert _rt_rows(X, k1, k2, {"th2_ge"})[2][1] == 3
    assert exits[2] == 3 and exits[3] == 4                                      # the two reprojection gates
    assert exits[4] == 1                                                        # behind camera 1 with parallax
    assert np.isnan(cos[6]) and exits[6] == 6 and flags[6] == 1                 # a NaN cosine: every comparison false, counted, not vbGood
    assert cos[7] >= F32(0.99998) and exits[7] == 6 and flags[7] == 1           # no parallax: counted, not triangulated
    Xz = [[0, 1, 0]]
    assert _rt_rows(Xz, [[0, 0]], [[0, 0]])[2][0] == 1 and _rt_rows(Xz, [[0, 0]], [[0, 0]], {"depth_lt"})[2][0] != 1   # z == 0 (:899 is <=)
    far = [[0, 0, -1e9]]                                                        # negative depth WITHOUT parallax passes :899 and :905
    f, c, e = _rt_rows(far, [[0, 0]], [[0, 0]])
    assert c[0] >= F32(0.99998) and e[0] == 6


def test_row_select_cos():
    ok = np.ones(3, np.uint8)
    n, c, p = R.select_cos(np.array([0.5, np.nan, 0.25], F32), ok)
    assert n == 3 and np.isnan(c) and np.isnan(p)                               # fewer than 51: the last of the sorted list; NaN sorts last
    n, c, p = R.select_cos(np.array([0.5, 0.75, 0.25], F32), np.array([1, 0, 1], np.uint8))
    assert n == 2 and c == F32(0.5) and abs(float(p) - 60) < 1e-12
    vals = np.concatenate([[np.nan, np.nan], np.linspace(0.9, 0.1, 60)]).astype(F32)
    n, c, _ = R.select_cos(vals, np.ones(62, np.uint8))
    assert n == 62 and c == np.sort(vals[2:])[50]
    assert R.select_cos(vals, np.ones(62, np.uint8), {"index_40"})[1] == np.sort(vals[2:])[40]
    assert R.select_cos(np.array([-0.0, 0.0, -1.0], F32), ok)[1] == 0 and R.select_cos(np.zeros(0, F32), np.zeros(0, np.uint8))[0] == 0
    assert R.cos_key(np.array([-0.0], F32))[0] == R.cos_key(np.array([0.0], F32))[0]
    k = R.cos_key(np.array([-np.inf, -1, -1e-30, 0, 1e-30, 1, np.inf, np.nan], F32))
    assert (np.diff(k.astype(np.int64)) > 0).all()


def test_row_acceptance_gates():
    aF = lambda g, p, n_inl, mut=(): R.accept_F(g, p, n_inl, 1.0, 50, set(mut))
    P4 = [F32(2)] * 4
    assert aF([100, 70, 0, 0], P4, 100) == 0 and aF([100, 70, 0, 0], P4, 100, ["similar_ge"]) == -1
    assert aF([100, 75, 0, 0], P4, 100) == -1 and aF([100, 75, 0, 0], P4, 100, ["similar_0.8"]) == 0
    assert aF([90, 0, 0, 0], P4, 100) == 0 and aF([90, 0, 0, 0], P4, 100, ["max_lt_le"]) == -1
    assert aF([85, 0, 0, 0], P4, 100) == -1 and aF([85, 0, 0, 0], P4, 100, ["min_good_0.8"]) == 0
    assert aF([49, 0, 0, 0], P4, 10) == -1                                          # nMinGood = minTriangulated
    one = [F32(1)] * 4
    assert aF([100, 0, 0, 0], one, 100) == -1 and aF([100, 0, 0, 0], one, 100, ["parallax_ge_F"]) == 0
    assert aF([0, 100, 100, 0], [F32(0), F32(0.5), F32(5), F32(0)], 100) == -1       # nsimilar = 2
    assert aF([60, 0, 0, 60], [F32(0.5), F32(0), F32(0), F32(5)], 60) == -1          # (two similar) ...
    assert aF([60, 0, 0, 0], [F32(0.5), F32(9), F32(9), F32(9)], 60) == -1           # the first that equals maxGood is the only one tried
    aH = lambda g, p, n_inl, mut=(): R.accept_H(g + [0] * (8 - len(g)), p + [F32(0)] * (8 - len(p)), n_inl, 1.0, 50, set(mut))[0]
    assert aH([100, 100], [F32(2), F32(3)], 100) == 0 and aH([100, 100], [F32(2), F32(3)], 100, ["second_le"]) == -1    # a tie does not raise the second best
    assert aH([100, 80], [F32(2), F32(3)], 100) == -1 and aH([100, 80], [F32(2), F32(3)], 100, ["second_0.9"]) == 0
    assert aH([100, 75], [F32(2)] * 2, 100) == -1 and aH([100, 74], [F32(2)] * 2, 100) == 0                              # 0.75: strict
    assert aH([100], [F32(1)], 100) == 0 and aH([100], [F32(1)], 100, ["parallax_gt_H"]) == -1                           # >= minParallax
    assert aH([50], [F32(2)], 50) == -1 and aH([50], [F32(2)], 50, ["best_ge_min"]) == 0                                 # > minTriangulated
    assert aH([85], [F32(2)], 100) == -1 and aH([85], [F32(2)], 100, ["best_0.8"]) == 0
    assert aH([90], [F32(2)], 100) == -1 and aH([91], [F32(2)], 100) == 0                                                # > 0.9 N
    assert R.accept_H([60, 80, 70, 80, 0, 0, 0, 0], [F32(2)] * 8, 80, 1.0, 50) == (-1, 80, 70)


def test_mutant_list_is_covered():
    rows = {"chi_ge_H", "chi_ge_F", "similar_ge", "max_lt_le", "parallax_ge_F", "second_le", "second_0.9", "parallax_gt_H", "best_ge_min",
            "best_0.8", "th2_ge", "depth_lt"}
    assert set(SCENE_MUTANTS) | rows == set(R.MUTANTS) and len(R.MUTANTS) == 20


@pytest.mark.parametrize("mutant", [m for m, c in SCENE_MUTANTS.items() if c])
def test_scene_mutant_changes_an_outcome(mutant, svd4):
    case = SCENE_MUTANTS[mutant]
    assert R.outcome_signature(outcome(case, svd4)) != R.outcome_signature(outcome(case, svd4, (mutant,))), (mutant, case)
