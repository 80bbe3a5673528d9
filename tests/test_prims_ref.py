"""The checker of tests/test_prims.py, proved without a GPU: the float64 restatement of every primitive of csrc/se3.h and
csrc/sim3_math.h (tests/prims_ref.py) against the exact values stored in tests/golden/prims_golden.npz, the library's HOST path of
asd_debug_prim (the header functions themselves, compiled for the CPU) against the restatement, and seeded mistakes, each of which
must fail the check that is there to catch it.

Figures (make_prims_golden.py prints them; DESIGN.md, "SE3/Sim3 primitives", has the table): over the well-conditioned families the f64
restatement stays below 3.5 u S; next to g2o's own thresholds its formulas cancel and reach 3.6e9 u S (s3_log, sigma just above 1e-5).
The host path equals the restatement bit for bit on EVERY family, the transcendental ones included (both call glibc).
"""
import os

import numpy as np
import pytest

from tests import prims_cases as pc
from tests import prims_ref as pr
from tests.conftest import GOLDEN, load_package

G = np.load(os.path.join(GOLDEN, "prims_golden.npz"))
FAMILIES = sorted(k[:-2] for k in G.files if k.endswith(".x"))
CASES = pc.families()
PAIRS = [(fam, op) for fam in FAMILIES for op in CASES[fam][0]]
BOUND_PAIRS = [(fam, op) for fam, op in PAIRS if pc.has_exact(op)]


def _host(op, x, fused=False):
    return load_package().capi.debug_prim(op, x, host=True, fused=fused)


def _worst(fam, got):
    return float(pr.ratios(got, G[fam + ".hi"], G[fam + ".lo"], G[fam + ".S"]).max())


def _rsqrt_ulps(fam, got):
    hi = G[fam + ".hi"]   # the correctly rounded 1 / sqrt(x)
    return float((np.abs(got - hi) / np.spacing(hi)).max())


def test_the_stored_families_are_the_generators():
    assert FAMILIES == sorted(CASES)
    for fam in FAMILIES:
        assert pr.same_bits(G[fam + ".x"], CASES[fam][1]).all(), fam
        assert (fam + ".hi" in G.files) == pc.has_exact(CASES[fam][0][0]), fam
    assert sorted(pc.MEASURED) == sorted(f"{op}@{fam}" for fam, op in BOUND_PAIRS if op != "asd_rsqrt")


def test_the_cases_reach_every_branch():
    """read from the comparisons the restatement records, so a changed generator cannot quietly stop covering one"""
    def recs(op, fams):
        return [tuple(pr._f64_item(op, row)[1]) for f in FAMILIES if f.split(".")[0] in fams for row in CASES[f][1]]

    # pose_oplus: (theta^2 < 1e-10, [theta^2 < 0.01], ...), and the flip of the last quat_normalize (the last comparison)
    r = recs("pose_oplus", ("pose_oplus_theta", "pose_oplus_flip"))
    assert {True} <= {x[0] for x in r} and {True, False} <= {x[1] for x in r if not x[0]}
    assert {True, False} <= {x[-1] for x in r}
    # the matrix -> quaternion conversions: trace > 0, and i = 0, 1, 2 below
    for op in ("rot_to_quat_eigen", "s3_quat_of_rot", "s3_quat_of_rot_eigen"):
        r = recs(op, ("rot_to_quat",))
        assert {(True,), (False, False, False), (False, True, False), (False, False, True), (False, True, True)} <= set(r), op
    R = G["rot_to_quat.x"]
    tie = lambda a, b, c: np.any((R[:, a] == R[:, b]) & (R[:, a] > R[:, c]) & (R[:, 0] + R[:, 4] + R[:, 8] <= 0))
    assert tie(4, 0, 8) and tie(8, 4, 0) and np.any((R[:, 0] == R[:, 4]) & (R[:, 4] == R[:, 8]) & (R[:, 0] == 0))
    # s3_exp and s3_log: the four (|sigma| < eps, theta < eps) branches
    for op, fam in (("s3_exp", "s3_exp"), ("s3_log", "s3_log")):
        assert {(a, b) for a in (True, False) for b in (True, False)} <= {x[:2] for x in recs(op, (fam,))}, op
    # s3_lu_solve3: first pivot row 0 / 1 / 2 x second swap, and ties
    r = recs("s3_lu_solve3", ("s3_lu_solve3",))
    assert {(p, s) for p in range(3) for s in (False, True)} <= {(2 if x[1] else 1 if x[0] else 0, x[2]) for x in r}
    # s3_solve7: the first non-positive pivot at each j, and none
    first_bad = {(x.index(True) if True in x else -1) for x in recs("s3_solve7", ("s3_solve7",))}
    assert first_bad == {-1, 0, 1, 2, 3, 4, 5, 6}
    # huber: e2 at delta^2 exactly and one ulp either side
    h = G["huber.x"]
    d2 = h[:, 1] * h[:, 1]
    assert np.any(h[:, 0] == d2) and np.any(h[:, 0] == np.nextafter(d2, 0)) and np.any(h[:, 0] == np.nextafter(d2, np.inf))
    assert {True, False} <= {x[0] for x in recs("quat_normalize", ("quat_normalize",))}


@pytest.mark.parametrize("fam,op", BOUND_PAIRS)
def test_f64_restatement_within_a_quarter_of_the_bar(fam, op):
    got = pr.f64(op, G[fam + ".x"])
    if op == "asd_rsqrt":   # its bar is the header's claim, not a measurement: 1 / sqrt(x) in two roundings stays within 1 ulp
        assert _rsqrt_ulps(fam, got) <= 1.0
        return
    worst = _worst(fam, got)
    print(f"{op}@{fam}: f64 restatement {worst:.4g} u S, bar {pc.BAR[f'{op}@{fam}']:g}")
    assert worst <= pc.BAR[f"{op}@{fam}"] / 4
    assert abs(worst - pc.MEASURED[f"{op}@{fam}"]) <= 1e-3 * worst, "prims_cases.MEASURED is not what the restatement gives"


@pytest.mark.parametrize("fused", [False, True], ids=["contract_off", "contracted"])
@pytest.mark.parametrize("fam,op", PAIRS)
def test_host_path(fam, op, fused):
    """the header functions on the CPU: bit for bit the restatement on the algebraic ops; within the bar wherever there is one"""
    x = G[fam + ".x"]
    pkg = load_package()
    if fused and pkg.capi.PRIM_OP[op] >= pkg.capi.PRIM_SE3_OPS:
        with pytest.raises(pkg.AsdError):
            _host(op, x, fused=True)
        return
    got = _host(op, x, fused)
    if op in pr.ALGEBRAIC:   # (x86-64 has no fused multiply-add to contract into, so this holds for both builds of the host code)
        ref = pr.f64(op, x)
        bad = np.nonzero(~pr.same_bits(got, ref).all(axis=1))[0]
        assert not len(bad), f"{op}@{fam}: rows {bad[:8]} differ from the restatement"
    if op == "asd_rsqrt":
        assert _rsqrt_ulps(fam, got) <= pc.RSQRT_ULPS
    elif pc.has_exact(op):
        assert _worst(fam, got) <= pc.BAR[f"{op}@{fam}"]
    if op == "quat_normalize":
        assert (got[:, 3] >= 0).all()


def _fails_bound(op, mut, fams):
    """some family's bar is exceeded by the mutant, and none by the restatement itself"""
    over = []
    for fam in FAMILIES:
        if fam.split(".")[0] in fams:
            bar = pc.BAR[f"{op}@{fam}"]
            assert _worst(fam, pr.f64(op, G[fam + ".x"])) <= bar
            w = _worst(fam, pr.f64(op, G[fam + ".x"], mut))
            if not w <= bar:
                over.append((fam, w, bar))
    return over


def _fails_bits(op, mut, fam):
    """rows on which the mutant's bits differ from the host path's (which the restatement itself matches: test_host_path)"""
    x = G[fam + ".x"]
    return np.nonzero(~pr.same_bits(_host(op, x), pr.f64(op, x, mut)).all(axis=1))[0]


def test_mutant_series_term_dropped():
    over = _fails_bound("pose_oplus", "drop_720", ("pose_oplus_theta", "pose_oplus_flip"))
    assert {f for f, _w, _b in over} == {"pose_oplus_theta.t1", "pose_oplus_flip.t1"}, over   # the series branch, and only it


def test_mutant_closed_form_below_eps():
    over = _fails_bound("pose_oplus", "closed_below_eps", ("pose_oplus_theta", "pose_oplus_flip"))
    assert "pose_oplus_theta.t0" in {f for f, _w, _b in over}, over
    for op in ("s3_exp", "s3_exp_eigen"):
        over = _fails_bound(op, "closed_below_eps", ("s3_exp",))
        assert {f for f, _w, _b in over} >= {"s3_exp.s0t0", "s3_exp.s3t0"}, over
        assert all(f.endswith("t0") for f, _w, _b in over), over


def test_mutant_trace_comparison():
    assert _fails_bound("rot_to_quat_eigen", "trace_ge", ("rot_to_quat",))
    for op in ("s3_quat_of_rot", "s3_quat_of_rot_eigen"):
        bad = _fails_bits(op, "trace_ge", "rot_to_quat")
        R = G["rot_to_quat.x"][bad]
        tr = R[:, 0] + (R[:, 4] + R[:, 8]) if op.endswith("eigen") else R[:, 0] + R[:, 4] + R[:, 8]
        assert len(bad) and (tr == 0).all()   # where the trace, in the op's own association, is exactly 0, and nowhere else


@pytest.mark.parametrize("mut", ["lu_no_pivot", "lu_last_wins", "lu_one_by_one"])
def test_mutant_lu(mut):
    assert len(_fails_bits("s3_lu_solve3", mut, "s3_lu_solve3"))


def test_mutant_plain_quaternion_product():
    assert len(_fails_bits("s3_mul_eigen", "plain_quat_product", "s3_mul"))
    assert not len(_fails_bits("s3_mul", "plain_quat_product", "s3_mul"))


def test_mutant_huber_comparison():
    bad = _fails_bits("huber", "huber_lt", "huber")
    h = G["huber.x"][bad]
    assert len(bad) and (h[:, 0] == h[:, 1] * h[:, 1]).all()   # at the kink, nowhere else


def test_regenerating_a_sample_reproduces_the_golden():
    pytest.importorskip("mpmath")
    for fam in FAMILIES:
        ops, x = CASES[fam]
        if not pc.has_exact(ops[0]):
            continue
        rows = np.arange(0, len(x), 7)
        hi, lo, S = pr.exact(ops[0], x[rows])
        assert pr.same_bits(hi, G[fam + ".hi"][rows]).all() and pr.same_bits(lo, G[fam + ".lo"][rows]).all(), fam
        assert np.allclose(S, G[fam + ".S"][rows], rtol=1e-12, atol=0), fam
        if fam + ".alt_rows" in G.files:
            rows, y = pc.pose_oplus_other_side(x)
            assert (rows == G[fam + ".alt_rows"]).all()
            hi, lo, S = pr.exact(ops[0], x[rows][:2], branches_of=y[:2])
            assert pr.same_bits(hi, G[fam + ".alt_hi"][:2]).all() and pr.same_bits(lo, G[fam + ".alt_lo"][:2]).all(), fam
