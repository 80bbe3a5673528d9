"""The fp64 primitives of csrc/se3.h and csrc/sim3_math.h on the device, each called directly through asd_debug_prim -- one launch
per (op, family, build) -- where the optimisers show them only behind several Levenberg iterations.

  * Bits.  The ops made of + - * / sqrt only, in the contract-off build, equal the float64 restatement (tests/prims_ref.py) bit for
    bit: the header's "IEEE division and square root, the reference's order of operations", tested.  The same for the device against
    the library's host path of that build.
  * Bounds.  The ops that carry transcendentals or the device rsqrt -- and, in the contracted build, the algebraic se3.h ops, where
    the device fuses multiply-adds the x86-64 host cannot -- stay within the bar of their family: |got - exact| <= bar u S, with the
    exact value and the sensitivity scale S from tests/golden/prims_golden.npz and the bar 4 x what the float64 restatement itself
    reaches (tests/prims_cases.py; tests/test_prims_ref.py proves the checker on the CPU).

Every test prints its figure before it asserts.  Measured on an MI355X: DESIGN.md, "SE3/Sim3 primitives".
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import prims_cases as pc
from tests import prims_ref as pr
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(GOLDEN, "prims_golden.npz"))
FAMILIES = sorted(k[:-2] for k in G.files if k.endswith(".x"))
CASES = pc.families()
PAIRS = [(fam, op) for fam in FAMILIES for op in CASES[fam][0]]
SE3 = ("asd_rsqrt", "quat_normalize", "quat_rotate", "pose_map", "pose_oplus", "rot_to_quat_eigen", "huber", "jac_pose")
BITS = [(fam, op) for fam, op in PAIRS if op in pr.ALGEBRAIC]
BOUNDS = [(fam, op, fused) for fam, op in PAIRS for fused in (False, True)
          if pc.has_exact(op) and (op in SE3 if fused else op not in pr.ALGEBRAIC)]
BUILD_IDS = {False: "contract_off", True: "contracted"}

_dev, _ref = {}, {}


def dev(hip, fam, op, fused=False):
    """the device's outputs, computed once per (family, op, build)"""
    key = (fam, op, fused)
    if key not in _dev:
        _dev[key] = hip.debug_prim(op, G[fam + ".x"], fused=fused)
    return _dev[key]


def ref64(fam, op):
    if (fam, op) not in _ref:
        _ref[fam, op] = pr.f64(op, G[fam + ".x"])
    return _ref[fam, op]


def _assert_same_bits(got, want, what):
    bad = np.nonzero(~pr.same_bits(got, want).all(axis=1))[0]
    print(f"{what}: {len(got) - len(bad)} of {len(got)} rows bit-equal")
    assert not len(bad), f"{what}: rows {bad[:8]} differ, the first by {np.abs(got[bad[0]] - want[bad[0]])}"


@pytest.mark.parametrize("fam,op", BITS)
def test_bits_against_the_f64_restatement(hip, fam, op):
    """NaNs compare equal: the flag and the x of a failed s3_solve7 and the inf / NaN pattern of a singular LU are part of this"""
    _assert_same_bits(dev(hip, fam, op), ref64(fam, op), f"{op}@{fam} device vs restatement")


@pytest.mark.parametrize("fam,op", BITS)
def test_bits_device_against_host(hip, fam, op):
    _assert_same_bits(dev(hip, fam, op), hip.debug_prim(op, G[fam + ".x"], host=True), f"{op}@{fam} device vs host path")


@pytest.mark.parametrize("fam,op,fused", BOUNDS, ids=[f"{o}@{f}-{BUILD_IDS[b]}" for f, o, b in BOUNDS])
def test_bounds(hip, fam, op, fused):
    got = dev(hip, fam, op, fused)
    hi = G[fam + ".hi"]
    assert np.isfinite(got).all()
    if op == "asd_rsqrt":   # the header's own claim: at most 2 ulp of the correctly rounded value
        ulps = float((np.abs(got - hi) / np.spacing(hi)).max())
        print(f"asd_rsqrt ({BUILD_IDS[fused]}): worst {ulps:.3g} ulp of the correctly rounded value, bar {pc.RSQRT_ULPS}")
        assert ulps <= pc.RSQRT_ULPS
        return
    r = pr.ratios(got, hi, G[fam + ".lo"], G[fam + ".S"])
    if fused and fam + ".alt_rows" in G.files:   # theta^2 within 4 ulp of 1e-10: either side's formula (pose_oplus_other_side)
        rows = G[fam + ".alt_rows"]
        alt = pr.ratios(got[rows], G[fam + ".alt_hi"], G[fam + ".alt_lo"], G[fam + ".alt_S"])
        other = alt.max(axis=1) < r[rows].max(axis=1)
        print(f"  {int(other.sum())} of {len(rows)} rows next to theta^2 = 1e-10 took the other side's branch")
        r[rows[other]] = alt[other]
    bar = pc.BAR[f"{op}@{fam}"]
    print(f"{op}@{fam} ({BUILD_IDS[fused]}): device worst {r.max():.4g} u S (row {r.max(axis=1).argmax()}), f64 restatement "
          f"{pc.MEASURED[f'{op}@{fam}']:.4g}, bar {bar:g}")
    assert r.max() <= bar
    if op == "quat_normalize":
        assert (got[:, 3] >= 0).all()
    if op == "pose_oplus":
        q = np.asarray(got[:, :4], np.longdouble)
        off = np.abs(np.sqrt((q * q).sum(axis=1)) - 1)
        print(f"  | |q| - 1 | worst {float(off.max() / pr.U):.3g} u")
        assert float(off.max()) <= 4 * pr.U
        assert (got[:, 3] >= 0).all()


@pytest.mark.parametrize("op", ["s3_oplus", "s3_oplus_eigen"])
def test_oplus_with_fix_scale_returns_the_scale_bits(hip, op):
    n = 0
    for fam in FAMILIES:
        if fam.startswith("s3_oplus."):
            x = G[fam + ".x"]
            fix = x[:, 15] != 0
            n += int(fix.sum())
            assert pr.same_bits(dev(hip, fam, op)[fix, 7], x[fix, 7]).all(), fam
    assert n >= 20


def test_two_runs_give_equal_bits(hip):
    for (fam, op, fused), first in list(_dev.items()) or [((f, o, False), dev(hip, f, o)) for f, o in PAIRS]:
        assert pr.same_bits(hip.debug_prim(op, G[fam + ".x"], fused=fused), first).all(), (fam, op, fused)


def test_refusals_and_the_empty_call(hip):
    lib = hip.lib
    lib.asd_debug_prim.restype = C.c_int32
    lib.asd_debug_prim.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    buf = np.full(64, 7.0)
    p = buf.ctypes.data_as(C.c_void_p)
    for op, flags, n, a, b in ((-1, 0, 1, p, p), (25, 0, 1, p, p), (8, 2, 1, p, p), (8, 3, 1, p, p), (0, 4, 1, p, p), (0, 0, -1, p, p),
                               (0, 0, 1, None, p), (0, 0, 1, p, None), (0, 1, 1, None, p)):
        assert lib.asd_debug_prim(hip.ctx, op, flags, n, a, b) == -1, (op, flags, n)
        assert "asd_debug_prim" in hip.last_error()
    assert lib.asd_debug_prim(None, 0, 0, 1, p, p) == -1          # the device path needs a context; the host path does not
    assert lib.asd_debug_prim(None, 0, 1, 1, p, p) == 0 and buf[0] == 1.0 / np.sqrt(7.0)
    buf[:] = 7.0
    for flags in (0, 1, 2, 3):
        assert lib.asd_debug_prim(hip.ctx, 4, flags, 0, p, p) == 0   # n = 0: OK, nothing launched, nothing written
    assert (buf == 7.0).all()
