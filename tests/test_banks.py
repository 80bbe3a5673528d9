"""The two device banks -- descriptors (asd_bank_put, asd_bank_put_from_frame) and map-point attributes (asd_mpbank_put) -- read back
through asd_debug_bank_get and compared with a NumPy mirror that the test updates by the same sequence of puts.  Every write is a copy,
so every comparison is bit for bit (uint32 views) and there is no tolerance anywhere.  A row the test has not written is never read:
fresh device memory is unspecified.  Capacity is per context, so a test that counts on a fresh 16384-row bank makes its own context."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_matcher import BOUNDS, _m1_case, make_frame, pose_T
from tests.test_track_chain import _frame_case, _pose7

pytestmark = pytest.mark.gpu

FIRST_CAP = 16384   # rows of a bank after its first small put


def _ctx(pkg):
    return pkg.AsdHip(n_features=500, max_width=640, max_height=240, max_patches=1024)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _desc(n, seed):
    """n descriptor rows, every value different; row 0 carries bit patterns a copy must not touch (-0, a denormal, inf)"""
    d = np.random.default_rng(seed).standard_normal((n, 128)).astype(np.float32)
    if n:
        d[0, :3] = np.array([-0.0, 1e-40, np.inf], np.float32)
    return d


def _attrs(n, seed):
    """(Xw, normal, min_dist, max_dist): four tables of different ranges, no symmetry between the columns"""
    rng = np.random.default_rng(seed)
    Xw = (rng.standard_normal((n, 3)) * 10).astype(np.float32)
    nrm = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    mind = rng.uniform(1, 2, n).astype(np.float32)
    maxd = rng.uniform(30, 60, n).astype(np.float32)
    return Xw, nrm, mind, maxd


class Mirror:
    """row -> 128 f32 (descriptor bank) and row -> 8 f32 (attribute bank: Xw, normal, min_dist, max_dist in that order)"""

    def __init__(self):
        self.desc, self.attr = {}, {}

    def put_desc(self, first, d):
        d = np.array(d, np.float32)
        for i in range(len(d)):
            self.desc[first + i] = d[i]

    def put_attr(self, first, Xw, nrm, mind, maxd):
        a = np.concatenate([np.array(Xw, np.float32).reshape(-1, 3), np.array(nrm, np.float32).reshape(-1, 3),
                            np.array(mind, np.float32).reshape(-1, 1), np.array(maxd, np.float32).reshape(-1, 1)], axis=1)
        for i in range(len(a)):
            self.attr[first + i] = a[i]

    @staticmethod
    def _runs(table):
        k = np.array(sorted(table), np.int64)
        if not len(k):
            return []
        return [(int(r[0]), len(r)) for r in np.split(k, np.nonzero(np.diff(k) != 1)[0] + 1)]

    def check(self, hip):
        """every row written so far reads back with the bits last written to it"""
        for first, n in self._runs(self.desc):
            got, _ = hip.bank_get(first, n, attr=False)
            exp = np.stack([self.desc[r] for r in range(first, first + n)])
            bad = np.nonzero((_bits(got) != _bits(exp)).any(axis=1))[0]
            assert not len(bad), f"descriptor bank: {len(bad)} of rows [{first}, {first + n}) differ, first at row {first + bad[0]}"
        for first, n in self._runs(self.attr):
            _, got = hip.bank_get(first, n, desc=False)
            exp = np.stack([self.attr[r] for r in range(first, first + n)])
            bad = np.nonzero((_bits(got) != _bits(exp)).any(axis=1))[0]
            assert not len(bad), f"attribute bank: {len(bad)} of rows [{first}, {first + n}) differ, first at row {first + bad[0]}"


def _put_desc(hip, mir, first, d):
    hip.bank_put(first, d)
    mir.put_desc(first, d)


def _put_attr(hip, mir, first, a):
    hip.mpbank_put(first, *a)
    mir.put_attr(first, *a)


def _put_frame(hip, mir, slot, frame_desc, first, n):
    hip.bank_put_from_frame(slot, first, n)
    mir.put_desc(first, frame_desc[:n])


def test_round_trip_of_the_three_puts(pkg):
    """n = 0, 1, 127, 1024 through each put, overlapping ranges (the later put wins), asd_bank_put_from_frame below, at and one above the
    frame's keypoint count, and the attribute row layout Xw, normal, min_dist, max_dist"""
    hip, mir = _ctx(pkg), Mirror()
    try:
        kps, fdesc = make_frame(1024, 71)
        hip.frame_set(2, kps, fdesc, BOUNDS)
        row = 0
        for k, n in enumerate((0, 1, 127, 1024)):
            _put_desc(hip, mir, row, _desc(n, 10 + k))
            _put_attr(hip, mir, row + 3, _attrs(n, 20 + k))
            _put_frame(hip, mir, 2, fdesc, row + 2000, n)
            mir.check(hip)
            row += n + 5
        # the layout, stated once without the mirror: a swapped column would show here by name
        Xw, nrm, mind, maxd = _attrs(127, 31)
        hip.mpbank_put(5000, Xw, nrm, mind, maxd)
        mir.put_attr(5000, Xw, nrm, mind, maxd)
        _, a = hip.bank_get(5000, 127, desc=False)
        assert np.array_equal(_bits(a[:, 0:3]), _bits(Xw)) and np.array_equal(_bits(a[:, 3:6]), _bits(nrm))
        assert np.array_equal(_bits(a[:, 6]), _bits(mind)) and np.array_equal(_bits(a[:, 7]), _bits(maxd))
        # overlapping ranges: the later put wins, whichever entry point made it
        _put_desc(hip, mir, 6000, _desc(1024, 41))
        _put_frame(hip, mir, 2, fdesc, 6500, 1024)          # over the upper half and beyond
        _put_desc(hip, mir, 6400, _desc(127, 42))            # across the seam
        _put_desc(hip, mir, 6450, _desc(1, 43))
        _put_attr(hip, mir, 6000, _attrs(1024, 44))
        _put_attr(hip, mir, 6900, _attrs(127, 45))
        _put_attr(hip, mir, 6899, _attrs(1, 46))
        mir.check(hip)
        # asd_bank_put_from_frame: n < F->n, n == F->n (both above), n == F->n + 1 is refused and writes nothing
        with pytest.raises(pkg.capi.AsdError) as e:
            hip.bank_put_from_frame(2, 9000, 1025)
        assert e.value.code == -1
        _put_frame(hip, mir, 2, fdesc, 9000, 1023)
        mir.check(hip)
    finally:
        hip.close()


@pytest.mark.parametrize("end", [FIRST_CAP - 1, FIRST_CAP, FIRST_CAP + 1])
def test_rows_survive_the_capacity_boundary_and_growth(pkg, end):
    """A put whose first_row + n is one below, at and one above the first capacity (16384 rows) of both banks, in a fresh context each,
    then rows 70000 .. 70999 for another growth: after every put the whole mirror reads back, so every earlier row survived the growth"""
    hip, mir = _ctx(pkg), Mirror()
    try:
        kps, fdesc = make_frame(1000, 72)
        hip.frame_set(2, kps, fdesc, BOUNDS)
        # rows the growths have to carry over, written by every entry point
        _put_desc(hip, mir, 0, _desc(127, 1))
        _put_frame(hip, mir, 2, fdesc, 8000, 1000)
        _put_attr(hip, mir, 0, _attrs(127, 2))
        _put_attr(hip, mir, 8000, _attrs(1000, 3))
        mir.check(hip)
        n = 300
        _put_desc(hip, mir, end - n, _desc(n, 4))
        mir.check(hip)
        _put_attr(hip, mir, end - n, _attrs(n, 5))
        mir.check(hip)
        _put_frame(hip, mir, 2, fdesc, 70000, 1000)
        mir.check(hip)
        _put_attr(hip, mir, 70000, _attrs(1000, 6))
        mir.check(hip)
    finally:
        hip.close()


def test_mpbank_put_staging_buffers(pkg):
    """asd_mpbank_put alternates between two pinned staging buffers.  Five puts in a row with no read in between (n = 1000, 10, 3000, 10,
    2999, disjoint rows): each turn's buffer is used again, then reallocated, while the other turn's upload may still be pending.  Then a
    put whose arrays the caller overwrites as soon as the call has returned ("the arrays are consumed on return")."""
    hip, mir = _ctx(pkg), Mirror()
    try:
        row = 100
        for k, n in enumerate((1000, 10, 3000, 10, 2999)):
            _put_attr(hip, mir, row, _attrs(n, 50 + k))
            row += n + 7
        Xw, nrm, mind, maxd = _attrs(1000, 60)
        keep = [x.copy() for x in (Xw, nrm, mind, maxd)]
        assert all(x.flags.c_contiguous and x.dtype == np.float32 for x in (Xw, nrm, mind, maxd))   # the binding passes these very arrays
        hip.mpbank_put(row, Xw, nrm, mind, maxd)
        Xw[:] = 7; nrm[:] = -3; mind[:] = 99; maxd[:] = 0
        mir.put_attr(row, *keep)
        mir.check(hip)
    finally:
        hip.close()


def _bracket_sequence(hip, mir, base, bracket, kps, fdesc, attrs):
    if bracket:
        hip.prep_async(1)
    hip.frame_set(2, kps, fdesc, BOUNDS)
    for c in range(20):
        _put_frame(hip, mir, 2, fdesc, base + c * 1000, 1000)
    _put_attr(hip, mir, base, attrs)
    if bracket:
        hip.prep_async(0)


@pytest.mark.parametrize("base", [0, 65536])
def test_bracket_leaves_the_same_bits_as_no_bracket(pkg, base):
    """Guard for the growth of the descriptor bank inside an asd_prep_async bracket: frame_set, twenty asd_bank_put_from_frame of 1000
    rows, one asd_mpbank_put of 20000 rows, once inside a bracket (everything on the context's second stream) and once without, on a
    fresh context each; asd_debug_bank_get waits for the context's own stream only, so it sees what a consumer enqueued after the bracket
    would see.  With base = 0 the bank grows past 16384 rows at the seventeenth put, with sixteen puts enqueued on the second stream: the
    growth has to wait for that stream before it carries the old rows over.  base = 65536 is the host loop's second region.
    The outcome before the fix depended on timing (the device usually drains the second stream while the host sits in hipMalloc): this
    test is required to pass with the fix, it was never run without it and is no proof that the unfixed growth lost rows."""
    kps, fdesc = make_frame(1000, 73)
    attrs = _attrs(20000, 74)
    for bracket in (True, False):
        hip, mir = _ctx(pkg), Mirror()
        try:
            _bracket_sequence(hip, mir, base, bracket, kps, fdesc, attrs)
            assert len(mir.desc) == 20000 and len(mir.attr) == 20000
            mir.check(hip)
        finally:
            hip.close()


def test_armed_descriptor_stage_survives_bank_puts(pkg, synth):
    """Guard for asd_bank_put's staging: the descriptor form of asd_track_motion_model uploads mp_desc through the pinned block that
    asd_bank_put stages its rows in.  Between the armed call and asd_track_finish one put reuses that block and a second, of 9000 rows,
    makes it grow (it starts at 8192 rows) -- the put has to let the stage's copy leave the block first.  asd_track_finish must return
    the synchronous call's bits.  Timing decided the outcome before the fix (the copy is usually gone long before the host gets there):
    this test is required to pass with the fix, it was never run without it and is no proof that the unfixed put corrupted a stage."""
    n, th = 300, 15.0
    kl, dl, kc, dc, Xw, has, mp_desc, T, K = _m1_case(synth, n, 4242)
    pose0 = _pose7(pose_T(rv=(0.012, -0.018, 0.006), t=(0.12, -0.04, 0.33)))
    other = _desc(9000, 75)

    def ctx():
        h = _ctx(pkg)
        h.frame_set(0, kc, dc, BOUNDS)
        h.frame_set(1, kl, dl, BOUNDS)
        return h
    a = ctx()
    try:
        exp = a.track_motion_model(0, 1, n, has, Xw, mp_desc, T, K, th, pose0, True)
    finally:
        a.close()
    assert exp[1] > 50 and exp[4] > 20   # the stage did real work
    b, mir = ctx(), Mirror()
    try:
        assert b.track_motion_model(0, 1, n, has, Xw, mp_desc, T, K, th, pose0, True, split=True) is None
        _put_desc(b, mir, 5000, other[:300])
        _put_desc(b, mir, 40000, other)
        got = b.track_finish()
        mir.check(b)
    finally:
        b.close()
    for x, y in zip(got, exp):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("base", [0, FIRST_CAP - 4, 100000])
def test_consumers_at_high_rows(pkg, oracle, synth, base):
    """asd_match_project_frame_bank and asd_track_local_points_rows with the map points at rows 0 .., 16380 .. (across the first capacity
    boundary) and 100000 ..: the bits of the descriptor-table forms on the same data, and the oracle's matches"""
    n = 300
    kl, dl, kc, dc, Xw, has, mp_desc, T, K, Xw2, nrm, mind, maxd = _frame_case(synth, n, 1200)
    n_cur = len(kc)
    desc2 = np.concatenate([mp_desc, mp_desc])
    pose0 = _pose7(pose_T(rv=(0.012, -0.018, 0.006), t=(0.12, -0.04, 0.33)))
    hip, mir = _ctx(pkg), Mirror()
    try:
        hip.frame_set(0, kc, dc, BOUNDS)
        hip.frame_set(1, kl, dl, BOUNDS)
        _put_desc(hip, mir, base, desc2)
        _put_attr(hip, mir, base, (Xw2, nrm, mind, maxd))
        mir.check(hip)
        rows1 = np.arange(base, base + n, dtype=np.int32)
        cand_rows = np.arange(base, base + 2 * n, dtype=np.int32)
        oc, ol = oracle.frame(kc, dc, BOUNDS), oracle.frame(kl, dl, BOUNDS)
        # frame to frame
        a, na = hip.match_project_frame(0, 1, n_cur, has, Xw, mp_desc, T, K, 15.0, True)
        b, nb = hip.match_project_frame_bank(0, 1, n_cur, has, Xw, rows1, T, K, 15.0, True)
        om, onm = oracle.match_project_frame(oc, ol, has, Xw, mp_desc, T, K, 15.0, True)
        np.testing.assert_array_equal(b, a)
        np.testing.assert_array_equal(b, om)
        assert na == nb == onm and nb > 50
        # local map: what Tracking does between the stages, then the stage by rows and by tables
        m1, n1, pose1, outl1, inl1 = hip.track_motion_model(0, 1, n_cur, has, Xw, mp_desc, T, K, 15.0, pose0, True)
        keep = (m1 >= 0) & (outl1 == 0)
        T1 = hip.pose7_to_tcw(pose1) if (m1 >= 0).sum() >= 3 else T
        in_frame = np.zeros(2 * n, bool)
        in_frame[m1[m1 >= 0]] = True
        sel = np.nonzero(~in_frame)[0].astype(np.int32)
        occ = keep.astype(np.uint8)
        cur_Xw = Xw[np.maximum(m1, 0)]
        by_tables = hip.track_local_points(0, n_cur, Xw2[sel], nrm[sel], mind[sel], maxd[sel], desc2[sel], T1, K, occ, cur_Xw, 1.0, 0.8, pose1)
        by_rows = hip.track_local_points_rows(0, n_cur, cand_rows[sel], T1, K, occ, cur_Xw, 1.0, 0.8, pose1)
        for x, y in zip(by_rows, by_tables):
            np.testing.assert_array_equal(x, y)
        in_view, proj, level, vc = oracle.frustum(oc, Xw2[sel], nrm[sel], mind[sel], maxd[sel], T1, K)
        om2, on2 = oracle.match_project_points(oc, in_view, proj, level, vc, desc2[sel], occ, 1.0, 0.8)
        np.testing.assert_array_equal(by_rows[0], om2)
        assert by_rows[1] == on2 and on2 > 0
    finally:
        hip.close()


def test_refusals_leave_the_banks_usable(pkg, synth):
    """Ranges the puts refuse before anything is allocated or enqueued -- negative first_row or n (-1), first_row + n past 2^31 and past
    ASD_BANK_MAX_ROWS (-5, the name in the message) -- and the reads asd_debug_bank_get refuses: a row at the bank's capacity, an open
    bracket, an armed stage.  After each refusal an ordinary put and read-back works, and the armed stage finishes with the synchronous
    call's bits.  (first_row = ASD_BANK_MAX_ROWS - 1 is legal and not attempted: it would allocate 2 GiB.)  These calls were only ever
    made against the fixed library: the 32-bit sum they replace wrote outside the allocation."""
    MAX = pkg.capi.BANK_MAX_ROWS
    assert f"#define ASD_BANK_MAX_ROWS (1 << {MAX.bit_length() - 1})" in open(os.path.join(ROOT, "include", "asd_slam.h")).read()
    n = 300
    kl, dl, kc, dc, Xw, has, mp_desc, T, K = _m1_case(synth, n, 4242)
    pose0 = _pose7(pose_T(rv=(0.012, -0.018, 0.006), t=(0.12, -0.04, 0.33)))
    d = _desc(1000, 80)
    Xa, na_, mi, ma = _attrs(1000, 81)
    hip, mir = _ctx(pkg), Mirror()
    state = {"row": 200}

    def still_works():
        r = state["row"]
        state["row"] += 11
        _put_desc(hip, mir, r, _desc(5, r))
        _put_attr(hip, mir, r + 2, _attrs(5, r + 1))
        _put_frame(hip, mir, 1, dl, r + 5, 3)
        mir.check(hip)

    def puts(first_row, cnt):
        """the three puts through the C ABI itself (the bindings take n from the arrays) -> [(name, rc, message)]"""
        L, i32 = hip.lib, C.c_int32
        out = []
        for name, call in (("asd_bank_put", lambda: L.asd_bank_put(hip.ctx, i32(first_row), i32(cnt), d.ctypes.data_as(C.c_void_p))),
                           ("asd_bank_put_from_frame", lambda: L.asd_bank_put_from_frame(hip.ctx, i32(2), i32(first_row), i32(cnt))),
                           ("asd_mpbank_put", lambda: L.asd_mpbank_put(hip.ctx, i32(first_row), i32(cnt), Xa.ctypes.data_as(C.c_void_p),
                                                                       na_.ctypes.data_as(C.c_void_p), mi.ctypes.data_as(C.c_void_p),
                                                                       ma.ctypes.data_as(C.c_void_p)))):
            rc = call()
            out.append((name, rc, hip.last_error()))
        return out
    try:
        hip.frame_set(0, kc, dc, BOUNDS)
        hip.frame_set(1, kl, dl, BOUNDS)
        hip.frame_set(2, *make_frame(1000, 84), BOUNDS)   # 1000 keypoints: the source of the refused asd_bank_put_from_frame calls
        exp = hip.track_motion_model(0, 1, n, has, Xw, mp_desc, T, K, 15.0, pose0, True)
        still_works()
        for first_row, cnt in ((-1, 10), (0, -1), (-1, -1)):
            for name, rc, _msg in puts(first_row, cnt):
                assert rc == -1, (name, first_row, cnt, rc)
            still_works()
        for first_row, cnt in ((2**31 - 500, 1000), (MAX, 1), (MAX - 100, 300)):
            for name, rc, msg in puts(first_row, cnt):
                assert rc == -5 and "ASD_BANK_MAX_ROWS" in msg and name in msg, (name, first_row, cnt, rc, msg)
            still_works()
        # reads: the last row of the first capacity is there, the row at the capacity is not
        _put_desc(hip, mir, FIRST_CAP - 1, _desc(1, 82))
        _put_attr(hip, mir, FIRST_CAP - 1, _attrs(1, 83))
        mir.check(hip)
        for kw in (dict(attr=False), dict(desc=False)):
            for first_row, cnt in ((FIRST_CAP, 1), (FIRST_CAP - 1, 2), (-1, 1), (0, -1), (2**31 - 1, 2)):
                with pytest.raises(pkg.capi.AsdError) as e:
                    hip.bank_get(first_row, cnt, **kw)
                assert e.value.code == -1
        still_works()
        hip.prep_async(1)
        with pytest.raises(pkg.capi.AsdError) as e:
            hip.bank_get(0, 1)
        assert e.value.code == -1 and "bracket" in str(e.value)
        hip.prep_async(0)
        still_works()
        assert hip.track_motion_model(0, 1, n, has, Xw, mp_desc, T, K, 15.0, pose0, True, split=True) is None
        with pytest.raises(pkg.capi.AsdError) as e:
            hip.bank_get(200, 1)
        assert e.value.code == -1
        for name, rc, msg in puts(MAX, 1):
            assert rc == -5, (name, rc, msg)
        got = hip.track_finish()
        for x, y in zip(got, exp):
            np.testing.assert_array_equal(x, y)
        still_works()
    finally:
        hip.close()
