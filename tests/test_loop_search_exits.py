"""Every way out of the four searches that decide a loop closure or a relocalisation -- asd_match_project_keyframe,
asd_match_project_sim3, asd_fuse_search_sim3, asd_match_sim3 -- reached by a crafted input (tests/loop_search_cases.py) and
compared with tests/loop_search_ref.py, a plain restatement written from the reference's source text.  On the CPU the
restatement is compared with the oracle, on the GPU the HIP entry points with both.

Coverage the reference reports over the crafted sets (exit sets at scale 1, the orientation and ORBdist sets, the crowded sets;
test_coverage asserts >= 3 of each; counts of this revision):

  relocalisation   invalid 94, outside_u 152, outside_v 4, too_near 3, too_far 3, window_empty 9, all_dropped 771,
                   above_orb_dist 262, matched 678, removed_by_orientation 43; level_below 9231, level_above 1928,
                   occupied_on_entry 467, claimed_earlier 3628, tie_first_wins 6, level_clamped_high 68,
                   behind_camera_went_on 75, bin_wrapped 11, rot_negative 276
  Scw search       invalid 95, behind 75, outside_image 165, too_near 3, too_far 3, viewing_angle 14, window_empty 3,
                   all_dropped 868, above_th_low 90, matched 571; matched_on_entry 762, claimed_earlier 3409, level_below 799,
                   level_above 221, tie_first_wins 6, level_clamped_high 42
  Fuse(Scw)        invalid 65, behind 51, outside_image 113, too_near 3, too_far 3, viewing_angle 14, window_empty 3,
                   all_dropped 6, above_th_low 3, matched 1016; level_below 4361, level_above 1392, tie_first_wins 6,
                   level_clamped_high 36, keypoint_chosen_twice 407
  SearchBySim3     1 -> 2: no_point 74, behind 3, outside_image 18, too_near 3, too_far 3, window_empty 3, all_dropped 6,
                   above_th_high 7, one_way 758; level_below 2008, level_above 846, tie_first_wins 6, level_clamped_high 3
                   2 -> 1: no_point 66, behind 3, outside_image 18, too_near 3, too_far 3, window_empty 3, all_dropped 6,
                   above_th_high 3, one_way 766; level_below 1979, level_above 849, tie_first_wins 6, level_clamped_high 3
                   pairs: only_12 112, only_21 120, mutual 646
  (level_clamped_low, and all_dropped through the level gate in the relocalisation search: unreachable, see loop_search_ref.py;
  a window wholly outside the grid: unreachable through these entry points, see loop_search_cases.py; bin 30 needs an angle
  outside [0, 360): the rows use 950 degrees.)
  Shapes, per function: lists of 1, 100, 128, 129 and 1253 to 1401 candidates, windows of 10 to 34 grid columns, a column range
  of 100 items inside a 13-column window, every border clipped, calls of 1, 7, 8, 9 and 16 to 19 queries; 6941 to 10988
  candidates in the call behind a call of 1 (the tail copy), 400000 in a fresh context (grow and run again).

Undecidable share (margin <= 1 in loop_search_ref's terms, the rows on a bound counted as decided), as test_undecidable_share
prints it: 0 % in every set.  The crafted rows keep their distance by construction; the map points of the crowded sets and the
field queries of the shape sets are the ones the reference alone finds at a margin above 2 (1796 of 1800, 1794 of 1800, 1190 of
1200 map points in reloc_crowded, scw_crowded_euroc, fuse_crowded; sim3_crowded clears the flag of the others).  The rows on a
bound are exact for Scw = 1 * Tcw alone, so the sets at scales 0.37 and 2.5 go without them.

Sensitivity (decided outputs changed per mutant of the reference over the crafted sets, in the order reloc / scw / fuse / sim3
where a mutant applies to several): <= made < 9 / 9 / 9 / 9; starting bestDist exchanged 6 / 36* / 18* / 12*; IsInImage closed
above 6 / 6 / 12 (scw, fuse, sim3); closed bounds made half-open 6; z < 0 gate added 3; level gate widened to pred + 1
27 / 18 / 15 (scw, fuse, sim3); narrowed to pred in the relocalisation search 3; viewing angle dropped 9 / 9; 0.8 and 1.2
dropped 51 / 39 / 39 / 69; claims dropped 9 / 27; last wins 12 / 36 / 18 / 18; Ow with the scale left in 12 / 6; sR12 and sR21
exchanged 71; mutual check dropped 54; tenth rule dropped 9; histogram holding the map point 22.
(*) A starting bestDist of 100 for 256 or the reverse changes no output of asd_match_project_sim3, asd_fuse_search_sim3 or
asd_match_sim3 whatever the input: their thresholds are 0.5 and 1.5, so a candidate between 100 and 256 is refused either way.
These three counts are of the bestDist the reference's loop ends with; the relocalisation search, whose ORBdist is an argument,
shows the difference in its output at ORBdist = 200 with a keypoint at 121.
"""
import functools

import numpy as np
import pytest

from tests import loop_search_cases as cases
from tests import loop_search_ref as ref

F32 = np.float32
EXITS = dict(reloc=(ref.RELOC_EXITS, ref.RELOC_COUNTERS), scw=(ref.SCW_EXITS, ref.SCW_COUNTERS), fuse=(ref.FUSE_SCW_EXITS, ref.FUSE_SCW_COUNTERS),
             sim3=(ref.SIM3_EXITS, ref.SIM3_COUNTERS))
PREFIXES = (1, 7, 8, 9)                                   # a workgroup of k_window_search holds 8 queries, one wave each


def _sets():
    """name -> the function that builds the set"""
    out = {}

    def add(thunk, name):
        out[name] = thunk
    add(cases.reloc_exits, "reloc_exits")
    add(lambda: cases.reloc_orb(0.25), "reloc_orb_0.25")
    add(lambda: cases.reloc_orb(200.0), "reloc_orb_200")
    for c in cases.ORI_CASES:
        add(functools.partial(cases.reloc_ori, c), "reloc_" + c)
    add(lambda: cases.crowded("reloc"), "reloc_crowded")
    for scale in cases.SCW_SCALES:
        add(lambda scale=scale: cases.with_scale(cases.scw_exits(), scale), "scw_exits@%g" % scale)
        add(lambda scale=scale: cases.with_scale(cases.fuse_exits(), scale), "fuse_exits@%g" % scale)
    add(lambda: cases.crowded("scw", True), "scw_crowded_euroc")
    add(lambda: cases.crowded("fuse"), "fuse_crowded")
    add(cases.sim3_exits, "sim3_exits")
    add(cases.sim3_bounds, "sim3_bounds")
    add(cases.sim3_crowded, "sim3_crowded")
    for kind in ("reloc", "scw", "fuse", "sim3"):
        add(functools.partial(cases.shapes, kind), kind + "_shapes_all")
        for n in PREFIXES:
            add(functools.partial(cases.shapes, kind, n), "%s_shapes_%d" % (kind, n))
    return out


SETS = _sets()
EXIT_SETS = [n for n in SETS if "shapes" not in n]        # what the census runs over
MUTANT_SETS = [n for n in EXIT_SETS if "crowded" not in n]
COUPLED = ("reloc", "scw")


@functools.lru_cache(None)
def get(name):
    """-> (the set, the reference's result)"""
    s = SETS[name]()
    return s, cases.run_ref(s)


def _names(s, r):
    return np.array(EXITS[s["fn"]][0])[r["exit"]]


# ------------------------------------------------------------------ CPU
def test_coverage():
    """a condition, not a measurement: over the crafted sets the reference reports every reachable exit and counter at least 3
    times, every crafted row leaves where it was built to, and the shape sets have the sizes at which k_window_search changes path"""
    got = {}
    for name in EXIT_SETS:
        s, r = get(name)
        if name.endswith(("@0.37", "@2.5")):
            continue                                       # the same rows as @1
        fn = s["fn"]
        parts = [("", r)] if fn != "sim3" else [("12.", r["d12"]), ("21.", r["d21"])]
        for tag, d in parts:
            for k, v in ref.census(d, *EXITS[fn]).items():
                got["%s.%s%s" % (fn, tag, k)] = got.get("%s.%s%s" % (fn, tag, k), 0) + v
        if fn == "sim3":
            for i, p in enumerate(ref.SIM3_PAIRS):
                got["sim3." + p] = got.get("sim3." + p, 0) + int(r["only_21"].sum() if p == "only_21" else (r["pair"] == i).sum())
    print(got)
    for k, v in got.items():
        assert v >= 3, (k, v)
    assert {k.split(".", 1)[1] for k in got if k.startswith("reloc.")} == set(ref.RELOC_EXITS + ref.RELOC_COUNTERS)
    # every crafted row leaves through its exit; the chains take best, second and third in index order and the fourth finds none
    for name in EXIT_SETS:
        s, r = get(name)
        for tag, d in ([("", r)] if s["fn"] != "sim3" else [("1", r["d12"]), ("2", r["d21"])]):
            crafted, names = s["crafted" + tag], _names(s, d)
            plain = np.array([c != "" and not c.startswith("chain") for c in crafted])
            np.testing.assert_array_equal(names[plain], crafted[plain], err_msg=name)
            chain = [np.nonzero(crafted == "chain%d" % n)[0] for n in range(4)]
            for a, b, c, e in zip(*chain):
                assert a < b < c < e and len({d["match"][a], d["match"][b], d["match"][c]}) == 3 and d["match"][e] == -1, name
                kx = s["kps"]["x"][[d["match"][a], d["match"][b], d["match"][c]]]
                assert kx[0] > kx[2] > kx[1], name         # the keypoints of a chain site: +0.7, -1.2, +0.5 px
            if s["fn"] in COUPLED and "exits" in name:
                assert len(chain[0]) >= 3
    # relocalisation: points behind the camera match, points on the camera plane do not; the bound rows: max is inside there only
    s, r = get("reloc_exits")
    assert ((r["behind_camera_went_on"] == 1) & (r["match"] >= 0)).sum() >= 3
    on_max = s["exact"] & (_names(s, r) == "matched")
    assert on_max.sum() >= 3 + 3 + 3 + 3                   # min_x, min_y, max_x, max_y
    for name in ("scw_exits@1", "fuse_exits@1"):
        s, r = get(name)
        assert (s["exact"] & (_names(s, r) == "matched")).sum() == 6 and (s["exact"] & (_names(s, r) == "outside_image")).sum() == 6 + 4
    # ties: the first in area order has the larger index
    for name in ("reloc_exits", "scw_exits@1", "fuse_exits@1"):
        s, r = get(name)
        won = [i for i in np.nonzero(r["tie_first_wins"] == 1)[0] if r["match"][i] >= 0 and
               (s["desc"][r["match"][i] - 1] == s["desc"][r["match"][i]]).all()]
        assert len(won) >= 3, name
    # shapes
    for kind in EXITS:
        s, r = get(kind + "_shapes_all")
        d = r["d12"] if kind == "sim3" else r
        n, cols, col = d["n_list"], d["n_cols"], d["max_column"]
        assert (n == 128).any() and (n == 129).any() and (n > 256).any(), kind
        assert ((n == 128) & (cols <= 16) & (col <= 64)).any() and ((n == 129) & (cols <= 16) & (col <= 64)).any(), kind
        assert (cols > 16).any() and ((cols <= 16) & (col > 64)).any(), kind
        assert len(s["kps2" if kind == "sim3" else "kps"]) <= 2000
        b, found = s["bounds2" if kind == "sim3" else "bounds"], n > 0
        for clipped in (d["u"] - d["radius"] < b[0], d["u"] + d["radius"] > b[1], d["v"] - d["radius"] < b[2], d["v"] + d["radius"] > b[3]):
            assert (clipped & found).any(), kind            # a window over each border that still holds a keypoint
    for n in PREFIXES:
        for kind in EXITS:
            s, _ = get("%s_shapes_%d" % (kind, n))
            assert len(s["has1"] if kind == "sim3" else s["valid"]) == n


def test_undecidable_share():
    """a condition, not a measurement: no undecidable row in a claim-coupled set or among the rows crafted for an exit (the rows
    on a bound are decided by construction), at most 2 % in the crowded sets of Fuse and SearchBySim3"""
    shares = {}
    for name in SETS:
        s, r = get(name)
        dec = cases.decided(s, r)
        shares[name] = float((~dec).mean())
        crowded_free = s["fn"] not in COUPLED and "crowded" in name
        assert shares[name] <= (0.02 if crowded_free else 0.0), (name, shares[name])
    print(shares)


@pytest.mark.parametrize("name", list(SETS) + ["fuse_grow"])
def test_oracle_matches_reference(oracle, name):
    s, r = (cases.fuse_grow(), cases.run_ref(cases.fuse_grow())) if name == "fuse_grow" else get(name)
    cases.check(s, r, cases.run_lib(oracle, s))


MUTANTS = [  # (name, functions, keyword arguments of the reference)
    ("accept_strict", ("reloc", "scw", "fuse", "sim3"), dict(accept_strict=True)),
    ("start_100", ("reloc", "scw"), dict(start=100)),
    ("start_256", ("fuse", "sim3"), dict(start=256)),
    ("is_in_image_closed_above", ("scw", "fuse", "sim3"), dict(closed_upper=True)),
    ("reloc_bounds_half_open", ("reloc",), dict(half_open=True)),
    ("reloc_depth_gate", ("reloc",), dict(depth_gate=True)),
    ("level_gate_to_pred_plus_1", ("scw", "fuse", "sim3"), dict(level_wide=True)),
    ("reloc_level_gate_to_pred", ("reloc",), dict(level_narrow=True)),
    ("no_viewing_angle", ("scw", "fuse"), dict(view_gate=False)),
    ("no_08_12_factors", ("reloc", "scw", "fuse", "sim3"), dict(drop_factors=True)),
    ("no_claims", ("reloc", "scw"), dict(no_claims=True)),
    ("last_wins", ("reloc", "scw", "fuse", "sim3"), dict(last_wins=True)),
    ("ow_with_scale", ("scw", "fuse"), dict(ow_scaled=True)),
    ("sr12_sr21_exchanged", ("sim3",), dict(swap_sr=True)),
    ("no_mutual_check", ("sim3",), dict(no_mutual=True)),
    ("no_tenth_rule", ("reloc",), dict(drop_tenth=True)),
    ("histogram_holds_map_point", ("reloc",), dict(hist_holds_mp=True)),
]
INTERNAL = {("start_100", "scw"), ("start_256", "fuse"), ("start_256", "sim3")}


def _changed(s, r, m):
    """decided outputs that differ between the reference r and its mutant m"""
    if s["fn"] in COUPLED:
        return int((cases.outputs(s, r)[0] != cases.outputs(s, m)[0]).sum())
    both = cases.decided(s, r) & cases.decided(s, m)
    return int((cases.outputs(s, r)[0] != cases.outputs(s, m)[0])[both].sum())


def _best_dist_changed(s, r, m):
    if s["fn"] == "sim3":
        return sum(_best_dist_changed(dict(fn="x"), r[d], m[d]) for d in ("d12", "d21"))
    a, b = r["best_dist"], m["best_dist"]
    return int(((a != b) & ~(np.isnan(a) & np.isnan(b)))[r["decidable"] & m["decidable"]].sum())


def test_reference_is_sensitive():
    """each mutant of the REFERENCE must change at least one decided output on the crafted sets, or the sets could not tell a
    kernel with that bug from a right one.  Three starting-value mutants change no output of the entry point whatever the input
    (no threshold reaches 100: what the starting value decides is only the bestDist the loop ends with); they are counted on the
    reference's bestDist, and asd_fuse_search_sim3's best_dist == 100 on unmatched points is asserted on the GPU."""
    changed = {}
    for mutant, fns, kw in MUTANTS:
        for fn in fns:
            n = 0
            for name in MUTANT_SETS:
                s, r = get(name)
                if s["fn"] == fn:
                    m = cases.run_ref(s, **kw)
                    n += _best_dist_changed(s, r, m) if (mutant, fn) in INTERNAL else _changed(s, r, m)
            changed["%s.%s" % (mutant, fn)] = n
    print(changed)
    for k, v in changed.items():
        assert v >= 1, (k, v)


# ------------------------------------------------------------------ GPU
def _check_hip(oracle, s, r, got):
    """HIP == reference on the decided elements, == oracle on every element; the counts; the entry point's own rules"""
    cases.check(s, r, got)
    exp = cases.run_lib(oracle, s)
    np.testing.assert_array_equal(got[0], exp[0], err_msg=s["name"])
    if s["fn"] == "fuse":
        np.testing.assert_array_equal(got[1].view(np.int32), exp[1].view(np.int32), err_msg=s["name"])
        assert (got[1][got[0] < 0] == 100).all() and (got[1][got[0] >= 0] <= ref.TH_LOW).all()
    else:
        assert got[1] == exp[1]
    if s["fn"] == "reloc" or s["fn"] == "sim3":
        assert got[1] == (got[0] >= 0).sum()
    if s["fn"] == "scw":
        keep = s["matched_kp"] != -1
        np.testing.assert_array_equal(got[0][keep], s["matched_kp"][keep])
        assert got[1] == (got[0][~keep] >= 0).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SETS))
def test_hip_equals_reference_and_oracle(hip, oracle, name):
    s, r = get(name)
    _check_hip(oracle, s, r, cases.run_lib(hip, s))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(EXITS))
def test_hip_tail_copy(hip, oracle, kind):
    """a call that writes more than 4096 candidates directly after a call of the same window_search kind that wrote fewer than
    100: the read-back that travels with the counts is sized by the previous call, the rest is copied afterwards"""
    small, rs = get(kind + "_shapes_1")
    big = cases.shapes(kind, None, True)
    rb = cases.run_ref(big)
    # SearchBySim3 searches twice (both kind 3): the small call's second search precedes the large call's first
    assert np.max(cases.n_candidates(small, rs)) < 100 and np.max(cases.n_candidates(big, rb)) > 4096
    _check_hip(oracle, small, rs, cases.run_lib(hip, small))
    _check_hip(oracle, big, rb, cases.run_lib(hip, big))


@pytest.mark.gpu
def test_hip_grow_and_run_again(pkg, oracle):
    """a fresh context has room for 2^18 candidates; the first call writes 400000: the buffers grow and the search runs again"""
    s = cases.fuse_grow()
    r = cases.run_ref(s)
    assert cases.n_candidates(s, r) > 1 << 18
    ctx = pkg.AsdHip(n_features=2000, max_width=1241, max_height=376, max_patches=4096)
    try:
        got = cases.run_lib(ctx, s)
        again = cases.run_lib(ctx, s)
    finally:
        ctx.close()
    _check_hip(oracle, s, r, got)
    np.testing.assert_array_equal(again[0], got[0])
    np.testing.assert_array_equal(again[1].view(np.int32), got[1].view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["reloc_crowded", "scw_crowded_euroc", "fuse_crowded", "sim3_crowded"])
def test_hip_repeats_bit_for_bit(hip, name):
    s, _ = get(name)
    first = cases.run_lib(hip, s)
    for _ in range(4):
        again = cases.run_lib(hip, s)
        np.testing.assert_array_equal(again[0], first[0])
        np.testing.assert_array_equal(np.asarray(again[1]).view(np.int32) if s["fn"] == "fuse" else again[1],
                                      np.asarray(first[1]).view(np.int32) if s["fn"] == "fuse" else first[1])
