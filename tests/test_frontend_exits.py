"""Extractor front half (csrc/frontend.hip E1-E5 + E7, csrc/quadtree.cpp), exit by exit: the plain reference
tests/frontend_ref.py against the C++ oracle (CPU) and against the HIP library (GPU) on the crafted inputs of
tests/frontend_cases.py.  Every comparison is of bytes, integers or single f32 operations: no tolerance anywhere but the
descriptor tolerance tests/test_frontend.py already carries (atol 2e-5)."""
import ctypes as C
import operator

import numpy as np
import pytest

from tests import frontend_cases as FC
from tests import frontend_ref as R

FIELDS = ("x", "y", "size", "angle", "response", "octave")
DESC_ATOL = 2e-5          # tests/test_frontend.py
DESC_SAMPLE = 40          # the oracle's naive convolution takes ~30 ms per patch


# ------------------------------------------------------------------ shared, computed once
@pytest.fixture(scope="module")
def cases(synth):
    return {c["name"]: c for c in FC.all_cases(synth)}


@pytest.fixture(scope="module")
def ref_results(cases):
    return {name: R.extract(c["img"], c["n_features"], 1.2, c["n_levels"]) for name, c in cases.items()}


CASE_NAMES = ([f"cells_x_{w}" for w in (723, 753, 783, 813, 843)] + ["cells_y_813", "cells_y_903", "no_cells_200x164", "nms_ties"]
              + [f"quadtree_{w}x{h}_s{s}_N{N}" for w, h, _, s, N in FC.QUADTREE_RANDOM] + ["quadtree_roots", "quadtree_tall_110x260"]
              + ["angles_dots", "angles_texture", "scene_333x251", "scene_crop_640x240"])


def test_case_names_complete(cases):
    assert sorted(CASE_NAMES) == sorted(cases)


def raw_arrays(keys):
    a = np.array(keys, np.float32).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2]


def assert_same_extraction(got, ref, what, n_levels, blurred_of=None):
    """got / ref: objects with level_size, level_image, raw_corners (the oracle's extractor, AsdHip) or a frontend_ref result"""
    def view(o):
        if isinstance(o, dict):
            return (lambda l: o["levels"][l].shape[::-1], lambda l: o["levels"][l], lambda l: raw_arrays(o["raw"][l]),
                    lambda l: o["blurred"][l])
        return o.level_size, o.level_image, o.raw_corners, lambda l: o.level_image(l, blurred=True)
    gs, gi, gr, gb = view(got)
    rs, ri, rr, rb = view(ref)
    for l in range(n_levels):
        assert tuple(gs(l)) == tuple(rs(l)), f"{what}: size of level {l}"
        np.testing.assert_array_equal(gi(l), ri(l), err_msg=f"{what}: level {l}")
        for a, b, f in zip(gr(l), rr(l), ("x", "y", "response")):
            assert len(a) == len(b), f"{what}: raw corner count, level {l}: {len(a)} vs {len(b)}"
            np.testing.assert_array_equal(a, b, err_msg=f"{what}: raw corner {f}, level {l}")
        if blurred_of is not None and (blurred_of == l).any():
            np.testing.assert_array_equal(gb(l), rb(l), err_msg=f"{what}: blurred level {l}")


def assert_same_keypoints(got, ref, what):
    assert len(got) == len(ref), f"{what}: {len(got)} vs {len(ref)} keypoints"
    for f in FIELDS:
        np.testing.assert_array_equal(got[f].view(np.uint32 if f != "octave" else np.int32),
                                      ref[f].view(np.uint32 if f != "octave" else np.int32), err_msg=f"{what}: {f}")


# ------------------------------------------------------------------ CPU: reference == oracle
@pytest.mark.parametrize("name", CASE_NAMES)
def test_reference_equals_oracle(oracle, cases, ref_results, name):
    c, r = cases[name], ref_results[name]
    ex = oracle.extractor(c["n_features"], 1.2, c["n_levels"])
    okps, opatches = ex.extract(c["img"])
    assert_same_extraction(r, ex, name, c["n_levels"], blurred_of=okps["octave"])
    assert_same_keypoints(r["kps"], okps, name)
    np.testing.assert_array_equal(r["patches"], opatches)
    assert sorted(r["blurred"]) == sorted(set(okps["octave"].tolist()))


@pytest.mark.parametrize("cfg", [(2000, 1.2, 8), (500, 1.2, 8), (4000, 1.2, 8), (1000, 1.2, 8), (300, 1.2, 3), (1500, 1.5, 5)])
def test_constructor_tables(oracle, cfg):
    t, o = R.tables(*cfg), oracle.extractor(*cfg).tables()
    for k in ("scale", "inv_scale", "sigma2", "inv_sigma2"):
        np.testing.assert_array_equal(t[k].view(np.uint32), o[k].view(np.uint32), err_msg=k)
    np.testing.assert_array_equal(t["features_per_level"], o["features_per_level"])
    np.testing.assert_array_equal(t["umax"], o["umax"])


def test_blur_kernel():
    assert R.gauss_kernel7() == [18, 34, 49, 55, 49, 34, 18]


# counters that no valid input can reach; the argument stands beside the name in frontend_ref.COUNTERS
UNREACHABLE = {"root_clamp"}


def test_every_branch_is_reached(ref_results):
    total = R.new_counters()
    for r in ref_results.values():
        for k, v in r["counters"].items():
            total[k] += v
    crafted = R.new_counters()
    for name, r in ref_results.items():
        if not name.startswith("scene_"):
            for k, v in r["counters"].items():
                crafted[k] += v
    assert [k for k in R.COUNTERS if not total[k] and k not in UNREACHABLE] == []
    assert [k for k in R.COUNTERS if not crafted[k] and k not in UNREACHABLE] == [], "reached by the scenes only"
    assert all(total[k] == 0 for k in UNREACHABLE)


def test_cell_geometry_is_the_designed_one(ref_results):
    """each crafted size takes the path it was chosen for"""
    want = {"cells_x_723": "interior_w3", "cells_x_753": "interior_w2", "cells_x_783": "interior_w1", "cells_x_813": "cell_skipped_x",
            "cells_x_843": "cell_skipped_x", "cells_y_813": "window_under_7", "cells_y_903": "row_skipped_y",
            "no_cells_200x164": "level_no_cells", "quadtree_tall_110x260": "nini_lt_1"}
    for name, key in want.items():
        assert ref_results[name]["counters"][key] > 0, (name, key)
    r = ref_results["no_cells_200x164"]
    assert [l.shape[::-1] for l in r["levels"][5:]] == [(80, 66), (67, 55), (56, 46)]
    assert len(r["raw"][5]) > 0 and r["raw"][6] == [] and r["raw"][7] == [] and r["kps"]["octave"].max() == 5
    r = ref_results["quadtree_tall_110x260"]
    assert len(r["raw"][0]) == 50 and len(r["kps"]) == 0


def test_cells_edge_dots(cases, ref_results):
    """every dot of the edge pattern is reported exactly where it was put, except the ones one pixel outside the valid range"""
    for name in CASE_NAMES[:7]:
        img = cases[name]["img"]
        h, w = img.shape
        ys, xs = np.nonzero(img != FC.BG)
        inside = {(int(x), int(y)) for x, y in zip(xs, ys) if 19 <= x <= w - 20 and 19 <= y <= h - 20}
        raw = {(int(x) + 16, int(y) + 16) for x, y, _ in ref_results[name]["raw"][0]}
        bars = {p for p in inside if (p[0] + 1, p[1]) in inside or (p[0] - 1, p[1]) in inside or (p[0], p[1] + 1) in inside or (p[0], p[1] - 1) in inside}
        assert raw - bars == inside - bars, name          # single dots: all of them, nothing else
        assert raw <= inside, name
        assert len(inside) < len(xs), name                 # the pattern does hold dots outside the valid range
        assert {p for p in raw if p in bars}, name         # the bars across a cell boundary survive


NMS_PRESENT = [(82, 28, 49), (83, 28, 49), (60, 54, 49), (60, 55, 49), (135, 40, 11), (155, 30, 49), (130, 70, 20), (160, 70, 19),
               (190, 70, 7), (19, 70, 49), (204, 30, 49), (100, 19, 49), (130, 120, 49), (95, 70, 20), (40, 105, 254)]
NMS_ABSENT = [(30, 30), (31, 30), (125, 30), (126, 30), (165, 40), (190, 105), (18, 80), (205, 40), (110, 18), (140, 121), (105, 80)]


def test_nms_ties_by_design(ref_results):
    """what tests/frontend_cases.nms_ties says of each dot, independent of any implementation"""
    raw = {(int(x) + 16, int(y) + 16): int(s) for x, y, s in ref_results["nms_ties"]["raw"][0]}
    for x, y, s in NMS_PRESENT:
        assert raw.get((x, y)) == s, (x, y, s, raw.get((x, y)))
    for p in NMS_ABSENT:
        assert p not in raw, p
    dark_block_corner = {p for p in raw if p not in {(x, y) for x, y, _ in NMS_PRESENT}}
    assert all(abs(x - 82) <= 2 and abs(y - 88) <= 2 for x, y in dark_block_corner), dark_block_corner


def test_angle_dots_by_design(ref_results):
    """angles_dots: the moments are (5 u, 5 v) summed over the extras, so the angle of each dot is fastAtan2 of small integers"""
    r = ref_results["angles_dots"]
    got = {(int(k["x"]), int(k["y"])): k["angle"] for k in r["kps"]}
    assert len(got) == len(FC.ANGLE_EXTRAS)
    for k, extras in enumerate(FC.ANGLE_EXTRAS):
        m10, m01 = 5 * sum(u for u, _ in extras), 5 * sum(v for _, v in extras)
        a = got[(30 + 40 * (k % 6), 30 + 40 * (k // 6))]
        assert a == R.fast_atan2(m01, m10)
        true = np.degrees(np.arctan2(m01, m10)) % 360 if extras else 0.0
        assert min(abs(a - true), 360 - abs(a - true)) < 0.3


# ------------------------------------------------------------------ CPU: the inputs discriminate (mutants of the reference)
def _nms_across_cells(level_img, x0, y0, x1, y1, th):
    """suppression also by neighbours that belong to the next cell: FAST on the window grown by one pixel (inside the level's
    FAST area), reported for the window's own positions only"""
    h, w = level_img.shape
    gx0, gy0, gx1, gy1 = max(x0 - 1, 16), max(y0 - 1, 16), min(x1 + 1, w - 16), min(y1 + 1, h - 16)
    keys, n_pass = R.fast_window(level_img[gy0:gy1, gx0:gx1], th)
    own = [(x + gx0 - x0, y + gy0 - y0, s) for x, y, s in keys]
    return [(x, y, s) for x, y, s in own if 3 <= x < x1 - x0 - 3 and 3 <= y < y1 - y0 - 3], n_pass


def _reflect(p, n):
    while p < 0 or p >= n:
        p = -p - 1 if p < 0 else 2 * n - 1 - p
    return p


def _fused_last_step(a, b, c, step):
    if step == 2:
        return np.float32(np.float64(a) * np.float64(b) + np.float64(c))     # the f32 product is exact in f64: one rounding less
    return np.float32(np.float32(a * b) + c)


CELLS = CASE_NAMES[:7]
QUAD = [n for n in CASE_NAMES if n.startswith("quadtree_") or n.startswith("scene_")]
# (name, attribute of frontend_ref, mutated value, cases to run, must the results change?)
MUTANTS = [
    ("nms_across_cell_boundaries", "_detect_window", _nms_across_cells, ["nms_ties"] + CELLS, True),
    ("gt_for_ge_at_ini_th", "_is_corner", lambda s, th: s > th + (1 if th == 20 else 0), ["nms_ties"], True),
    ("gt_for_ge_at_min_th", "_is_corner", lambda s, th: s > th + (1 if th == 7 else 0), ["nms_ties"], True),
    ("retry_decided_by_pixels_passing", "_retry_needed", lambda keys, n_pass: n_pass == 0, ["nms_ties"], True),
    ("non_strict_nms", "_nms_greater", np.greater_equal, ["nms_ties"], True),
    # the two skip constants differ in the reference (6 in x, 3 in y).  Either value in either place gives the same corners, because a
    # window that one constant skips and the other does not is narrower than 7 and cv::FAST finds nothing in it: the HIP cell table
    # (which drops both kinds) relies on exactly this
    ("y_skip_constant_6", "SKIP_Y", 6, CELLS + ["nms_ties", "scene_333x251"], False),
    ("x_skip_constant_3", "SKIP_X", 3, CELLS + ["nms_ties", "scene_333x251"], False),
    ("sort_tie_by_reverse_creation_order", "_sort_key", lambda e: (e[0], -e[1].seq), QUAD, True),
    ("ge_in_response_pick", "_response_greater", operator.ge, QUAD, True),
    ("children_pushed_at_the_back", "_push_child", lambda nodes, c: nodes.append(c), QUAD, True),
    ("reflect_for_reflect_101", "_border_index", _reflect, ["angles_texture", "nms_ties"], True),
    ("ax_gt_ay", "_first_of", operator.gt, ["angles_dots"], True),
    ("one_fused_multiply_add", "_mul_add", _fused_last_step, ["angles_texture", "scene_333x251"], True),
    # multiplying by scale[0] == 1.0f changes nothing, so "the scale is applied at level 0 too" cannot be seen; the mutant that can
    # be is the inverted test (level 0 scaled, i.e. untouched, and the upper levels left in level coordinates)
    ("scale_applied_at_level_0_too", "FIRST_SCALED_LEVEL_TEST", lambda level, zero: True, ["scene_333x251"], False),
    ("scale_applied_at_level_0_only", "FIRST_SCALED_LEVEL_TEST", operator.eq, ["scene_333x251", "no_cells_200x164"], True),
]


def _same(a, b):
    if len(a["kps"]) != len(b["kps"]) or a["kps"].tobytes() != b["kps"].tobytes() or a["patches"].tobytes() != b["patches"].tobytes():
        return False
    if [[tuple(map(float, k)) for k in lv] for lv in a["raw"]] != [[tuple(map(float, k)) for k in lv] for lv in b["raw"]]:
        return False
    if len(a["levels"]) != len(b["levels"]) or not all(np.array_equal(x, y) for x, y in zip(a["levels"], b["levels"])):
        return False
    return sorted(a["blurred"]) == sorted(b["blurred"]) and all(np.array_equal(a["blurred"][l], b["blurred"][l]) for l in a["blurred"])


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutants_of_the_reference(monkeypatch, cases, ref_results, mutant):
    name, attr, value, on, must_change = mutant
    monkeypatch.setattr(R, attr, value)
    changed = [n for n in on if not _same(R.extract(cases[n]["img"], cases[n]["n_features"], 1.2, cases[n]["n_levels"]), ref_results[n])]
    if must_change:
        assert changed, f"no crafted input notices the mutant {name}"
    else:
        assert not changed, f"{name} is meant to be equivalent, but changes {changed}"


def dump_quadtree_inputs(ref_results, path):
    """the raw corner lists of the quadtree cases as text (one case per block: `name minX maxX minY maxY N n`, then n lines x y response),
    for a stand-alone sanitizer build of csrc/quadtree.cpp.  No test calls it: the program that reads the file (a main() around
    asd_distribute_octtree, built with -fsanitize=address,undefined) is a one-off and not part of the tree.  From a Python prompt at
    the repository root, with `synth` the package's synth module:
        from tests import frontend_cases as FC, frontend_ref as R, test_frontend_exits as T
        T.dump_quadtree_inputs({c["name"]: R.extract(c["img"], c["n_features"], 1.2, c["n_levels"]) for c in FC.all_cases(synth)}, "quadtree_inputs.txt")"""
    with open(path, "w") as f:
        for name, r in ref_results.items():
            for l, keys in enumerate(r["raw"]):
                h, w = r["levels"][l].shape
                f.write(f"{name}:{l} 16 {w - 16} 16 {h - 16} {int(r['tables']['features_per_level'][l])} {len(keys)}\n")
                for x, y, s in keys:
                    f.write(f"{float(x)} {float(y)} {float(s)}\n")


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx1(pkg, synth):
    """one level: the crafted dot images"""
    ctx = pkg.AsdHip(n_features=2000, n_levels=1, max_width=843, max_height=903, max_patches=4096)
    ctx.load_weights(synth.asdnet_weights(0))
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ctx8(pkg, synth):
    ctx = pkg.AsdHip(n_features=2000, n_levels=8, max_width=640, max_height=251, max_patches=4096)
    ctx.load_weights(synth.asdnet_weights(0))
    yield ctx
    ctx.close()


def _check_case(ctx, oracle, synth, c, r):
    name = c["name"]
    kps, desc = ctx.extract(c["img"], n_features_override=c["n_features"])
    ex = oracle.extractor(c["n_features"], 1.2, c["n_levels"])
    okps, _ = ex.extract(c["img"])
    assert_same_extraction(ctx, r, f"{name}: HIP vs reference", c["n_levels"], blurred_of=r["kps"]["octave"])
    assert_same_extraction(ctx, ex, f"{name}: HIP vs oracle", c["n_levels"], blurred_of=okps["octave"])
    assert_same_keypoints(kps, r["kps"], f"{name}: HIP vs reference")
    assert_same_keypoints(kps, okps, f"{name}: HIP vs oracle")
    np.testing.assert_array_equal(ctx.patches(), r["patches"], err_msg=f"{name}: patches")
    assert desc.shape == (len(kps), 128)
    if len(kps):
        sub = np.unique(np.linspace(0, len(kps) - 1, min(len(kps), DESC_SAMPLE)).astype(int))
        odesc = oracle.asdnet_forward(synth.asdnet_weights(0), r["patches"][sub])
        np.testing.assert_allclose(desc[sub], odesc, atol=DESC_ATOL, rtol=0)
    return kps, desc


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_hip_equals_reference_and_oracle(ctx1, ctx8, oracle, synth, cases, ref_results, name):
    c = cases[name]
    _check_case(ctx1 if c["n_levels"] == 1 else ctx8, oracle, synth, c, ref_results[name])


@pytest.mark.gpu
def test_scale_tables_on_device(pkg, oracle):
    for cfg in [(2000, 1.2, 8), (500, 1.2, 8), (4000, 1.2, 8), (1000, 1.2, 8), (300, 1.2, 3), (1500, 1.5, 5)]:
        ctx = pkg.AsdHip(n_features=cfg[0], scale_factor=cfg[1], n_levels=cfg[2], max_width=320, max_height=240, max_patches=cfg[0])
        try:
            t, ref, o = ctx.scale_tables(), R.tables(*cfg), oracle.extractor(*cfg).tables()
            for k in ("scale", "inv_scale", "sigma2", "inv_sigma2"):
                np.testing.assert_array_equal(t[k].view(np.uint32), ref[k].view(np.uint32), err_msg=f"{cfg} {k}")
                np.testing.assert_array_equal(t[k].view(np.uint32), o[k].view(np.uint32), err_msg=f"{cfg} {k}")
            np.testing.assert_array_equal(t["features_per_level"], ref["features_per_level"])
            np.testing.assert_array_equal(t["features_per_level"], o["features_per_level"])
        finally:
            ctx.close()


@pytest.mark.gpu
def test_repeated_sizes_on_one_context(ctx1, oracle, synth, cases, ref_results):
    """configure_size rebuilds its tables when the size changes; what came before must not show"""
    for name in ("cells_x_783", "cells_x_813", "cells_x_783", "cells_y_903", "nms_ties", "cells_x_783"):
        _check_case(ctx1, oracle, synth, cases[name], ref_results[name])


@pytest.mark.gpu
def test_patches_read_back_refuses_under_outstanding_submission(ctx8, cases):
    c = cases["scene_333x251"]
    ref_k, ref_d = ctx8.extract(c["img"])
    ref_p = ctx8.patches()
    assert ref_p.shape == (len(ref_k), 32, 32)
    p = ctx8.device_alloc(c["img"].nbytes)
    try:
        ctx8.h2d(p, c["img"])
        ctx8.extract_submit(p, 333, 251, 333, device_resident=True)
        with pytest.raises(Exception, match="outstanding"):
            ctx8.patches()
        k, d = ctx8.extract_wait()
        np.testing.assert_array_equal(k, ref_k)
        np.testing.assert_array_equal(d, ref_d)
    finally:
        ctx8.device_free(p)
    # asd_describe takes the same device buffer: afterwards there is nothing of the extraction to read back
    ctx8.extract(c["img"])
    assert len(ctx8.patches()) == len(ref_k)
    ctx8.describe(ref_p[:8])
    assert ctx8.patches().shape == (0, 32, 32)
    ctx8.extract(c["img"])
    np.testing.assert_array_equal(ctx8.patches(), ref_p)


# ---- image hand-over
COPY_WIDTHS = (248, 249, 250, 247)       # = 0, 1, 2, 3 (mod 4)
COPY_STRIDE_EXTRA = (0, 1, 2, 3, 64)
COPY_H = 170


def _place(buf, img, stride, offset):
    """the image's rows at buf[base + y * stride], base = the largest address = offset (mod 4) that still fits: the image ends in the
    allocation's last four bytes, and exactly at its last byte when the sizes allow"""
    h, w = img.shape
    span = (h - 1) * stride + w
    base = len(buf) - span
    base -= (base - offset) % 4
    assert base >= 0 and base % 4 == offset
    for y in range(h):
        buf[base + y * stride: base + y * stride + w] = img[y]
    return base, base + span == len(buf)


@pytest.mark.gpu
def test_copy_every_entry_stride_and_alignment(ctx8, synth):
    """k_copy_image and the runtime's pitched copy: every entry point, widths = 0..3 (mod 4), strides width + {0, 1, 2, 3, 64}, source
    rows starting 0..3 bytes into a dword, the image ending at the allocation's last byte -- all equal to the contiguous pageable call.
    Level 0 is read back and compared byte for byte after the two synchronous entries.  A submission's pyramid lives in whichever of the
    read-ahead extractor's two front-half states took the job, and no read-back names that state, so for the two extract_submit entries
    equality of every keypoint and descriptor (8 levels, FAST over the whole of [16, w - 16) x [16, h - 16) of each) stands in for the
    level image; they hand the image over through the same frontend_image_to_device / k_copy_image as extract_device."""
    full = synth.scene_frame(8, w=250, h=COPY_H)
    cap = (3 + (COPY_H - 1) * (250 + 64) + 250 + 3) // 4 * 4     # whole dwords: the kernel's last aligned load stays inside
    d_buf = ctx8.device_alloc(cap)
    h_ptr = ctx8.host_alloc(cap)
    pinned = np.frombuffer((C.c_uint8 * cap).from_address(h_ptr.value), np.uint8)
    stage = np.empty(cap, np.uint8)
    exact_end = 0
    try:
        for w in COPY_WIDTHS:
            img = np.ascontiguousarray(full[:, :w])
            ref_k, ref_d = ctx8.extract(img)
            ref_l0 = ctx8.level_image(0)
            np.testing.assert_array_equal(ref_l0, img)
            assert len(ref_k) > 100
            for extra in COPY_STRIDE_EXTRA:
                stride = w + extra
                for offset in range(4):
                    what = f"width {w} stride {stride} offset {offset}"
                    stage[:] = 0xA5
                    base, at_end = _place(stage, img, stride, offset)
                    exact_end += at_end
                    # pageable host memory, strided view
                    view = np.lib.stride_tricks.as_strided(stage[base:], shape=(COPY_H, w), strides=(stride, 1), writeable=False)
                    k, d = ctx8.extract(view)
                    np.testing.assert_array_equal(ctx8.level_image(0), img, err_msg=f"pageable, {what}")
                    np.testing.assert_array_equal(k, ref_k, err_msg=f"pageable, {what}")
                    np.testing.assert_array_equal(d, ref_d, err_msg=f"pageable, {what}")
                    # device memory, synchronous
                    ctx8.h2d(d_buf, stage)
                    k, d = ctx8.extract_device(C.c_void_p(d_buf.value + base), w, COPY_H, stride)
                    np.testing.assert_array_equal(ctx8.level_image(0), img, err_msg=f"extract_device, {what}")
                    np.testing.assert_array_equal(k, ref_k, err_msg=f"extract_device, {what}")
                    np.testing.assert_array_equal(d, ref_d, err_msg=f"extract_device, {what}")
                    # device memory and pinned host memory through the read-ahead extractor
                    pinned[:] = stage
                    ctx8.extract_submit(C.c_void_p(d_buf.value + base), w, COPY_H, stride, device_resident=True)
                    ctx8.extract_submit(C.c_void_p(h_ptr.value + base), w, COPY_H, stride, device_resident=False)
                    for entry in ("submit device", "submit pinned"):
                        k, d = ctx8.extract_wait()
                        np.testing.assert_array_equal(k, ref_k, err_msg=f"{entry}, {what}")
                        np.testing.assert_array_equal(d, ref_d, err_msg=f"{entry}, {what}")
        assert exact_end >= 10      # a quarter of the placements end on the allocation's last byte
    finally:
        ctx8.device_free(d_buf)
        ctx8.lib.asd_host_free(ctx8.ctx, h_ptr)


# ---- error exits
def _still_works(ctx, oracle, synth, cases, ref_results, name):
    _check_case(ctx, oracle, synth, cases[name], ref_results[name])


@pytest.mark.gpu
def test_error_exits_by_message(pkg, ctx1, ctx8, oracle, synth, cases, ref_results):
    small = synth.scene_frame(1, w=199, h=163)
    _still_works(ctx8, oracle, synth, cases, ref_results, "no_cells_200x164")
    with pytest.raises(Exception, match="too small for level 7"):
        ctx8.extract(small)
    # the refused size had already overwritten the level geometry: the size extracted before it must be configured afresh
    _still_works(ctx8, oracle, synth, cases, ref_results, "no_cells_200x164")
    with pytest.raises(Exception, match="exceeds ctx capacity"):
        ctx8.extract(np.full((252, 641), 90, np.uint8))
    with pytest.raises(Exception, match="exceeds ctx capacity"):
        ctx1.extract(np.full((904, 200), 90, np.uint8))
    _still_works(ctx8, oracle, synth, cases, ref_results, "no_cells_200x164")
    img = cases["nms_ties"]["img"]
    d = ctx1.device_alloc(img.nbytes)
    try:
        ctx1.h2d(d, img)
        with pytest.raises(Exception, match="stride"):
            ctx1.extract_device(d, img.shape[1], img.shape[0], img.shape[1] - 1)
        with pytest.raises(Exception, match="stride"):
            ctx1.extract_submit(d, img.shape[1], img.shape[0], img.shape[1] - 1)
    finally:
        ctx1.device_free(d)
    _still_works(ctx1, oracle, synth, cases, ref_results, "nms_ties")
    with pytest.raises(Exception, match="exceeds max_patches"):
        ctx1.extract(img, n_features_override=4097)
    _still_works(ctx1, oracle, synth, cases, ref_results, "nms_ties")
    # the quadtree stops at >= N nodes, so it may hand back more keypoints than asked for: a context without headroom overflows
    c = cases["quadtree_332x120_s3_N70"]
    assert len(ref_results[c["name"]]["kps"]) > 70
    tight = pkg.AsdHip(n_features=70, n_levels=1, max_width=332, max_height=120, max_patches=70)
    try:
        tight.load_weights(synth.asdnet_weights(0))
        with pytest.raises(Exception, match="more keypoints than max_patches"):
            tight.extract(c["img"])
        c5 = cases["quadtree_332x120_s1_N80"]          # 60 corners: fits
        k, _ = tight.extract(c5["img"])
        assert_same_keypoints(k, R.extract(c5["img"], 70, 1.2, 1)["kps"], "after the overflow")
    finally:
        tight.close()
