"""tests/local_ba_graph_ref.py pinned on the hand-worked maps of tests/local_ba_graph_cases.py, and the two argument structs of the binding
against the layout include/asd_slam.h gives them.  No device."""
import ctypes as C
import os
import re

import pytest

from tests import local_ba_graph_ref as ref
from tests.local_ba_graph_cases import assert_erase, assert_graph, erase_cases, flags_of, graph_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", graph_cases(), ids=lambda c: c["name"])
def test_graph_of_the_hand_worked_maps(case):
    m = case["map"]
    before = (m._copy().kf_points, set(m.pt_bad), set(m.kf_bad))
    got = ref.graph(m, case["kf"], case["neigh"])
    assert_graph(got, case["graph"], case["name"])
    assert (m.kf_points, m.pt_bad, m.kf_bad) == before
    rows = sorted(case["observations"])
    assert m.observations(rows) == [case["observations"][r] for r in rows]


def test_what_the_lists_case_is_there_for():
    case = graph_cases()[0]
    g, m = case["graph"], case["map"]
    assert 8 in m.kf_bad and 8 in case["neigh"] and 8 not in g["local_kfs"] and 8 not in g["e_kf"] and 8 in m.obs[105]   # a bad neighbour
    assert 99 in g["local_kfs"] and 99 not in m.kf_points and 99 in g["pose_kfs"]                                        # one not in the table
    assert 103 in m.pt_bad and 103 in m.kf_points[10] and -1 in m.kf_points[10] and 103 not in g["local_rows"]
    assert g["local_rows"].count(101) == 1 and 101 in m.kf_points[10] and 101 in m.kf_points[7]
    assert g["fixed_kfs"] != sorted(g["fixed_kfs"])                                                                      # discovered out of id order
    assert 12 in g["local_kfs"] and 12 not in g["e_kf"]                                                                  # a keyframe without an edge
    assert g["point_rank"] != sorted(g["point_rank"])
    assert 40 in m.kf_bad and 40 not in g["fixed_kfs"]


@pytest.mark.parametrize("case", erase_cases(), ids=lambda c: c["name"])
@pytest.mark.parametrize("apply", [False, True])
def test_erase_policy_of_the_hand_worked_maps(case, apply):
    m = case["map"]._copy()
    g = ref.graph(m, case["kf"], case["neigh"])
    assert_graph(g, case["graph"], case["name"])
    seats = dict(case["ref_kf"])
    before = m._copy()
    got = ref.erase(m, g, flags_of(case), apply, ref_kf=seats)
    assert_erase(got, case["result"], case["name"])
    if not apply:
        assert m.kf_points == before.kf_points and m.pt_bad == before.pt_bad and m.obs == before.obs and seats == case["ref_kf"]
        return
    assert m.kf_points == case["after"] and sorted(m.pt_bad) == case["bad_after"]
    for p, k in case["ref_after"].items():
        assert seats[p] == k, p
    # the sequential seat and the closed form of the header agree: new_ref is taken exactly when mpRefKF was among the erased keyframes
    erased_kfs = {}
    for e in case["flagged"]:
        erased_kfs.setdefault(g["local_rows"][g["point_rank"].index(g["e_point"][e])], set()).add(g["e_kf"][e])
    for i, p in enumerate(g["local_rows"]):
        if p in m.pt_bad:
            continue
        closed = got["new_ref"][i] if case["ref_kf"][p] in erased_kfs.get(p, ()) else case["ref_kf"][p]
        assert seats[p] == closed, p
    # the table mirrors mObservations afterwards
    for p, o in m.obs.items():
        for k, idx in o.items():
            assert m.kf_points[k][idx] == p
    assert sum(x >= 0 for row in m.kf_points.values() for x in row) == sum(len(o) for o in m.obs.values())


def _header_layout(name):
    """the fields of `typedef struct name { ... }` in include/asd_slam.h with the offsets the C ABI gives them (int32_t: 4 bytes, any
    pointer: 8, natural alignment) -> ([(field, offset)], sizeof)"""
    text = open(os.path.join(ROOT, "include", "asd_slam.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, off, align = [], 0, 1
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        size = 8 if "*" in decl else {"int32_t": 4, "uint8_t": 1, "double": 8, "float": 4}[decl.replace("const ", "").split()[0]]
        off = (off + size - 1) // size * size
        fields.append((re.findall(r"[A-Za-z_][A-Za-z_0-9]*", decl)[-1], off))
        off += size
        align = max(align, size)
    return fields, (off + align - 1) // align * align


@pytest.mark.parametrize("name, size", [("asd_ba_graph_args", 160), ("asd_ba_apply_args", 56)])
def test_the_bindings_structs_have_the_headers_layout(pkg, name, size):
    st = getattr(pkg.capi, name)
    fields, total = _header_layout(name)
    assert total == size and C.sizeof(st) == size
    assert [f for f, _ in fields] == [f for f, _ in st._fields_]
    for f, off in fields:
        assert getattr(st, f).offset == off, f
