"""The host-built active structure of LocalBA / BundleAdjustment (asd-slam_amd/csrc/ba_structure.h) through host/test_ba_structure
(no device, no library): every table the program prints equals tests/ba_structure_ref.py's restatement from the definition, on hand-worked
maps, the edge cases below and seeded random problems, with every upper block and with the sparse block selection."""
import os
import random
import subprocess

import pytest

from tests.ba_structure_ref import structure
from tests.conftest import ROOT

PROBE = os.path.join(ROOT, "asd-slam_amd", "host", "test_ba_structure")

# name -> (P, L, fixed, [(point, pose), ...])
CASES = {
    "worked": (3, 2, [1, 0, 0], [(0, 2), (0, 0), (0, 1), (1, 1)]),
    "all_fixed": (2, 2, [1, 1], [(0, 0), (1, 1), (1, 0)]),                       # nPf = 0
    "one_edge": (1, 1, [0], [(0, 0)]),
    "one_edge_fixed": (1, 1, [1], [(0, 0)]),
    "dup_free": (2, 2, [0, 0], [(0, 1), (0, 0), (0, 1), (1, 0)]),               # pose 1 observes point 0 twice
    "dup_free_thrice": (2, 1, [0, 0], [(0, 1), (0, 1), (0, 0), (0, 1)]),
    "dup_fixed": (3, 2, [0, 1, 0], [(0, 1), (0, 2), (0, 1), (1, 0), (0, 0)]),   # the fixed pose observes point 0 twice
    "fixed_not_prefix": (5, 3, [0, 1, 0, 1, 0], [(0, 4), (0, 3), (1, 2), (1, 0), (2, 1), (2, 4), (0, 0)]),
    "idle_vertices": (4, 4, [0, 0, 1, 0], [(3, 3), (0, 0), (3, 0), (0, 2)]),    # pose 1 and points 1, 2 without edges
    "no_shared_landmark": (3, 3, [0, 0, 0], [(0, 0), (1, 1), (2, 2), (2, 0)]),  # poses 0 and 1, 1 and 2 share nothing
}


def _random_case(seed):
    r = random.Random(seed)
    P, L = r.randint(1, 12), r.randint(1, 20)
    E = r.randint(1, 80)
    fixed = [int(r.random() < 0.35) for _ in range(P)]
    edges = [(r.randrange(L), r.randrange(P)) for _ in range(E)]   # duplicates happen
    return P, L, fixed, edges


for _s in range(40):
    CASES[f"random{_s}"] = _random_case(1000 + _s)


def _text(P, L, fixed, edges, all_blocks):
    return " ".join(map(str, [P, L, len(edges), int(all_blocks)] + list(fixed) + [v for pt, ps in edges for v in (ps, pt)])) + "\n"


def _parse(block):
    out = {}
    for ln in block:
        name, _, rest = ln.partition(":")
        vals = rest.split()
        out[name] = [tuple(map(int, v.split(","))) for v in vals] if name == "pairs" else [int(v) for v in vals]
    return out


@pytest.fixture(scope="module")
def program_output():
    """one run of the program over every case in both modes"""
    if not os.path.exists(PROBE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "asd-slam_amd", "csrc"), "../host/test_ba_structure"])
    keys = [(name, ab) for name in CASES for ab in (True, False)]
    r = subprocess.run([PROBE], input="".join(_text(*CASES[n], ab) for n, ab in keys), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    blocks, cur = [], []
    for ln in r.stdout.splitlines():
        if ln == "end":
            blocks.append(_parse(cur))
            cur = []
        else:
            cur.append(ln)
    assert len(blocks) == len(keys) and not cur
    return dict(zip(keys, blocks))


@pytest.mark.parametrize("all_blocks", [True, False], ids=["all_blocks", "blocks_with_pairs"])
@pytest.mark.parametrize("name", list(CASES))
def test_tables_equal_the_restatement(program_output, name, all_blocks):
    P, L, fixed, edges = CASES[name]
    want = structure(P, L, fixed, [ps for _, ps in edges], [pt for pt, _ in edges], all_blocks)
    got = program_output[(name, all_blocks)]
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], (name, all_blocks, k)


def test_worked_example_by_hand(program_output):
    for ab in (True, False):   # every block of this map has a pair: the two selections agree
        g = program_output[("worked", ab)]
        assert g["counts"] == [2, 2, 4, 3, 4]
        assert g["pose_h"] == [-1, 0, 1] and g["pt_h"] == [0, 1] and g["pose_of_h"] == [1, 2] and g["pt_of_h"] == [0, 1]
        assert g["pt_start"] == [0, 3, 4] and g["act"] == [1, 2, 0, 3]
        assert g["ps_start"] == [0, 2, 3] and g["ps_edges"] == [1, 3, 2] and g["ps_h"] == [0, 1, 0]
        assert list(zip(g["blk_i"], g["blk_j"])) == [(0, 0), (0, 1), (1, 1)]
        assert g["pair_start"] == [0, 2, 3, 4] and g["pairs"] == [(1, 1), (3, 3), (1, 2), (2, 2)] and g["pair_h"] == [0, 1, 0, 0]


def test_hand_worked_edge_cases(program_output):
    g = program_output[("all_fixed", True)]
    assert g["counts"] == [0, 2, 3, 0, 0] and g["pose_h"] == [-1, -1] and g["act"] == [0, 1, 2] and g["ps_start"] == [0]
    assert g["pair_start"] == [0] and g["pairs"] == [] and g["blk_i"] == []
    g = program_output[("one_edge", False)]
    assert g["counts"] == [1, 1, 1, 1, 1] and g["pairs"] == [(0, 0)] and g["pair_start"] == [0, 1] and g["ps_edges"] == [0]
    # pose 1 twice on point 0: act = [1 (pose 0), 0, 2 (pose 1, edge order), 3]; block (1, 1) holds (1,1) (1,2) (2,1) (2,2)
    g = program_output[("dup_free", True)]
    assert g["act"] == [1, 0, 2, 3]
    assert g["pair_start"] == [0, 2, 4, 8]
    assert g["pairs"] == [(0, 0), (3, 3), (0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2)]
    assert g["pair_h"] == [0, 1, 0, 0, 0, 0, 0, 0]
    # the fixed pose twice on point 0: its two edges lead the landmark in edge order and make no pair
    g = program_output[("dup_fixed", True)]
    assert g["act"] == [0, 2, 4, 1, 3] and g["pose_h"] == [0, -1, 1]
    assert g["pairs"] == [(2, 2), (4, 4), (2, 3), (3, 3)] and g["pair_start"] == [0, 2, 3, 4]
    # poses 0 and 2 share point 2; (0, 1) and (1, 2) share nothing
    g = program_output[("no_shared_landmark", False)]
    assert list(zip(g["blk_i"], g["blk_j"])) == [(0, 0), (0, 2), (1, 1), (2, 2)]
    g = program_output[("no_shared_landmark", True)]
    assert list(zip(g["blk_i"], g["blk_j"])) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    assert g["pair_start"] == [0, 2, 2, 3, 4, 4, 5]
