"""The restatement of KeyFrameDatabase.cc (tests/kfdb_ref.py) against hand-computed cases, one per rule of the two queries, and the
revisit sequence's coverage of those rules.  No GPU: this pins the reference that tests/test_kfdb.py compares the library with."""
import numpy as np
import pytest

from tests import kfdb_cases, kfdb_ref


@pytest.mark.parametrize("case", kfdb_cases.HAND_CASES, ids=lambda c: c.__name__)
def test_hand_case(case):
    case(kfdb_cases.RefDriver(kfdb_ref.L1))


def test_scores_by_hand():
    v1 = (np.array([1, 4, 9], np.int32), np.array([0.5, 0.25, 0.25]))
    v2 = (np.array([4, 9, 12], np.int32), np.array([0.5, 0.125, 0.375]))
    # common words 4 and 9.  L1: (|0.25-0.5| - 0.25 - 0.5) + (|0.25-0.125| - 0.25 - 0.125) = -0.5 - 0.25 -> 0.375
    assert kfdb_ref.score(kfdb_ref.L1, v1, v2) == 0.375
    # products: 0.125 + 0.03125 = 0.15625; L2: 1 - sqrt(1 - 0.15625) = 1 - sqrt(0.84375)
    assert kfdb_ref.score(kfdb_ref.DOT, v1, v2) == 0.15625
    assert kfdb_ref.score(kfdb_ref.L2, v1, v2) == 1.0 - 0.84375 ** 0.5
    assert kfdb_ref.score(kfdb_ref.L2, (v1[0], 4 * v1[1]), (v2[0], 4 * v2[1])) == 1.0   # sum 2.5 >= 1: clamped
    disjoint = (np.array([2, 3], np.int32), np.array([0.5, 0.5]))
    s = kfdb_ref.score(kfdb_ref.L1, v1, disjoint)
    assert s == 0 and np.signbit(s)   # -score / 2.0 of an empty sum
    assert kfdb_ref.score(kfdb_ref.L2, v1, disjoint) == 0.0 and kfdb_ref.score(kfdb_ref.DOT, v1, disjoint) == 0.0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_revisit_sequence_is_not_vacuous(seed):
    db = kfdb_cases.RefDriver(kfdb_ref.L1)
    loop_hit, n_loop, reloc_hit, n_reloc = kfdb_cases.revisit_sequence(db, seed)
    c = db.db.count
    print(f"seed {seed}: cut {c.cut_by_min_common}, best-is-neighbour {c.best_is_neighbour}, duplicates {c.duplicate}, "
          f"dropped-by-retain {c.dropped_by_retain}, stale reloc scores {c.stale_reloc_score}; loop {loop_hit}/{n_loop}, reloc {reloc_hit}/{n_reloc}")
    assert n_loop == 110 and n_reloc == 30 and loop_hit > 0 and reloc_hit > 0
    assert c.cut_by_min_common > 0 and c.best_is_neighbour > 0 and c.duplicate > 0 and c.dropped_by_retain > 0 and c.stale_reloc_score > 0
