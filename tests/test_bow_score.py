"""asd_bow_score (host only: no context, no GPU) against the restatement of L1 / L2 / DotProductScoring::score in tests/kfdb_ref.py:
bit-equal f64."""
import numpy as np
import pytest

from tests import kfdb_ref

SCORINGS = [kfdb_ref.L1, kfdb_ref.L2, kfdb_ref.DOT]


def vec(rng, n, n_words=100000, norm=None):
    ids = np.sort(rng.choice(n_words, n, replace=False)).astype(np.int32)
    vals = rng.uniform(0.2, 3.0, n)
    if norm == kfdb_ref.L1:
        vals = vals / np.abs(vals).sum()
    elif norm == kfdb_ref.L2:
        vals = vals / np.sqrt((vals * vals).sum())
    return ids, vals


def overlapping(rng, base, n, frac, norm):
    """n words, about frac of them base's"""
    k = min(int(round(frac * n)), len(base[0]))
    own = rng.choice(base[0], k, replace=False)
    rest = np.setdiff1d(np.arange(100000, 100000 + 4 * n), base[0])[: n - k]
    ids = np.unique(np.concatenate([own, rest])).astype(np.int32)
    vals = rng.uniform(0.2, 3.0, len(ids))
    if norm == kfdb_ref.L1:
        vals = vals / np.abs(vals).sum()
    elif norm == kfdb_ref.L2:
        vals = vals / np.sqrt((vals * vals).sum())
    return ids, vals


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


@pytest.mark.parametrize("scoring", SCORINGS)
def test_disjoint_identical_single(pkg, scoring):
    rng = np.random.default_rng(3)
    a = vec(rng, 50, norm=scoring)
    b = (a[0] + 200000, a[1])
    s = pkg.capi.bow_score(scoring, a, b)
    assert s == 0 and s == kfdb_ref.score(scoring, a, b)   # disjoint (L1: -0.0, compared by value)
    s = pkg.capi.bow_score(scoring, a, a)
    assert same_bits(s, kfdb_ref.score(scoring, a, a))
    if scoring != kfdb_ref.DOT:
        assert abs(s - 1.0) < 1e-7   # a normalised vector against itself
    one, other = (np.array([7], np.int32), np.array([0.75])), (np.array([7], np.int32), np.array([0.5]))
    assert same_bits(pkg.capi.bow_score(scoring, one, other), kfdb_ref.score(scoring, one, other))
    assert pkg.capi.bow_score(kfdb_ref.L1, one, other) == 0.5 and pkg.capi.bow_score(kfdb_ref.DOT, one, other) == 0.375
    empty = (np.zeros(0, np.int32), np.zeros(0))
    assert pkg.capi.bow_score(scoring, empty, a) == 0 and pkg.capi.bow_score(scoring, empty, empty) == 0


@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2000])
def test_bit_equal_over_sizes_and_overlaps(pkg, scoring, n):
    rng = np.random.default_rng(100 * scoring + n)
    base = vec(rng, n, norm=scoring)
    for frac in (0.0, 0.1, 0.5, 0.9, 1.0):
        for m in (n, max(1, n // 2), n + 17):
            other = overlapping(rng, base, m, frac, scoring)
            for v1, v2 in ((base, other), (other, base)):
                got, ref = pkg.capi.bow_score(scoring, v1, v2), kfdb_ref.score(scoring, v1, v2)
                assert same_bits(got, ref) or (got == 0 and ref == 0), (n, m, frac, got, ref)


def test_l2_clamp(pkg):
    a = (np.array([1, 2, 3], np.int32), np.array([1.0, 0.5, 0.5]))
    assert pkg.capi.bow_score(kfdb_ref.L2, a, a) == 1.0 == kfdb_ref.score(kfdb_ref.L2, a, a)       # sum 1.5 >= 1
    b = (np.array([1], np.int32), np.array([1.0]))
    assert pkg.capi.bow_score(kfdb_ref.L2, b, b) == 1.0                                            # sum exactly 1
    c = (np.array([1], np.int32), np.array([0.75]))
    assert same_bits(pkg.capi.bow_score(kfdb_ref.L2, b, c), 1.0 - 0.25 ** 0.5)                     # 0.75 < 1: 1 - sqrt(0.25)


def test_refused_arguments(pkg):
    a = (np.array([1, 2, 3], np.int32), np.array([0.5, 0.25, 0.25]))
    for scoring in (2, 3, 4):
        with pytest.raises(pkg.AsdError) as e:
            pkg.capi.bow_score(scoring, a, a)
        assert e.value.code == -1 and "not offered" in str(e.value)
    for scoring in (-1, 6):
        with pytest.raises(pkg.AsdError) as e:
            pkg.capi.bow_score(scoring, a, a)
        assert e.value.code == -1
    for bad in ((np.array([1, 3, 2], np.int32), a[1]), (np.array([1, 2, 2], np.int32), a[1])):
        for v1, v2 in ((bad, a), (a, bad)):
            with pytest.raises(pkg.AsdError) as e:
                pkg.capi.bow_score(kfdb_ref.L1, v1, v2)
            assert e.value.code == -1 and "ascending" in str(e.value)
