"""asd_kfdb_*: the keyframe database and its two queries on the device against the literal restatement of KeyFrameDatabase.cc in
tests/kfdb_ref.py (pinned by tests/test_kfdb_ref.py).  Scored lists (ids equal, scores bit-equal as f32), candidate lists and every
entry's query fields must be equal after every call (kfdb_cases.PairDriver); asd_kfdb_score must be bit-equal as f64."""
import numpy as np
import pytest

from tests import kfdb_cases, kfdb_ref
from tests.kfdb_cases import F32, PairDriver, bow

pytestmark = pytest.mark.gpu

SCORINGS = [kfdb_ref.L1, kfdb_ref.L2, kfdb_ref.DOT]


@pytest.mark.parametrize("case", kfdb_cases.HAND_CASES, ids=lambda c: c.__name__)
def test_hand_case(hip, case):
    case(PairDriver(hip, kfdb_ref.L1))


def _values(rng, n, scoring):
    v = rng.uniform(0.2, 3.0, n)
    if scoring == kfdb_ref.L1:
        v = v / np.abs(v).sum()
    elif scoring == kfdb_ref.L2:
        v = v / np.sqrt((v * v).sum())
    return v


@pytest.mark.parametrize("scoring", SCORINGS)
def test_kernel_edges(hip, pkg, scoring):
    """entry sizes around the 64-lane chunk, the smallest and the largest query, word ids of a k = 10, L = 6 vocabulary, and an entry
    whose only common word is its last: counts (the entries' fields), the smallest common word (the list order) and scores exact"""
    rng = np.random.default_rng(7 + scoring)
    n_words = 1000000
    q_ids = np.sort(rng.choice(n_words - 1, 4095, replace=False))
    q_ids = np.append(q_ids, n_words - 1).astype(np.int32)           # 4096 words, the last one 999 999
    outside = np.setdiff1d(np.arange(0, n_words, 7), q_ids)
    q = (q_ids, _values(rng, len(q_ids), scoring))
    db = PairDriver(hip, scoring)
    kf = 0
    for n in (0, 1, 63, 64, 65, 129):
        for frac in (0.0, 0.5, 1.0):
            k = int(round(frac * n))
            ids = np.unique(np.concatenate([rng.choice(q_ids, k, replace=False), rng.choice(outside, n - k, replace=False)])).astype(np.int32)
            db.add(kf, (ids, _values(rng, len(ids), scoring)), global_map=kf % 2 == 0)
            kf += 1
    for n in (1, 64, 65, 129):   # the only common word is the entry's last (999 999), in the last lane of its last chunk
        ids = np.append(np.sort(rng.choice(outside, n - 1, replace=False)), n_words - 1).astype(np.int32)
        db.add(kf, (ids, _values(rng, n, scoring)))
        kf += 1
    for n in (64, 129):          # ... and its first
        ids = np.append(q_ids[0], np.sort(rng.choice(outside[outside > q_ids[0]], n - 1, replace=False))).astype(np.int32)
        db.add(kf, (ids, _values(rng, n, scoring)))
        kf += 1
    every = db.ids()
    db.score(q, every)
    db.reloc(q)
    db.reloc(q, only_global_map=True)
    db.loop(q, [3, 8], 0.0)
    for w in (int(q_ids[0]), int(q_ids[2000]), n_words - 1, 5):   # one-word queries (5: most likely in no entry)
        one = (np.array([w], np.int32), np.array([1.0]))
        db.score(one, every)
        db.loop(one, [], 0.0)
        db.reloc(one)
    # 6000 words = 72 KB of LDS: above the 64 KB a kernel gets without asking
    wide_ids = np.union1d(q_ids, rng.choice(outside, 6000 - len(q_ids), replace=False)).astype(np.int32)
    wide = (wide_ids, _values(rng, len(wide_ids), scoring))
    db.score(wide, every)
    db.reloc(wide)
    ref_count = db.ref.db.count
    assert ref_count.cut_by_min_common > 0
    # a query larger than the LDS takes is refused, not truncated
    big = (np.arange(14000, dtype=np.int32), np.full(14000, 1.0 / 14000))
    with pytest.raises(pkg.AsdError) as e:
        hip.kfdb_query_reloc(big)
    assert e.value.code == -5


@pytest.mark.parametrize("scoring", SCORINGS)
def test_score_named_entries(hip, pkg, scoring):
    rng = np.random.default_rng(40 + scoring)
    db = PairDriver(hip, scoring)
    pool = np.arange(3000)
    for kf in range(200):
        ids = np.sort(rng.choice(pool, int(rng.integers(1, 300)), replace=False)).astype(np.int32)
        b = (ids, _values(rng, len(ids), scoring))
        db.ref.add(1000 + 3 * kf, b)
        db.dev.add(1000 + 3 * kf, b)
    ids = np.sort(rng.choice(pool, 1500, replace=False)).astype(np.int32)
    q = (ids, _values(rng, 1500, scoring))
    s1 = db.score(q, [1000 + 3 * 77])
    assert len(s1) == 1
    order = [1000 + 3 * int(k) for k in rng.permutation(200)]
    s200 = db.score(q, order)
    assert s200[order.index(1000 + 3 * 77)] == s1[0]
    # the same scores from the host-only entry point
    for k in order[:20]:
        assert pkg.capi.bow_score(scoring, q, db.ref.db.kfs[k].bow) == s200[order.index(k)]
    assert len(hip.kfdb_score(q, [])) == 0
    with pytest.raises(pkg.AsdError) as e:
        hip.kfdb_score(q, [1000, 1001])   # 1001 is not in the database
    assert e.value.code == -1
    with pytest.raises(pkg.AsdError) as e:
        hip.kfdb_add(1000, q)             # already present
    assert e.value.code == -1
    with pytest.raises(pkg.AsdError) as e:
        hip.kfdb_add(5, (np.array([3, 3], np.int32), np.array([0.5, 0.5])))
    assert e.value.code == -1


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_revisit_sequence(hip, seed):
    db = PairDriver(hip, kfdb_ref.L1)
    loop_hit, n_loop, reloc_hit, n_reloc = kfdb_cases.revisit_sequence(db, seed)
    c = db.ref.db.count
    print(f"seed {seed}: cut {c.cut_by_min_common}, best-is-neighbour {c.best_is_neighbour}, duplicates {c.duplicate}, "
          f"dropped-by-retain {c.dropped_by_retain}, stale reloc scores {c.stale_reloc_score}; loop {loop_hit}/{n_loop}, reloc {reloc_hit}/{n_reloc}")
    assert n_loop == 110 and n_reloc == 30 and loop_hit > 0 and reloc_hit > 0
    assert c.cut_by_min_common > 0 and c.best_is_neighbour > 0 and c.duplicate > 0 and c.dropped_by_retain > 0 and c.stale_reloc_score > 0


def test_growth(hip):
    """600 entries of 150 words: the arena (and the entry table) grow while entries are live; queries before and after agree with the
    restatement, and so do the live counts after every third entry has gone"""
    rng = np.random.default_rng(5)
    db = PairDriver(hip, kfdb_ref.L1)
    n_words = 6000
    places = [rng.choice(n_words, 400, replace=False) for _ in range(30)]

    def entry(place):
        ids = np.sort(rng.choice(places[place], 150, replace=False)).astype(np.int32)
        return ids, _values(rng, 150, kfdb_ref.L1)

    def add(kf):
        b = entry(kf % 30)
        db.ref.add(kf, b, global_map=kf % 5 != 0)
        db.dev.add(kf, b, global_map=kf % 5 != 0)

    def neigh(kf):
        return [kf - 30, kf + 30, kf + 60, 100000]

    def queries():
        for place in (0, 17):
            q = entry(place)
            _, cand = db.loop(q, [place, place + 30], 0.01, neigh=neigh)
            assert cand
            _, cand = db.reloc(q, only_global_map=place == 17, neigh=neigh)
            assert cand

    for kf in range(150):
        add(kf)
    live, words, slot_cap, word_cap, growths = hip.kfdb_debug()
    assert (live, words, growths) == (150, 150 * 150, 0) and word_cap < 600 * 150
    queries()
    for kf in range(150, 600):
        add(kf)
    live, words, slot_cap, word_cap, growths = hip.kfdb_debug()
    assert (live, words) == (600, 600 * 150) and growths >= 1 and word_cap >= 600 * 150 and slot_cap >= 600
    queries()
    every = db.ids()
    db.score(entry(3), every)
    for kf in range(0, 600, 3):
        db.ref.erase(kf)
        db.dev.erase(kf)
    live, words, _, _, _ = hip.kfdb_debug()
    assert (live, words) == (400, 400 * 150)
    queries()
    g0 = hip.kfdb_debug()[4]
    for kf in range(600, 1100):   # freed slots are taken again, and the next growth closes the holes
        add(kf)
    live, words, _, word_cap, growths = hip.kfdb_debug()
    assert (live, words) == (900, 900 * 150) and growths > g0 and word_cap >= words
    queries()
    db.check_fields()


def test_clear_and_scoring(hip, pkg, synth):
    a, b = bow({1: 0.5, 2: 0.25}), bow({1: 0.25, 2: 0.5})
    for scoring in SCORINGS:
        hip.kfdb_clear(scoring)
        assert hip.kfdb_debug()[:2] == (0, 0)
        hip.kfdb_add(4, a)
        assert hip.kfdb_debug()[:2] == (1, 2)
        assert hip.kfdb_score(b, [4])[0] == kfdb_ref.score(scoring, b, a)
        kf, sc = hip.kfdb_query_reloc(b)
        assert list(kf) == [4] and sc[0] == F32(kfdb_ref.score(scoring, b, a))
        assert hip.last_stage_ms("kfdb") > 0
    hip.kfdb_clear(kfdb_ref.L1)
    assert hip.kfdb_debug()[:2] == (0, 0)
    kf, sc = hip.kfdb_query_loop(b, [], 0.0)
    assert len(kf) == 0 and len(hip.kfdb_select(0, [])) == 0
    with pytest.raises(pkg.AsdError) as e:
        hip.kfdb_score(b, [4])
    assert e.value.code == -1
    for scoring in (2, 3, 4, 6, -2):
        with pytest.raises(pkg.AsdError) as e:
            hip.kfdb_clear(scoring)
        assert e.value.code == -1
    # select must follow the query whose state it uses
    hip.kfdb_add(1, a)
    hip.kfdb_add(2, b)
    kf, _ = hip.kfdb_query_loop(a, [], 0.0)
    assert list(kf) == [1, 2]
    with pytest.raises(pkg.AsdError) as e:
        hip.kfdb_select(0, [[2]])
    assert e.value.code == -1
    assert list(hip.kfdb_select(0, [[2], []])) == [1]
    hip.kfdb_erase(2)
    with pytest.raises(pkg.AsdError) as e:
        hip.kfdb_select(0, [[2], []])
    assert e.value.code == -1
    # -1 = the loaded vocabulary's scoring; a context of its own, so that no other test's vocabulary is in the way
    own = pkg.AsdHip(n_features=500, max_width=320, max_height=240, max_patches=1000)
    try:
        with pytest.raises(pkg.AsdError) as e:
            own.kfdb_clear(-1)
        assert e.value.code == -1
        own.voc_load(synth.vocabulary(k=4, L=2, seed=1), weighting=0, scoring=kfdb_ref.DOT)
        own.kfdb_clear(-1)
        own.kfdb_add(4, a)
        assert own.kfdb_score(b, [4])[0] == kfdb_ref.score(kfdb_ref.DOT, b, a) == 0.25
    finally:
        own.close()
