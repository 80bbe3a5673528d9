"""Shared by tests/test_kfdb_ref.py (CPU) and tests/test_kfdb.py (GPU): drivers with one interface over the restatement
(tests/kfdb_ref.py) and over the library's asd_kfdb_* calls, the hand-built cases with their expected values written out, and the
generator of the revisit sequence.

The hand cases use L1 scoring with dyadic positive values: the term |vi - wi| - |vi| - |wi| is then exactly -2 min(vi, wi), so the
score of two vectors is the sum of min(vi, wi) over their common words, exact in f64 and in f32 -- every expected number below can be
checked by hand.
"""
import numpy as np

from tests import kfdb_ref

F32 = np.float32


def bow(words):
    """{word: value} -> (ascending ids, values)"""
    ids = sorted(words)
    return np.array(ids, np.int32), np.array([words[w] for w in ids], np.float64)


def _neigh(neigh):
    if neigh is None:
        return lambda kf: []
    if callable(neigh):
        return neigh
    return lambda kf: neigh.get(kf, [])


class RefDriver:
    def __init__(self, scoring=kfdb_ref.L1):
        self.db = kfdb_ref.KeyFrameDatabase(scoring)

    def clear(self, scoring):
        self.db.clear(scoring)

    def add(self, kf, q, global_map=True):
        self.db.add(kf, q, global_map)

    def erase(self, kf):
        self.db.erase(kf)

    def ids(self):
        return sorted(self.db.kfs)

    def score(self, q, kfs):
        return self.db.score(q, kfs)

    def loop(self, q, connected, min_score, only_global_map=False, neigh=None):
        return self.db.detect_loop_candidates(q, connected, min_score, only_global_map, _neigh(neigh))

    def reloc(self, q, only_global_map=False, neigh=None):
        return self.db.detect_relocalization_candidates(q, only_global_map, _neigh(neigh))

    def fields(self, kf):
        return self.db.fields(kf)


class HipDriver:
    """the same interface over AsdHip.kfdb_*: a query is query_* followed by select with the scored keyframes' neighbours"""

    def __init__(self, hip, scoring=kfdb_ref.L1):
        self.hip = hip
        self.live = set()
        hip.kfdb_clear(scoring)

    def clear(self, scoring):
        self.hip.kfdb_clear(scoring)
        self.live = set()

    def add(self, kf, q, global_map=True):
        self.hip.kfdb_add(kf, q, global_map)
        self.live.add(kf)

    def erase(self, kf):
        self.hip.kfdb_erase(kf)
        self.live.discard(kf)

    def ids(self):
        return sorted(self.live)

    def score(self, q, kfs):
        return self.hip.kfdb_score(q, kfs)

    def loop(self, q, connected, min_score, only_global_map=False, neigh=None):
        kf, sc = self.hip.kfdb_query_loop(q, connected, min_score, only_global_map)
        cand = self.hip.kfdb_select(0, [_neigh(neigh)(int(k)) for k in kf])
        return [(int(k), F32(s)) for k, s in zip(kf, sc)], [int(c) for c in cand]

    def reloc(self, q, only_global_map=False, neigh=None):
        kf, sc = self.hip.kfdb_query_reloc(q, only_global_map)
        cand = self.hip.kfdb_select(1, [_neigh(neigh)(int(k)) for k in kf])
        return [(int(k), F32(s)) for k, s in zip(kf, sc)], [int(c) for c in cand]

    def fields(self, kf):
        return self.hip.kfdb_debug(kf)


def same_scored(a, b):
    return len(a) == len(b) and all(x[0] == y[0] and F32(x[1]) == F32(y[1]) for x, y in zip(a, b))


class PairDriver:
    """runs the restatement and the library side by side; every output and, after every call, every entry's fields must be equal"""

    def __init__(self, hip, scoring=kfdb_ref.L1):
        self.ref, self.dev = RefDriver(scoring), HipDriver(hip, scoring)

    def check_fields(self):
        assert self.ref.ids() == self.dev.ids()
        for kf in self.ref.ids():
            a, b = self.ref.fields(kf), self.dev.fields(kf)
            assert a == b, (kf, a, b)

    def clear(self, scoring):
        self.ref.clear(scoring)
        self.dev.clear(scoring)

    def add(self, kf, q, global_map=True):
        self.ref.add(kf, q, global_map)
        self.dev.add(kf, q, global_map)
        self.check_fields()

    def erase(self, kf):
        self.ref.erase(kf)
        self.dev.erase(kf)
        self.check_fields()

    def ids(self):
        return self.ref.ids()

    def score(self, q, kfs):
        a, b = self.ref.score(q, kfs), self.dev.score(q, kfs)
        assert a.dtype == b.dtype == np.float64 and np.array_equal(a, b), (a, b)
        return a

    def _both(self, a, b):
        assert same_scored(a[0], b[0]), (a[0], b[0])
        assert a[1] == b[1], (a[1], b[1])
        self.check_fields()
        return a

    def loop(self, q, connected, min_score, only_global_map=False, neigh=None):
        return self._both(self.ref.loop(q, connected, min_score, only_global_map, neigh),
                          self.dev.loop(q, connected, min_score, only_global_map, neigh))

    def reloc(self, q, only_global_map=False, neigh=None):
        return self._both(self.ref.reloc(q, only_global_map, neigh), self.dev.reloc(q, only_global_map, neigh))

    def fields(self, kf):
        return self.ref.fields(kf)


# ---- hand-built cases: case(db) runs on any driver above (db is fresh: empty, L1) and asserts the values worked out by hand ----

A, B, C, D = 11, 5, 42, 7   # ids in no particular order: nothing may depend on them


def _four_single_word_entries(db):
    # every entry shares exactly one word with the query {10, 20, 30} (all 0.5): maxCommonWords = 1, minCommonWords = 0, all are scored,
    # and the score is the entry's own value
    db.add(A, bow({30: 0.125}))
    db.add(B, bow({20: 0.25}))
    db.add(C, bow({10: 0.375}))
    db.add(D, bow({20: 0.5, 99: 1.0}))
    return bow({10: 0.5, 20: 0.5, 30: 0.5})


def case_list_order(db):
    q = _four_single_word_entries(db)
    scored, cand = db.loop(q, [], 0.0)
    # word 10: C; word 20: B before D (add order); word 30: A
    assert same_scored(scored, [(C, 0.375), (B, 0.25), (D, 0.5), (A, 0.125)])
    # no neighbours: bestAccScore = 0.5, retain > 0.55f * 0.5 = 0.275
    assert cand == [C, D]
    f = db.fields(B)
    assert f["loop_stamped"] and f["loop_words"] == 1 and f["loop_score"] == F32(0.25) and not f["reloc_stamped"]


def case_order_after_erase_and_readd(db):
    q = _four_single_word_entries(db)
    db.erase(B)
    db.erase(12345)   # unknown: nothing happens
    db.add(B, bow({20: 0.25}))
    scored, cand = db.loop(q, [], 0.0)
    assert same_scored(scored, [(C, 0.375), (D, 0.5), (B, 0.25), (A, 0.125)])   # B now behind D in word 20's list
    assert cand == [C, D]
    scored, _ = db.reloc(q)
    assert same_scored(scored, [(C, 0.375), (D, 0.5), (B, 0.25), (A, 0.125)])


def case_connected_excluded(db):
    q = _four_single_word_entries(db)
    scored, cand = db.loop(q, [D, 777], 0.0)   # (777 is not in the database)
    assert same_scored(scored, [(C, 0.375), (B, 0.25), (A, 0.125)])
    assert cand == [C, B]   # bestAccScore 0.375, retain > 0.20625
    f = db.fields(D)   # visited, so its word count was reset and incremented, but never stamped
    assert not f["loop_stamped"] and f["loop_words"] == 1 and f["loop_score"] == F32(0.0)


def case_min_common_words_truncation(db):
    X, Y, Z, W = 1, 2, 3, 4
    db.add(X, bow({1: 0.25, 2: 0.25, 3: 0.25}))
    db.add(Y, bow({1: 0.125, 2: 0.125}))
    db.add(Z, bow({3: 0.5}))
    db.add(W, bow({2: 0.5, 50: 0.5}))
    # loop: maxCommonWords = 3, 3 * 0.6f = 1.8000001 -> 1 (rounding would give 2): two words pass, one word does not (strict >)
    scored, _ = db.loop(bow({1: 0.5, 2: 0.5, 3: 0.5}), [], 0.0)
    assert same_scored(scored, [(X, 0.75), (Y, 0.25)])
    assert db.fields(Z)["loop_stamped"] and db.fields(Z)["loop_words"] == 1 and db.fields(Z)["loop_score"] == F32(0.0)
    # reloc: query {1, 2}: maxCommonWords = 2, 2 * 0.8f = 1.6 -> 1 (rounding would give 2): two words pass, one does not
    scored, cand = db.reloc(bow({1: 0.5, 2: 0.5}))
    assert same_scored(scored, [(X, 0.5), (Y, 0.25)])
    assert cand == [X]   # retain > 0.75f * 0.5 = 0.375
    assert db.fields(W)["reloc_stamped"] and db.fields(W)["reloc_words"] == 1 and db.fields(W)["reloc_score"] == F32(0.0)
    # loop with maxCommonWords = 5: 5 * 0.6f = 3.0000001 -> 3: four words pass, three do not
    db.add(10, bow({1: 0.5, 2: 0.5, 3: 0.5, 4: 0.5, 5: 0.5}))
    db.add(11, bow({1: 0.25, 2: 0.25, 3: 0.25, 4: 0.25}))
    db.add(12, bow({3: 0.25, 4: 0.25, 5: 0.25}))
    scored, _ = db.loop(bow({1: 0.5, 2: 0.5, 3: 0.5, 4: 0.5, 5: 0.5}), [], 0.0)
    assert same_scored(scored, [(10, 2.5), (11, 1.0)])


def case_score_equal_to_min_score_is_kept(db):
    db.add(A, bow({1: 0.25}))
    db.add(B, bow({2: 0.125}))
    scored, cand = db.loop(bow({1: 0.5, 2: 0.5}), [], 0.25)
    assert same_scored(scored, [(A, 0.25)])
    assert cand == [A]
    assert db.fields(B)["loop_score"] == F32(0.125)   # stored in front of the si >= minScore test


def case_loop_score_stored_for_rejected_keyframe(db):
    P, N = 3, 9
    db.add(P, bow({1: 0.25}), global_map=True)
    db.add(N, bow({1: 0.375}), global_map=False)
    scored, cand = db.loop(bow({1: 0.5}), [], 0.0, only_global_map=True, neigh={P: [N, 555]})
    assert same_scored(scored, [(P, 0.25)])
    assert db.fields(N)["loop_score"] == F32(0.375) and db.fields(N)["loop_stamped"]
    assert cand == [N]   # the group of P sums N's stored score (0.625) and N, the better of the two, stands for the group


def case_reloc_stale_score(db):
    G, NG = 3, 9
    db.add(G, bow({1: 0.25}), global_map=True)
    db.add(NG, bow({1: 0.5}), global_map=False)
    # 1: NG is stamped and counted but not scored; the group of G sums its mRelocScore, which no query has written: 0.0f
    scored, cand = db.reloc(bow({1: 0.5}), only_global_map=True, neigh={G: [NG]})
    assert same_scored(scored, [(G, 0.25)]) and cand == [G]
    f = db.fields(NG)
    assert f["reloc_stamped"] and f["reloc_words"] == 1 and f["reloc_score"] == F32(0.0)
    # 2: both scored; NG's score becomes 0.5
    scored, cand = db.reloc(bow({1: 0.5}), only_global_map=False)
    assert same_scored(scored, [(G, 0.25), (NG, 0.5)]) and cand == [NG]
    # 3: only_global_map again, a weaker query: G scores 0.125, and NG enters G's group with the 0.5 query 2 left on it
    scored, cand = db.reloc(bow({1: 0.125}), only_global_map=True, neigh={G: [NG]})
    assert same_scored(scored, [(G, 0.125)])
    assert cand == [NG]
    assert db.fields(NG)["reloc_score"] == F32(0.5)


def case_best_of_group_and_duplicates(db):
    db.add(A, bow({1: 0.25}))
    db.add(B, bow({1: 0.5}))
    db.add(C, bow({1: 0.125}))
    # groups: A + B = 0.75 best B; B alone 0.5 best B; C + A = 0.375 best A.  retain > 0.55f * 0.75 = 0.4125: the first two, both B
    scored, cand = db.loop(bow({1: 1.0}), [], 0.0, neigh={A: [B], C: [A]})
    assert same_scored(scored, [(A, 0.25), (B, 0.5), (C, 0.125)])
    assert cand == [B]
    scored, cand = db.reloc(bow({1: 1.0}), neigh={A: [B], C: [A]})
    assert cand == [B]   # retain > 0.75f * 0.75 = 0.5625: only the first group


def case_retain_exactly_at_the_bound(db):
    v = float(F32(0.55))                      # the f32 0.55f as f64: the L1 score of {w: v} against {w: 1.0} is exactly v
    v_up = float(np.nextafter(F32(0.55), F32(1.0)))
    db.add(A, bow({1: 1.0}))
    db.add(B, bow({2: v}))
    db.add(C, bow({3: v_up}))
    q = bow({1: 1.0, 2: 1.0, 3: 1.0})
    scored, cand = db.loop(q, [], 0.0)
    assert same_scored(scored, [(A, 1.0), (B, F32(0.55)), (C, F32(v_up))])
    assert cand == [A, C]                     # bestAccScore = 1: B's 0.55f is not > 0.55f * 1.0f
    db.add(D, bow({4: 0.75}))
    scored, cand = db.reloc(bow({1: 1.0, 4: 1.0}))
    assert same_scored(scored, [(A, 1.0), (D, 0.75)]) and cand == [A]   # 0.75 is not > 0.75f * 1.0f


def case_empty_results(db):
    q = bow({1: 0.5, 2: 0.5})
    assert db.loop(q, [], 0.0) == ([], [])    # empty database
    assert db.reloc(q) == ([], [])
    db.add(A, bow({7: 0.5}))
    db.add(B, bow({}))                        # an empty BowVector: a legal entry no query finds
    assert db.loop(q, [], 0.0) == ([], [])    # no common word
    assert db.reloc(q) == ([], [])
    assert not db.fields(A)["loop_stamped"] and not db.fields(A)["reloc_stamped"]
    db.add(C, bow({1: 0.125}))
    assert db.loop(q, [], 0.5) == ([], [])    # lScoreAndMatch empty: everything below minScore
    assert db.fields(C)["loop_score"] == F32(0.125)
    assert db.loop(bow({}), [], 0.0) == ([], [])
    assert db.loop(q, [C], 0.0) == ([], [])   # the only sharing keyframe is connected
    assert db.reloc(q, only_global_map=True) == ([(C, F32(0.125))], [C])


HAND_CASES = [case_list_order, case_order_after_erase_and_readd, case_connected_excluded, case_min_common_words_truncation,
              case_score_equal_to_min_score_is_kept, case_loop_score_stored_for_rejected_keyframe, case_reloc_stale_score,
              case_best_of_group_and_duplicates, case_retain_exactly_at_the_bound, case_empty_results]


# ---- the revisit sequence ----

N_WORDS, N_PLACES, N_KF = 4096, 24, 120


def place_of(i):
    return (i // 3) % N_PLACES if i < 72 else ((i - 72) // 2) % N_PLACES


def make_bow(rng, pools, place):
    """40-139 words of the place's pool, the first 60 of the next place's, 0-29 noise words; values in [0.2, 3], L1-normalised"""
    own = rng.choice(pools[place], int(rng.integers(40, 140)), replace=False)
    noise = rng.integers(0, N_WORDS, int(rng.integers(0, 30)))
    ids = np.unique(np.concatenate([own, pools[(place + 1) % N_PLACES][:60], noise])).astype(np.int32)
    vals = rng.uniform(0.2, 3.0, len(ids))
    return ids, vals / np.abs(vals).sum()


def neighbours_of(kf):
    return [j for j in range(kf - 5, kf + 6) if j != kf and 0 <= j < N_KF]


def revisit_sequence(db, seed):
    """LoopClosing::DetectLoop's sequence for every keyframe from the tenth on, with erases and relocalisation queries in between;
    returns (loop queries with candidates, loop queries, reloc queries with candidates, reloc queries)"""
    rng = np.random.default_rng(seed)
    pools = [rng.choice(N_WORDS, 160, replace=False) for _ in range(N_PLACES)]
    n_loop = n_loop_hit = n_reloc = n_reloc_hit = 0
    for i in range(N_KF):
        q = make_bow(rng, pools, place_of(i))
        if i >= 10:
            connected = list(range(i - 8, i))
            min_score = F32(min(F32(s) for s in db.score(q, connected)))   # LoopClosing.cc:154-168
            _scored, cand = db.loop(q, connected, min_score, only_global_map=(i % 4 == 3), neigh=neighbours_of)
            n_loop += 1
            n_loop_hit += bool(cand)
        db.add(i, q, global_map=i < 80)
        if i % 7 == 6 and i > 20:
            db.erase(i - 15)
        if i >= 30 and i % 3 == 0:
            f = make_bow(rng, pools, int(rng.integers(N_PLACES)))
            _scored, cand = db.reloc(f, only_global_map=bool((i // 3) % 2), neigh=neighbours_of)
            n_reloc += 1
            n_reloc_hit += bool(cand)
    return n_loop_hit, n_loop, n_reloc_hit, n_reloc
