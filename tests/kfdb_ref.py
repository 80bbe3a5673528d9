"""A literal Python restatement of the reference's KeyFrameDatabase (src/vslam/src/KeyFrameDatabase.cc) and of the three scorings the
library offers (src/dbow2/DBoW2/ScoringObject.cpp:23-120, :271-311): the reference of tests/test_kfdb*.py and tests/test_bow_score.py.

It is written the way the reference is: real inverted lists (one Python list of keyframe objects per word, appended by add(), searched
and cut by erase()), the per-keyframe query fields as persistent attributes of the keyframe objects, the float expressions in
np.float32 and the scores as a Python-float (f64) loop in ascending word order.  It deliberately does NOT use the
(smallest common word, add sequence) ordering the library sorts by: that shortcut is what the tests check.

The reference's own ScoringObject.cpp cannot be compiled for the tests (it includes TemplatedVocabulary.h, which needs OpenCV), so this
restatement is pinned by the hand-computed cases of tests/test_kfdb_ref.py instead.

Two things differ from the reference on purpose, as in the library (include/asd_slam.h): a query stamps with a fresh number per call
(the reference stamps with the querying keyframe's / frame's id), and mLoopScore / mRelocScore start at 0.0f (the reference leaves them
uninitialised).
"""
import math

import numpy as np

L1, L2, DOT = 0, 1, 5
F32 = np.float32


def score(scoring, v1, v2):
    """TemplatedVocabulary::score(v1, v2); v = (ascending word ids, values).  The lower_bound jumps of the reference visit the common
    words in ascending order, as this merge does."""
    id1, x1 = [int(i) for i in v1[0]], [float(x) for x in v1[1]]
    id2, x2 = [int(i) for i in v2[0]], [float(x) for x in v2[1]]
    s = 0.0
    i = j = 0
    while i < len(id1) and j < len(id2):
        if id1[i] == id2[j]:
            vi, wi = x1[i], x2[j]
            if scoring == L1:
                s += math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi)
            elif scoring in (L2, DOT):
                s += vi * wi
            else:
                raise ValueError(scoring)
            i += 1
            j += 1
        elif id1[i] < id2[j]:
            i += 1
        else:
            j += 1
    if scoring == L1:
        return -s / 2.0
    if scoring == L2:
        return 1.0 if s >= 1 else 1.0 - math.sqrt(1.0 - s)
    return s


class KeyFrame:
    def __init__(self, kf_id, bow, global_map):
        self.id = int(kf_id)
        self.bow = (np.asarray(bow[0], np.int32).copy(), np.asarray(bow[1], np.float64).copy())
        self.global_map = bool(global_map)
        self.loop_query = None
        self.loop_words = 0
        self.loop_score = F32(0.0)
        self.reloc_query = None
        self.reloc_words = 0
        self.reloc_score = F32(0.0)


class Counters:
    """what a run exercised (tests assert that a sequence is not vacuous)"""

    def __init__(self):
        self.cut_by_min_common = 0     # a listed keyframe that the minCommonWords gate kept from being scored
        self.best_is_neighbour = 0     # a group whose best keyframe is a neighbour
        self.duplicate = 0             # a candidate suppressed by spAlreadyAddedKF
        self.dropped_by_retain = 0     # a group at or below minScoreToRetain
        self.stale_reloc_score = 0     # a neighbour stamped by this reloc query, not scored by it, with a non-zero earlier score


class KeyFrameDatabase:
    def __init__(self, scoring=L1):
        self.scoring = scoring
        self.inverted = {}     # mvInvertedFile: word id -> list of KeyFrame, in add() order
        self.kfs = {}          # id -> KeyFrame (the caller's pointers)
        self.stamp = 0
        self.last_loop = None
        self.last_reloc = None
        self.count = Counters()

    def add(self, kf_id, bow, global_map=True):
        assert kf_id not in self.kfs
        kf = KeyFrame(kf_id, bow, global_map)
        self.kfs[kf.id] = kf
        for w in kf.bow[0]:
            self.inverted.setdefault(int(w), []).append(kf)

    def erase(self, kf_id):
        kf = self.kfs.pop(kf_id, None)
        if kf is None:
            return
        for w in kf.bow[0]:
            lst = self.inverted[int(w)]
            for k, other in enumerate(lst):
                if other is kf:
                    del lst[k]
                    break

    def clear(self, scoring=None):
        self.inverted = {}
        self.kfs = {}
        self.last_loop = self.last_reloc = None
        if scoring is not None:
            self.scoring = scoring

    def score(self, bow, kf_ids):
        return np.array([score(self.scoring, bow, self.kfs[k].bow) for k in kf_ids], np.float64)

    def fields(self, kf_id):
        kf = self.kfs[kf_id]
        return dict(loop_stamped=kf.loop_query is not None and kf.loop_query == self.last_loop, loop_words=kf.loop_words,
                    reloc_stamped=kf.reloc_query is not None and kf.reloc_query == self.last_reloc, reloc_words=kf.reloc_words,
                    loop_score=F32(kf.loop_score), reloc_score=F32(kf.reloc_score))

    # KeyFrameDatabase::DetectLoopCandidates (:80-204).  neighbours(id) = GetBestCovisibilityKeyFrames(10) as ids.
    # -> (lScoreAndMatch as [(id, f32 si)], vpLoopCandidates as [id])
    def detect_loop_candidates(self, bow, connected, min_score, only_global_map, neighbours):
        self.stamp += 1
        query = self.last_loop = self.stamp
        min_score = F32(min_score)
        connected = {self.kfs[c] for c in connected if c in self.kfs}
        sharing = []
        for w in bow[0]:
            for kfi in self.inverted.get(int(w), []):
                if kfi.loop_query != query:
                    kfi.loop_words = 0
                    if kfi not in connected:
                        kfi.loop_query = query
                        sharing.append(kfi)
                kfi.loop_words += 1
        if not sharing:
            return [], []
        max_common = 0
        for kfi in sharing:
            if kfi.loop_words > max_common:
                max_common = kfi.loop_words
        min_common = int(F32(max_common) * F32(0.6))
        score_and_match = []
        for kfi in sharing:
            if kfi.loop_words > min_common:
                si = F32(score(self.scoring, bow, kfi.bow))
                kfi.loop_score = si
                if si >= min_score:
                    if (only_global_map and kfi.global_map) or not only_global_map:
                        score_and_match.append((si, kfi))
            else:
                self.count.cut_by_min_common += 1
        scored = [(k.id, s) for s, k in score_and_match]
        if not score_and_match:
            return scored, []
        acc_and_match = []
        best_acc = min_score
        for si, kfi in score_and_match:
            best_score = si
            acc = si
            best = kfi
            for nid in neighbours(kfi.id):
                kf2 = self.kfs.get(nid)
                if kf2 is None:   # a keyframe outside the database: its mnLoopQuery is not this query's
                    continue
                if kf2.loop_query == query and kf2.loop_words > min_common:
                    acc = F32(acc + kf2.loop_score)
                    if kf2.loop_score > best_score:
                        best = kf2
                        best_score = kf2.loop_score
            if best is not kfi:
                self.count.best_is_neighbour += 1
            acc_and_match.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        retain = F32(F32(0.55) * best_acc)
        return scored, self._retain(acc_and_match, retain)

    # KeyFrameDatabase::DetectRelocalizationCandidates (:206-322)
    def detect_relocalization_candidates(self, bow, only_global_map, neighbours):
        self.stamp += 1
        query = self.last_reloc = self.stamp
        sharing = []
        for w in bow[0]:
            for kfi in self.inverted.get(int(w), []):
                if kfi.reloc_query != query:
                    kfi.reloc_words = 0
                    kfi.reloc_query = query
                    if (only_global_map and kfi.global_map) or not only_global_map:
                        sharing.append(kfi)
                kfi.reloc_words += 1
        if not sharing:
            return [], []
        max_common = 0
        for kfi in sharing:
            if kfi.reloc_words > max_common:
                max_common = kfi.reloc_words
        min_common = int(F32(max_common) * F32(0.8))
        score_and_match = []
        scored_now = set()
        for kfi in sharing:
            if kfi.reloc_words > min_common:
                si = F32(score(self.scoring, bow, kfi.bow))
                kfi.reloc_score = si
                score_and_match.append((si, kfi))
                scored_now.add(kfi.id)
            else:
                self.count.cut_by_min_common += 1
        scored = [(k.id, s) for s, k in score_and_match]
        if not score_and_match:
            return scored, []
        acc_and_match = []
        best_acc = F32(0.0)
        for si, kfi in score_and_match:
            best_score = si
            acc = best_score
            best = kfi
            for nid in neighbours(kfi.id):
                kf2 = self.kfs.get(nid)
                if kf2 is None:
                    continue
                if kf2.reloc_query != query:
                    continue
                if kf2.id not in scored_now and kf2.reloc_score != 0:
                    self.count.stale_reloc_score += 1
                acc = F32(acc + kf2.reloc_score)
                if kf2.reloc_score > best_score:
                    best = kf2
                    best_score = kf2.reloc_score
            if best is not kfi:
                self.count.best_is_neighbour += 1
            acc_and_match.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        retain = F32(F32(0.75) * best_acc)
        return scored, self._retain(acc_and_match, retain)

    def _retain(self, acc_and_match, retain):
        already = set()
        out = []
        for acc, kfi in acc_and_match:
            if acc > retain:
                if kfi not in already:
                    out.append(kfi.id)
                    already.add(kfi)
                else:
                    self.count.duplicate += 1
            else:
                self.count.dropped_by_retain += 1
        return out
