"""A plain Python restatement of LocalMapping::KeyFrameCulling (LocalMapping.cc:739-809, the monocular path) and of
MapPoint::Observations() (nObs, MapPoint.cc:110-117), the yardstick of asd_keyframe_culling and asd_map_observations.

It is tests/local_map_ref.RefMap with one more thing per keyframe: octave[kf][idx] = mvKeysUn[idx].octave.  The in-loop
pKF->SetBadFlag() is restated with what it does to the observation structure (KeyFrame.cc:739-741 -> MapPoint::EraseObservation,
MapPoint.cc:119-142 -> MapPoint::SetBadFlag, :180-197): the culled keyframe's observations go in ascending keypoint index, a point left
with <= 2 observations turns bad at that moment and loses every observation it has.  The spanning tree and the covisibility graph are
the caller's and are not restated.

The table keeps MapPoint::isBad() apart from the entries, so one case exists here that the reference cannot reach: a point that is
flagged bad and still has entries.  Such a point counts in nobody's nMPs; its entry in a culled keyframe's row goes like every other,
it is not reported again in bad_rows and its entries in other rows stay.
"""
import numpy as np

from tests.local_map_ref import RefMap

KEPT, CULLED, TO_BE_ERASED, SKIPPED = 0, 1, 2, 3


def map_point_culling(recent, observations, n_current_kf_id, th_obs=2):
    """LocalMapping::MapPointCulling (LocalMapping.cc:261-297, monocular: cnThObs = 2) over mlpRecentAddedMapPoints as records
    (row, mnFirstKFid, mnFound, mnVisible, isBad); observations[i] = Observations() of record i.
    -> (positions to SetBadFlag, rows of the list afterwards)"""
    set_bad, left = [], []
    for i, (row, first, found, visible, is_bad) in enumerate(recent):
        if is_bad:
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.float32(found) / np.float32(visible)        # GetFoundRatio: static_cast<float>(mnFound) / mnVisible
        if ratio < np.float32(0.25):
            set_bad.append(i)
        elif n_current_kf_id - first >= 2 and observations[i] <= th_obs:
            set_bad.append(i)
        elif n_current_kf_id - first >= 3:
            pass
        else:
            left.append(row)
    return set_bad, left


class CullingMap(RefMap):
    def __init__(self):
        super().__init__()
        self.octave = {}       # keyframe -> list of octaves, one per keypoint; absent = never given

    # ---- octaves belong to the keypoints: they live and die with the row's length
    def put_keyframe(self, kf, points):
        old_n = len(self.kf_points[kf]) if kf in self.kf_points else None
        super().put_keyframe(kf, points)
        if old_n != len(self.kf_points[kf]):
            self.octave.pop(kf, None)

    def erase_keyframe(self, kf):
        super().erase_keyframe(kf)
        self.octave.pop(kf, None)

    def put_octaves(self, kf, octaves):
        assert len(octaves) == len(self.kf_points[kf]) and all(0 <= int(o) < 16 for o in octaves)
        self.octave[kf] = [int(o) for o in octaves]

    # ---- MapPoint::Observations()
    def observations(self, rows):
        return [len(self.obs.get(int(r), {})) for r in rows]

    # ---- KeyFrame::SetBadFlag's effect on the observations (KeyFrame.cc:739-741)
    def _set_bad_flag(self, kf, bad_rows):
        self.kf_bad.add(kf)
        row = self.kf_points[kf]
        for idx in range(len(row)):
            p = row[idx]
            if p < 0:
                continue
            self.obs[p].pop(kf, None)                          # MapPoint::EraseObservation: nObs--
            row[idx] = -1
            if p in self.pt_bad:
                continue
            if len(self.obs[p]) <= 2:                          # MapPoint.cc:136-141 -> SetBadFlag
                self.pt_bad.add(p)
                bad_rows.append(p)
                for other, oidx in self.obs[p].items():        # pKF->EraseMapPointMatch(idx)
                    self.kf_points[other][oidx] = -1
                self.obs[p].clear()

    def keyframe_culling(self, cand, flags, apply):
        """-> dict(decision, n_mps, n_redundant, bad_rows); with apply the map is mutated, without it the map is left as it was"""
        m = self if apply else self._copy()
        decision, n_mps, n_red, bad_rows = [], [], [], []
        for kf, fl in zip(cand, flags):
            kf, fl = int(kf), int(fl)
            if (fl & 1) or kf == 0:                            # :751-754
                decision.append(SKIPPED); n_mps.append(0); n_red.append(0)
                continue
            nm = nr = 0
            for idx, p in enumerate(m.kf_points[kf]):
                if p < 0 or p in m.pt_bad:
                    continue
                nm += 1
                if len(m.obs[p]) > 3:                          # :776
                    level = m.octave[kf][idx]
                    n = 0
                    for other, oidx in m.obs[p].items():
                        if other == kf:
                            continue
                        if m.octave[other][oidx] <= level + 1:
                            n += 1
                            if n >= 3:
                                break
                    if n >= 3:
                        nr += 1
            n_mps.append(nm); n_red.append(nr)
            if not nr > 0.9 * nm:                              # :805, in double as there
                decision.append(KEPT)
            elif fl & 2:                                       # mbNotErase: mbToBeErased = true and nothing else (KeyFrame.cc:729-733)
                decision.append(TO_BE_ERASED)
            else:
                decision.append(CULLED)
                m._set_bad_flag(kf, bad_rows)
        return dict(decision=decision, n_mps=n_mps, n_redundant=n_red, bad_rows=bad_rows)

    def _copy(self):
        c = CullingMap()
        c.kf_points = {k: list(v) for k, v in self.kf_points.items()}
        c.obs = {p: dict(o) for p, o in self.obs.items()}
        c.kf_bad, c.pt_bad = set(self.kf_bad), set(self.pt_bad)
        c.cov, c.children, c.parent = dict(self.cov), dict(self.children), dict(self.parent)
        c.octave = {k: list(v) for k, v in self.octave.items()}
        return c

    @classmethod
    def from_map(cls, m, octave=None):
        """a RefMap (tests.local_map_cases.random_map) with octaves added"""
        c = cls()
        c.kf_points = {k: list(v) for k, v in m.kf_points.items()}
        c.obs = {p: dict(o) for p, o in m.obs.items()}
        c.kf_bad, c.pt_bad = set(m.kf_bad), set(m.pt_bad)
        c.cov, c.children, c.parent = dict(m.cov), dict(m.children), dict(m.parent)
        for kf, o in (octave or {}).items():
            c.put_octaves(kf, o)
        return c
