"""A plain Python restatement of Tracking::SearchLocalPoints' skip loop (Tracking.cc:803-841), Tracking::UpdateLocalMap
(:871-1015) and KeyFrame::UpdateConnections (KeyFrame.cc:533-637), the yardstick of asd_update_local_map and
asd_map_shared_counts.

It keeps what the reference keeps: per map point the observation dict (MapPoint::mObservations, keyframe -> keypoint index) and
per keyframe the point list (KeyFrame::mvpMapPoints, -1 = none).  Points and keyframes are named by plain integers (for a point:
its bank row).  The ONE stated rule: where the reference walks a std::map<KeyFrame*, ...> or a std::set<KeyFrame*> in pointer
order, the walk here is in ascending keyframe id.  A keyframe that links name but the map does not hold has no points and is not
bad -- a pointer the host still holds.
"""


class RefMap:
    def __init__(self):
        self.kf_points = {}    # KeyFrame::mvpMapPoints: keyframe -> list of point ids, -1 = none
        self.obs = {}          # MapPoint::mObservations: point -> {keyframe: keypoint index}
        self.kf_bad = set()    # KeyFrame::isBad()
        self.pt_bad = set()    # MapPoint::isBad()
        self.cov = {}          # GetBestCovisibilityKeyFrames(10): keyframe -> ids in its order
        self.children = {}     # GetChilds(): keyframe -> ids
        self.parent = {}       # GetParent(): keyframe -> id or -1

    # ---- the map's own bookkeeping (AddObservation / EraseObservation / Replace / SetBadFlag)
    def put_keyframe(self, kf, points):
        """create or replace a keyframe's point list; links and flag of a replaced keyframe stay"""
        for p in self.kf_points.get(kf, []):
            if p >= 0:
                self.obs[p].pop(kf, None)
        self.kf_points[kf] = [int(p) for p in points]
        for idx, p in enumerate(self.kf_points[kf]):
            if p >= 0:
                assert kf not in self.obs.setdefault(p, {}), "a point occurs at most once per keyframe"
                self.obs[p][kf] = idx

    def set_entry(self, kf, idx, point):
        old = self.kf_points[kf][idx]
        if old >= 0:
            self.obs[old].pop(kf, None)
        self.kf_points[kf][idx] = int(point)
        if point >= 0:
            assert kf not in self.obs.setdefault(int(point), {}), "a point occurs at most once per keyframe"
            self.obs[int(point)][kf] = idx

    def erase_keyframe(self, kf):
        for p in self.kf_points.pop(kf, []):
            if p >= 0:
                self.obs[p].pop(kf, None)
        self.kf_bad.discard(kf)
        self.cov.pop(kf, None)
        self.children.pop(kf, None)
        self.parent.pop(kf, None)

    def set_links(self, kf, cov, children, parent):
        self.cov[kf] = [int(x) for x in cov][:10]
        self.children[kf] = sorted(int(x) for x in children)
        self.parent[kf] = int(parent)

    # ---- Tracking::UpdateLocalKeyFrames (:907-1015)
    def update_local_keyframes(self, cur_points, prev_kfs, max_kfs=80):
        """-> (mvpLocalKeyFrames, pKFmax or -1)"""
        counter = {}                                           # keyframeCounter
        for p in cur_points:                                   # :910-927, one pass per KEYPOINT
            if p < 0:
                continue
            if p in self.pt_bad:
                continue
            for kf in sorted(self.obs.get(p, {})):
                counter[kf] = counter.get(kf, 0) + 1
        if not counter:                                        # :929-930
            return list(prev_kfs), -1
        mx, kf_max = 0, -1
        local, marked = [], set()                              # marked: mnTrackReferenceForFrame == this frame
        for kf in sorted(counter):                             # :939-954
            if kf in self.kf_bad:
                continue
            if counter[kf] > mx:
                mx, kf_max = counter[kf], kf
            local.append(kf)
            marked.add(kf)
        n_voted = len(local)                                   # the end iterator is taken before anything is appended
        for i in range(n_voted):                               # :958-1008
            if len(local) > max_kfs:
                break
            kf = local[i]
            for nb in self.cov.get(kf, [])[:10]:
                if nb not in self.kf_bad:
                    if nb not in marked:
                        local.append(nb)
                        marked.add(nb)
                        break
            for ch in sorted(self.children.get(kf, [])):
                if ch not in self.kf_bad:
                    if ch not in marked:
                        local.append(ch)
                        marked.add(ch)
                        break
            par = self.parent.get(kf, -1)
            if par >= 0:                                       # no bad test; the break leaves the OUTER loop (:1004)
                if par not in marked:
                    local.append(par)
                    marked.add(par)
                    break
        return local, kf_max

    # ---- Tracking::UpdateLocalPoints (:881-905)
    def update_local_points(self, local_kfs):
        out, taken = [], set()                                 # taken: mnTrackReferenceForFrame == this frame
        for kf in local_kfs:                                   # no bad test on the keyframe
            for p in self.kf_points.get(kf, []):
                if p < 0:
                    continue
                if p in taken:
                    continue
                if p not in self.pt_bad:
                    out.append(p)
                    taken.add(p)
        return out

    # ---- Tracking::SearchLocalPoints, the two loops in front of isInFrustum (:806-834)
    def search_list(self, local_points, cur_points, seen_points):
        last_seen = set(int(p) for p in seen_points if p >= 0)  # stamped when TrackWithMotionModel dropped the match (:705-707)
        for p in cur_points:                                   # :806-823
            if p >= 0 and p not in self.pt_bad:
                last_seen.add(int(p))
        out = []
        for p in local_points:                                 # :827-834
            if p in last_seen:
                continue
            if p in self.pt_bad:
                continue
            out.append(p)
        return out

    def update_local_map(self, cur_points, seen_points=(), prev_kfs=(), max_kfs=80):
        cur = [int(p) for p in cur_points]
        kfs, ref = self.update_local_keyframes(cur, [int(k) for k in prev_kfs], max_kfs)
        pts = self.update_local_points(kfs)
        return dict(local_kfs=kfs, ref_kf=ref, local_rows=pts, search_rows=self.search_list(pts, cur, seen_points))

    # ---- KeyFrame::UpdateConnections (KeyFrame.cc:533-637)
    def shared_counts(self, kf):
        """KFcounter (:541-573) as (keyframe, count) in ascending id"""
        counter = {}
        for p in self.kf_points[kf]:
            if p < 0:
                continue
            if p in self.pt_bad:
                continue
            for other in sorted(self.obs.get(p, {})):
                if other == kf:
                    continue
                counter[other] = counter.get(other, 0) + 1
        return sorted(counter.items())

    def update_connections(self, kf, th=15):
        """-> (mvpOrderedConnectedKeyFrames, mvOrderedWeights), or ([], []) when KFcounter is empty (:577-637)"""
        counter = self.shared_counts(kf)
        if not counter:
            return [], []
        nmax, kf_max = 0, -1
        pairs = []
        for other, w in counter:
            if w > nmax:
                nmax, kf_max = w, other
            if w >= th:
                pairs.append((w, other))
        if not pairs:
            pairs.append((nmax, kf_max))
        pairs.sort()                                           # ascending (weight, keyframe); push_front reverses
        pairs.reverse()
        return [k for _, k in pairs], [w for w, _ in pairs]
