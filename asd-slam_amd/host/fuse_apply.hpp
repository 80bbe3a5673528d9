// fuse_apply.hpp -- the side-effect half of ORBmatcher::Fuse and MapPoint::Replace as asd_fuse_apply states them (include/asd_slam.h),
// over FLAT host tables: the keyframes' rows plus an observer list per point.  No device, no library: a caller without an observation
// table on the device uses it, tools/fuse_apply_times.py times it as the baseline, host/test_fuse_apply_rule.cpp runs it alone.
//
//   mode 0  Fuse(pKF, vpMapPoints, th), ORBmatcher.cc:842-957 without the search
//   mode 1  Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) :986-1083 + the loop of LoopClosing::SearchAndFuse, LoopClosing.cc:619-627
//   mode 2  the loop fusion of LoopClosing::CorrectLoop, LoopClosing.cc:540-555
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace asd {

struct FuseMap {
  std::vector<std::vector<int32_t>> rows;                          // per keyframe (by index): KeyFrame::mvpMapPoints as bank rows, -1 = none
  std::vector<std::vector<std::pair<int32_t, int32_t>>> obs;       // per bank row: MapPoint::mObservations as (keyframe index, keypoint index)
  std::vector<uint8_t> bad;                                        // per bank row: MapPoint::isBad()
  std::vector<uint32_t> stamp; uint32_t step = 0;                  // per keyframe: the Replace that met the winner there last

  void Reserve(int32_t row) {
    if (row >= (int32_t)obs.size()) { obs.resize((size_t)row + 1); bad.resize((size_t)row + 1, 0); }
  }
  // the observer lists from the rows (a point at most once per row: the table's precondition)
  void BuildObservers() {
    for (auto& o : obs) o.clear();
    for (size_t k = 0; k < rows.size(); ++k)
      for (size_t i = 0; i < rows[k].size(); ++i)
        if (rows[k][i] >= 0) { Reserve(rows[k][i]); obs[rows[k][i]].emplace_back((int32_t)k, (int32_t)i); }
    stamp.assign(rows.size(), 0u);
  }
  int32_t Observations(int32_t p) const { return p < (int32_t)obs.size() ? (int32_t)obs[p].size() : 0; }
  bool IsInKeyFrame(int32_t p, int32_t k) const {
    if (p >= (int32_t)obs.size()) return false;
    for (const auto& o : obs[p]) if (o.first == k) return true;
    return false;
  }
};

struct FuseApplyResult {
  std::vector<uint8_t> action;
  std::vector<int32_t> other, obs_cand, obs_other, n_moved, n_dropped;
  int32_t n_fused = 0;
};

// loser->Replace(winner), MapPoint.cc:206-244; false = both are the same point (:208-209)
inline bool FuseReplace(FuseMap& M, int32_t loser, int32_t winner, int32_t* moved, int32_t* dropped) {
  *moved = 0; *dropped = 0;
  if (loser == winner) return false;
  M.Reserve(loser > winner ? loser : winner);
  if (++M.step == 0) { M.stamp.assign(M.rows.size(), 0u); M.step = 1; }
  for (const auto& o : M.obs[winner]) M.stamp[o.first] = M.step;
  std::vector<std::pair<int32_t, int32_t>> obs;
  obs.swap(M.obs[loser]);                      // obs = mObservations; mObservations.clear()
  M.bad[loser] = 1;                            // mbBad = true
  for (const auto& o : obs) {
    if (M.stamp[o.first] != M.step) {          // !pMP->IsInKeyFrame(pKF): ReplaceMapPointMatch + AddObservation
      M.rows[o.first][o.second] = winner;
      M.obs[winner].push_back(o);
      ++*moved;
    } else {                                   // EraseMapPointMatch
      M.rows[o.first][o.second] = -1;
      ++*dropped;
    }
  }
  return true;
}

// asd_fuse_apply's rule over M for the keyframe with index k; apply = false works on a copy and leaves M as it was
inline FuseApplyResult FuseApplyRule(FuseMap& map, int32_t k, int mode, const int32_t* cand, const int32_t* best_idx, int32_t n, bool apply) {
  FuseMap copy;
  if (!apply) copy = map;
  FuseMap& M = apply ? map : copy;
  FuseApplyResult R;
  R.action.assign(n, 0); R.other.assign(n, -1); R.obs_cand.assign(n, 0); R.obs_other.assign(n, 0); R.n_moved.assign(n, 0); R.n_dropped.assign(n, 0);
  std::vector<int32_t>& row = M.rows[k];
  std::vector<int32_t> found;                  // spAlreadyFound, :979 (mode 1)
  if (mode == 1) for (const int32_t p : row) if (p >= 0) found.push_back(p);
  std::vector<uint8_t> in_found;
  if (mode == 1) { in_found.assign(M.obs.size(), 0); for (const int32_t p : found) in_found[p] = 1; }
  std::vector<int32_t> noted;                  // vpReplacePoint
  auto do_replace = [&](int32_t i, int32_t loser, int32_t winner) {
    R.obs_cand[i] = M.Observations(cand[i]); R.obs_other[i] = M.Observations(R.other[i]);
    if (!FuseReplace(M, loser, winner, &R.n_moved[i], &R.n_dropped[i])) R.action[i] = 5;
  };
  for (int32_t i = 0; i < n; ++i) {
    const int32_t p = cand[i], b = best_idx[i];
    if (p < 0 || b < 0) continue;
    M.Reserve(p);
    if (mode == 0 && (M.bad[p] || M.IsInKeyFrame(p, k))) { R.action[i] = 7; continue; }                              // :849
    if (mode == 1 && (M.bad[p] || (p < (int32_t)in_found.size() && in_found[p]))) { R.action[i] = 7; continue; }     // :992
    const int32_t q = row[b];
    if (q < 0) {
      R.obs_cand[i] = M.Observations(p);
      if (mode == 2 && M.IsInKeyFrame(p, k)) { R.action[i] = 6; continue; }   // not restated: the row would hold the point twice
      M.obs[p].emplace_back(k, b);             // AddObservation
      row[b] = p;                              // AddMapPoint
      R.action[i] = 1;
      continue;
    }
    R.other[i] = q;
    if (mode == 2) { R.action[i] = 3; do_replace(i, q, p); }
    else if (M.bad[q]) { R.action[i] = 4; R.obs_cand[i] = M.Observations(p); R.obs_other[i] = M.Observations(q); }   // :942 / :1073
    else if (mode == 1) { R.action[i] = 3; noted.push_back(i); }
    else if (M.Observations(q) > M.Observations(p)) { R.action[i] = 2; do_replace(i, p, q); }                        // :944-945
    else { R.action[i] = 3; do_replace(i, q, p); }
  }
  for (const int32_t i : noted) do_replace(i, R.other[i], cand[i]);           // LoopClosing.cc:619-627: no test at all
  for (int32_t i = 0; i < n; ++i) R.n_fused += R.action[i] >= 1 && R.action[i] <= 5;
  return R;
}

}  // namespace asd
