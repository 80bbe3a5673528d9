// local_ba_graph_cpu.cpp -- the host-side comparison of tools/local_ba_graph_times.py: the lists and edges of LocalBundleAdjustment and its
// erase policy, as include/asd_slam.h states them for asd_local_ba_graph / asd_local_ba_apply, over FLAT host tables: the keyframes' rows
// keyframe-major and every point's observations point-major in ascending keyframe id (what a host keeps as mObservations; built before the
// clock starts).  Sequential stamps and one erased pair after the other, one thread.  Keyframe k of the file has the id k + 1.
//
//   local_ba_graph_cpu FILE REPS   FILE: int32 n_kf, n_kp, n_rows, kf, n_neigh; rows[n_kf][n_kp] int32; octave[n_kf][n_kp] u8;
//                                  kf_bad[n_kf] u8; pt_bad[n_rows] u8; neigh[n_neigh] int32 (keyframe indices)
// Edge e is flagged when e % 20 == 7.  Prints JSON: graph_ms and erase_ms (medians), the counts, and a checksum per step.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {
struct Sum {
  long long cs = 0, i = 0;
  void add(long long v) { cs = (cs + ((v + 1) % 1000003ll) * (i % 89 + 1)) % 2147483647ll; ++i; }
};
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const int reps = atoi(argv[2]);
  int32_t h[5];
  if (fread(h, 4, 5, f) != 5) return 2;
  const int n_kf = h[0], n_kp = h[1], n_rows = h[2], kf0 = h[3], n_neigh = h[4];
  const size_t n_ent = (size_t)n_kf * n_kp;
  std::vector<int32_t> rows(n_ent), neigh(n_neigh);
  std::vector<uint8_t> octave(n_ent), kf_bad(n_kf), pt_bad0(n_rows);
  if (fread(rows.data(), 4, n_ent, f) != n_ent || fread(octave.data(), 1, n_ent, f) != n_ent || fread(kf_bad.data(), 1, n_kf, f) != (size_t)n_kf ||
      fread(pt_bad0.data(), 1, n_rows, f) != (size_t)n_rows || fread(neigh.data(), 4, n_neigh, f) != (size_t)n_neigh)
    return 2;
  fclose(f);
  // mObservations: per point (keyframe, keypoint index) in ascending keyframe
  std::vector<int32_t> start(n_rows + 1, 0);
  for (size_t e = 0; e < n_ent; ++e) if (rows[e] >= 0) ++start[rows[e] + 1];
  for (int r = 0; r < n_rows; ++r) start[r + 1] += start[r];
  std::vector<int32_t> obs_kf(start[n_rows]), obs_idx(start[n_rows]), fill(start.begin(), start.end() - 1);
  for (int k = 0; k < n_kf; ++k)
    for (int i = 0; i < n_kp; ++i) {
      const int r = rows[(size_t)k * n_kp + i];
      if (r >= 0) { obs_kf[fill[r]] = k; obs_idx[fill[r]] = i; ++fill[r]; }
    }
  std::vector<int32_t> ba_local_kf(n_kf, -1), ba_fixed_kf(n_kf, -1), ba_local_mp(n_rows, -1);
  std::vector<int32_t> local_kfs, local_rows, fixed_kfs, pose_kfs, point_rank, e_point, e_pose, e_kf, e_idx, e_oct, pose_of(n_kf), rank_of(n_rows), sorted_rows;
  std::vector<uint8_t> pose_fixed;
  std::vector<double> tg, te;
  Sum sg, se;
  int n_erased = 0;
  std::vector<int32_t> bad_rows, new_ref;
  for (int rep = 0; rep < reps; ++rep) {
    const int stamp = rep;   // (a fresh mnId per call, as the reference's stamps)
    auto t0 = std::chrono::steady_clock::now();
    local_kfs.clear(); local_rows.clear(); fixed_kfs.clear(); pose_kfs.clear(); pose_fixed.clear(); point_rank.clear();
    e_point.clear(); e_pose.clear(); e_kf.clear(); e_idx.clear(); e_oct.clear();
    local_kfs.push_back(kf0); ba_local_kf[kf0] = stamp;
    for (int k : neigh) { ba_local_kf[k] = stamp; if (!kf_bad[k]) local_kfs.push_back(k); }
    for (int k : local_kfs)
      for (int i = 0; i < n_kp; ++i) {
        const int r = rows[(size_t)k * n_kp + i];
        if (r >= 0 && !pt_bad0[r] && ba_local_mp[r] != stamp) { local_rows.push_back(r); ba_local_mp[r] = stamp; }
      }
    for (int r : local_rows)
      for (int o = start[r]; o < start[r + 1]; ++o) {
        const int k = obs_kf[o];
        if (ba_local_kf[k] != stamp && ba_fixed_kf[k] != stamp) { ba_fixed_kf[k] = stamp; if (!kf_bad[k]) fixed_kfs.push_back(k); }
      }
    pose_kfs = local_kfs; pose_kfs.insert(pose_kfs.end(), fixed_kfs.begin(), fixed_kfs.end());
    std::sort(pose_kfs.begin(), pose_kfs.end());
    for (size_t i = 0; i < pose_kfs.size(); ++i) { pose_of[pose_kfs[i]] = (int)i; pose_fixed.push_back(ba_local_kf[pose_kfs[i]] != stamp); }
    sorted_rows = local_rows;
    std::sort(sorted_rows.begin(), sorted_rows.end());
    for (size_t i = 0; i < sorted_rows.size(); ++i) rank_of[sorted_rows[i]] = (int)i;
    for (int r : local_rows) {
      point_rank.push_back(rank_of[r]);
      for (int o = start[r]; o < start[r + 1]; ++o) {
        const int k = obs_kf[o];
        if (kf_bad[k]) continue;
        e_point.push_back(rank_of[r]); e_pose.push_back(pose_of[k]); e_kf.push_back(k + 1); e_idx.push_back(obs_idx[o]);
        e_oct.push_back(octave[(size_t)k * n_kp + obs_idx[o]]);
      }
    }
    auto t1 = std::chrono::steady_clock::now();
    tg.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    // the erase policy on copies made outside the clock (the tables stay as they are for the next repetition)
    std::vector<int32_t> rows_w(rows), n_obs(n_rows);
    std::vector<uint8_t> pt_bad(pt_bad0), gone(obs_kf.size(), 0);
    for (int r = 0; r < n_rows; ++r) n_obs[r] = start[r + 1] - start[r];
    const size_t E = e_kf.size();
    t0 = std::chrono::steady_clock::now();
    n_erased = 0; bad_rows.clear(); new_ref.assign(local_rows.size(), -1);
    std::vector<uint8_t> lost(local_rows.size(), 0);
    for (size_t e = 0; e < E; ++e) {
      if (e % 20 != 7) continue;
      const int r = sorted_rows[e_point[e]], k = e_kf[e] - 1;
      if (pt_bad[r]) continue;                                   // the observations are gone: both calls are no-ops
      rows_w[(size_t)k * n_kp + e_idx[e]] = -1;                  // EraseMapPointMatch
      for (int o = start[r]; o < start[r + 1]; ++o) if (obs_kf[o] == k) gone[o] = 1;   // EraseObservation
      --n_obs[r]; ++n_erased;
      if (n_obs[r] <= 2) {                                       // SetBadFlag
        pt_bad[r] = 1; bad_rows.push_back(r);
        for (int o = start[r]; o < start[r + 1]; ++o) if (!gone[o]) rows_w[(size_t)obs_kf[o] * n_kp + obs_idx[o]] = -1;
      }
    }
    for (size_t e = 0; e < E; ++e) if (e % 20 == 7) lost[e_point[e]] = 1;   // (by rank)
    for (size_t i = 0; i < local_rows.size(); ++i) {
      const int r = local_rows[i];
      if (!lost[rank_of[r]] || pt_bad[r]) continue;
      for (int o = start[r]; o < start[r + 1]; ++o) if (!gone[o]) { new_ref[i] = obs_kf[o] + 1; break; }
    }
    t1 = std::chrono::steady_clock::now();
    te.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
  }
  for (int v : local_kfs) sg.add(v + 1);
  for (int v : local_rows) sg.add(v);
  for (int v : fixed_kfs) sg.add(v + 1);
  for (int v : pose_kfs) sg.add(v + 1);
  for (int v : pose_fixed) sg.add(v);
  for (int v : point_rank) sg.add(v);
  for (size_t e = 0; e < e_kf.size(); ++e) { sg.add(e_point[e]); sg.add(e_pose[e]); sg.add(e_kf[e]); sg.add(e_idx[e]); sg.add(e_oct[e]); }
  se.add(n_erased);
  for (int v : bad_rows) se.add(v);
  for (int v : new_ref) se.add(v);
  std::sort(tg.begin(), tg.end());
  std::sort(te.begin(), te.end());
  printf("{\"graph_ms\": %.6f, \"erase_ms\": %.6f, \"points\": %zu, \"fixed\": %zu, \"poses\": %zu, \"edges\": %zu, \"erased\": %d, \"bad\": %zu, "
         "\"graph_checksum\": %lld, \"erase_checksum\": %lld}\n",
         tg[tg.size() / 2], te[te.size() / 2], local_rows.size(), fixed_kfs.size(), pose_kfs.size(), e_kf.size(), n_erased, bad_rows.size(), sg.cs, se.cs);
  return 0;
}
