// local_map_cpu.cpp -- the host-side comparison of tools/local_map_times.py: Tracking::UpdateLocalMap with SearchLocalPoints' skip loop
// (Tracking.cc:827-841, :871-1015) and KFcounter of KeyFrame::UpdateConnections (KeyFrame.cc:541-573), restated in C++ over FLAT tables
// (the keyframes' rows as one array, the observations as a CSR list per point in ascending keyframe) -- not over the reference's
// pointer graph, whose std::map copies per matched point cost more than this.  Same rules as tests/local_map_ref.py.
//
//   local_map_cpu FILE REPS      FILE: int32 n_kf, n_kp, n_rows, n_cur, n_seen, kf_counts; rows[n_kf][n_kp]; cur[n_cur]; seen[n_seen]
//   (keyframe ids are 0 .. n_kf-1; covisibles of k: k-1, k+1, k-2, k+2, ..., k-5, k+5 inside the range; child k+1; parent k-1; nothing bad)
// Prints JSON: update_local_map_ms, shared_counts_ms (medians), the counts and a checksum of the lists.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const int reps = atoi(argv[2]);
  int32_t h[6];
  if (fread(h, 4, 6, f) != 6) return 2;
  const int n_kf = h[0], n_kp = h[1], n_rows = h[2], n_cur = h[3], n_seen = h[4], kf_counts = h[5];
  std::vector<int32_t> rows((size_t)n_kf * n_kp), cur(n_cur), seen(n_seen);
  if (fread(rows.data(), 4, rows.size(), f) != rows.size() || fread(cur.data(), 4, n_cur, f) != (size_t)n_cur || fread(seen.data(), 4, n_seen, f) != (size_t)n_seen) return 2;
  fclose(f);
  // MapPoint::mObservations as CSR: point -> keyframes ascending
  std::vector<int> start(n_rows + 1, 0);
  for (int32_t r : rows) if (r >= 0) ++start[r + 1];
  for (int i = 0; i < n_rows; ++i) start[i + 1] += start[i];
  std::vector<int> obs(start[n_rows]), fill(start.begin(), start.end() - 1);
  for (int k = 0; k < n_kf; ++k)
    for (int i = 0; i < n_kp; ++i) { const int r = rows[(size_t)k * n_kp + i]; if (r >= 0) obs[fill[r]++] = k; }
  std::vector<int> counter(n_kf, 0), kf_stamp(n_kf, 0), pt_stamp(n_rows, 0), seen_stamp(n_rows, 0);
  std::vector<int> voted, local, points, search;
  std::vector<double> t_map, t_cnt;
  long long checksum = 0;
  int n_counts = 0;
  for (int rep = 1; rep <= reps; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    voted.clear(); local.clear(); points.clear(); search.clear();
    for (int p : cur) {
      if (p < 0) continue;
      for (int o = start[p]; o < start[p + 1]; ++o) { if (!counter[obs[o]]++) voted.push_back(obs[o]); }
    }
    std::sort(voted.begin(), voted.end());   // keyframeCounter walks in ascending keyframe
    int mx = 0, ref = -1;
    for (int k : voted) { if (counter[k] > mx) { mx = counter[k]; ref = k; } local.push_back(k); kf_stamp[k] = rep; }
    const size_t n0 = local.size();
    for (size_t i = 0; i < n0; ++i) {
      if (local.size() > 80) break;
      const int k = local[i];
      for (int d = 1; d <= 5; ++d) {
        bool took = false;
        for (int nb : {k - d, k + d})
          if (nb >= 0 && nb < n_kf && kf_stamp[nb] != rep) { local.push_back(nb); kf_stamp[nb] = rep; took = true; break; }
        if (took) break;
      }
      if (k + 1 < n_kf && kf_stamp[k + 1] != rep) { local.push_back(k + 1); kf_stamp[k + 1] = rep; }
      if (k - 1 >= 0 && kf_stamp[k - 1] != rep) { local.push_back(k - 1); kf_stamp[k - 1] = rep; break; }
    }
    for (int k : voted) counter[k] = 0;
    for (int p : cur) if (p >= 0) seen_stamp[p] = rep;
    for (int p : seen) seen_stamp[p] = rep;
    for (int k : local)
      for (int i = 0; i < n_kp; ++i) {
        const int r = rows[(size_t)k * n_kp + i];
        if (r < 0 || pt_stamp[r] == rep) continue;
        pt_stamp[r] = rep;
        points.push_back(r);
      }
    for (int r : points) if (seen_stamp[r] != rep) search.push_back(r);
    const auto t1 = std::chrono::steady_clock::now();
    t_map.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    if (rep == reps) {
      checksum = (long long)local.size() + 3ll * points.size() + 7ll * search.size() + ref;
      for (size_t i = 0; i < points.size(); ++i) checksum = (checksum + (long long)points[i] * (long long)(i % 97 + 1)) % 2147483647ll;
      for (size_t i = 0; i < local.size(); ++i) checksum = (checksum + (long long)local[i] * (long long)(i % 89 + 1)) % 2147483647ll;
    }
    // KFcounter of keyframe kf_counts
    const auto t2 = std::chrono::steady_clock::now();
    voted.clear();
    for (int i = 0; i < n_kp; ++i) {
      const int p = rows[(size_t)kf_counts * n_kp + i];
      if (p < 0) continue;
      for (int o = start[p]; o < start[p + 1]; ++o) { if (obs[o] != kf_counts && !counter[obs[o]]++) voted.push_back(obs[o]); }
    }
    std::sort(voted.begin(), voted.end());
    n_counts = (int)voted.size();
    long long cs = 0;
    for (int k : voted) { cs += (long long)k * counter[k]; counter[k] = 0; }
    const auto t3 = std::chrono::steady_clock::now();
    t_cnt.push_back(std::chrono::duration<double, std::milli>(t3 - t2).count());
    if (rep == reps) checksum = (checksum + cs) % 2147483647ll;
  }
  std::sort(t_map.begin(), t_map.end());
  std::sort(t_cnt.begin(), t_cnt.end());
  printf("{\"update_local_map_ms\": %.6f, \"shared_counts_ms\": %.6f, \"n_local_kfs\": %zu, \"n_local\": %zu, \"n_search\": %zu, \"n_counts\": %d, \"checksum\": %lld}\n",
         t_map[t_map.size() / 2], t_cnt[t_cnt.size() / 2], local.size(), points.size(), search.size(), n_counts, checksum);
  return 0;
}
