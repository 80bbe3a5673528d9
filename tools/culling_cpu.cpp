// culling_cpu.cpp -- the host-side comparison of tools/culling_times.py: LocalMapping::KeyFrameCulling (LocalMapping.cc:739-809,
// monocular) with the in-loop SetBadFlag's effect on the observations, restated in C++ over FLAT tables (the keyframes' rows and octaves
// as two arrays, the observations as a CSR list of (keyframe, keypoint) per point) -- not over the reference's pointer graph, whose
// std::map copy per map point costs more than this.  One thread.  Same rules as tests/culling_ref.py; nothing is applied: a culled
// keyframe and a point turned bad are stamped for the length of one call, as asd_keyframe_culling with apply = 0 leaves the table alone.
//
//   culling_cpu FILE REPS     FILE: int32 n_kf, n_kp, n_rows, n_cand; rows[n_kf][n_kp] int32; octaves[n_kf][n_kp] uint8; cand[n_cand] int32
//   (keyframes are 0 .. n_kf-1, none is skipped, no point is bad at the start)
// Prints JSON: culling_ms (median), the number culled and turned bad, and a checksum of decisions, counts and bad rows.
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
  int32_t h[4];
  if (fread(h, 4, 4, f) != 4) return 2;
  const int n_kf = h[0], n_kp = h[1], n_rows = h[2], n_cand = h[3];
  std::vector<int32_t> rows((size_t)n_kf * n_kp), cand(n_cand);
  std::vector<uint8_t> oct((size_t)n_kf * n_kp);
  if (fread(rows.data(), 4, rows.size(), f) != rows.size() || fread(oct.data(), 1, oct.size(), f) != oct.size() ||
      fread(cand.data(), 4, n_cand, f) != (size_t)n_cand)
    return 2;
  fclose(f);
  // MapPoint::mObservations as CSR: point -> entries (keyframe * n_kp + keypoint)
  std::vector<int> start(n_rows + 1, 0);
  for (int32_t r : rows) if (r >= 0) ++start[r + 1];
  for (int i = 0; i < n_rows; ++i) start[i + 1] += start[i];
  std::vector<int64_t> obs(start[n_rows]);
  std::vector<int> fill(start.begin(), start.end() - 1);
  for (int k = 0; k < n_kf; ++k)
    for (int i = 0; i < n_kp; ++i) { const int r = rows[(size_t)k * n_kp + i]; if (r >= 0) obs[fill[r]++] = (int64_t)k * n_kp + i; }
  std::vector<int> kf_gone(n_kf, 0), pt_gone(n_rows, 0);
  std::vector<int> decision(n_cand), n_mps(n_cand), n_red(n_cand), bad;
  std::vector<double> t;
  for (int rep = 1; rep <= reps; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    bad.clear();
    for (int c = 0; c < n_cand; ++c) {
      const int kf = cand[c];
      const int32_t* row = rows.data() + (size_t)kf * n_kp;
      const uint8_t* lv = oct.data() + (size_t)kf * n_kp;
      int nm = 0, nr = 0;
      for (int i = 0; i < n_kp; ++i) {
        const int p = row[i];
        if (p < 0 || pt_gone[p] == rep) continue;
        ++nm;
        int total = 0, n = 0;
        for (int o = start[p]; o < start[p + 1]; ++o) {
          const int other = (int)(obs[o] / n_kp);
          if (kf_gone[other] == rep) continue;
          ++total;
          if (other != kf && oct[obs[o]] <= lv[i] + 1) ++n;
        }
        if (total > 3 && n >= 3) ++nr;
      }
      n_mps[c] = nm; n_red[c] = nr;
      decision[c] = 10 * nr > 9 * nm;
      if (!decision[c]) continue;
      kf_gone[kf] = rep;
      for (int i = 0; i < n_kp; ++i) {
        const int p = row[i];
        if (p < 0 || pt_gone[p] == rep) continue;
        int total = 0;
        for (int o = start[p]; o < start[p + 1]; ++o) total += kf_gone[(int)(obs[o] / n_kp)] != rep;
        if (total <= 2) { pt_gone[p] = rep; bad.push_back(p); }
      }
    }
    const auto t1 = std::chrono::steady_clock::now();
    t.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
  }
  long long checksum = 0, culled = 0;
  for (int c = 0; c < n_cand; ++c) {
    checksum = (checksum + (long long)(decision[c] + 3 * n_mps[c] + 7 * n_red[c]) * (c % 97 + 1)) % 2147483647ll;
    culled += decision[c];
  }
  for (size_t i = 0; i < bad.size(); ++i) checksum = (checksum + (long long)bad[i] * (long long)(i % 89 + 1)) % 2147483647ll;
  std::sort(t.begin(), t.end());
  printf("{\"culling_ms\": %.6f, \"culled\": %lld, \"n_bad\": %zu, \"checksum\": %lld}\n", t[t.size() / 2], culled, bad.size(), checksum);
  return 0;
}
