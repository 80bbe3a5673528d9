// normal_depth_cpu.cpp -- the host-side comparison of tools/normal_depth_times.py: MapPoint::SetWorldPos + MapPoint::UpdateNormalAndDepth
// (MapPoint.cc:361-407) for the points of one write-back, with the library's arithmetic (csrc/normal_depth.h, -ffp-contract=off), over
// FLAT tables -- the observers of every point handed over point-major, already in ascending keyframe id, which a host that walks
// mObservations has to build first.  No point is bad, every point has its reference keyframe among its observers.  One thread.
//
//   normal_depth_cpu FILE REPS     FILE: int32 n_kf, n_pts, n_obs; centres[n_kf][3] f32; Xw[n_pts][3] f32; start[n_pts + 1] int32;
//                                  obs_kf[n_obs] int32 (ascending per point); ref[n_pts] int32 (index into the point's observers);
//                                  scale_level[n_pts] f32; scale_top f32
// Prints JSON: update_ms (median) and a checksum over the bit patterns of normal, min and max.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../asd-slam_amd/csrc/normal_depth.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const int reps = atoi(argv[2]);
  int32_t h[3];
  if (fread(h, 4, 3, f) != 3) return 2;
  const int n_kf = h[0], n_pts = h[1], n_obs = h[2];
  std::vector<float> centre(3 * (size_t)n_kf), Xw(3 * (size_t)n_pts), scale_level(n_pts);
  std::vector<int32_t> start(n_pts + 1), obs(n_obs), ref(n_pts);
  float scale_top = 0.f;
  if (fread(centre.data(), 4, centre.size(), f) != centre.size() || fread(Xw.data(), 4, Xw.size(), f) != Xw.size() ||
      fread(start.data(), 4, start.size(), f) != start.size() || fread(obs.data(), 4, obs.size(), f) != obs.size() ||
      fread(ref.data(), 4, ref.size(), f) != ref.size() || fread(scale_level.data(), 4, scale_level.size(), f) != scale_level.size() ||
      fread(&scale_top, 4, 1, f) != 1)
    return 2;
  fclose(f);
  std::vector<float> bank(8 * (size_t)n_pts, 0.f);   // mWorldPos, mNormalVector, mfMinDistance, mfMaxDistance per point
  std::vector<double> t;
  for (int rep = 0; rep < reps; ++rep) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int p = 0; p < n_pts; ++p) {
      float* row = bank.data() + 8 * (size_t)p;
      row[0] = Xw[3 * (size_t)p]; row[1] = Xw[3 * (size_t)p + 1]; row[2] = Xw[3 * (size_t)p + 2];   // SetWorldPos
      float sum[3] = {0.f, 0.f, 0.f}, unit[3];
      double nrm_ref = 0.0;
      const int n = start[p + 1] - start[p];
      for (int k = 0; k < n; ++k) {
        const double nrm = asd_nd_unit(row, centre.data() + 3 * (size_t)obs[start[p] + k], unit);
        asd_nd_add(sum, unit);
        if (k == ref[p]) nrm_ref = nrm;
      }
      asd_nd_finish(sum, n, nrm_ref, scale_level[p], scale_top, row + 3, row + 6, row + 7);
    }
    const auto t1 = std::chrono::steady_clock::now();
    t.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
  }
  long long checksum = 0;
  for (int p = 0; p < n_pts; ++p)
    for (int k = 3; k < 8; ++k) {
      uint32_t u;
      memcpy(&u, &bank[8 * (size_t)p + k], 4);
      checksum = (checksum + (long long)(u % 1000003u) * (long long)((p * 5 + k) % 89 + 1)) % 2147483647ll;
    }
  std::sort(t.begin(), t.end());
  printf("{\"update_ms\": %.6f, \"checksum\": %lld}\n", t[t.size() / 2], checksum);
  return 0;
}
