// test_gba.cpp -- probe for asd::Optimizer::BundleAdjustment / GlobalBundleAdjustemnt and asd::Tracking::InitialMapScale
// (asd_adapters.hpp); tests/test_gba_host.py reads its output.
//
//   test_gba PROBLEM_FILE
//     on the device.  The file (text; floats as C99 hex): "nKF nMP nIterations bRobust", K[4]; per keyframe "mnId bad in_set", Tcw[16],
//     "nKeys nLevels", per key "x y octave", mvInvLevelSigma2[nLevels]; per map point "mnId bad", Xw[3], "nObs", per observation
//     "keyframe keypoint".  Prints JSON: rc, iterations, trials, n_edges, chi2, kf_written, mp_written, not_included, Tcw, Xw.
//   test_gba --scale FILE
//     no device.  The file: TcwIni[16], TcwCur[16], "nKeys nPoints nTracked", iniPoints[nKeys], Xw[3 nPoints].  Prints JSON: ok, median,
//     TcwCur, Xw.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "asd_adapters.hpp"

namespace {

bool read_floats(FILE* f, float* out, size_t n) {
  for (size_t i = 0; i < n; ++i) if (fscanf(f, "%a", out + i) != 1) return false;
  return true;
}

void print_floats(const char* name, const float* v, size_t n, bool last = false) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < n; ++i) printf("%s\"%a\"", i ? ", " : "", (double)v[i]);
  printf("]%s", last ? "" : ", ");
}

void print_bytes(const char* name, const std::vector<uint8_t>& v) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", (int)v[i]);
  printf("], ");
}

int scale_mode(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
  float TcwIni[16], TcwCur[16];
  int nKeys = 0, nPoints = 0, nTracked = 0;
  if (!read_floats(f, TcwIni, 16) || !read_floats(f, TcwCur, 16) || fscanf(f, "%d %d %d", &nKeys, &nPoints, &nTracked) != 3) return 2;
  std::vector<int32_t> ini(nKeys);
  for (int32_t& x : ini) if (fscanf(f, "%d", &x) != 1) return 2;
  std::vector<float> Xw((size_t)nPoints * 3);
  if (!read_floats(f, Xw.data(), Xw.size())) return 2;
  fclose(f);
  float median = 0;
  const bool ok = asd::Tracking::InitialMapScale(TcwIni, TcwCur, ini, Xw, nTracked, &median);
  printf("{\"ok\": %d, \"median\": \"%a\", ", (int)ok, (double)median);
  print_floats("TcwCur", TcwCur, 16);
  print_floats("Xw", Xw.data(), Xw.size(), true);
  printf("}\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "--scale")) return scale_mode(argv[2]);
  if (argc < 2) { fprintf(stderr, "usage: %s PROBLEM_FILE | --scale FILE\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int nKF = 0, nMP = 0, nIterations = 0, bRobust = 0;
  asd::Camera K{};
  if (fscanf(f, "%d %d %d %d", &nKF, &nMP, &nIterations, &bRobust) != 4 || !read_floats(f, &K.fx, 1) || !read_floats(f, &K.fy, 1) ||
      !read_floats(f, &K.cx, 1) || !read_floats(f, &K.cy, 1))
    return 2;
  std::vector<asd::Optimizer::BAKeyFrame> kfs(nKF);
  std::vector<std::vector<asd_keypoint>> keys(nKF);
  std::vector<std::vector<float>> sigma(nKF);
  for (int i = 0; i < nKF; ++i) {
    unsigned long id = 0;
    int bad = 0, in_set = 0, nKeys = 0, nLevels = 0;
    if (fscanf(f, "%lu %d %d", &id, &bad, &in_set) != 3 || !read_floats(f, kfs[i].Tcw, 16) || fscanf(f, "%d %d", &nKeys, &nLevels) != 2) return 2;
    kfs[i].mnId = id; kfs[i].bad = bad != 0; kfs[i].in_set = in_set != 0;
    keys[i].assign(nKeys, asd_keypoint{});
    for (asd_keypoint& k : keys[i]) {
      int oct = 0;
      if (!read_floats(f, &k.x, 1) || !read_floats(f, &k.y, 1) || fscanf(f, "%d", &oct) != 1) return 2;
      k.octave = oct;
    }
    sigma[i].resize(nLevels);
    if (!read_floats(f, sigma[i].data(), sigma[i].size())) return 2;
    kfs[i].mvKeysUn = &keys[i]; kfs[i].mvInvLevelSigma2 = &sigma[i];
  }
  std::vector<asd::Optimizer::BAMapPoint> mps(nMP);
  for (int i = 0; i < nMP; ++i) {
    unsigned long id = 0;
    int bad = 0, nObs = 0;
    if (fscanf(f, "%lu %d", &id, &bad) != 2 || !read_floats(f, mps[i].Xw, 3) || fscanf(f, "%d", &nObs) != 1) return 2;
    mps[i].mnId = id; mps[i].bad = bad != 0;
    for (int o = 0; o < nObs; ++o) {
      int kf = 0;
      unsigned long idx = 0;
      if (fscanf(f, "%d %lu", &kf, &idx) != 2 || kf < 0 || kf >= nKF || idx >= keys[kf].size()) return 2;
      mps[i].observations.emplace_back(kf, (size_t)idx);
    }
  }
  fclose(f);
  try {
    asd::Context ctx(500, 1.2f, 8, 20, 7, 640, 480);
    const asd::Optimizer::BAResult r = asd::Optimizer::GlobalBundleAdjustemnt(ctx, kfs, mps, K, nIterations, nullptr, bRobust != 0);
    printf("{\"rc\": %d, \"iterations\": %d, \"trials\": %d, \"n_edges\": %d, \"chi2\": \"%a\", ", r.rc, r.iterations, r.trials, r.n_edges, r.chi2);
    print_bytes("kf_written", r.kf_written);
    print_bytes("mp_written", r.mp_written);
    print_bytes("not_included", r.vbNotIncludedMP);
    print_floats("Tcw", r.Tcw.data(), r.Tcw.size());
    print_floats("Xw", r.Xw.data(), r.Xw.size(), true);
    printf("}\n");
    if (r.rc != ASD_OK) fprintf(stderr, "asd_bundle_adjustment: %s\n", ctx.error());
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
