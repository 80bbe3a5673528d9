// test_essential_graph.cpp -- probe for asd::Optimizer::OptimizeEssentialGraph (asd_adapters.hpp); tests/test_essgraph_host.py and
// tests/test_essgraph.py read its output.
//
//   test_essential_graph PROBLEM_FILE
//     on the device.  The file (text; floats and doubles as C99 hex): "nKF nMP nLC pLoopKF pCurKF bFixScale nIterations"; per keyframe
//     "mnId parent hasCorrected hasNonCorrected", Tcw[16], corrected[8], nonCorrected[8], "nChildren" children, "nLoopEdges" loop edges,
//     "nCovisibles" then "keyframe weight" each; per LoopConnections entry "keyframe n" and n keyframes; per map point Xw[3],
//     "refKF mnCorrectedByKF mnCorrectedReference".  Prints JSON: rc, iterations, trials, n_edges, chi2, sim3, Tcw, Xw.
//   test_essential_graph --edges PROBLEM_FILE
//     no device.  Prints JSON: the flat problem of asd::Optimizer::EssentialGraphProblem -- e_i, e_j, fixed, sim3, e_meas.
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
bool read_doubles(FILE* f, double* out, size_t n) {
  for (size_t i = 0; i < n; ++i) if (fscanf(f, "%la", out + i) != 1) return false;
  return true;
}
bool read_ints(FILE* f, std::vector<int>& out) {
  int n = 0;
  if (fscanf(f, "%d", &n) != 1 || n < 0) return false;
  out.resize(n);
  for (int& v : out) if (fscanf(f, "%d", &v) != 1) return false;
  return true;
}

template <class T>
void print_hex(const char* name, const T* v, size_t n, bool last = false) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < n; ++i) printf("%s\"%a\"", i ? ", " : "", (double)v[i]);
  printf("]%s", last ? "" : ", ");
}
template <class T>
void print_ints(const char* name, const std::vector<T>& v) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", (int)v[i]);
  printf("], ");
}

}  // namespace

int main(int argc, char** argv) {
  const bool edges_only = argc >= 3 && !strcmp(argv[1], "--edges");
  if (argc < 2 || (argc < 3 && !strcmp(argv[1], "--edges"))) { fprintf(stderr, "usage: %s [--edges] PROBLEM_FILE\n", argv[0]); return 2; }
  const char* path = argv[edges_only ? 2 : 1];
  FILE* f = fopen(path, "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
  int nKF = 0, nMP = 0, nLC = 0, pLoopKF = 0, pCurKF = 0, bFixScale = 0, nIterations = 0;
  if (fscanf(f, "%d %d %d %d %d %d %d", &nKF, &nMP, &nLC, &pLoopKF, &pCurKF, &bFixScale, &nIterations) != 7 || nKF < 0 || nMP < 0 || nLC < 0) return 2;
  auto kf_ok = [&](int k) { return k >= 0 && k < nKF; };
  std::vector<asd::Optimizer::EGKeyFrame> kfs(nKF);
  for (asd::Optimizer::EGKeyFrame& kf : kfs) {
    int hc = 0, hn = 0, nCov = 0;
    if (fscanf(f, "%lu %d %d %d", &kf.mnId, &kf.parent, &hc, &hn) != 4 || !read_floats(f, kf.Tcw, 16) || !read_doubles(f, kf.corrected.v, 8) ||
        !read_doubles(f, kf.nonCorrected.v, 8) || !read_ints(f, kf.children) || !read_ints(f, kf.loopEdges) || fscanf(f, "%d", &nCov) != 1 || nCov < 0)
      return 2;
    kf.hasCorrected = hc != 0; kf.hasNonCorrected = hn != 0;
    kf.covisibles.resize(nCov);
    for (std::pair<int, int>& c : kf.covisibles) if (fscanf(f, "%d %d", &c.first, &c.second) != 2 || !kf_ok(c.first)) return 2;
    if (kf.parent < -1 || kf.parent >= nKF) return 2;
    for (int k : kf.children) if (!kf_ok(k)) return 2;
    for (int k : kf.loopEdges) if (!kf_ok(k)) return 2;
  }
  if (nKF > 0 && (!kf_ok(pLoopKF) || !kf_ok(pCurKF))) return 2;
  asd::Optimizer::EGLoopConnections lc(nLC);
  for (std::pair<int, std::vector<int>>& m : lc) {
    if (fscanf(f, "%d", &m.first) != 1 || !kf_ok(m.first) || !read_ints(f, m.second)) return 2;
    for (int k : m.second) if (!kf_ok(k)) return 2;
  }
  std::vector<asd::Optimizer::EGMapPoint> mps(nMP);
  for (asd::Optimizer::EGMapPoint& mp : mps)
    if (!read_floats(f, mp.Xw, 3) || fscanf(f, "%d %lu %lu", &mp.refKF, &mp.mnCorrectedByKF, &mp.mnCorrectedReference) != 3 || !kf_ok(mp.refKF)) return 2;
  fclose(f);
  if (edges_only) {
    const asd::Optimizer::EGProblem p = asd::Optimizer::EssentialGraphProblem(kfs, pLoopKF, pCurKF, lc);
    printf("{");
    print_ints("e_i", p.e_i);
    print_ints("e_j", p.e_j);
    print_ints("fixed", p.fixed);
    print_hex("sim3", p.sim3.data(), p.sim3.size());
    print_hex("e_meas", p.e_meas.data(), p.e_meas.size(), true);
    printf("}\n");
    return 0;
  }
  try {
    asd::Context ctx(500, 1.2f, 8, 20, 7, 640, 480);
    const asd::Optimizer::EGResult r = asd::Optimizer::OptimizeEssentialGraph(ctx, kfs, mps, pLoopKF, pCurKF, lc, bFixScale != 0, nIterations);
    printf("{\"rc\": %d, \"iterations\": %d, \"trials\": %d, \"n_edges\": %d, \"chi2\": \"%a\", ", r.rc, r.iterations, r.trials, r.n_edges, r.chi2);
    print_hex("sim3", r.sim3.data(), r.sim3.size());
    print_hex("Tcw", r.Tcw.data(), r.Tcw.size());
    print_hex("Xw", r.Xw.data(), r.Xw.size(), true);
    printf("}\n");
    if (r.rc != ASD_OK) fprintf(stderr, "asd_optimize_essential_graph: %s\n", ctx.error());
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
