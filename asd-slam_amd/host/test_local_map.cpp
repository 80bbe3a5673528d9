// test_local_map.cpp -- probe for asd::Tracking::UpdateLocalMap and asd::KeyFrame::UpdateConnections (asd_adapters.hpp) over the
// context's observation table; tests/test_local_map_host.py reads its output.
//
//   test_local_map PROBLEM_FILE
//     The file (text, integers): "nKF nBadPoints"; per keyframe "mnId bad parent nKeys nCov nChildren", the row (nKeys bank rows, -1 =
//     none), GetBestCovisibilityKeyFrames(10) as ids, GetChilds() as ids ascending; the bad points' rows; "nQueries", per query
//     "nCur nSeen nPrev maxKeyFrames", mCurrentFrame.mvpMapPoints as rows, the rows stamped with mnLastFrameSeen, mvpLocalKeyFrames;
//     "nConnections" and that many keyframe ids.  Prints JSON: queries [{rc, local_kfs, ref_kf, local_rows, search_rows}], connections
//     [{rc, kfs, weights, ordered, ordered_weights, kf_max, best}].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "asd_adapters.hpp"

namespace {

bool read_ints(FILE* f, std::vector<int32_t>& v, size_t n) {
  v.resize(n);
  for (size_t i = 0; i < n; ++i) if (fscanf(f, "%d", &v[i]) != 1) return false;
  return true;
}

void print_ints(const char* name, const std::vector<int32_t>& v, bool last = false) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", v[i]);
  printf("]%s", last ? "" : ", ");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s PROBLEM_FILE\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  try {
    asd::Context ctx(500, 1.2f, 8, 20, 7, 640, 480);
    int nKF = 0, nBad = 0;
    if (fscanf(f, "%d %d", &nKF, &nBad) != 2) return 2;
    struct Links { int32_t id, bad, parent; std::vector<int32_t> cov, children; };
    std::vector<Links> links(nKF);
    for (Links& L : links) {
      int nKeys = 0, nCov = 0, nCh = 0;
      std::vector<int32_t> row;
      if (fscanf(f, "%d %d %d %d %d %d", &L.id, &L.bad, &L.parent, &nKeys, &nCov, &nCh) != 6 || !read_ints(f, row, nKeys) || !read_ints(f, L.cov, nCov) ||
          !read_ints(f, L.children, nCh))
        return 2;
      if (asd_map_put(ctx.get(), L.id, nKeys, row.data()) != ASD_OK) { fprintf(stderr, "asd_map_put: %s\n", ctx.error()); return 3; }
    }
    for (const Links& L : links) {
      if (asd_map_kf_links(ctx.get(), L.id, (int32_t)L.cov.size(), L.cov.data(), (int32_t)L.children.size(), L.children.data(), L.parent) != ASD_OK ||
          asd_map_kf_bad(ctx.get(), L.id, L.bad) != ASD_OK) {
        fprintf(stderr, "asd_map_kf_links: %s\n", ctx.error());
        return 3;
      }
    }
    std::vector<int32_t> bad;
    if (!read_ints(f, bad, nBad)) return 2;
    if (asd_map_point_bad(ctx.get(), nBad, bad.data(), 1) != ASD_OK) { fprintf(stderr, "asd_map_point_bad: %s\n", ctx.error()); return 3; }
    int nQ = 0;
    if (fscanf(f, "%d", &nQ) != 1) return 2;
    printf("{\"queries\": [");
    for (int q = 0; q < nQ; ++q) {
      int nCur = 0, nSeen = 0, nPrev = 0, maxKF = 0;
      std::vector<int32_t> cur, seen;
      asd::Tracking::LocalMap L;
      if (fscanf(f, "%d %d %d %d", &nCur, &nSeen, &nPrev, &maxKF) != 4 || !read_ints(f, cur, nCur) || !read_ints(f, seen, nSeen) ||
          !read_ints(f, L.mvpLocalKeyFrames, nPrev))
        return 2;
      const int rc = asd::Tracking::UpdateLocalMap(ctx, cur, seen, L, maxKF);
      if (rc != ASD_OK) fprintf(stderr, "asd_update_local_map: %s\n", ctx.error());
      printf("%s{\"rc\": %d, \"ref_kf\": %d, ", q ? ", " : "", rc, L.mpReferenceKF);
      print_ints("local_kfs", L.mvpLocalKeyFrames);
      print_ints("local_rows", L.mvpLocalMapPoints);
      print_ints("search_rows", L.vpSearch, true);
      printf("}");
    }
    printf("], \"connections\": [");
    int nC = 0;
    if (fscanf(f, "%d", &nC) != 1) return 2;
    for (int i = 0; i < nC; ++i) {
      int32_t kf = 0;
      if (fscanf(f, "%d", &kf) != 1) return 2;
      const asd::KeyFrame::Connections R = asd::KeyFrame::UpdateConnections(ctx, kf);
      if (R.rc != ASD_OK) fprintf(stderr, "asd_map_shared_counts: %s\n", ctx.error());
      printf("%s{\"rc\": %d, \"kf_max\": %d, ", i ? ", " : "", R.rc, R.pKFmax);
      print_ints("kfs", R.kfs);
      print_ints("weights", R.weights);
      print_ints("ordered", R.mvpOrderedConnectedKeyFrames);
      print_ints("ordered_weights", R.mvOrderedWeights);
      print_ints("best", R.Best(), true);
      printf("}");
    }
    printf("]}\n");
    fclose(f);
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
