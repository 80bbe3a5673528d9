// test_culling.cpp -- probe for asd::LocalMapping::KeyFrameCulling and asd::LocalMapping::MapPointCulling (asd_adapters.hpp) over the
// context's observation table; tests/test_culling_host.py reads its output.
//
//   test_culling PROBLEM_FILE
//     The file (text, integers): "nKF nBadPoints"; per keyframe "mnId bad nKeys", the row (nKeys bank rows, -1 = none), the octaves; the bad
//     points' rows; "nCalls", per call "nCand apply", the candidates' ids, their flags; "nRecent nCurrentKFid", per record
//     "row mnFirstKFid mnFound mnVisible isBad"; "nRows" and that many bank rows.  The calls run in order on one table, MapPointCulling
//     and the observation counts behind them.  Prints JSON: calls [{rc, decision, n_mps, n_redundant, bad_rows}], points {rc, set_bad,
//     recent}, observations [..].
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
    for (int k = 0; k < nKF; ++k) {
      int id = 0, isBad = 0, nKeys = 0;
      std::vector<int32_t> row, oct;
      if (fscanf(f, "%d %d %d", &id, &isBad, &nKeys) != 3 || !read_ints(f, row, nKeys) || !read_ints(f, oct, nKeys)) return 2;
      const std::vector<uint8_t> oct8(oct.begin(), oct.end());
      if (asd_map_put(ctx.get(), id, nKeys, row.data()) != ASD_OK || asd_map_put_octaves(ctx.get(), id, nKeys, oct8.data()) != ASD_OK ||
          asd_map_kf_bad(ctx.get(), id, isBad) != ASD_OK) {
        fprintf(stderr, "asd_map_put: %s\n", ctx.error());
        return 3;
      }
    }
    std::vector<int32_t> bad;
    if (!read_ints(f, bad, nBad)) return 2;
    if (asd_map_point_bad(ctx.get(), nBad, bad.data(), 1) != ASD_OK) { fprintf(stderr, "asd_map_point_bad: %s\n", ctx.error()); return 3; }
    int nCalls = 0;
    if (fscanf(f, "%d", &nCalls) != 1) return 2;
    printf("{\"calls\": [");
    for (int q = 0; q < nCalls; ++q) {
      int nCand = 0, apply = 0;
      std::vector<int32_t> cand, fl;
      if (fscanf(f, "%d %d", &nCand, &apply) != 2 || !read_ints(f, cand, nCand) || !read_ints(f, fl, nCand)) return 2;
      const asd::LocalMapping::Culling R = asd::LocalMapping::KeyFrameCulling(ctx, cand, std::vector<uint8_t>(fl.begin(), fl.end()), apply != 0);
      if (R.rc != ASD_OK) fprintf(stderr, "asd_keyframe_culling: %s\n", ctx.error());
      printf("%s{\"rc\": %d, ", q ? ", " : "", R.rc);
      print_ints("decision", std::vector<int32_t>(R.decision.begin(), R.decision.end()));
      print_ints("n_mps", R.nMPs);
      print_ints("n_redundant", R.nRedundantObservations);
      print_ints("bad_rows", R.badPoints, true);
      printf("}");
    }
    int nRecent = 0, nCurrentKFid = 0;
    if (fscanf(f, "%d %d", &nRecent, &nCurrentKFid) != 2) return 2;
    std::vector<asd::RecentMapPoint> recent(nRecent);
    for (asd::RecentMapPoint& p : recent) {
      int isBad = 0;
      if (fscanf(f, "%d %d %d %d %d", &p.row, &p.mnFirstKFid, &p.mnFound, &p.mnVisible, &isBad) != 5) return 2;
      p.isBad = isBad != 0;
    }
    const asd::MapPointCullingResult P = asd::LocalMapping::MapPointCulling(ctx, recent, nCurrentKFid);
    if (P.rc != ASD_OK) fprintf(stderr, "asd_map_observations: %s\n", ctx.error());
    std::vector<int32_t> left;
    for (const asd::RecentMapPoint& p : P.recent) left.push_back(p.row);
    printf("], \"points\": {\"rc\": %d, ", P.rc);
    print_ints("set_bad", std::vector<int32_t>(P.setBad.begin(), P.setBad.end()));
    print_ints("recent", left, true);
    int nRows = 0;
    std::vector<int32_t> rows;
    if (fscanf(f, "%d", &nRows) != 1 || !read_ints(f, rows, nRows)) return 2;
    std::vector<int32_t> obs(nRows);
    if (asd_map_observations(ctx.get(), nRows, rows.data(), obs.data()) != ASD_OK) { fprintf(stderr, "asd_map_observations: %s\n", ctx.error()); return 3; }
    printf("}, ");
    print_ints("observations", obs, true);
    printf("}\n");
    fclose(f);
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
