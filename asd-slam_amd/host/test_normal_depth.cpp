// test_normal_depth.cpp -- probe for asd::KeyFrame::SetPose, asd::MapPoint::UpdateNormalAndDepth and asd::Optimizer::WriteBack
// (asd_adapters.hpp) over the context's observation table and attribute bank; tests/test_normal_depth_host.py reads its output.
//
//   test_normal_depth PROBLEM_FILE
//     The file (text): "nKF nBadPoints nBankRows"; per keyframe "mnId nKeys Owx Owy Owz", the row (nKeys bank rows, -1 = none), the octaves;
//     the bad points' rows; nBankRows lines of 8 floats (Xw, normal, min, max: asd_mpbank_put's row 0 ..); "nCalls", per call "n hasXw", the
//     rows, their mpRefKF ids and, with hasXw, 3 n floats.  A call without Xw is MapPoint::UpdateNormalAndDepth, one with Xw is
//     Optimizer::WriteBack (all centres handed over again, then the points).  Prints JSON, every float as its bit pattern: calls [{rc,
//     status, normal, min_dist, max_dist (the first form only), bank: the rows' 8 words as the bank holds them afterwards}].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "asd_adapters.hpp"

namespace {

bool read_ints(FILE* f, std::vector<int32_t>& v, size_t n) {
  v.resize(n);
  for (size_t i = 0; i < n; ++i) if (fscanf(f, "%d", &v[i]) != 1) return false;
  return true;
}
bool read_floats(FILE* f, std::vector<float>& v, size_t n) {
  v.resize(n);
  for (size_t i = 0; i < n; ++i) { double d; if (fscanf(f, "%lf", &d) != 1) return false; v[i] = (float)d; }
  return true;
}
void print_bits(const char* name, const float* v, size_t n, bool last = false) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < n; ++i) { uint32_t u; memcpy(&u, v + i, 4); printf("%s%u", i ? ", " : "", u); }
  printf("]%s", last ? "" : ", ");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s PROBLEM_FILE\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  try {
    asd::Context ctx(500, 1.2f, 8, 20, 7, 640, 480);
    int nKF = 0, nBad = 0, nBank = 0;
    if (fscanf(f, "%d %d %d", &nKF, &nBad, &nBank) != 3) return 2;
    std::vector<int32_t> kfIds;
    std::vector<float> Ow;
    for (int k = 0; k < nKF; ++k) {
      int id = 0, nKeys = 0;
      std::vector<int32_t> row, oct;
      std::vector<float> c;
      if (fscanf(f, "%d %d", &id, &nKeys) != 2 || !read_floats(f, c, 3) || !read_ints(f, row, nKeys) || !read_ints(f, oct, nKeys)) return 2;
      const std::vector<uint8_t> oct8(oct.begin(), oct.end());
      if (asd_map_put(ctx.get(), id, nKeys, row.data()) != ASD_OK || asd_map_put_octaves(ctx.get(), id, nKeys, oct8.data()) != ASD_OK) {
        fprintf(stderr, "asd_map_put: %s\n", ctx.error());
        return 3;
      }
      kfIds.push_back(id);
      Ow.insert(Ow.end(), c.begin(), c.end());
    }
    if (asd::KeyFrame::SetPose(ctx, kfIds, Ow) != ASD_OK) { fprintf(stderr, "asd_map_kf_centers: %s\n", ctx.error()); return 3; }
    std::vector<int32_t> bad;
    if (!read_ints(f, bad, nBad)) return 2;
    if (asd_map_point_bad(ctx.get(), nBad, bad.data(), 1) != ASD_OK) { fprintf(stderr, "asd_map_point_bad: %s\n", ctx.error()); return 3; }
    std::vector<float> bank;
    if (!read_floats(f, bank, 8 * (size_t)nBank)) return 2;
    {
      std::vector<float> X(3 * (size_t)nBank), N(3 * (size_t)nBank), mn(nBank), mx(nBank);
      for (int r = 0; r < nBank; ++r) {
        for (int k = 0; k < 3; ++k) { X[3 * r + k] = bank[8 * r + k]; N[3 * r + k] = bank[8 * r + 3 + k]; }
        mn[r] = bank[8 * r + 6]; mx[r] = bank[8 * r + 7];
      }
      if (asd_mpbank_put(ctx.get(), 0, nBank, X.data(), N.data(), mn.data(), mx.data()) != ASD_OK) { fprintf(stderr, "asd_mpbank_put: %s\n", ctx.error()); return 3; }
    }
    int nCalls = 0;
    if (fscanf(f, "%d", &nCalls) != 1) return 2;
    printf("{\"calls\": [");
    for (int q = 0; q < nCalls; ++q) {
      int n = 0, hasXw = 0;
      std::vector<int32_t> rows, refs;
      std::vector<float> Xw;
      if (fscanf(f, "%d %d", &n, &hasXw) != 2 || !read_ints(f, rows, n) || !read_ints(f, refs, n) || (hasXw && !read_floats(f, Xw, 3 * (size_t)n))) return 2;
      int rc;
      std::vector<uint8_t> status;
      printf("%s{", q ? ", " : "");
      if (hasXw) {
        rc = asd::Optimizer::WriteBack(ctx, kfIds, Ow, rows, refs, Xw, &status);
      } else {
        const asd::MapPoint::NormalAndDepth R = asd::MapPoint::UpdateNormalAndDepth(ctx, rows, refs);
        rc = R.rc;
        status = R.status;
        print_bits("normal", R.mNormalVector.data(), R.mNormalVector.size());
        print_bits("min_dist", R.mfMinDistance.data(), R.mfMinDistance.size());
        print_bits("max_dist", R.mfMaxDistance.data(), R.mfMaxDistance.size());
      }
      if (rc != ASD_OK) fprintf(stderr, "asd_update_normal_and_depth: %s\n", ctx.error());
      printf("\"rc\": %d, \"status\": [", rc);
      for (size_t i = 0; i < status.size(); ++i) printf("%s%d", i ? ", " : "", (int)status[i]);
      printf("], ");
      std::vector<float> now(8 * (size_t)n);
      for (int i = 0; i < n; ++i)
        if (asd_debug_bank_get(ctx.get(), rows[i], 1, nullptr, now.data() + 8 * (size_t)i) != ASD_OK) { fprintf(stderr, "asd_debug_bank_get: %s\n", ctx.error()); return 3; }
      print_bits("bank", now.data(), now.size(), true);
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
