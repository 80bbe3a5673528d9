// test_local_ba_graph.cpp -- probe for asd::Optimizer::LocalBundleAdjustmentGraph and the table form of asd::Optimizer::LocalBundleAdjustment
// (asd_adapters.hpp) over the context's observation table and attribute bank; tests/test_local_ba_graph_host.py reads its output.
//
//   test_local_ba_graph PROBLEM_FILE
//     The file (text): "nKF nBadPoints nBankRows"; per keyframe "mnId isBad globalMapFlag nKeys", 16 floats Tcw, the row (nKeys bank rows,
//     -1 = none), the octaves, 2 nKeys floats mvKeysUn[i].pt; the bad points' rows; nBankRows lines of 8 floats (asd_mpbank_put's row 0 ..);
//     nBankRows lines "globalMapFlag mpRefKF"; "fx fy cx cy"; "kf nNeigh" and the neighbours; "stop": 0 = no pbStopFlag, 1 = a flag that stays
//     false, 2 = a flag that is set.
//     Prints JSON, every float as its bit pattern: graph {the lists}, then rc, stopped, second_round, erase, n_erased, bad_rows, Tcw, rows,
//     mpRefKF, Xw, status, iters, bank (all rows as the bank holds them afterwards), observations (Observations() of every bank row).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
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
void print_bits(const char* name, const float* v, size_t n) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < n; ++i) { uint32_t u; memcpy(&u, v + i, 4); printf("%s%u", i ? ", " : "", u); }
  printf("], ");
}
template <class T>
void print_ints(const char* name, const std::vector<T>& v, bool last = false) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", (int)v[i]);
  printf("]%s", last ? "" : ", ");
}

struct KF { bool global = false; std::vector<float> Tcw, keys; };
struct View {
  std::map<int32_t, KF> kfs;
  std::vector<int32_t> pt_global, pt_ref;
  float k[4];
  const float* Tcw(int32_t kf) const { return kfs.at(kf).Tcw.data(); }
  bool fixed(int32_t kf) const { return kfs.at(kf).global; }
  bool inTable(int32_t kf) const { return kfs.count(kf) != 0; }
  const float* keysUn(int32_t kf) const { return kfs.at(kf).keys.data(); }
  const float* K() const { return k; }
  bool global(int32_t row) const { return pt_global[row] != 0; }
  int32_t refKF(int32_t row) const { return pt_ref[row]; }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s PROBLEM_FILE\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  try {
    asd::Context ctx(500, 1.2f, 8, 20, 7, 640, 480);
    int nKF = 0, nBad = 0, nBank = 0;
    if (fscanf(f, "%d %d %d", &nKF, &nBad, &nBank) != 3) return 2;
    View view;
    std::vector<int32_t> kfIds;
    std::vector<float> Ow;
    for (int k = 0; k < nKF; ++k) {
      int id = 0, isBad = 0, global = 0, nKeys = 0;
      std::vector<int32_t> row, oct;
      KF kf;
      if (fscanf(f, "%d %d %d %d", &id, &isBad, &global, &nKeys) != 4 || !read_floats(f, kf.Tcw, 16) || !read_ints(f, row, nKeys) || !read_ints(f, oct, nKeys) ||
          !read_floats(f, kf.keys, 2 * (size_t)nKeys))
        return 2;
      kf.global = global != 0;
      const std::vector<uint8_t> oct8(oct.begin(), oct.end());
      if (asd_map_put(ctx.get(), id, nKeys, row.data()) != ASD_OK || asd_map_put_octaves(ctx.get(), id, nKeys, oct8.data()) != ASD_OK ||
          (isBad && asd_map_kf_bad(ctx.get(), id, 1) != ASD_OK)) {
        fprintf(stderr, "asd_map_put: %s\n", ctx.error());
        return 3;
      }
      kfIds.push_back(id);
      const float* T = kf.Tcw.data();
      for (int r = 0; r < 3; ++r) Ow.push_back(-(T[r] * T[3] + T[4 + r] * T[7] + T[8 + r] * T[11]));
      view.kfs[id] = kf;
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
    view.pt_global.resize(nBank); view.pt_ref.resize(nBank);
    for (int r = 0; r < nBank; ++r) if (fscanf(f, "%d %d", &view.pt_global[r], &view.pt_ref[r]) != 2) return 2;
    std::vector<float> K;
    if (!read_floats(f, K, 4)) return 2;
    for (int k = 0; k < 4; ++k) view.k[k] = K[k];
    int kf = 0, nNeigh = 0, stop = 0;
    std::vector<int32_t> neigh;
    if (fscanf(f, "%d %d", &kf, &nNeigh) != 2 || !read_ints(f, neigh, nNeigh) || fscanf(f, "%d", &stop) != 1) return 2;
    fclose(f);

    const asd::Optimizer::LocalBAGraph G = asd::Optimizer::LocalBundleAdjustmentGraph(ctx, kf, neigh);
    if (G.rc != ASD_OK) { fprintf(stderr, "asd_local_ba_graph: %s\n", ctx.error()); return 3; }
    printf("{\"graph\": {");
    print_ints("local_kfs", G.lLocalKeyFrames); print_ints("local_rows", G.lLocalMapPoints); print_ints("fixed_kfs", G.lFixedCameras);
    print_ints("pose_kfs", G.pose_kfs); print_ints("pose_fixed", G.pose_fixed); print_ints("point_rank", G.point_rank);
    print_ints("e_point", G.e_point); print_ints("e_pose", G.e_pose); print_ints("e_kf", G.e_kf); print_ints("e_idx", G.e_idx);
    print_ints("e_octave", G.e_octave, true);
    printf("}, ");
    const bool flag = stop == 2;
    const asd::Optimizer::LocalBAResult R = asd::Optimizer::LocalBundleAdjustment(ctx, kf, neigh, view, stop ? &flag : nullptr);
    if (R.rc != ASD_OK) fprintf(stderr, "LocalBundleAdjustment: %s\n", ctx.error());
    printf("\"rc\": %d, \"stopped\": %d, \"second_round\": %d, \"n_erased\": %d, \"iters\": [%d, %d], ", R.rc, (int)R.stopped, (int)R.second_round, R.n_erased,
           R.ba.iters_first, R.ba.iters_second);
    print_ints("erase", R.erase); print_ints("bad_rows", R.bad_rows); print_ints("rows", R.rows); print_ints("mpRefKF", R.mpRefKF);
    print_ints("status", R.status);
    print_bits("Tcw", R.Tcw.data(), R.Tcw.size()); print_bits("Ow", R.Ow.data(), R.Ow.size()); print_bits("Xw", R.Xw.data(), R.Xw.size());
    std::vector<float> now(8 * (size_t)nBank);
    if (nBank && asd_debug_bank_get(ctx.get(), 0, nBank, nullptr, now.data()) != ASD_OK) { fprintf(stderr, "asd_debug_bank_get: %s\n", ctx.error()); return 3; }
    print_bits("bank", now.data(), now.size());
    std::vector<int32_t> all(nBank), obs(nBank);
    for (int r = 0; r < nBank; ++r) all[r] = r;
    if (nBank && asd_map_observations(ctx.get(), nBank, all.data(), obs.data()) != ASD_OK) { fprintf(stderr, "asd_map_observations: %s\n", ctx.error()); return 3; }
    print_ints("observations", obs, true);
    printf("}\n");
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
