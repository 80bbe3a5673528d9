// test_fuse_apply_rule.cpp -- asd_fuse_apply's rule over flat host tables (fuse_apply.hpp) alone: no device, no library, so it can be
// built with -fsanitize=address,undefined (`make ../host/test_fuse_apply_rule_asan`) and run anywhere.  tests/test_fuse_apply_host.py
// reads its output.
//
//   test_fuse_apply_rule problem.txt
//     "nKF nBad", per keyframe "id n" and its row, the bad rows, "nCalls", per call "kf mode n apply", the candidates, best_idx.
//     Prints JSON {calls: [{action, other, obs_cand, obs_other, n_moved, n_dropped, n_fused}], rows: [[id, [row]]], bad: [rows]}.
#include <cstdio>
#include <cstdlib>
#include <map>

#include "fuse_apply.hpp"

static void print_list(const char* name, const std::vector<int32_t>& v, const char* tail) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", v[i]);
  printf("]%s", tail);
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s problem.txt\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int nKF = 0, nBad = 0;
  if (fscanf(f, "%d %d", &nKF, &nBad) != 2 || nKF < 0 || nBad < 0) return 2;
  asd::FuseMap M;
  std::vector<int32_t> ids(nKF);
  std::map<int32_t, int32_t> index;
  M.rows.resize(nKF);
  for (int k = 0; k < nKF; ++k) {
    int n = 0;
    if (fscanf(f, "%d %d", &ids[k], &n) != 2 || n < 0) return 2;
    index[ids[k]] = k;
    M.rows[k].resize(n);
    for (int i = 0; i < n; ++i) if (fscanf(f, "%d", &M.rows[k][i]) != 1) return 2;
  }
  M.BuildObservers();
  for (int i = 0; i < nBad; ++i) {
    int p = 0;
    if (fscanf(f, "%d", &p) != 1 || p < 0) return 2;
    M.Reserve(p);
    M.bad[p] = 1;
  }
  int nCalls = 0;
  if (fscanf(f, "%d", &nCalls) != 1 || nCalls < 0) return 2;
  printf("{\"calls\": [");
  for (int c = 0; c < nCalls; ++c) {
    int kf = 0, mode = 0, n = 0, apply = 0;
    if (fscanf(f, "%d %d %d %d", &kf, &mode, &n, &apply) != 4 || n < 0 || mode < 0 || mode > 2 || !index.count(kf)) return 2;
    std::vector<int32_t> cand(n), best(n);
    for (int i = 0; i < n; ++i) if (fscanf(f, "%d", &cand[i]) != 1) return 2;
    for (int i = 0; i < n; ++i) if (fscanf(f, "%d", &best[i]) != 1 || best[i] >= (int)M.rows[index[kf]].size()) return 2;
    const asd::FuseApplyResult R = asd::FuseApplyRule(M, index[kf], mode, cand.data(), best.data(), n, apply != 0);
    printf("%s{", c ? ", " : "");
    print_list("action", std::vector<int32_t>(R.action.begin(), R.action.end()), ", ");
    print_list("other", R.other, ", ");
    print_list("obs_cand", R.obs_cand, ", ");
    print_list("obs_other", R.obs_other, ", ");
    print_list("n_moved", R.n_moved, ", ");
    print_list("n_dropped", R.n_dropped, ", ");
    printf("\"n_fused\": %d}", R.n_fused);
  }
  printf("], \"rows\": [");
  for (int k = 0; k < nKF; ++k) {
    printf("%s[%d, {", k ? ", " : "", ids[k]);
    print_list("row", M.rows[k], "}]");
  }
  printf("], ");
  std::vector<int32_t> bad;
  for (size_t p = 0; p < M.bad.size(); ++p) if (M.bad[p]) bad.push_back((int32_t)p);
  print_list("bad", bad, "}\n");
  fclose(f);
  return 0;
}
