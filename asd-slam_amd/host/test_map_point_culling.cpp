// test_map_point_culling.cpp -- the list rule of LocalMapping::MapPointCulling (map_point_culling.hpp) alone: no device, no library, so
// it can be built with -fsanitize=address,undefined (`make ../host/test_map_point_culling_asan`) and run anywhere.
// tests/test_culling_host.py reads its output.
//
//   test_map_point_culling nCurrentKFid  < records
//     stdin: "n", then per record "row mnFirstKFid mnFound mnVisible isBad observations".  Prints JSON {set_bad, recent}.
#include <cstdio>
#include <cstdlib>

#include "map_point_culling.hpp"

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s nCurrentKFid < records\n", argv[0]); return 2; }
  const int32_t nCurrentKFid = atoi(argv[1]);
  int n = 0;
  if (scanf("%d", &n) != 1 || n < 0) return 2;
  std::vector<asd::RecentMapPoint> recent(n);
  std::vector<int32_t> obs(n);
  for (int i = 0; i < n; ++i) {
    int isBad = 0;
    if (scanf("%d %d %d %d %d %d", &recent[i].row, &recent[i].mnFirstKFid, &recent[i].mnFound, &recent[i].mnVisible, &isBad, &obs[i]) != 6) return 2;
    recent[i].isBad = isBad != 0;
  }
  const asd::MapPointCullingResult R = asd::MapPointCullingRule(recent, obs, nCurrentKFid);
  printf("{\"set_bad\": [");
  for (size_t i = 0; i < R.setBad.size(); ++i) printf("%s%zu", i ? ", " : "", R.setBad[i]);
  printf("], \"recent\": [");
  for (size_t i = 0; i < R.recent.size(); ++i) printf("%s%d", i ? ", " : "", R.recent[i].row);
  printf("]}\n");
  return 0;
}
