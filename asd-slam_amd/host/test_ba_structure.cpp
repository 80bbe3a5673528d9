// The host-built active structure (csrc/ba_structure.h) from a problem file: a probe binary for tests/test_ba_structure_host.py.  No
// device, no library.
//   test_ba_structure [FILE]      (stdin without FILE)
// Input, whitespace separated; several problems may follow one another:
//   P L E all_blocks   fixed[0 .. P)   then E x (e_pose e_point)
// Output per problem: the counts, then every table on a line of its own ("name: v v v ..."; pairs as a,b), read back from the block
// at the layout's offsets; "end" closes a problem.
#include <cstdio>
#include <cstdlib>

#include "../csrc/ba_structure.h"

static void line(const char* name, const char* base, size_t off, int n) {
  const int* v = reinterpret_cast<const int*>(base + off);
  printf("%s:", name);
  for (int i = 0; i < n; ++i) printf(" %d", v[i]);
  printf("\n");
}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int P, L, E, all, n_problems = 0;
  while (fscanf(f, "%d %d %d %d", &P, &L, &E, &all) == 4) {
    if (P < 0 || L < 0 || E < 0) { fprintf(stderr, "negative size\n"); return 2; }
    std::vector<uint8_t> fixed(P);
    std::vector<int> e_pose(E), e_point(E);
    for (int p = 0; p < P; ++p) { int v; if (fscanf(f, "%d", &v) != 1) return 2; fixed[p] = (uint8_t)(v != 0); }
    for (int e = 0; e < E; ++e) {
      if (fscanf(f, "%d %d", &e_pose[e], &e_point[e]) != 2) return 2;
      if (e_pose[e] < 0 || e_pose[e] >= P || e_point[e] < 0 || e_point[e] >= L) { fprintf(stderr, "edge %d references vertex out of range\n", e); return 2; }
    }
    BaStructure bs;
    bs.count(P, L, E, e_pose.data(), e_point.data(), fixed.data(), all != 0);
    const BaStructLayout lay = bs.layout();
    // exactly lay.bytes, from the heap: a write past the block or in front of it is the sanitizer build's to report
    char* base = static_cast<char*>(malloc(lay.bytes));
    if (!base) return 2;
    bs.fill(base, lay);
    const int nps = reinterpret_cast<const int*>(base + lay.ps_start)[bs.nPf];
    printf("counts: %d %d %d %d %zu\n", bs.nPf, bs.nLa, bs.Ea, bs.nblk, bs.npairs);
    line("pose_h", base, lay.pose_h, P); line("pt_h", base, lay.pt_h, L);
    line("pose_of_h", base, lay.pose_of_h, bs.nPf); line("pt_of_h", base, lay.pt_of_h, bs.nLa);
    line("pt_start", base, lay.pt_start, bs.nLa + 1); line("act", base, lay.act, bs.Ea);
    line("ps_start", base, lay.ps_start, bs.nPf + 1); line("ps_edges", base, lay.ps_edges, nps); line("ps_h", base, lay.ps_h, nps);
    line("blk_i", base, lay.blk_i, bs.nblk); line("blk_j", base, lay.blk_j, bs.nblk);
    line("pair_start", base, lay.pair_start, bs.nblk + 1);
    const int* pairs = reinterpret_cast<const int*>(base + lay.pairs);
    printf("pairs:");
    for (size_t i = 0; i < bs.npairs; ++i) printf(" %d,%d", pairs[2 * i], pairs[2 * i + 1]);
    printf("\n");
    line("pair_h", base, lay.pair_h, (int)bs.npairs);
    printf("end\n");
    free(base);
    ++n_problems;
  }
  if (f != stdin) fclose(f);
  return n_problems > 0 ? 0 : 2;
}
