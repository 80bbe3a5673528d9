// test_pnp_solver.cpp -- probe for asd::PnPsolver and asd::Tracking::RelocalizationRound (asd_adapters.hpp); tests/test_pnp_solver_host.py
// reads its output.
//
//   test_pnp_solver --params N PROBABILITY MIN_INLIERS MAX_ITERATIONS MIN_SET EPSILON
//     no device.  Prints "min_inliers A max_its B": asd_pnp_ransac_parameters.
//   test_pnp_solver --draws SEED N E0 E1 ...
//     no device.  A solver over N correspondences with SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) and a stream seeded with
//     srand(SEED); one iterate(5) per Ek, stepped through Begin / End with a scripted outcome: Ek = -1 no iteration returns a model,
//     Ek = k iteration k of the call does.  Prints per call: n_iter, the RandomInt results of the iterations that ran, the raw values consumed.
//   test_pnp_solver PROBLEM_FILE
//     on the device.  The file (text; floats as C99 hex): "nraw" and nraw raw rand() values, "match_at", "ncand", then per candidate
//     "NF N", K[4], indices[N], P3Dw[3N], P2D[2N], sigma2[N].  Prints JSON: "single": per candidate alone on a fresh stream, iterate(5)
//     until bNoMore or a pose; "round": passes of Tracking::RelocalizationRound (5 iterations each) over all candidates until the scripted
//     tail reports bMatch -- it does at its match_at-th call (0-based; -1 never) -- or every candidate is discarded.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "asd_adapters.hpp"

namespace {

struct Cand {
  int NF = 0, N = 0;
  asd::Camera K{};
  std::vector<size_t> idx;
  std::vector<float> P3D, P2D, sigma2;
};

bool read_floats(FILE* f, std::vector<float>& v) {
  for (float& x : v) if (fscanf(f, "%a", &x) != 1) return false;
  return true;
}

struct Scripted {   // the raw values of the file, then an error
  std::vector<int> raw;
  size_t at = 0;
  bool ran_out = false;
  int next() { if (at < raw.size()) return raw[at++]; ran_out = true; return 0; }
};

void print_call(const asd::PnPsolver& s, bool got, bool bNoMore, int nInliers, const std::vector<bool>& inl, const float* Tcw) {
  printf("{\"pose\": %d, \"no_more\": %d, \"n_inliers\": %d, \"iterations\": %d, \"best_inliers\": %d, \"inliers\": [", (int)got, (int)bNoMore,
         nInliers, s.GetIterations(), s.GetBestInliers());
  bool first = true;
  for (size_t i = 0; i < inl.size(); ++i)
    if (inl[i]) { printf("%s%zu", first ? "" : ", ", i); first = false; }
  printf("], \"Tcw\": [");
  if (got)
    for (int i = 0; i < 16; ++i) printf("%s\"%a\"", i ? ", " : "", (double)Tcw[i]);
  printf("], \"raw\": [");
  for (size_t i = 0; i < s.LastRawConsumed().size(); ++i) printf("%s%d", i ? ", " : "", s.LastRawConsumed()[i]);
  printf("]}");
}

int params_mode(int argc, char** argv) {
  if (argc != 8) return 2;
  int32_t mi = 0, its = 0;
  if (asd_pnp_ransac_parameters(atoi(argv[2]), atof(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), (float)atof(argv[7]), &mi, &its) != ASD_OK) return 3;
  printf("min_inliers %d max_its %d\n", mi, its);
  return 0;
}

int draws_mode(int argc, char** argv) {
  if (argc < 5) return 2;
  const int seed = atoi(argv[2]), N = atoi(argv[3]);
  std::srand((unsigned)seed);
  asd::DrawStream stream;   // ::rand
  std::vector<size_t> idx(N);
  for (int i = 0; i < N; ++i) idx[i] = (size_t)i;
  const asd::Camera K{1, 1, 0, 0};
  asd::PnPsolver solver(nullptr, N, idx, std::vector<float>(3 * N, 1.f), std::vector<float>(2 * N, 1.f), std::vector<float>(N, 1.f), K, stream);
  solver.SetRansacParameters(0.99, 10, 300, 4, 0.5f, 5.991f);
  printf("min_inliers %d max_its %d\n", solver.GetMinInliers(), solver.GetMaxIterations());
  for (int a = 4; a < argc; ++a) {
    const int early = atoi(argv[a]);
    asd_pnp_ransac_problem p;
    if (!solver.Begin(5, p)) { printf("call no_more\n"); continue; }
    const bool ret = early >= 0 && early < p.n_iter;
    p.found = ret; p.iterations_done = ret ? early + 1 : p.n_iter; p.best_updated = 0; p.n_inliers = 0;
    printf("call n_iter %d draws", p.n_iter);
    for (int k = 0; k < 4 * p.iterations_done; ++k) printf(" %d", p.draws[k]);
    bool bNoMore; std::vector<bool> inl; int nInl; float Tcw[16];
    solver.End(p, bNoMore, inl, nInl, Tcw);
    printf(" raw");
    for (int v : solver.LastRawConsumed()) printf(" %d", v);
    printf(" iterations %d no_more %d pending %zu\n", solver.GetIterations(), (int)bNoMore, stream.Pending());
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "--params")) return params_mode(argc, argv);
  if (argc >= 2 && !strcmp(argv[1], "--draws")) return draws_mode(argc, argv);
  if (argc < 2) { fprintf(stderr, "usage: %s PROBLEM_FILE | --draws SEED N E0 E1 ... | --params N P MIN MAXITS MINSET EPS\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int nraw = 0, match_at = 0, ncand = 0;
  if (fscanf(f, "%d", &nraw) != 1 || nraw < 0) return 2;
  std::vector<int> raw(nraw);
  for (int& v : raw) if (fscanf(f, "%d", &v) != 1) return 2;
  if (fscanf(f, "%d %d", &match_at, &ncand) != 2 || ncand < 1) return 2;
  std::vector<Cand> cands(ncand);
  for (Cand& c : cands) {
    if (fscanf(f, "%d %d", &c.NF, &c.N) != 2) return 2;
    if (fscanf(f, "%f %f %f %f", &c.K.fx, &c.K.fy, &c.K.cx, &c.K.cy) != 4) return 2;
    c.idx.resize(c.N);
    for (size_t& v : c.idx) if (fscanf(f, "%zu", &v) != 1) return 2;
    c.P3D.resize(3 * c.N); c.P2D.resize(2 * c.N); c.sigma2.resize(c.N);
    if (!read_floats(f, c.P3D) || !read_floats(f, c.P2D) || !read_floats(f, c.sigma2)) return 2;
  }
  fclose(f);
  try {
    asd::Context ctx(500, 1.2f, 8, 20, 7, 640, 480);
    auto make = [&](const Cand& c, asd::DrawStream& st) {
      std::unique_ptr<asd::PnPsolver> s(new asd::PnPsolver(ctx.get(), c.NF, c.idx, c.P3D, c.P2D, c.sigma2, c.K, st));
      s->SetRansacParameters(0.99, 10, 300, 4, 0.5f, 5.991f);   // Tracking.cc:1141
      return s;
    };
    printf("{\"single\": [");
    for (int ci = 0; ci < ncand; ++ci) {
      Scripted src{raw};
      asd::DrawStream st([&src] { return src.next(); }, 2147483647.0);
      auto s = make(cands[ci], st);
      printf("%s{\"min_inliers\": %d, \"max_its\": %d, \"calls\": [", ci ? ", " : "", s->GetMinInliers(), s->GetMaxIterations());
      for (int call = 0;; ++call) {
        bool bNoMore = false; std::vector<bool> inl; int nInl = 0; float Tcw[16];
        const bool got = s->iterate(5, bNoMore, inl, nInl, Tcw);
        printf("%s", call ? ", " : "");
        print_call(*s, got, bNoMore, nInl, inl, Tcw);
        if (got || bNoMore) break;
      }
      printf("], \"pending\": %zu, \"source_at\": %zu, \"ran_out\": %d}", st.Pending(), src.at, (int)src.ran_out);
    }
    printf("], \"round\": {\"tails\": [");
    {
      Scripted src{raw};
      asd::DrawStream st([&src] { return src.next(); }, 2147483647.0);
      std::vector<std::unique_ptr<asd::PnPsolver>> own;
      std::vector<asd::PnPsolver*> solvers;
      for (const Cand& c : cands) { own.push_back(make(c, st)); solvers.push_back(own.back().get()); }
      std::vector<bool> discarded(ncand, false);
      int tails = 0, matched = -1, passes = 0;
      auto live = [&] { int n = 0; for (bool d : discarded) n += !d; return n; };
      while (live() > 0 && matched < 0) {   // :1156
        ++passes;
        matched = asd::Tracking::RelocalizationRound(ctx, solvers, discarded, 5, [&](int i, const float* Tcw, const std::vector<bool>& inl, int nInl) {
          printf("%s{\"candidate\": %d, \"pass\": %d, \"call\": ", tails ? ", " : "", i, passes);
          print_call(*solvers[i], true, false, nInl, inl, Tcw);
          printf("}");
          return tails++ == match_at;
        });
      }
      printf("], \"matched\": %d, \"passes\": %d, \"iterations\": [", matched, passes);
      for (int i = 0; i < ncand; ++i) printf("%s%d", i ? ", " : "", solvers[i]->GetIterations());
      printf("], \"best_inliers\": [");
      for (int i = 0; i < ncand; ++i) printf("%s%d", i ? ", " : "", solvers[i]->GetBestInliers());
      printf("], \"discarded\": [");
      for (int i = 0; i < ncand; ++i) printf("%s%d", i ? ", " : "", (int)discarded[i]);
      printf("], \"pending\": %zu, \"source_at\": %zu, \"ran_out\": %d}}\n", st.Pending(), src.at, (int)src.ran_out);
    }
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
