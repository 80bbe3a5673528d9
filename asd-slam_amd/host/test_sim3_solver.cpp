// test_sim3_solver.cpp -- probe for asd::DrawStream, asd::Sim3Solver and the RANSAC rounds of asd::LoopClosing::ComputeSim3
// (asd_adapters.hpp); tests/test_sim3_solver_ref.py and tests/test_sim3_solver_host.py read its output.
//
//   test_sim3_solver --draws SEED N MIN_INLIERS E0 E1 ...
//     no device.  A solver over N correspondences with SetRansacParameters(0.99, MIN_INLIERS, 300) and a stream seeded with
//     srand(SEED); one iterate(5) per Ek, stepped through Begin / End with a scripted outcome: Ek = -1 no iteration returns a model,
//     Ek = k iteration k of the call does.  Prints per call: n_iter, the RandomInt results of the iterations that ran, the raw values consumed.
//   test_sim3_solver PROBLEM_FILE
//     on the device.  The file (text; floats as C99 hex): "nraw" and nraw raw rand() values, "n_reject", "ncand", then per candidate
//     "N1 N fix_scale min_inliers max_its", K1[4], K2[4], indices1[N], X1c[3N], X2c[3N], max_err1[N], max_err2[N].  Prints JSON:
//     "single": per candidate alone on a fresh stream, iterate(5) until bNoMore or a model; "multi": the rounds of ComputeSim3 over
//     all candidates (LoopClosing::Sim3Round, 5 iterations each) until a model is accepted -- the first n_reject models are treated as
//     LoopClosing.cc:364 treats a failed optimisation: the round goes on with the candidates behind.
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
  int N1 = 0, N = 0, fix = 0, min_inliers = 0, max_its = 0;
  asd::Camera K1{}, K2{};
  std::vector<size_t> idx1;
  std::vector<float> X1, X2, e1, e2;
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

void print_call(const asd::Sim3Solver& s, bool got, bool bNoMore, int nInliers, const std::vector<bool>& inl) {
  printf("{\"model\": %d, \"no_more\": %d, \"n_inliers\": %d, \"iterations\": %d, \"best_inliers\": %d, \"inliers\": [", (int)got, (int)bNoMore,
         nInliers, s.GetIterations(), s.GetBestInliers());
  bool first = true;
  for (size_t i = 0; i < inl.size(); ++i)
    if (inl[i]) { printf("%s%zu", first ? "" : ", ", i); first = false; }
  printf("], \"R\": [");
  for (int i = 0; i < 9; ++i) printf("%s\"%a\"", i ? ", " : "", (double)s.GetEstimatedRotation()[i]);
  printf("], \"t\": [");
  for (int i = 0; i < 3; ++i) printf("%s\"%a\"", i ? ", " : "", (double)s.GetEstimatedTranslation()[i]);
  printf("], \"s\": \"%a\", \"raw\": [", (double)s.GetEstimatedScale());
  for (size_t i = 0; i < s.LastRawConsumed().size(); ++i) printf("%s%d", i ? ", " : "", s.LastRawConsumed()[i]);
  printf("]}");
}

int draws_mode(int argc, char** argv) {
  if (argc < 6) return 2;
  const int seed = atoi(argv[2]), N = atoi(argv[3]), min_inliers = atoi(argv[4]);
  std::srand((unsigned)seed);
  asd::DrawStream stream;   // ::rand
  std::vector<size_t> idx1(N);
  for (int i = 0; i < N; ++i) idx1[i] = (size_t)i;
  const asd::Camera K{1, 1, 0, 0};
  asd::Sim3Solver solver(nullptr, N, idx1, std::vector<float>(3 * N, 1.f), std::vector<float>(3 * N, 1.f), std::vector<float>(N, 1.f),
                         std::vector<float>(N, 1.f), K, K, false, stream);
  solver.SetRansacParameters(0.99, min_inliers, 300);
  printf("max_its %d\n", solver.GetMaxIterations());
  for (int a = 5; a < argc; ++a) {
    const int early = atoi(argv[a]);
    asd_sim3_ransac_problem p;
    if (!solver.Begin(5, p)) { printf("call no_more\n"); continue; }
    const bool ret = early >= 0 && early < p.n_iter;
    p.found = ret; p.iterations_done = ret ? early + 1 : p.n_iter; p.best_updated = 0; p.n_inliers = 0;
    printf("call n_iter %d draws", p.n_iter);
    for (int k = 0; k < 3 * p.iterations_done; ++k) printf(" %d", p.draws[k]);
    bool bNoMore; std::vector<bool> inl; int nInl;
    solver.End(p, bNoMore, inl, nInl);
    printf(" raw");
    for (int v : solver.LastRawConsumed()) printf(" %d", v);
    printf(" iterations %d no_more %d pending %zu\n", solver.GetIterations(), (int)bNoMore, stream.Pending());
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "--draws")) return draws_mode(argc, argv);
  if (argc < 2) { fprintf(stderr, "usage: %s PROBLEM_FILE | --draws SEED N MIN_INLIERS E0 E1 ...\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int nraw = 0, n_reject = 0, ncand = 0;
  if (fscanf(f, "%d", &nraw) != 1 || nraw < 0) return 2;
  std::vector<int> raw(nraw);
  for (int& v : raw) if (fscanf(f, "%d", &v) != 1) return 2;
  if (fscanf(f, "%d %d", &n_reject, &ncand) != 2 || ncand < 1) return 2;
  std::vector<Cand> cands(ncand);
  for (Cand& c : cands) {
    if (fscanf(f, "%d %d %d %d %d", &c.N1, &c.N, &c.fix, &c.min_inliers, &c.max_its) != 5) return 2;
    if (fscanf(f, "%f %f %f %f %f %f %f %f", &c.K1.fx, &c.K1.fy, &c.K1.cx, &c.K1.cy, &c.K2.fx, &c.K2.fy, &c.K2.cx, &c.K2.cy) != 8) return 2;
    c.idx1.resize(c.N);
    for (size_t& v : c.idx1) if (fscanf(f, "%zu", &v) != 1) return 2;
    c.X1.resize(3 * c.N); c.X2.resize(3 * c.N); c.e1.resize(c.N); c.e2.resize(c.N);
    if (!read_floats(f, c.X1) || !read_floats(f, c.X2) || !read_floats(f, c.e1) || !read_floats(f, c.e2)) return 2;
  }
  fclose(f);
  try {
    asd::Context ctx(500, 1.2f, 8, 20, 7, 640, 480);
    auto make = [&](const Cand& c, asd::DrawStream& st) {
      std::unique_ptr<asd::Sim3Solver> s(new asd::Sim3Solver(ctx.get(), c.N1, c.idx1, c.X1, c.X2, c.e1, c.e2, c.K1, c.K2, c.fix != 0, st));
      s->SetRansacParameters(0.99, c.min_inliers, c.max_its);
      return s;
    };
    printf("{\"single\": [");
    for (int ci = 0; ci < ncand; ++ci) {
      Scripted src{raw};
      asd::DrawStream st([&src] { return src.next(); }, 2147483647.0);
      auto s = make(cands[ci], st);
      printf("%s{\"max_its\": %d, \"calls\": [", ci ? ", " : "", s->GetMaxIterations());
      for (int call = 0;; ++call) {
        bool bNoMore = false; std::vector<bool> inl; int nInl = 0;
        const bool got = s->iterate(5, bNoMore, inl, nInl);
        printf("%s", call ? ", " : "");
        print_call(*s, got, bNoMore, nInl, inl);
        if (got || bNoMore) break;
      }
      printf("], \"ran_out\": %d}", (int)src.ran_out);
    }
    printf("], \"multi\": {\"hits\": [");
    {
      Scripted src{raw};
      asd::DrawStream st([&src] { return src.next(); }, 2147483647.0);
      std::vector<std::unique_ptr<asd::Sim3Solver>> own;
      std::vector<asd::Sim3Solver*> solvers;
      for (const Cand& c : cands) { own.push_back(make(c, st)); solvers.push_back(own.back().get()); }
      std::vector<bool> discarded(ncand, false);
      int hits = 0, accepted = -1, rounds = 0;
      auto live = [&] { int n = 0; for (bool d : discarded) n += !d; return n; };
      while (live() > 0 && accepted < 0) {
        ++rounds;
        for (int from = 0; from < ncand && accepted < 0;) {
          std::vector<bool> inl; int nInl = 0;
          const int i = asd::LoopClosing::Sim3Round(ctx, solvers, discarded, from, 5, inl, nInl);
          if (i < 0) break;
          printf("%s{\"candidate\": %d, \"round\": %d, \"call\": ", hits ? ", " : "", i, rounds);
          print_call(*solvers[i], true, false, nInl, inl);
          printf("}");
          if (hits++ >= n_reject) accepted = i;
          from = i + 1;
        }
      }
      printf("], \"accepted\": %d, \"rounds\": %d, \"iterations\": [", accepted, rounds);
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
