// test_ransac_common.cpp -- the host-callable pieces of csrc/ransac.h without a device (tests/test_ransac_common_host.py).
//
//  (a) ransac_sample<K>, K = 3, 4, 8, against the literal replay (a vector 0 .. n-1, take [r], overwrite with back(), pop_back()):
//      every draw tuple at n = K and n = K + 1 -- where the aliasing cases live: r == size - 1, a position drawn twice, the back
//      element already overridden -- and 10^5 seeded tuples at n = 64 and n = 2000.
//  (b) jacobi_svd<true> and <false> on seeded 16x9, 8x9, 6x5, 6x3 and 3x3 matrices, a 6x5 with a zero column and a 6x5 with two equal
//      columns:
//       * the columns of W are mutually orthogonal: |w_p . w_q| <= DBL_EPSILON |W|_F^2 (the sweep's own test is DBL_EPSILON |w_p| |w_q|);
//       * W V^T reproduces the input: every element to 8 DBL_EPSILON |A|_F.  An element goes through at most sweeps x (n - 1) <= ~80
//         rotations of ~1 ulp of its column's norm each, errors of either sign: "a few ulp" of the whole matrix's norm;
//       * on a matrix of full column rank the two template forms return identical bits (the floor test never fires).  8x9, the zero
//         column and the equal columns have a null column -- what the floor is for -- and are reported, not compared.
// Prints one line per check and "ok" at the end; the exit status is the number of failed checks.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../csrc/ransac.h"

namespace {

int failures = 0;

template <int K>
bool sample_equals_replay(const int32_t* draws, const int n) {
  std::vector<int> avail(n);
  for (int i = 0; i < n; ++i) avail[i] = i;
  int want[K], got[K];
  for (int j = 0; j < K; ++j) {
    const int r = draws[j];
    want[j] = avail[r];
    avail[r] = avail.back();
    avail.pop_back();
  }
  ransac_sample<K>(draws, n, got);
  return memcmp(want, got, sizeof want) == 0;
}

template <int K>
void test_sample() {
  long long bad = 0, count = 0;
  for (int n = K; n <= K + 1; ++n) {   // every tuple: draw j in [0, n - 1 - j]
    int32_t d[K] = {};
    for (;;) {
      bad += !sample_equals_replay<K>(d, n);
      ++count;
      int j = K - 1;
      while (j >= 0 && ++d[j] > n - 1 - j) d[j--] = 0;
      if (j < 0) break;
    }
  }
  std::mt19937_64 rng(1000 + K);
  for (const int n : {64, 2000})
    for (int t = 0; t < 100000; ++t) {
      int32_t d[K];
      for (int j = 0; j < K; ++j) d[j] = (int32_t)(rng() % (unsigned long long)(n - j));
      bad += !sample_equals_replay<K>(d, n);
      ++count;
    }
  printf("sample K=%d: %lld tuples, %lld differ from the replay\n", K, count, bad);
  failures += bad != 0;
}

struct Svd {
  std::vector<double> W, V, sig;
};
template <bool kNullFloor>
Svd run_svd(const std::vector<double>& A, const int m, const int n) {
  Svd r{A, std::vector<double>((size_t)n * n), std::vector<double>(n)};
  jacobi_svd<kNullFloor>(r.W.data(), r.V.data(), r.sig.data(), m, n, 60);
  return r;
}

// the two figures of one decomposition, each as a multiple of its bound's unit
void check_svd(const char* name, const char* form, const std::vector<double>& A, const int m, const int n, const Svd& r) {
  double fro2 = 0.0, w2 = 0.0;
  for (const double a : A) fro2 += a * a;
  for (const double w : r.W) w2 += w * w;
  double orth = 0.0, rec = 0.0;
  for (int p = 0; p < n - 1; ++p)
    for (int q = p + 1; q < n; ++q) {
      double gamma = 0.0;
      for (int i = 0; i < m; ++i) gamma += r.W[i * n + p] * r.W[i * n + q];
      orth = std::fmax(orth, std::fabs(gamma));
    }
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < n; ++j) {
      long double s = 0.0L;
      for (int k = 0; k < n; ++k) s += (long double)r.W[i * n + k] * (long double)r.V[j * n + k];
      rec = std::fmax(rec, std::fabs((double)(s - (long double)A[i * n + j])));
    }
  const double orth_u = orth / (DBL_EPSILON * w2), rec_u = rec / (DBL_EPSILON * std::sqrt(fro2));
  const bool ok = orth_u <= 1.0 && rec_u <= 8.0;
  printf("svd %-10s %s: max |w_p.w_q| = %.3f eps |W|^2 (bound 1), max |W V^T - A| = %.3f eps |A| (bound 8)%s\n", name, form, orth_u, rec_u,
         ok ? "" : "  FAILED");
  failures += !ok;
}

void test_svd(const char* name, const std::vector<double>& A, const int m, const int n, const bool full_rank) {
  const Svd t = run_svd<true>(A, m, n), f = run_svd<false>(A, m, n);
  check_svd(name, "<true> ", A, m, n, t);
  check_svd(name, "<false>", A, m, n, f);
  const bool same = memcmp(t.W.data(), f.W.data(), t.W.size() * 8) == 0 && memcmp(t.V.data(), f.V.data(), t.V.size() * 8) == 0 &&
                    memcmp(t.sig.data(), f.sig.data(), t.sig.size() * 8) == 0;
  if (full_rank) {
    printf("svd %-10s <true> and <false>: %s\n", name, same ? "identical bits" : "DIFFERENT BITS  FAILED");
    failures += !same;
  } else {
    printf("svd %-10s <true> and <false>: %s (a null column: not compared)\n", name, same ? "identical bits" : "different bits");
  }
}

std::vector<double> seeded(const int m, const int n, const unsigned seed) {
  std::mt19937_64 rng(seed);
  std::vector<double> A((size_t)m * n);
  for (double& a : A) a = (double)(long long)(rng() >> 11) / 9007199254740992.0 * 2.0 - 1.0;   // [-1, 1), 53 bits
  return A;
}

}  // namespace

int main() {
  test_sample<3>();
  test_sample<4>();
  test_sample<8>();
  test_svd("16x9", seeded(16, 9, 1), 16, 9, true);
  test_svd("8x9", seeded(8, 9, 2), 8, 9, false);
  test_svd("6x5", seeded(6, 5, 3), 6, 5, true);
  test_svd("6x3", seeded(6, 3, 4), 6, 3, true);
  test_svd("3x3", seeded(3, 3, 5), 3, 3, true);
  std::vector<double> Z = seeded(6, 5, 6), E = seeded(6, 5, 7);
  for (int i = 0; i < 6; ++i) { Z[i * 5 + 2] = 0.0; E[i * 5 + 3] = E[i * 5 + 1]; }
  test_svd("6x5 zero", Z, 6, 5, false);
  test_svd("6x5 equal", E, 6, 5, false);
  if (!failures) printf("ok\n");
  return failures;
}
