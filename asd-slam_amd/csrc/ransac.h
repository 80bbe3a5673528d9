// ransac.h -- what the three device RANSACs share: sim3_ransac.hip (Sim3Solver), pnp_ransac.hip (PnPsolver), initializer.hip (Initializer).
//
// Each of them is two kernels -- one workgroup per hypothesis (sample, model, score all correspondences), then one workgroup per problem
// (the reference's sequential rule over the scores) -- behind one entry point that validates, packs one upload block, launches the two
// and unpacks one result block.  The parts that do not depend on the model are here, each once:
//  * ransac_sample<K>    the swap-with-back sampling of K correspondences (host + device)
//  * jacobi_svd<floor>   the one-sided Jacobi SVD of the small dense systems (host + device)
//  * ransac_mask_bit     one decision out of the ballot words (host + device)
//  * ransac_ballot_word  a wave's 64 decisions into their word; ransac_score: the scoring loop around it with the count
//  * wg_sum              the workgroup sum of N doubles in one fixed shape (sim3.hip's Levenberg passes use it too)
//  * ransac_check_call, ransac_check_draws, ransac_runs_nothing, RansacRecords, ransac_run: the host half of an entry point
// The first three compile as plain C++ (host/test_ransac_common.cpp tests them without a device); the rest needs hipcc.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include "ctx.h"
#define ASD_HD __host__ __device__ inline
#define ASD_UNROLL _Pragma("unroll")
#else
#define ASD_HD inline
#define ASD_UNROLL
#endif

// The reference keeps vAvailableIndices = 0 .. n-1; draw j takes position r = draws[j] and moves the back element (position n-1-j) there.
// K draws touch at most K-1 positions before the last read, so the vector is the identity plus overrides: idx[j] is what position
// draws[j] holds, a later override of a position in front of an earlier one.  Integers only, fully unrolled: no private array is
// indexed by a run-time value.
template <int K>
ASD_HD void ransac_sample(const int32_t* draws, const int n, int (&idx)[K]) {
  int opos[K], oval[K];
  ASD_UNROLL
  for (int j = 0; j < K; ++j) {
    const int r = draws[j], back = n - j - 1;
    int v = r, b = back;
    ASD_UNROLL
    for (int m = 0; m < K; ++m)
      if (m < j) {
        if (opos[m] == r) v = oval[m];
        if (opos[m] == back) b = oval[m];
      }
    idx[j] = v;
    opos[j] = r; oval[j] = b;
  }
}

// one-sided (Hestenes) Jacobi SVD of W [m][n]: on return W = U Sigma (orthogonal columns), V [n][n] the right vectors, sig[j] = |W[:, j]|.
// Ends when a sweep rotates nothing; max_sweeps only bounds a NaN input.  kNullFloor: a column at rounding level of the whole matrix is a
// null column and is not orthogonalised against noise (the Initializer's A has one by construction; F: 8 rows for 9 columns).
template <bool kNullFloor>
ASD_HD void jacobi_svd(double* W, double* V, double* sig, const int m, const int n, const int max_sweeps) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) V[i * n + j] = i == j ? 1.0 : 0.0;
  double floor2 = 0.0;
  if (kNullFloor) {
    double fro2 = 0.0;
    for (int i = 0; i < m * n; ++i) fro2 += W[i] * W[i];
    floor2 = (8.0 * DBL_EPSILON) * (8.0 * DBL_EPSILON) * fro2;
  }
  for (int sweep = 0; sweep < max_sweeps; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int i = 0; i < m; ++i) {
          const double wp = W[i * n + p], wq = W[i * n + q];
          alpha += wp * wp; beta += wq * wq; gamma += wp * wq;
        }
        if (kNullFloor && (alpha <= floor2 || beta <= floor2)) continue;   // nothing to orthogonalise against noise
        if (!(fabs(gamma) > DBL_EPSILON * sqrt(alpha * beta))) continue;   // orthogonal to rounding (or NaN)
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int i = 0; i < m; ++i) {
          const double wp = W[i * n + p], wq = W[i * n + q];
          W[i * n + p] = c * wp - s * wq;
          W[i * n + q] = s * wp + c * wq;
        }
        for (int i = 0; i < n; ++i) {
          const double vp = V[i * n + p], vq = V[i * n + q];
          V[i * n + p] = c * vp - s * vq;
          V[i * n + q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  for (int j = 0; j < n; ++j) {
    double s2 = 0.0;
    for (int i = 0; i < m; ++i) s2 += W[i * n + j] * W[i * n + j];
    sig[j] = sqrt(s2);
  }
}

// decision i of a hypothesis: bit i & 63 of ballot word i >> 6
ASD_HD uint8_t ransac_mask_bit(const unsigned long long* mask, const int i) { return (uint8_t)((mask[i >> 6] >> (i & 63)) & 1ull); }

#if defined(__HIPCC__)

constexpr int kRansacThreads = 256, kRansacWaves = kRansacThreads / 64;   // the workgroup of all six kernels

// One trip of a scoring loop: the 64 decisions of this wave as one ballot word.  Every lane of the workgroup must get here (uniform trip
// count); the last trip's waves beyond the correspondences have no word.
__device__ inline void ransac_ballot_word(const bool in, const int base, const int words, unsigned long long* mask) {
  const unsigned long long bal = __ballot(in);
  const int word = (base >> 6) + (int)(threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0 && word < words) mask[word] = bal;
}

// The scoring loop of a hypothesis by the whole workgroup: inlier(i) for every correspondence i < n, the ballot words into mask, and
// the count in one fixed shape (wave butterfly, then the waves in order) returned to every thread.  Two barriers: the first lets s_cnt
// [kRansacWaves] be used again while a thread may still be reading the previous count.
template <class Pred>
__device__ inline int ransac_score(const int n, const int words, unsigned long long* mask, int* s_cnt, Pred inlier) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int mine = 0;
  for (int base = 0; base < n; base += kRansacThreads) {   // (uniform trip count: every lane reaches the ballot)
    const int i = base + t;
    const bool in = i < n && inlier(i);
    ransac_ballot_word(in, base, words, mask);
    mine += in ? 1 : 0;
  }
  for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off);
  asd_syncthreads();   // (the previous count has been read by everyone)
  if (lane == 0) s_cnt[wave] = mine;
  asd_syncthreads();
  int c = s_cnt[0];
  for (int w = 1; w < kRansacWaves; ++w) c += s_cnt[w];
  return c;
}

// acc[N] -> sums[0 .. N): lanes of a wave by butterfly, then the waves in order.  Two barriers; every thread may read sums behind it.
// Called by a whole workgroup of WAVES waves; red and sums are its LDS.
template <int N, int WAVES, int M>
__device__ inline void wg_sum(double (&acc)[N], double (&red)[WAVES][M], double (&sums)[M]) {
  static_assert(N <= M, "the LDS rows hold fewer sums than the caller adds");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) red[wave][k] = v;
  }
  asd_syncthreads();
  if (threadIdx.x < N) {
    double s = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += red[w][threadIdx.x];   // fixed order
    sums[threadIdx.x] = s;
  }
  asd_syncthreads();
}

// ---- the host half of an entry point

// the arguments every entry point checks first: ASD_OK, or the status to return (with the message set where there is one)
inline int ransac_check_call(asd_ctx* ctx, const char* name, const int32_t n_problems, const void* p, const int32_t max_problems) {
  if (ctx && asd_track_busy(ctx, name)) return ASD_ERR_INVALID;
  if (!ctx || n_problems < 0 || (n_problems > 0 && !p)) return ASD_ERR_INVALID;
  if (n_problems > max_problems) {
    ctx->set_error("%s: %d problems in one call, the limit is %d", name, n_problems, max_problems);
    return ASD_ERR_CAPACITY;
  }
  return ASD_OK;
}

// draws [n_iter][K] of problem j over n correspondences: draw i of an iteration indexes a vector of n - i elements
inline bool ransac_check_draws(asd_ctx* ctx, const char* name, const int32_t j, const int32_t* draws, const int32_t n_iter, const int K,
                               const int32_t n) {
  for (int32_t k = 0; k < n_iter; ++k)
    for (int i = 0; i < K; ++i) {
      const int32_t r = draws[K * k + i];
      if (r < 0 || r > n - 1 - i) {
        ctx->set_error("%s: problem %d: draws[%d][%d] = %d is outside [0, %d]", name, j, k, i, r, n - 1 - i);
        return false;
      }
    }
  return true;
}

// a problem of asd_sim3_ransac / asd_pnp_ransac that has no iteration to run: with enough correspondences iterate()'s loop body is not
// entered; with fewer than min_inliers the reference returns at once and nothing else is written
template <class Problem>
inline void ransac_runs_nothing(Problem& q) {
  q.found = 0; q.iterations_done = 0;
  if (q.n < q.min_inliers) return;
  q.best_updated = 0; q.n_inliers = 0;
  if (q.inliers && q.n > 0) memset(q.inliers, 0, (size_t)q.n);
}

// the records of the last call, kept for the asd_debug_* entry point: problem j's are recs[first[j] .. first[j] + count[j])
template <class Rec>
struct RansacRecords {
  std::vector<Rec> recs;
  std::vector<int32_t> first, count;
  void reset(const size_t n_problems) {
    recs.clear();
    first.assign(n_problems, 0);
    count.assign(n_problems, 0);
  }
};

// The launch sequence of a call whose problem j brings hyps[j] hypothesis workgroups (0: the problem runs nothing).  Begins the upload
// and result blocks and the scratch arena with room for the caller's estimates beside what is placed here: Prob[n_problems] and the
// hypothesis-to-problem map in the upload block, Rec[n_recs] in the result block.  pack(j, prob) fills problem j (zeroed, hyp_first
// set) and reserves what it points to; launch_hyp(grid, probs, map, recs) and launch_select(grid, probs, recs) enqueue the two kernels
// on ctx->stream.  *ms = the device time of upload and kernels; ms_hyp (optional) = of upload and the first kernel.  Leaves the records
// and each problem's first / count in `out`; the result block stays valid until the next call begins it.
template <class Prob, class Rec, class Pack, class LaunchHyp, class LaunchSelect>
inline int ransac_run(asd_ctx* ctx, const std::vector<int32_t>& hyps, const size_t up_bytes, const size_t down_bytes, const size_t scratch_bytes,
                      const size_t n_recs, float* ms, float* ms_hyp, RansacRecords<Rec>& out, Pack pack, LaunchHyp launch_hyp,
                      LaunchSelect launch_select) {
  const size_t n_problems = hyps.size();
  size_t total = 0;
  for (const int32_t c : hyps) total += (size_t)c;
  (void)hipSetDevice(ctx->cfg.device);
  hipStream_t st = ctx->stream;
  ASD_HIP_CHECK(ctx, ctx->up.begin(st, up_bytes + n_problems * sizeof(Prob) + total * 4 + 1024));
  ASD_HIP_CHECK(ctx, ctx->down.begin(st, down_bytes + n_recs * sizeof(Rec) + 1024));
  ASD_HIP_CHECK(ctx, ctx->scratch.reserve(scratch_bytes));
  const size_t off_probs = ctx->up.reserve(n_problems * sizeof(Prob)), off_map = ctx->up.reserve(total * 4);
  const size_t off_recs = ctx->down.reserve(n_recs * sizeof(Rec));
  Prob* hp = ctx->up.host<Prob>(off_probs);
  int32_t* hmap = ctx->up.host<int32_t>(off_map);
  size_t hyp = 0;
  for (size_t j = 0; j < n_problems; ++j) {
    memset(&hp[j], 0, sizeof(Prob));
    hp[j].hyp_first = (int32_t)hyp;
    if (!hyps[j]) continue;  // n = n_iter = 0: the second kernel's workgroup of this problem touches nothing
    pack((int32_t)j, hp[j]);
    for (int32_t k = 0; k < hyps[j]; ++k) hmap[hyp + k] = (int32_t)j;
    hyp += (size_t)hyps[j];
  }
  ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, st));
  ASD_HIP_CHECK(ctx, ctx->up.upload(st));
  launch_hyp((unsigned)total, ctx->up.dev<Prob>(off_probs), ctx->up.dev<int32_t>(off_map), ctx->down.dev<Rec>(off_recs));
  ASD_HIP_CHECK(ctx, hipGetLastError());
  if (ms_hyp) ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev2, st));
  launch_select((unsigned)n_problems, ctx->up.dev<Prob>(off_probs), ctx->down.dev<Rec>(off_recs));
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, st));
  ASD_HIP_CHECK(ctx, ctx->down.download(st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  ASD_HIP_CHECK(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
  if (ms_hyp) ASD_HIP_CHECK(ctx, hipEventElapsedTime(ms_hyp, ctx->ev0, ctx->ev2));
  const Rec* recs = ctx->down.host<Rec>(off_recs);
  out.recs.assign(recs, recs + n_recs);
  for (size_t j = 0; j < n_problems; ++j) { out.first[j] = hp[j].hyp_first; out.count[j] = hyps[j]; }
  return ASD_OK;
}

#endif  // __HIPCC__
