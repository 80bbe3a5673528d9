// sim3_ransac.hip -- Sim3Solver (reference src/vslam/src/Sim3Solver.cc) on the device: asd_sim3_ransac.
//
// Sim3Solver::iterate (:140-207) is a loop of independent hypotheses -- sample three correspondences (:163-177), Horn's closed form on
// them (ComputeSim3, :226-337), score all N correspondences in both directions (CheckInliers, :340-364) -- followed by a sequential rule
// over the scores (:183-200).  The two halves are the two kernels:
//  * k_sim3_hyp, one workgroup per hypothesis of every problem of the call.  Thread 0 replays the sampling (ransac_sample) and evaluates
//    the model in f64 (a 4x4 cyclic Jacobi is a few hundred operations: not worth spreading), rounds it to f32 once, and the workgroup
//    scores the correspondences in the reference's un-fused f32 operation order (this file is compiled with -ffp-contract=off).
//  * k_sim3_select, one workgroup per problem.  Thread 0 walks the counts in hypothesis order with the reference's rule, the workgroup
//    expands the returned hypothesis's ballot words into inliers[n].
// The sampling, the scoring loop with its ballot words and count, and the host half of the call are ransac.h's.
// No atomics: a call is one bit pattern.  Everything the host reads travels in the context's one result block.
#include "ctx.h"
#include "ransac.h"

namespace {

constexpr int kJacobiSweeps = 24;  // a 4x4 symmetric matrix is diagonal to the last bit after 5-7 sweeps; the cap only bounds a NaN input

// what one hypothesis leaves (result block; asd_debug_sim3_ransac reads the host copy)
struct Sim3HypRec {
  double q[4];   // w x y z, unit
  float T12[16], T21[16], R12[9], t12[3], s;
  int32_t idx[3], count;
};
static_assert(sizeof(Sim3HypRec) == 232, "Sim3HypRec is laid out without holes");

// one problem as the kernels see it (upload block); every pointer is device memory
struct Sim3RansacProb {
  int32_t n, n_iter, hyp_first, fix_scale, min_inliers, best_in, words, pad;
  float K1[4], K2[4];
  const float *X1, *X2, *e1, *e2, *im1, *im2;   // [n][3] x 2, [n] x 2, observed image points [n][2] x 2
  const int32_t* draws;                         // [n_iter][3]
  unsigned long long* masks;                    // [n_iter][words]
  uint8_t* inliers;                             // [n] out
  int32_t* result;                              // [8] out: best_inliers, best_updated, best hypothesis, found, iterations_done, n_inliers
};

struct Sim3Model { float T12[12], T21[12]; };   // rows 0-2 of mT12i / mT21i

// top eigenvector of the symmetric 4x4 A (upper triangle read) by cyclic Jacobi: rotations (p, q) in row order, each annihilating a[p][q]
// with the smaller of the two angles; ends when every off-diagonal element is zero or at the sweep cap.  Returns the column of the
// accumulated rotations that belongs to the largest diagonal element (the first of equal ones).
__host__ __device__ inline void sim3_top_eigenvector(double (&a)[4][4], double (&q)[4]) {
  double v[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    bool zero = true;
    for (int p = 0; p < 3; ++p)
      for (int r = p + 1; r < 4; ++r) zero = zero && a[p][r] == 0.0;
    if (zero) break;
    for (int p = 0; p < 3; ++p)
      for (int r = p + 1; r < 4; ++r) {
        const double apr = a[p][r];
        if (apr == 0.0) continue;
        const double theta = (a[r][r] - a[p][p]) / (2.0 * apr);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        a[p][p] -= t * apr;
        a[r][r] += t * apr;
        a[p][r] = 0.0;
        for (int k = 0; k < 4; ++k) {
          if (k != p && k != r) {
            const int kp0 = k < p ? k : p, kp1 = k < p ? p : k, kr0 = k < r ? k : r, kr1 = k < r ? r : k;
            const double akp = a[kp0][kp1], akr = a[kr0][kr1];
            a[kp0][kp1] = c * akp - s * akr;
            a[kr0][kr1] = s * akp + c * akr;
          }
          const double vkp = v[k][p], vkr = v[k][r];
          v[k][p] = c * vkp - s * vkr;
          v[k][r] = s * vkp + c * vkr;
        }
      }
  }
  int top = 0;
  for (int i = 1; i < 4; ++i) if (a[i][i] > a[top][top]) top = i;
  for (int k = 0; k < 4; ++k) q[k] = v[k][top];
}

// thread 0 of a hypothesis: sampling (:163-177) and ComputeSim3 (:226-337).  (__host__ too: a CPU build can step through it)
__host__ __device__ inline void sim3_hypothesis(const Sim3RansacProb& P, const int k, Sim3HypRec& rec, Sim3Model& mdl) {
  int idx[3];
  ransac_sample<3>(P.draws + 3 * k, P.n, idx);
  double P1[3][3], P2[3][3], O1[3], O2[3];   // [point][xyz]
  for (int i = 0; i < 3; ++i)
    for (int c = 0; c < 3; ++c) { P1[i][c] = (double)P.X1[3 * idx[i] + c]; P2[i][c] = (double)P.X2[3 * idx[i] + c]; }
  for (int c = 0; c < 3; ++c) {   // :215-224
    O1[c] = ((P1[0][c] + P1[1][c]) + P1[2][c]) / 3.0;
    O2[c] = ((P2[0][c] + P2[1][c]) + P2[2][c]) / 3.0;
    for (int i = 0; i < 3; ++i) { P1[i][c] -= O1[c]; P2[i][c] -= O2[c]; }
  }
  double M[3][3];   // M = Pr2 * Pr1^T (:243)
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) M[a][b] = (P2[0][a] * P1[0][b] + P2[1][a] * P1[1][b]) + P2[2][a] * P1[2][b];
  double N[4][4] = {};   // :251-260 (upper triangle)
  N[0][0] = M[0][0] + M[1][1] + M[2][2];
  N[0][1] = M[1][2] - M[2][1];
  N[0][2] = M[2][0] - M[0][2];
  N[0][3] = M[0][1] - M[1][0];
  N[1][1] = M[0][0] - M[1][1] - M[2][2];
  N[1][2] = M[0][1] + M[1][0];
  N[1][3] = M[2][0] + M[0][2];
  N[2][2] = -M[0][0] + M[1][1] - M[2][2];
  N[2][3] = M[1][2] + M[2][1];
  N[3][3] = -M[0][0] - M[1][1] + M[2][2];
  double q[4];
  sim3_top_eigenvector(N, q);
  const double qn = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
  for (int i = 0; i < 4; ++i) q[i] /= qn;
  // the rotation of the unit quaternion.  The reference takes ang = atan2(|vec|, w), the angle-axis vector 2 ang vec / |vec| and cv::Rodrigues
  // (:274-284): the rotation by 2 ang about vec, which is this matrix for q and for -q alike (ang becomes pi - ang and the axis flips)
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                          {2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)},
                          {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)}};
  double s = 1.0;
  if (!P.fix_scale) {   // :292-309: nom = Pr1 . P3, den = sum of P3^2, P3 = R * Pr2
    double nom = 0.0, den = 0.0;
    for (int i = 0; i < 3; ++i)
      for (int r = 0; r < 3; ++r) {
        const double p3 = (R[r][0] * P2[i][0] + R[r][1] * P2[i][1]) + R[r][2] * P2[i][2];
        nom += P1[i][r] * p3;
        den += p3 * p3;
      }
    s = nom / den;
  }
  double t[3], sR[3][3], sRinv[3][3], tinv[3];
  for (int r = 0; r < 3; ++r) {   // :316, :323
    for (int c = 0; c < 3; ++c) sR[r][c] = s * R[r][c];
    t[r] = O1[r] - ((sR[r][0] * O2[0] + sR[r][1] * O2[1]) + sR[r][2] * O2[2]);
  }
  for (int r = 0; r < 3; ++r) {   // :332-335
    for (int c = 0; c < 3; ++c) sRinv[r][c] = (1.0 / s) * R[c][r];
    tinv[r] = -((sRinv[r][0] * t[0] + sRinv[r][1] * t[1]) + sRinv[r][2] * t[2]);
  }
  for (int i = 0; i < 4; ++i) rec.q[i] = q[i];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      rec.R12[3 * r + c] = (float)R[r][c];
      rec.T12[4 * r + c] = (float)sR[r][c];
      rec.T21[4 * r + c] = (float)sRinv[r][c];
    }
    rec.t12[r] = (float)t[r];
    rec.T12[4 * r + 3] = (float)t[r];
    rec.T21[4 * r + 3] = (float)tinv[r];
  }
  for (int c = 0; c < 3; ++c) { rec.T12[12 + c] = 0.f; rec.T21[12 + c] = 0.f; }
  rec.T12[15] = 1.f; rec.T21[15] = 1.f;
  rec.s = (float)s;
  for (int i = 0; i < 3; ++i) rec.idx[i] = idx[i];
  for (int i = 0; i < 12; ++i) { mdl.T12[i] = rec.T12[i]; mdl.T21[i] = rec.T21[i]; }
}

// Project (:382-403) of one point and the squared distance to the observed image point (:350-354), f32, no contraction
__host__ __device__ inline float sim3_reproj_err(const float* T, const float* K, const float X, const float Y, const float Z, const float ou, const float ov,
                                        const bool observed_first) {
  const float xc = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
  const float yc = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
  const float zc = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
  const float invz = 1.0f / zc;
  const float x = xc * invz, y = yc * invz;
  const float u = K[0] * x + K[2], v = K[1] * y + K[3];
  const float du = observed_first ? ou - u : u - ou, dv = observed_first ? ov - v : v - ov;
  return du * du + dv * dv;
}

__global__ __launch_bounds__(kRansacThreads) void k_sim3_hyp(const Sim3RansacProb* probs, const int32_t* hyp_prob, Sim3HypRec* recs) {
  __shared__ Sim3Model mdl;
  __shared__ int s_cnt[kRansacWaves];
  const int h = blockIdx.x, t = threadIdx.x;
  const Sim3RansacProb P = probs[hyp_prob[h]];
  const int k = h - P.hyp_first;
  if (t == 0) {
    Sim3HypRec rec;
    sim3_hypothesis(P, k, rec, mdl);
    rec.count = 0;
    recs[h] = rec;
  }
  asd_syncthreads();
  float T12[12], T21[12];
  for (int i = 0; i < 12; ++i) { T12[i] = mdl.T12[i]; T21[i] = mdl.T21[i]; }
  const int c = ransac_score(P.n, P.words, P.masks + (size_t)k * P.words, s_cnt, [&](const int i) {
    // dist1 = mvP1im1 - Project(mvX3Dc2, T12, K1), dist2 = Project(mvX3Dc1, T21, K2) - mvP2im2 (:343-351)
    const float err1 = sim3_reproj_err(T12, P.K1, P.X2[3 * i], P.X2[3 * i + 1], P.X2[3 * i + 2], P.im1[2 * i], P.im1[2 * i + 1], true);
    const float err2 = sim3_reproj_err(T21, P.K2, P.X1[3 * i], P.X1[3 * i + 1], P.X1[3 * i + 2], P.im2[2 * i], P.im2[2 * i + 1], false);
    return err1 < P.e1[i] && err2 < P.e2[i];   // :356
  });
  if (t == 0) recs[h].count = c;
}

__global__ __launch_bounds__(kRansacThreads) void k_sim3_select(const Sim3RansacProb* probs, const Sim3HypRec* recs) {
  __shared__ int s_found;
  const Sim3RansacProb P = probs[blockIdx.x];
  const int t = threadIdx.x;
  if (P.n_iter == 0) return;   // a problem that runs nothing (the whole workgroup leaves: no barrier is skipped by a part of it)
  if (t == 0) {
    int best = P.best_in, best_h = -1, found = -1, done = P.n_iter;
    for (int k = 0; k < P.n_iter; ++k) {
      const int c = recs[P.hyp_first + k].count;
      if (c >= best) {                                   // :183
        best = c;
        best_h = k;
        if (c > P.min_inliers) { found = k; done = k + 1; break; }   // :192-199
      }
    }
    s_found = found;
    P.result[0] = best; P.result[1] = best_h >= 0; P.result[2] = best_h; P.result[3] = found >= 0; P.result[4] = done;
    P.result[5] = found >= 0 ? best : 0; P.result[6] = 0; P.result[7] = 0;
  }
  asd_syncthreads();
  const int found = s_found;
  const unsigned long long* const mask = found >= 0 ? P.masks + (size_t)found * P.words : nullptr;
  for (int i = t; i < P.n; i += kRansacThreads) P.inliers[i] = mask ? ransac_mask_bit(mask, i) : (uint8_t)0;
}

using Sim3RansacState = RansacRecords<Sim3HypRec>;

}  // namespace

void sim3_ransac_free(asd_ctx* ctx) {
  delete static_cast<Sim3RansacState*>(ctx->sim3_ransac);
  ctx->sim3_ransac = nullptr;
}

extern "C" {

int asd_sim3_ransac(asd_ctx* ctx, int32_t n_problems, asd_sim3_ransac_problem* p) {
  if (const int e = ransac_check_call(ctx, "asd_sim3_ransac", n_problems, p, ASD_SIM3_RANSAC_MAX_PROBLEMS)) return e;
  // ---- validation: nothing is written before every problem has passed
  std::vector<int32_t> hyps(n_problems, 0);   // the iterations of a problem that runs
  size_t total = 0, up_bytes = 0, down_bytes = 0, mask_bytes = 0;
  for (int32_t j = 0; j < n_problems; ++j) {
    const asd_sim3_ransac_problem& q = p[j];
    if (q.n < 0 || q.n_iter < 0) { ctx->set_error("asd_sim3_ransac: problem %d: negative n or n_iter", j); return ASD_ERR_INVALID; }
    if (q.n < q.min_inliers || q.n_iter == 0) continue;   // :146-150; no iteration left: nothing to launch
    if (q.n > ASD_SIM3_RANSAC_MAX_N) {
      ctx->set_error("asd_sim3_ransac: problem %d: %d correspondences, the limit is %d", j, q.n, ASD_SIM3_RANSAC_MAX_N);
      return ASD_ERR_CAPACITY;
    }
    if (q.n < 3) { ctx->set_error("asd_sim3_ransac: problem %d: n = %d, an iteration samples three correspondences", j, q.n); return ASD_ERR_INVALID; }
    if (!q.X1c || !q.X2c || !q.max_err1 || !q.max_err2 || !q.draws || !q.inliers) {
      ctx->set_error("asd_sim3_ransac: problem %d: null array", j);
      return ASD_ERR_INVALID;
    }
    if (!ransac_check_draws(ctx, "asd_sim3_ransac", j, q.draws, q.n_iter, 3, q.n)) return ASD_ERR_INVALID;
    hyps[j] = q.n_iter;
    total += (size_t)q.n_iter;
    if (total > ASD_SIM3_RANSAC_MAX_HYPOTHESES) {
      ctx->set_error("asd_sim3_ransac: problem %d brings the call to %zu iterations, the limit is %d", j, total, ASD_SIM3_RANSAC_MAX_HYPOTHESES);
      return ASD_ERR_CAPACITY;
    }
    up_bytes += (size_t)q.n * 48 + (size_t)q.n_iter * 12 + 8 * 256;
    down_bytes += (size_t)q.n + 32 + 2 * 256;
    mask_bytes += AsdDevBuf::padded((size_t)q.n_iter * (((size_t)q.n + 63) / 64) * 8);
  }
  if (!ctx->sim3_ransac) ctx->sim3_ransac = new Sim3RansacState();
  Sim3RansacState* S = static_cast<Sim3RansacState*>(ctx->sim3_ransac);
  S->reset(n_problems);
  for (int32_t j = 0; j < n_problems; ++j)
    if (!hyps[j]) ransac_runs_nothing(p[j]);   // :146-150, or no iteration left (:158)
  ctx->ms_sim3_ransac = 0;
  if (total == 0) return ASD_OK;
  std::vector<size_t> off_inl(n_problems, 0), off_res(n_problems, 0);
  hipStream_t st = ctx->stream;
  const auto pack = [&](const int32_t j, Sim3RansacProb& d) {
    const asd_sim3_ransac_problem& q = p[j];
    const size_t n = (size_t)q.n;
    d.n = q.n; d.n_iter = q.n_iter; d.fix_scale = q.fix_scale ? 1 : 0; d.min_inliers = q.min_inliers; d.best_in = q.best_inliers;
    d.words = (int32_t)((n + 63) / 64);
    memcpy(d.K1, q.K1, 16); memcpy(d.K2, q.K2, 16);
    d.X1 = ctx->up.dev<float>(ctx->up.add(q.X1c, n * 12));
    d.X2 = ctx->up.dev<float>(ctx->up.add(q.X2c, n * 12));
    d.e1 = ctx->up.dev<float>(ctx->up.add(q.max_err1, n * 4));
    d.e2 = ctx->up.dev<float>(ctx->up.add(q.max_err2, n * 4));
    // FromCameraToImage (:405-423), once per problem, in the arithmetic of Project (f32, no contraction, IEEE division)
    const size_t off_im1 = ctx->up.reserve(n * 8), off_im2 = ctx->up.reserve(n * 8);
    float *im1 = ctx->up.host<float>(off_im1), *im2 = ctx->up.host<float>(off_im2);
    for (size_t i = 0; i < n; ++i) {
      float invz = 1.0f / q.X1c[3 * i + 2], x = q.X1c[3 * i] * invz, y = q.X1c[3 * i + 1] * invz;
      im1[2 * i] = q.K1[0] * x + q.K1[2]; im1[2 * i + 1] = q.K1[1] * y + q.K1[3];
      invz = 1.0f / q.X2c[3 * i + 2]; x = q.X2c[3 * i] * invz; y = q.X2c[3 * i + 1] * invz;
      im2[2 * i] = q.K2[0] * x + q.K2[2]; im2[2 * i + 1] = q.K2[1] * y + q.K2[3];
    }
    d.im1 = ctx->up.dev<float>(off_im1);
    d.im2 = ctx->up.dev<float>(off_im2);
    d.draws = ctx->up.dev<int32_t>(ctx->up.add(q.draws, (size_t)q.n_iter * 12));
    d.masks = ctx->scratch.carve<unsigned long long>((size_t)q.n_iter * d.words);
    off_inl[j] = ctx->down.reserve(n);
    off_res[j] = ctx->down.reserve(32);
    d.inliers = ctx->down.dev<uint8_t>(off_inl[j]);
    d.result = ctx->down.dev<int32_t>(off_res[j]);
  };
  const int e = ransac_run<Sim3RansacProb>(
      ctx, hyps, up_bytes, down_bytes, mask_bytes + 256, total, &ctx->ms_sim3_ransac, nullptr, *S, pack,
      [&](unsigned grid, const Sim3RansacProb* probs, const int32_t* map, Sim3HypRec* recs) {
        hipLaunchKernelGGL(k_sim3_hyp, dim3(grid), dim3(kRansacThreads), 0, st, probs, map, recs);
      },
      [&](unsigned grid, const Sim3RansacProb* probs, const Sim3HypRec* recs) {
        hipLaunchKernelGGL(k_sim3_select, dim3(grid), dim3(kRansacThreads), 0, st, probs, recs);
      });
  if (e != ASD_OK) return e;
  for (int32_t j = 0; j < n_problems; ++j) {
    if (!hyps[j]) continue;
    asd_sim3_ransac_problem& q = p[j];
    const int32_t* r = ctx->down.host<int32_t>(off_res[j]);
    q.best_inliers = r[0];
    q.best_updated = r[1];
    if (r[1]) {   // :185-190
      const Sim3HypRec& b = S->recs[S->first[j] + r[2]];
      memcpy(q.R12, b.R12, sizeof q.R12);
      memcpy(q.t12, b.t12, sizeof q.t12);
      memcpy(q.T12, b.T12, sizeof q.T12);
      q.s12 = b.s;
    }
    q.found = r[3];
    q.iterations_done = r[4];
    q.n_inliers = r[5];
    memcpy(q.inliers, ctx->down.host<uint8_t>(off_inl[j]), (size_t)q.n);
  }
  return ASD_OK;
}

int32_t asd_debug_sim3_ransac(const asd_ctx* ctx, int32_t problem, int32_t hypothesis, asd_sim3_ransac_debug* out) {
  if (!ctx || !out) return ASD_ERR_INVALID;
  const Sim3RansacState* S = static_cast<const Sim3RansacState*>(ctx->sim3_ransac);
  if (!S || problem < 0 || problem >= (int32_t)S->count.size() || hypothesis < 0 || hypothesis >= S->count[problem]) return ASD_ERR_INVALID;
  const Sim3HypRec& r = S->recs[(size_t)S->first[problem] + hypothesis];
  memcpy(out->idx, r.idx, sizeof out->idx);
  out->count = r.count;
  memcpy(out->T12, r.T12, sizeof out->T12);
  memcpy(out->T21, r.T21, sizeof out->T21);
  out->s = r.s;
  memcpy(out->q, r.q, sizeof out->q);
  return ASD_OK;
}

}  // extern "C"
