// sim3.hip -- Optimizer::OptimizeSim3 (reference src/vslam/src/Optimizer.cc:1002-1194) on the device: asd_optimize_sim3.
//
// One persistent workgroup per call, as k_pose_opt (ba.hip): the Levenberg loop of g2o (optimization_algorithm_levenberg.cpp:61-164)
// is a state machine run by thread 0 between the passes over the edges.  What differs from PoseOptimization:
//  * the edge classes have no analytic Jacobian (types_seven_dof_expmap.h:147, :169, :191), so g2o differentiates numerically
//    (base_binary_edge.hpp:130-206): central differences, delta = 1e-9, each perturbed estimate Sim3(+-delta e_d) * estimate through
//    oplusImpl.  That is the reference's optimiser and this kernel does the same -- an analytic Jacobian converges to another point of
//    the differencing noise floor.  The 14 perturbed Sim3s and their inverses depend on the vertex only: 15 lanes build them once per
//    linearisation into LDS, and an edge costs 15 maps and projections;
//  * so a linearisation is 15 times a plain evaluation, and the two are separate passes: an iteration is one linearising pass at the
//    current estimate (errors, robust chi2, H, b -- g2o's computeActiveErrors + buildSystem) and one error-only pass per trial;
//  * two rounds, the second continuing from the first's estimate; the re-classification between them reads chi2() WITHOUT
//    computeError() (:1146, :1180): the errors of the round's last computeActiveErrors, i.e. of its last pass -- after a round that
//    ended on a rejected trial, the rejected trial's.  The kernel keeps the Sim3 of the last pass (S.eval) and re-evaluates there
//    with the pass's own arithmetic, as PoseOptimization's re-classification does.
// Reductions have one fixed shape (wg_sum, ransac.h: wave butterfly, then the waves in order) and there are no atomics: a call is one bit pattern.
// The edge data stays in global memory (SoA [12][n], read once per pass).
#include "ctx.h"
#include "ransac.h"
#include "sim3_math.h"

namespace {

constexpr int kSim3Threads = 256, kSim3Waves = kSim3Threads / 64;
constexpr int kSim3Sums = 37;   // 28 upper H, 7 b, robust chi2, active edges
constexpr int kSim3TraceInts = ASD_SIM3_OPT_DEBUG_INTS;
static_assert(kSim3TraceInts == 12, "k_sim3_opt writes 2 x 4 + 4 values");

struct Sim3OptArgs {
  int n;
  const double* soa;   // [12][n]: P1c xyz, P2c xyz, obs1 uv, obs2 uv, inv_sigma2_1, inv_sigma2_2
  uint8_t* keep;       // [n] out (and the active set of round two)
  double* io;          // out: sim3[8], then int32: trace[12], n_in, early
  double sim3[8];
  double K1[4], K2[4];
  double th2;          // (double)th2
  double huber;        // (double)sqrtf(th2): Optimizer.cc:1048 computes the kernel's delta in float
  int fix_scale;
};

struct Sim3Shared {
  Sim3d cur, bak, eval;       // the estimate, the estimate in front of the trial, where the last pass evaluated the errors
  Sim3d P[15], Pinv[15];      // linearisation: [0] the estimate, [1 + 2 d] / [2 + 2 d] = Sim3(+-delta e_d) * estimate, and their inverses
  double H[49], b[7], x[7];
  double sums[kSim3Sums + 3];
  double red[kSim3Waves][kSim3Sums + 3];
  double lambda, ni, currentChi, iniChi;
  int qmax, cont, ok, it, nBadIt;
  int tr[4];   // per round: active edges, iterations (optimize()'s return), trials, ended on a rejected trial
};

struct Sim3Pair {
  double X1, Y1, Z1, X2, Y2, Z2, u1, v1, u2, v2, is1, is2;
};
__device__ inline Sim3Pair sim3_load(const Sim3OptArgs& a, int i) {
  const size_t n = (size_t)a.n;
  const double* p = a.soa + i;
  return Sim3Pair{p[0], p[n], p[2 * n], p[3 * n], p[4 * n], p[5 * n], p[6 * n], p[7 * n], p[8 * n], p[9 * n], p[10 * n], p[11 * n]};
}

// the two errors of a pair at (S, Sinv): e12 = obs1 - K1 project(S P2c), e21 = obs2 - K2 project(S^-1 P1c)
__device__ inline void sim3_errors(const Sim3OptArgs& a, const Sim3Pair& p, const Sim3d& S, const Sim3d& Sinv, double (&e)[4]) {
  s3_project_error(S, p.X2, p.Y2, p.Z2, p.u1, p.v1, a.K1[0], a.K1[1], a.K1[2], a.K1[3], e[0], e[1]);
  s3_project_error(Sinv, p.X1, p.Y1, p.Z1, p.u2, p.v2, a.K2[0], a.K2[1], a.K2[2], a.K2[3], e[2], e[3]);
}

// error-only pass at S.cur (a Levenberg trial: computeActiveErrors + activeRobustChi2): S.sums[0] = robust chi2
__device__ inline void sim3_pass_errors(const Sim3OptArgs& a, Sim3Shared& S) {
  const Sim3d Sc = S.cur, Si = s3_inverse(Sc);
  double acc[1] = {0.0};
  for (int i = threadIdx.x; i < a.n; i += kSim3Threads) {
    if (!a.keep[i]) continue;
    const Sim3Pair p = sim3_load(a, i);
    double e[4], r0, r1;
    sim3_errors(a, p, Sc, Si, e);
    huber(s3_chi2(e[0], e[1], p.is1), a.huber, r0, r1);
    acc[0] += r0;
    huber(s3_chi2(e[2], e[3], p.is2), a.huber, r0, r1);
    acc[0] += r0;
  }
  wg_sum(acc, S.red, S.sums);
}

// H (upper, 28) and b (7) of one edge: J = numeric 2 x 7, weighted Omega = rho' inv_sigma2 I, b += J^T (-(Omega e) rho')
__device__ inline void sim3_add_edge(double (&acc)[kSim3Sums], const double (&J0)[7], const double (&J1)[7], double e0, double e1, double isg,
                                     double rho1) {
  const double om = rho1 * isg;
  const double r0 = -(isg * e0) * rho1, r1 = -(isg * e1) * rho1;
  int k = 0;
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    const double w0 = J0[r] * om, w1 = J1[r] * om;
#pragma unroll
    for (int c = r; c < 7; ++c) { acc[k] += w0 * J0[c] + w1 * J1[c]; ++k; }
  }
#pragma unroll
  for (int r = 0; r < 7; ++r) acc[28 + r] += J0[r] * r0 + J1[r] * r1;
}

// linearising pass at S.cur: the perturbed estimates, then per active pair the errors at the estimate and the central differences
// (base_binary_edge.hpp:147-198: scalar = 1 / (2 delta), column d = scalar * (e(+delta) - e(-delta))).
// S.sums[0..27] = upper H, [28..34] = b, [35] = robust chi2, [36] = active edges
__device__ inline void sim3_pass_linearise(const Sim3OptArgs& a, Sim3Shared& S) {
  if (threadIdx.x < 15) {
    const int k = threadIdx.x;
    Sim3d P = S.cur;
    if (k > 0) {
      const int d = (k - 1) >> 1;
      const double delta = (k & 1) ? 1e-9 : -1e-9;
      double u[7];
#pragma unroll
      for (int q = 0; q < 7; ++q) u[q] = q == d ? delta : 0.0;
      P = s3_oplus(S.cur, u, a.fix_scale != 0);
    }
    S.P[k] = P;
    S.Pinv[k] = s3_inverse(P);
  }
  asd_syncthreads();
  const double scalar = 1.0 / (2 * 1e-9);
  double acc[kSim3Sums];
#pragma unroll
  for (int k = 0; k < kSim3Sums; ++k) acc[k] = 0.0;
  for (int i = threadIdx.x; i < a.n; i += kSim3Threads) {
    if (!a.keep[i]) continue;
    const Sim3Pair p = sim3_load(a, i);
    double e[4], Ja[7], Jb[7], Jc[7], Jd[7];
    sim3_errors(a, p, S.P[0], S.Pinv[0], e);
#pragma unroll
    for (int d = 0; d < 7; ++d) {
      double ep[4], em[4];
      sim3_errors(a, p, S.P[1 + 2 * d], S.Pinv[1 + 2 * d], ep);
      sim3_errors(a, p, S.P[2 + 2 * d], S.Pinv[2 + 2 * d], em);
      Ja[d] = scalar * (ep[0] - em[0]); Jb[d] = scalar * (ep[1] - em[1]);
      Jc[d] = scalar * (ep[2] - em[2]); Jd[d] = scalar * (ep[3] - em[3]);
    }
    double r0, r1;
    huber(s3_chi2(e[0], e[1], p.is1), a.huber, r0, r1);
    acc[35] += r0;
    sim3_add_edge(acc, Ja, Jb, e[0], e[1], p.is1, r1);
    huber(s3_chi2(e[2], e[3], p.is2), a.huber, r0, r1);
    acc[35] += r0;
    sim3_add_edge(acc, Jc, Jd, e[2], e[3], p.is2, r1);
    acc[36] += 2.0;
  }
  wg_sum(acc, S.red, S.sums);
}

// thread 0, behind a linearising pass: the head of OptimizationAlgorithmLevenberg::solve (levenberg.cpp:74-101)
__device__ inline void sim3_begin_iteration(Sim3Shared& S) {
  S.currentChi = S.sums[35];
  S.iniChi = S.sums[35];
  int k = 0;
  for (int r = 0; r < 7; ++r)
    for (int c = r; c < 7; ++c) { S.H[r * 7 + c] = S.sums[k]; S.H[c * 7 + r] = S.sums[k]; ++k; }
  for (int r = 0; r < 7; ++r) S.b[r] = S.sums[28 + r];
  if (S.it == 0) {   // computeLambdaInit: tau = 1e-5
    double md = 0;
    for (int j = 0; j < 7; ++j) md = fmax(fabs(S.H[j * 8]), md);
    S.lambda = 1e-5 * md;
    S.ni = 2;
    S.nBadIt = 0;
  }
  S.qmax = 0;
}

// thread 0: solve (H + lambda I) x = b, estimate <- Sim3(x) * estimate (levenberg.cpp:103-115); the next pass evaluates it
__device__ inline void sim3_next_trial(const Sim3OptArgs& a, Sim3Shared& S) {
  S.bak = S.cur;
  double H[49], b[7], x[7];
#pragma unroll
  for (int q = 0; q < 49; ++q) H[q] = S.H[q];
#pragma unroll
  for (int q = 0; q < 7; ++q) b[q] = S.b[q];
  const bool ok = s3_solve7(H, S.lambda, b, x);
#pragma unroll
  for (int q = 0; q < 7; ++q) { x[q] = ok ? x[q] : 0.0; S.x[q] = x[q]; }
  S.ok = ok ? 1 : 0;
  if (ok) S.cur = s3_oplus(S.cur, x, a.fix_scale != 0);
  S.eval = S.cur;
  S.tr[2]++;
  S.cont = 1;
}

// thread 0, behind a trial's pass: accept or reject (levenberg.cpp:124-163).  Leaves S.cont = 1 another trial (already solved and
// applied), 2 the next iteration, 0 the round is over
__device__ inline void sim3_after_trial(const Sim3OptArgs& a, Sim3Shared& S, int cap) {
  double tempChi = S.sums[0];
  if (!S.ok) tempChi = 1.7976931348623157e308;
  double rho = S.currentChi - tempChi;
  double scale = 0;
  for (int j = 0; j < 7; ++j) scale += S.x[j] * (S.lambda * S.x[j] + S.b[j]);
  scale += 1e-3;
  rho /= scale;
  bool accepted = false;
  if (rho > 0 && isfinite(tempChi)) {
    const double q = 2 * rho - 1;
    double alpha = 1. - q * q * q;
    alpha = fmin(alpha, 2. / 3.);
    S.lambda *= fmax(1. / 3., alpha);
    S.ni = 2;
    S.currentChi = tempChi;
    accepted = true;
  } else {
    S.lambda *= S.ni;
    S.ni *= 2;
    S.cur = S.bak;
  }
  S.qmax++;
  if (rho < 0 && S.qmax < 10) { sim3_next_trial(a, S); return; }
  bool stop = S.qmax == 10 || rho == 0;
  if (!stop) {
    if ((S.iniChi - S.currentChi) * 1e3 < S.iniChi) S.nBadIt++; else S.nBadIt = 0;
    if (S.nBadIt >= 3) stop = true;
  }
  S.it++;
  S.tr[1] = S.it;
  const bool over = stop || S.it >= cap;
  if (over) S.tr[3] = accepted ? 0 : 1;
  S.cont = over ? 0 : 2;
}

__global__ __launch_bounds__(kSim3Threads) void k_sim3_opt(Sim3OptArgs a) {
  __shared__ Sim3Shared S;
  const int t = threadIdx.x;
  int32_t* const trc = reinterpret_cast<int32_t*>(a.io + 8);   // trace[12], n_in, early
  for (int i = t; i < a.n; i += kSim3Threads) a.keep[i] = 1;   // (each thread reads back only the flags it wrote itself)
  if (t == 0) {
    S.cur = Sim3d{a.sim3[0], a.sim3[1], a.sim3[2], a.sim3[3], a.sim3[4], a.sim3[5], a.sim3[6], a.sim3[7]};
    S.eval = S.cur;
    for (int q = 0; q < kSim3TraceInts; ++q) trc[q] = -1;
  }
  asd_syncthreads();
  int nBad = 0, nIn = 0, early = 0;
  for (int round = 0; round < 2; ++round) {
    const int cap = round == 0 ? 5 : (nBad > 0 ? 10 : 5);   // Optimizer.cc:1135, :1158-1162
    if (t == 0) { S.it = 0; S.tr[0] = 0; S.tr[1] = -1; S.tr[2] = 0; S.tr[3] = 0; }
    for (;;) {   // iterations of optimize(cap)
      sim3_pass_linearise(a, S);
      if (t == 0) {
        // (there is an active edge in every round: n == 0 returns on the host, round two runs on 10 pairs or more)
        if (S.it == 0) S.tr[0] = (int)(S.sums[36] + 0.5);
        S.eval = S.cur;
        sim3_begin_iteration(S);
        sim3_next_trial(a, S);
      }
      asd_syncthreads();
      while (S.cont == 1) {   // trials
        sim3_pass_errors(a, S);
        if (t == 0) sim3_after_trial(a, S, cap);
        asd_syncthreads();
      }
      if (S.cont == 0) break;
      asd_syncthreads();   // every wave has read S.cont before thread 0 of the next pass can write it again
    }
    // ---- re-classification (:1137-1156, :1172-1187): chi2() as the round's last pass left it, either edge over th2 drops the pair
    const Sim3d Se = S.eval, Si = s3_inverse(Se);
    double cnt[2] = {0.0, 0.0};
    for (int i = t; i < a.n; i += kSim3Threads) {
      if (!a.keep[i]) continue;
      const Sim3Pair p = sim3_load(a, i);
      double e[4];
      sim3_errors(a, p, Se, Si, e);
      if (s3_chi2(e[0], e[1], p.is1) > a.th2 || s3_chi2(e[2], e[3], p.is2) > a.th2) { a.keep[i] = 0; cnt[0] += 1.0; }
      else cnt[1] += 1.0;
    }
    wg_sum(cnt, S.red, S.sums);
    if (round == 0) nBad = (int)(S.sums[0] + 0.5); else nIn = (int)(S.sums[1] + 0.5);
    if (t == 0) { trc[4 * round] = S.tr[0]; trc[4 * round + 1] = S.tr[1]; trc[4 * round + 2] = S.tr[2]; trc[4 * round + 3] = S.tr[3]; }
    asd_syncthreads();   // S.sums and S.tr are read: the next round may write them
    if (round == 0 && a.n - nBad < 10) { early = 1; break; }   // :1164-1165
  }
  if (t == 0) {
    const Sim3d o = S.cur;
    a.io[0] = o.qx; a.io[1] = o.qy; a.io[2] = o.qz; a.io[3] = o.qw; a.io[4] = o.tx; a.io[5] = o.ty; a.io[6] = o.tz; a.io[7] = o.s;
    trc[8] = nBad; trc[9] = nBad > 0 ? 10 : 5; trc[10] = early; trc[11] = a.n;
    trc[12] = nIn; trc[13] = early;
  }
}

struct Sim3State {
  int32_t trace[kSim3TraceInts];
  Sim3State() { for (int32_t& v : trace) v = -1; }
};

Sim3State* sim3_state(asd_ctx* ctx) {
  if (!ctx->sim3) ctx->sim3 = new Sim3State();
  return static_cast<Sim3State*>(ctx->sim3);
}

}  // namespace

void sim3_free(asd_ctx* ctx) {
  delete static_cast<Sim3State*>(ctx->sim3);
  ctx->sim3 = nullptr;
}

extern "C" {

int asd_optimize_sim3(asd_ctx* ctx, double* sim3, int32_t n, const double* P1c, const double* P2c, const double* obs1,
                      const double* obs2, const double* inv_sigma2_1, const double* inv_sigma2_2, const double* K1,
                      const double* K2, float th2, int32_t fix_scale, uint8_t* keep, int32_t* n_in) {
  if (ctx && asd_track_busy(ctx, "asd_optimize_sim3")) return ASD_ERR_INVALID;
  if (!ctx || !sim3 || n < 0 || n > 65535 || !K1 || !K2 || !n_in || !(th2 > 0) ||
      (n > 0 && (!P1c || !P2c || !obs1 || !obs2 || !inv_sigma2_1 || !inv_sigma2_2 || !keep)))
    return ASD_ERR_INVALID;
  Sim3State* s = sim3_state(ctx);
  if (n == 0) {   // g2o's optimize() returns -1 on the empty graph; nCorrespondences - nBad < 10: return 0, g2oS12 untouched
    const int32_t tr[kSim3TraceInts] = {0, -1, 0, 0, -1, -1, -1, -1, 0, 5, 1, 0};
    memcpy(s->trace, tr, sizeof tr);
    *n_in = 0;
    return ASD_OK;
  }
  (void)hipSetDevice(ctx->cfg.device);
  hipStream_t st = ctx->stream;
  ASD_HIP_CHECK(ctx, ctx->up.begin(st, (size_t)n * 96 + 256));
  ASD_HIP_CHECK(ctx, ctx->down.begin(st, (size_t)n + 1024));
  const size_t off_soa = ctx->up.reserve((size_t)n * 96);
  double* h = ctx->up.host<double>(off_soa);
  const size_t N = (size_t)n;
  for (size_t i = 0; i < N; ++i) {
    for (int k = 0; k < 3; ++k) { h[k * N + i] = P1c[3 * i + k]; h[(3 + k) * N + i] = P2c[3 * i + k]; }
    for (int k = 0; k < 2; ++k) { h[(6 + k) * N + i] = obs1[2 * i + k]; h[(8 + k) * N + i] = obs2[2 * i + k]; }
    h[10 * N + i] = inv_sigma2_1[i];
    h[11 * N + i] = inv_sigma2_2[i];
  }
  const size_t off_io = ctx->down.reserve(64 + (kSim3TraceInts + 2) * 4), off_keep = ctx->down.reserve(N);
  Sim3OptArgs a{};
  a.n = n;
  a.soa = ctx->up.dev<double>(off_soa);
  a.keep = ctx->down.dev<uint8_t>(off_keep);
  a.io = ctx->down.dev<double>(off_io);
  memcpy(a.sim3, sim3, 64);
  memcpy(a.K1, K1, 32);
  memcpy(a.K2, K2, 32);
  a.th2 = (double)th2;
  a.huber = (double)sqrtf(th2);
  a.fix_scale = fix_scale ? 1 : 0;
  ASD_HIP_CHECK(ctx, ctx->up.upload(st));
  ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, st));
  hipLaunchKernelGGL(k_sim3_opt, dim3(1), dim3(kSim3Threads), 0, st, a);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, st));
  ASD_HIP_CHECK(ctx, ctx->down.download(st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  ASD_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->ms_sim3, ctx->ev0, ctx->ev1));
  const double* io = ctx->down.host<double>(off_io);
  const int32_t* trc = reinterpret_cast<const int32_t*>(io + 8);
  memcpy(s->trace, trc, sizeof s->trace);
  memcpy(keep, ctx->down.host<uint8_t>(off_keep), N);
  *n_in = trc[12];
  if (!trc[13]) memcpy(sim3, io, 64);   // the early return leaves g2oS12 as it was (:1165 is in front of :1191)
  return ASD_OK;
}

int32_t asd_debug_optimize_sim3(const asd_ctx* ctx, int32_t out[ASD_SIM3_OPT_DEBUG_INTS]) {
  if (!ctx || !out) return ASD_ERR_INVALID;
  const Sim3State* s = static_cast<const Sim3State*>(ctx->sim3);
  for (int k = 0; k < kSim3TraceInts; ++k) out[k] = s ? s->trace[k] : -1;
  return ASD_OK;
}

}  // extern "C"
