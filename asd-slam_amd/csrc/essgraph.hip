// essgraph.hip -- Optimizer::OptimizeEssentialGraph (reference src/vslam/src/Optimizer.cc:737-1000) on the device:
// asd_optimize_essential_graph.  A Sim3 pose graph: one 7-DoF vertex per keyframe, one EdgeSim3 per edge, 20 Levenberg iterations.
//
// The edge class has no analytic Jacobian, so g2o differentiates numerically (base_binary_edge.hpp:130-206; see sim3.hip for what
// that means for the noise floor) and this file does the same.  Per Levenberg iteration:
//   k_eg_linearize  32 lanes per edge, two edges per wave: lane 0 the error at the estimate, lanes 1-14 the error with vertex i moved
//                   by +-delta along each of its 7 directions, lanes 15-28 the same for vertex j (29 evaluations of
//                   log(C S_i S_j^-1)); then the two 7x7 Jacobians, A^T A, A^T B, B^T B and the two 7-vectors -A^T e, -B^T e
//   k_eg_begin      one workgroup: chi2 at the estimate, the head of OptimizationAlgorithmLevenberg::solve
// and per trial:
//   k_eg_assemble   one workgroup per block row of the free active vertices: clears its strip of the lower triangle of the dense
//                   n x n system, then sums each block's edges in edge order (incidence lists built once per call by the host),
//                   adds lambda to the diagonal and builds b the same way.  The matrix is rebuilt for every trial, as
//                   asd_bundle_adjustment rebuilds its reduced system: the factorisation overwrites it
//   gba_solve_enqueue (gba.hip)  the tiled f64 Cholesky, at every size
//   k_eg_update     push + oplus: Sim3(dx) * estimate per free vertex
//   k_eg_error      the error and chi2 alone
//   k_eg_control    one workgroup: chi2 of the trial, accept or reject (pop), next lambda, end of iteration / of the run
// The Levenberg state lives on the device; a launch behind the end of the run is a no-op, and the host looks at a pinned mirror of
// the state between chunks of trials.  Every sum has one fixed shape and there are no atomics: a call is one bit pattern.
// Built with -ffp-contract=off, as sim3.hip: the rounding of these functions is the optimiser's noise floor.
#include <algorithm>
#include <map>

#include "gba.h"
#include "sim3_math.h"

namespace {

constexpr int kEgChunk = 4;        // Levenberg trials enqueued between two looks at the mirrored state
constexpr int kEgBlk = 161;        // doubles per linearised edge: A^T A [49], A^T B [49], B^T B [49], -A^T e [7], -B^T e [7]
constexpr int kEgEdgesPerWg = 8;   // k_eg_linearize: 256 threads, 32 lanes per edge

struct EgLm {
  double lambda, ni, currentChi, iniChi, chi2_final;
  int first, need_lin, done, chol_ok, qmax, nBad, it, trials, cap, pad;
};

struct EgDev {
  int K, E, nF, n, fix_scale;
  Sim3d* cur;              // [K] the estimates
  Sim3d* bak;              // [K] push / pop
  const Sim3d* entry;      // [K] vScw as given
  const Sim3d* meas;       // [E]
  const int* e_i;          // [E]
  const int* e_j;          // [E]
  const int* hidx;         // [K] block row of a free active vertex, else -1
  const int* vof;          // [nF] its keyframe row
  const int* vinc_start;   // [nF + 1] per block row: its edges in edge order, entry = 2 edge + side
  const int* vinc;
  const int* prow_start;   // [nF + 1] per block row: its distinct pairs (lower triangle)
  const int* pair_col;     // per pair: block column
  const int* pent_start;   // per pair: its edges in edge order, entry = 2 edge + transposed
  const int* pent;
  double* blk;             // [E][kEgBlk]
  double* err;             // [E][7]
  double* chi2e;           // [E]
  double* A;               // [n][n]
  double* b;               // [n]
  double* x;               // [n]
  EgLm* lm;
  EgLm* lm_host;           // pinned mirror
  int* it_trials;          // [cap]
};

// sum of f(k), k < n, over one workgroup of 256 threads: every thread its strided part in order, the lanes of a wave by butterfly, then
// the waves in order.  Two barriers; every thread gets the sum.
template <class F>
__device__ inline double eg_block_sum(int n, F f) {
  __shared__ double red[4];
  double v = 0.0;
  for (int k = threadIdx.x; k < n; k += 256) v += f(k);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  asd_syncthreads();
  const double s = ((red[0] + red[1]) + red[2]) + red[3];
  asd_syncthreads();   // (every thread has read: the next sum may write)
  return s;
}

// BaseEdge::chi2() with the identity as information: e . e
__device__ inline double eg_chi2(const double (&e)[7]) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 7; ++k) s += e[k] * e[k];
  return s;
}

__global__ __launch_bounds__(256) void k_eg_linearize(EgDev d) {
  __shared__ double errs[kEgEdgesPerWg][29][7];
  __shared__ double Js[kEgEdgesPerWg][2][49];
  if (d.lm->done || !d.lm->need_lin) return;
  const int slot = threadIdx.x >> 5, lane = threadIdx.x & 31;
  const int e = blockIdx.x * kEgEdgesPerWg + slot;
  const bool valid = e < d.E;
  bool free_i = false, free_j = false;
  if (valid) {
    const int i = d.e_i[e], j = d.e_j[e];
    free_i = d.hidx[i] >= 0; free_j = d.hidx[j] >= 0;
    if (lane < 29) {
      Sim3d Si = d.cur[i], Sj = d.cur[j];
      const Sim3d C = d.meas[e];
      if (lane >= 1) {
        const int side = lane >= 15 ? 1 : 0, q = (lane - 1) - 14 * side, dir = q >> 1;
        const double delta = (q & 1) ? -1e-9 : 1e-9;
        double u[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) u[k] = k == dir ? delta : 0.0;
        if (side == 0) Si = s3_oplus<true>(Si, u, d.fix_scale != 0);
        else Sj = s3_oplus<true>(Sj, u, d.fix_scale != 0);
      }
      double ev[7];
      s3_edge_error(C, Si, Sj, ev);
#pragma unroll
      for (int k = 0; k < 7; ++k) errs[slot][lane][k] = ev[k];
      if (lane == 0) {   // computeActiveErrors at the head of the iteration
#pragma unroll
        for (int k = 0; k < 7; ++k) d.err[(size_t)e * 7 + k] = ev[k];
        d.chi2e[e] = eg_chi2(ev);
      }
    }
  }
  asd_syncthreads();
  // column dir of a Jacobian = scalar * (e(+delta) - e(-delta)) (base_binary_edge.hpp:147-198); none for a fixed vertex
  const double scalar = 1.0 / (2 * 1e-9);
  if (valid)
    for (int idx = lane; idx < 98; idx += 32) {
      const int side = idx / 49, r = (idx % 49) / 7, dir = idx % 7;
      const int kp = 1 + 14 * side + 2 * dir;
      const bool fr = side ? free_j : free_i;
      Js[slot][side][r * 7 + dir] = fr ? scalar * (errs[slot][kp][r] - errs[slot][kp + 1][r]) : 0.0;
    }
  asd_syncthreads();
  if (valid)
    for (int idx = lane; idx < kEgBlk; idx += 32) {
      double s = 0.0;
      if (idx < 147) {
        const int which = idx / 49, a = (idx % 49) / 7, c = idx % 7;
        const double* L = Js[slot][which == 2 ? 1 : 0];
        const double* R = Js[slot][which == 0 ? 0 : 1];
#pragma unroll
        for (int r = 0; r < 7; ++r) s += L[r * 7 + a] * R[r * 7 + c];
      } else {
        const int side = (idx - 147) / 7, a = (idx - 147) % 7;
        const double* L = Js[slot][side];
#pragma unroll
        for (int r = 0; r < 7; ++r) s += L[r * 7 + a] * -errs[slot][0][r];
      }
      d.blk[(size_t)e * kEgBlk + idx] = s;
    }
}

// the head of OptimizationAlgorithmLevenberg::solve (levenberg.cpp:82-101) behind a linearisation
__global__ __launch_bounds__(256) void k_eg_begin(EgDev d) {
  if (d.lm->done || !d.lm->need_lin) return;
  const double sum = eg_block_sum(d.E, [&](int k) { return d.chi2e[k]; });
  if (threadIdx.x == 0) {
    EgLm& S = *d.lm;
    S.currentChi = sum; S.iniChi = sum;
    if (S.first) { S.lambda = 1e-16; S.ni = 2; S.nBad = 0; S.first = 0; }   // computeLambdaInit with setUserLambdaInit(1e-16)
    S.qmax = 0;
    S.need_lin = 0;
  }
}

__global__ __launch_bounds__(256) void k_eg_assemble(EgDev d) {
  if (d.lm->done) return;
  const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t n = (size_t)d.n;
  const double lambda = d.lm->lambda;
  const int width = 7 * r + 7;
  for (int idx = t; idx < 7 * width; idx += 256) d.A[(size_t)(7 * r + idx / width) * n + idx % width] = 0.0;
  asd_syncthreads();
  const int p0 = d.prow_start[r], np = d.prow_start[r + 1] - p0;
  for (int task = wave; task <= np; task += 4) {
    if (task == 0) {   // the diagonal block + lambda I, and b
      const int k0 = d.vinc_start[r], k1 = d.vinc_start[r + 1];
      if (lane < 49) {
        double s = 0.0;
        for (int k = k0; k < k1; ++k) { const int v = d.vinc[k]; s += d.blk[(size_t)(v >> 1) * kEgBlk + ((v & 1) ? 98 : 0) + lane]; }
        const int a = lane / 7, c = lane % 7;
        d.A[(size_t)(7 * r + a) * n + 7 * r + c] = a == c ? s + lambda : s;
      } else if (lane < 56) {
        double s = 0.0;
        for (int k = k0; k < k1; ++k) { const int v = d.vinc[k]; s += d.blk[(size_t)(v >> 1) * kEgBlk + ((v & 1) ? 154 : 147) + (lane - 49)]; }
        d.b[7 * r + (lane - 49)] = s;
      }
    } else if (lane < 49) {
      const int p = p0 + task - 1, col = d.pair_col[p];
      const int a = lane / 7, c = lane % 7;
      double s = 0.0;
      for (int k = d.pent_start[p]; k < d.pent_start[p + 1]; ++k) {
        const int v = d.pent[k];
        s += d.blk[(size_t)(v >> 1) * kEgBlk + 49 + ((v & 1) ? c * 7 + a : a * 7 + c)];
      }
      d.A[(size_t)(7 * r + a) * n + 7 * col + c] = s;
    }
  }
}

// push, then update: estimate <- Sim3(dx) * estimate (levenberg.cpp:103, :115).  A failed factorisation applies nothing: the trial is
// rejected and the estimate popped either way
__global__ __launch_bounds__(64) void k_eg_update(EgDev d) {
  if (d.lm->done) return;
  const int h = blockIdx.x * 64 + threadIdx.x;
  if (h >= d.nF) return;
  const int v = d.vof[h];
  const Sim3d S = d.cur[v];
  d.bak[v] = S;
  if (!d.lm->chol_ok) return;
  double u[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) u[k] = d.x[7 * h + k];
  d.cur[v] = s3_oplus<true>(S, u, d.fix_scale != 0);
}

// computeActiveErrors: the error and chi2 of every edge at the estimate.  force: the pass in front of the run and behind a
// linearisation-free call
__global__ __launch_bounds__(64) void k_eg_error(EgDev d, int force) {
  if (!force && d.lm->done) return;
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= d.E) return;
  double ev[7];
  s3_edge_error(d.meas[e], d.cur[d.e_i[e]], d.cur[d.e_j[e]], ev);
#pragma unroll
  for (int k = 0; k < 7; ++k) d.err[(size_t)e * 7 + k] = ev[k];
  d.chi2e[e] = eg_chi2(ev);
}

// behind a trial: accept or reject, next lambda, end of iteration / of the run (levenberg.cpp:124-163, sparse_optimizer.cpp:376-414)
__global__ __launch_bounds__(256) void k_eg_control(EgDev d) {
  __shared__ int s_pop;
  if (d.lm->done) return;
  const int ok = d.lm->chol_ok;
  const double lambda = d.lm->lambda;
  double tempChi = eg_block_sum(d.E, [&](int k) { return d.chi2e[k]; });
  // computeScale; the x of a failed solve is not looked at (tempChi = max makes rho negative whatever the scale)
  double scale = eg_block_sum(ok ? d.n : 0, [&](int k) { const double xk = d.x[k]; return xk * (lambda * xk + d.b[k]); });
  if (threadIdx.x == 0) {
    EgLm& S = *d.lm;
    if (!ok) tempChi = 1.7976931348623157e308;
    double rho = S.currentChi - tempChi;
    scale += 1e-3;
    rho /= scale;
    int pop = 0;
    if (rho > 0 && isfinite(tempChi)) {
      const double q = 2 * rho - 1;
      double alpha = 1. - q * q * q;
      alpha = fmin(alpha, 2. / 3.);
      S.lambda *= fmax(1. / 3., alpha);
      S.ni = 2;
      S.currentChi = tempChi;
    } else {
      S.lambda *= S.ni;
      S.ni *= 2;
      pop = 1;
    }
    S.qmax++;
    S.trials++;
    if (!(rho < 0 && S.qmax < 10)) {
      bool stop = S.qmax == 10 || rho == 0;
      if (!stop) {
        if ((S.iniChi - S.currentChi) * 1e3 < S.iniChi) S.nBad++; else S.nBad = 0;
        if (S.nBad >= 3) stop = true;
      }
      d.it_trials[S.it] = S.qmax;
      S.it++;
      if (stop || S.it >= S.cap) S.done = 1; else S.need_lin = 1;
    }
    s_pop = pop;
  }
  asd_syncthreads();
  if (s_pop)
    for (int h = threadIdx.x; h < d.nF; h += 256) { const int v = d.vof[h]; d.cur[v] = d.bak[v]; }
  if (threadIdx.x == 0) *d.lm_host = *d.lm;
}

// activeChi2() of the stored errors, and the state once more for the host
__global__ __launch_bounds__(256) void k_eg_final(EgDev d) {
  const double sum = eg_block_sum(d.E, [&](int k) { return d.chi2e[k]; });
  if (threadIdx.x == 0) { d.lm->chi2_final = sum; *d.lm_host = *d.lm; }
}

// Sim3:[sR t;0 1] -> SE3:[R t/s;0 1] as float (Optimizer.cc:955-963)
__global__ __launch_bounds__(64) void k_eg_tcw(int K, const Sim3d* __restrict__ cur, float* __restrict__ T) {
  const int v = blockIdx.x * 64 + threadIdx.x;
  if (v >= K) return;
  const Sim3d S = cur[v];
  double R[9];
  s3_rot_of_quat(S, R);
  const double k = 1. / S.s;
  const double tt[3] = {S.tx * k, S.ty * k, S.tz * k};
  float* o = T + (size_t)v * 16;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) o[i * 4 + j] = (float)R[i * 3 + j];
    o[i * 4 + 3] = (float)tt[i];
  }
  o[12] = o[13] = o[14] = 0.f;
  o[15] = 1.f;
}

// correctedSwr.map(Srw.map(X)) (Optimizer.cc:988-996), a thread per point
__global__ __launch_bounds__(256) void k_eg_points(int n_mp, const int* __restrict__ ref, const Sim3d* __restrict__ entry,
                                                   const Sim3d* __restrict__ cur, float* __restrict__ X) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_mp) return;
  const int r = ref[p];
  const double x[3] = {(double)X[3 * (size_t)p], (double)X[3 * (size_t)p + 1], (double)X[3 * (size_t)p + 2]};
  double c[3], w[3];
  s3_map(entry[r], x, c);
  s3_map(s3_inverse(cur[r]), c, w);
  X[3 * (size_t)p] = (float)w[0]; X[3 * (size_t)p + 1] = (float)w[1]; X[3 * (size_t)p + 2] = (float)w[2];
}

struct EgState {
  AsdDevBuf dev;   // the call's device arrays, carved out of one grow-only block
  EgLm* h_lm = nullptr;
  int forms[4] = {-1, -1, -1, -1};
  std::vector<int> trials;
};

EgState* eg_state(asd_ctx* ctx) {
  if (!ctx->essgraph) ctx->essgraph = new EgState();
  return static_cast<EgState*>(ctx->essgraph);
}

int eg_check(asd_ctx* ctx, const asd_essgraph_problem* pr, const asd_essgraph_result* res) {
  if (!ctx || !pr || !res || pr->n_kf < 0 || pr->n_edges < 0 || pr->n_mp < 0 || (pr->n_kf > 0 && (!pr->sim3 || !pr->fixed)) ||
      (pr->n_edges > 0 && (!pr->e_i || !pr->e_j || !pr->e_meas || !res->edge_chi2)) || (pr->n_mp > 0 && (!pr->mp_ref || !pr->mp_Xw)))
    return ASD_ERR_INVALID;
  if (pr->n_kf > ASD_ESSGRAPH_MAX_KEYFRAMES) { ctx->set_error("asd_optimize_essential_graph: %d keyframes exceed ASD_ESSGRAPH_MAX_KEYFRAMES = %d", pr->n_kf, ASD_ESSGRAPH_MAX_KEYFRAMES); return ASD_ERR_CAPACITY; }
  if (pr->n_edges > ASD_ESSGRAPH_MAX_EDGES) { ctx->set_error("asd_optimize_essential_graph: %d edges exceed ASD_ESSGRAPH_MAX_EDGES = %d", pr->n_edges, ASD_ESSGRAPH_MAX_EDGES); return ASD_ERR_CAPACITY; }
  if (pr->n_mp > ASD_ESSGRAPH_MAX_POINTS) { ctx->set_error("asd_optimize_essential_graph: %d map points exceed ASD_ESSGRAPH_MAX_POINTS = %d", pr->n_mp, ASD_ESSGRAPH_MAX_POINTS); return ASD_ERR_CAPACITY; }
  if (pr->n_iterations > ASD_ESSGRAPH_MAX_ITERATIONS) { ctx->set_error("asd_optimize_essential_graph: %d iterations exceed ASD_ESSGRAPH_MAX_ITERATIONS = %d", pr->n_iterations, ASD_ESSGRAPH_MAX_ITERATIONS); return ASD_ERR_CAPACITY; }
  for (int e = 0; e < pr->n_edges; ++e) {
    const int i = pr->e_i[e], j = pr->e_j[e];
    if (i < 0 || i >= pr->n_kf || j < 0 || j >= pr->n_kf) { ctx->set_error("asd_optimize_essential_graph: edge %d names a keyframe row outside [0, %d)", e, pr->n_kf); return ASD_ERR_INVALID; }
    if (i == j) { ctx->set_error("asd_optimize_essential_graph: edge %d connects keyframe row %d with itself", e, i); return ASD_ERR_INVALID; }
  }
  for (int p = 0; p < pr->n_mp; ++p)
    if (pr->mp_ref[p] < 0 || pr->mp_ref[p] >= pr->n_kf) { ctx->set_error("asd_optimize_essential_graph: map point %d names a keyframe row outside [0, %d)", p, pr->n_kf); return ASD_ERR_INVALID; }
  return ASD_OK;
}

int eg_impl(asd_ctx* ctx, EgState* s, asd_essgraph_problem* pr, asd_essgraph_result* res) {
  const int K = pr->n_kf, E = pr->n_edges, M = pr->n_mp;
  hipStream_t st = ctx->stream;
  (void)hipSetDevice(ctx->cfg.device);
  int rc;
  for (int& v : s->forms) v = -1;
  s->trials.clear();
  res->chi2 = 0; res->iterations = -1; res->trials = 0;

  // ---- active structure (sparse_optimizer.cpp:206-267): a vertex is active when an edge names it, free when it is not fixed
  std::vector<int> hidx(K, -1), vof;
  int n_active = 0;
  {
    std::vector<uint8_t> act(K, 0);
    for (int e = 0; e < E; ++e) { act[pr->e_i[e]] = 1; act[pr->e_j[e]] = 1; }
    for (int v = 0; v < K; ++v) {
      n_active += act[v];
      if (act[v] && !pr->fixed[v]) { hidx[v] = (int)vof.size(); vof.push_back(v); }
    }
  }
  const int nF = (int)vof.size(), n = 7 * nF;
  if (E > 0 && nF == 0) {
    ctx->set_error("asd_optimize_essential_graph: %d edges but no free keyframe among their vertices", E);
    return ASD_ERR_INVALID;
  }
  const int iterations = E > 0 ? std::max(pr->n_iterations, 0) : 0;
  // incidence lists, once per call: per block row its edges in edge order, per distinct pair of block rows its edges in edge order
  std::vector<int> vinc_start(nF + 1, 0), vinc, prow_start(nF + 1, 0), pair_col, pent_start(1, 0), pent;
  {
    std::vector<std::vector<int>> inc(nF);
    std::vector<std::map<int, std::vector<int>>> prs(nF);   // row -> column -> entries
    for (int e = 0; e < E; ++e) {
      const int hi = hidx[pr->e_i[e]], hj = hidx[pr->e_j[e]];
      if (hi >= 0) inc[hi].push_back(2 * e);
      if (hj >= 0) inc[hj].push_back(2 * e + 1);
      if (hi >= 0 && hj >= 0) {   // the block (row, column) of the lower triangle is A^T B when the row is vertex i, its transpose otherwise
        if (hi > hj) prs[hi][hj].push_back(2 * e);
        else prs[hj][hi].push_back(2 * e + 1);
      }
    }
    for (int h = 0; h < nF; ++h) {
      vinc.insert(vinc.end(), inc[h].begin(), inc[h].end());
      vinc_start[h + 1] = (int)vinc.size();
      for (const auto& kv : prs[h]) {
        pair_col.push_back(kv.first);
        pent.insert(pent.end(), kv.second.begin(), kv.second.end());
        pent_start.push_back((int)pent.size());
      }
      prow_start[h + 1] = (int)pair_col.size();
    }
  }

  // ---- buffers
  const size_t szK = AsdDevBuf::padded((size_t)std::max(K, 1) * sizeof(Sim3d)), szE = AsdDevBuf::padded((size_t)std::max(E, 1) * sizeof(Sim3d));
  std::vector<int> ints;
  auto put = [&](const int* v, size_t cnt) { const size_t o = ints.size(); ints.insert(ints.end(), v, v + cnt); ints.resize((ints.size() + 63) / 64 * 64, 0); return o; };
  const size_t o_ei = put(pr->e_i, E), o_ej = put(pr->e_j, E), o_hidx = put(hidx.data(), K), o_vof = put(vof.data(), nF),
               o_vs = put(vinc_start.data(), vinc_start.size()), o_vi = put(vinc.data(), vinc.size()), o_ps = put(prow_start.data(), prow_start.size()),
               o_pc = put(pair_col.data(), pair_col.size()), o_pes = put(pent_start.data(), pent_start.size()), o_pe = put(pent.data(), pent.size()),
               o_ref = put(pr->mp_ref, M);
  const size_t o_trials = ints.size();
  ints.resize(ints.size() + (size_t)std::max(iterations, 1), 0);
  const size_t sz_est = 3 * szK + szE, sz_ints = ints.size() * 4, sz_blk = (size_t)std::max(E, 1) * kEgBlk * 8, sz_err = (size_t)std::max(E, 1) * 8 * 8,
               sz_A = std::max((size_t)n * n, (size_t)1) * 8, sz_vec = (size_t)std::max(n, 1) * 2 * 8,
               sz_tail = (size_t)std::max(K, 1) * 64 + (size_t)std::max(M, 1) * 12;
  ASD_HIP_CHECK(ctx, s->dev.reserve(AsdDevBuf::padded(sz_est) + AsdDevBuf::padded(sz_ints) + AsdDevBuf::padded(sz_blk) + AsdDevBuf::padded(sz_err) +
                                    AsdDevBuf::padded(sz_A) + AsdDevBuf::padded(sz_vec) + AsdDevBuf::padded(sizeof(EgLm)) + AsdDevBuf::padded(sz_tail)));
  if (!s->h_lm) ASD_HIP_CHECK(ctx, hipHostMalloc(reinterpret_cast<void**>(&s->h_lm), sizeof(EgLm)));

  char* eb = s->dev.carve<char>(sz_est);
  int* ib = s->dev.carve<int>(ints.size());
  EgDev d{};
  d.K = K; d.E = E; d.nF = nF; d.n = n; d.fix_scale = pr->fix_scale ? 1 : 0;
  d.cur = reinterpret_cast<Sim3d*>(eb); d.bak = reinterpret_cast<Sim3d*>(eb + szK); d.entry = reinterpret_cast<Sim3d*>(eb + 2 * szK);
  d.meas = reinterpret_cast<Sim3d*>(eb + 3 * szK);
  d.e_i = ib + o_ei; d.e_j = ib + o_ej; d.hidx = ib + o_hidx; d.vof = ib + o_vof; d.vinc_start = ib + o_vs; d.vinc = ib + o_vi;
  d.prow_start = ib + o_ps; d.pair_col = ib + o_pc; d.pent_start = ib + o_pes; d.pent = ib + o_pe;
  d.it_trials = ib + o_trials;
  d.blk = s->dev.carve<double>(sz_blk / 8);
  d.err = s->dev.carve<double>(sz_err / 8); d.chi2e = d.err + (size_t)std::max(E, 1) * 7;
  d.A = s->dev.carve<double>(sz_A / 8);
  d.b = s->dev.carve<double>(sz_vec / 8); d.x = d.b + std::max(n, 1);
  d.lm = s->dev.carve<EgLm>(1); d.lm_host = s->h_lm;
  float* d_T = s->dev.carve<float>(sz_tail / 4);
  float* d_X = d_T + (size_t)std::max(K, 1) * 16;

  // ---- upload.  The estimate, its push buffer and the entry copy all start as the input
  static_assert(sizeof(Sim3d) == 64, "a Sim3 is the 8 doubles of the C ABI");
  for (int c = 0; c < 3; ++c)
    if (K > 0) ASD_HIP_CHECK(ctx, hipMemcpyAsync(eb + c * szK, pr->sim3, (size_t)K * 64, hipMemcpyHostToDevice, st));
  if (E > 0) ASD_HIP_CHECK(ctx, hipMemcpyAsync(eb + 3 * szK, pr->e_meas, (size_t)E * 64, hipMemcpyHostToDevice, st));
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(ib, ints.data(), ints.size() * 4, hipMemcpyHostToDevice, st));
  if (M > 0) ASD_HIP_CHECK(ctx, hipMemcpyAsync(d_X, pr->mp_Xw, (size_t)M * 12, hipMemcpyHostToDevice, st));
  EgLm lm0{};
  lm0.first = 1; lm0.need_lin = 1; lm0.done = iterations <= 0 ? 1 : 0; lm0.chol_ok = 1; lm0.cap = iterations;
  *s->h_lm = lm0;
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(d.lm, &lm0, sizeof lm0, hipMemcpyHostToDevice, st));
  ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, st));
  s->forms[0] = n_active; s->forms[1] = nF; s->forms[2] = E; s->forms[3] = iterations > 0 ? (n + kGbaTile - 1) / kGbaTile : 0;

  int iters = E > 0 ? 0 : -1, trials = 0;
  if (E > 0) {
    const int gE = (E + 63) / 64;
    // every edge's error at the entry estimate: optimize() computes it at the head of its first iteration; a run without one reports these
    hipLaunchKernelGGL(k_eg_error, dim3(gE), dim3(64), 0, st, d, 1);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    auto enqueue_trial = [&]() -> int {
      hipLaunchKernelGGL(k_eg_linearize, dim3((E + kEgEdgesPerWg - 1) / kEgEdgesPerWg), dim3(256), 0, st, d);
      hipLaunchKernelGGL(k_eg_begin, dim3(1), dim3(256), 0, st, d);
      hipLaunchKernelGGL(k_eg_assemble, dim3(nF), dim3(256), 0, st, d);
      const int r2 = gba_solve_enqueue(ctx, st, d.A, d.b, d.x, n, &d.lm->done, &d.lm->chol_ok, true);
      if (r2 != ASD_OK) return r2;
      hipLaunchKernelGGL(k_eg_update, dim3((nF + 63) / 64), dim3(64), 0, st, d);
      hipLaunchKernelGGL(k_eg_error, dim3(gE), dim3(64), 0, st, d, 0);
      hipLaunchKernelGGL(k_eg_control, dim3(1), dim3(256), 0, st, d);
      ASD_HIP_CHECK(ctx, hipGetLastError());
      return ASD_OK;
    };
    const int max_trials = iterations * 10 + kEgChunk;
    int enqueued = 0;
    bool finished = iterations <= 0;
    while (!finished && enqueued < max_trials) {
      for (int c = 0; c < kEgChunk; ++c) if ((rc = enqueue_trial()) != ASD_OK) return rc;
      enqueued += kEgChunk;
      ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
      finished = s->h_lm->done != 0;
    }
    if (!finished) { ctx->set_error("asd_optimize_essential_graph: the Levenberg state did not finish"); return ASD_ERR_NUMERIC; }
    hipLaunchKernelGGL(k_eg_final, dim3(1), dim3(256), 0, st, d);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  if (pr->Tcw_out && K > 0) hipLaunchKernelGGL(k_eg_tcw, dim3((K + 63) / 64), dim3(64), 0, st, K, d.cur, d_T);
  if (M > 0) hipLaunchKernelGGL(k_eg_points, dim3((M + 255) / 256), dim3(256), 0, st, M, ib + o_ref, d.entry, d.cur, d_X);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, st));
  if (K > 0) ASD_HIP_CHECK(ctx, hipMemcpyAsync(pr->sim3, d.cur, (size_t)K * 64, hipMemcpyDeviceToHost, st));
  if (E > 0) ASD_HIP_CHECK(ctx, hipMemcpyAsync(res->edge_chi2, d.chi2e, (size_t)E * 8, hipMemcpyDeviceToHost, st));
  if (pr->Tcw_out && K > 0) ASD_HIP_CHECK(ctx, hipMemcpyAsync(pr->Tcw_out, d_T, (size_t)K * 64, hipMemcpyDeviceToHost, st));
  if (M > 0) ASD_HIP_CHECK(ctx, hipMemcpyAsync(pr->mp_Xw, d_X, (size_t)M * 12, hipMemcpyDeviceToHost, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  ASD_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->ms_essgraph, ctx->ev0, ctx->ev1));
  if (E > 0) {
    iters = s->h_lm->it; trials = s->h_lm->trials;
    res->chi2 = s->h_lm->chi2_final;
    s->trials.assign(iters, 0);
    if (iters > 0) ASD_HIP_CHECK(ctx, hipMemcpy(s->trials.data(), d.it_trials, (size_t)iters * 4, hipMemcpyDeviceToHost));
  }
  res->iterations = iters; res->trials = trials;
  return ASD_OK;
}

}  // namespace

void essgraph_free(asd_ctx* ctx) {
  if (!ctx->essgraph) return;
  EgState* s = static_cast<EgState*>(ctx->essgraph);
  s->dev.release();
  if (s->h_lm) (void)hipHostFree(s->h_lm);
  delete s;
  ctx->essgraph = nullptr;
}

extern "C" {

int asd_optimize_essential_graph(asd_ctx* ctx, asd_essgraph_problem* pr, asd_essgraph_result* res) {
  int rc = eg_check(ctx, pr, res);
  if (rc != ASD_OK) return rc;
  if (asd_track_busy(ctx, "asd_optimize_essential_graph")) return ASD_ERR_INVALID;
  if (ba_lane_busy(ctx, "asd_optimize_essential_graph")) return ASD_ERR_INVALID;
  return eg_impl(ctx, eg_state(ctx), pr, res);
}

int32_t asd_debug_essgraph_forms(const asd_ctx* ctx, int32_t out[4]) {
  if (!ctx || !out) return ASD_ERR_INVALID;
  const EgState* s = static_cast<const EgState*>(ctx->essgraph);
  for (int k = 0; k < 4; ++k) out[k] = s ? s->forms[k] : -1;
  return ASD_OK;
}

int32_t asd_debug_essgraph_trials(const asd_ctx* ctx, int32_t* out, int32_t cap) {
  if (!ctx || (cap > 0 && !out) || cap < 0) return ASD_ERR_INVALID;
  const EgState* s = static_cast<const EgState*>(ctx->essgraph);
  const int n = s ? (int)s->trials.size() : 0;
  for (int k = 0; k < cap; ++k) out[k] = k < n ? s->trials[k] : -1;
  return n;
}

}  // extern "C"
