// pnp_ransac.hip -- PnPsolver (reference src/vslam/src/PnPsolver.cc) on the device: asd_pnp_ransac.
//
// PnPsolver::iterate (:165-258) is a loop of independent hypotheses -- sample four correspondences (:188-201), EPnP on them (compute_pose,
// :477-525), score all N correspondences (CheckInliers, :308-339) -- followed by a sequential rule over the scores that calls Refine (:260-305,
// EPnP on the inlier set of the best model) whenever the best model changes.  The two halves are the two kernels:
//  * k_pnp_hyp, one workgroup per hypothesis of every problem of the call.  Thread 0 replays the sampling (ransac_sample) and evaluates EPnP in
//    f64 (the small solves work in LDS: no dynamically indexed private array; the 12x12 Jacobi is spread over the lanes of thread 0's wave,
//    bit for bit what one lane would compute), the workgroup scores the correspondences in
//    the reference's mixed f32/f64 operation order (this file is compiled with -ffp-contract=off).
//  * k_pnp_select, one workgroup per problem.  It walks the counts in hypothesis order with the reference's rule; a Refine is the same
//    compute_pose with the whole workgroup over the points of the best mask -- six workgroup-wide sums of fixed shape through LDS (centroid,
//    PW0^T PW0, the 78 entries of M^T M, pc0 / pw0, ABt, the reprojection sums of the three candidates), the small algebra between them on
//    thread 0 -- and the same CheckInliers.  alphas and pcs are recomputed per point where they are needed: no per-point scratch.
// One templated compute_pose serves both: <false> is the first wave over the four sampled points, <true> the workgroup over a mask.
// The sampling, the one-sided Jacobi SVD, the scoring loop with its ballot words and count, the workgroup sums and the host half of the
// call are ransac.h's.
// No atomics: a call is one bit pattern.  Everything the host reads travels in the context's one result block.
#include "ctx.h"
#include "ransac.h"

#include <cfloat>

namespace {

constexpr int kPnpThreads = kRansacThreads, kPnpWaves = kRansacWaves;
constexpr int kPnpSymSweeps = 30;   // cyclic Jacobi, 12x12: the off-diagonal part is exactly zero after 8-12 sweeps; the cap bounds a NaN input
constexpr int kPnpSvdSweeps = 40;   // one-sided Jacobi on at most 6x5
constexpr int kPnpMaxSums = 78;     // the upper triangle of M^T M

// what one compute_pose leaves (result block; asd_debug_pnp_ransac reads the host copy)
struct PnpRec {
  double R[9], t[3], cws[12], v[48], eig[4], rep[3], betas[4];
  int32_t idx[4], count, N, hypothesis, pad;
};
static_assert(sizeof(PnpRec) == 83 * 8 + 32, "PnpRec is laid out without holes");

// one problem as the kernels see it (upload block); every pointer is device memory
struct PnpRansacProb {
  int32_t n, n_iter, hyp_first, min_inliers, best_in, words, pad0, pad1;
  float K[4];
  const float *P3D, *P2D, *maxe;   // [n][3], [n][2], [n]
  const int32_t* draws;            // [n_iter][4]
  unsigned long long* masks;       // [n_iter][words]
  unsigned long long* refmask;     // [words]: mvbRefinedInliers of the last Refine
  uint8_t *best_mask, *inliers;    // [n] out each
  int32_t* result;                 // [8] out: best_inliers, best_updated, best hypothesis, found, iterations_done, n_inliers, Refines, -
};

struct PnpShared {
  double red[kPnpWaves][kPnpMaxSums], sums[kPnpMaxSums];
  double cws[4][3], ci[9];
  double A[144], V[144];           // the symmetric Jacobi's matrix and rotations (12x12, or 3x3 in their first entries)
  double v[4][12], lam[4];         // ut rows 11, 10, 9, 8 and their eigenvalues
  double L[60], rho[6], betas[3][4], ccs[3][4][3];
  double pc0[3][3], pw0[3], Rs[3][9], ts[3][3], rep[3];
  double R[9], t[3];
  double w[128];                   // workspace of the small solves
  int N, first, m;
};

// the correspondences of one compute_pose
struct PnpPts {
  const float *P3D, *P2D;
  int n, m;                          // all correspondences; those of this compute_pose
  int idx[4];                        // <false>: the sampled four, in draw order
  const unsigned long long* mask;    // <true>: bit i = correspondence i takes part, in ascending order
  double fu, fv, uc, vc;
};

template <bool BLOCK, typename F>
__device__ inline void pnp_for_each(const PnpPts& pts, F f) {
  if (!BLOCK) {
    if ((threadIdx.x & 63) != 0) return;   // lane 0 has the four points; the rest of its wave is there for the Jacobi
    for (int j = 0; j < 4; ++j) f(pts.idx[j]);
  } else {
    for (int i = threadIdx.x; i < pts.n; i += kPnpThreads)
      if (ransac_mask_bit(pts.mask, i)) f(i);
  }
}

// S.sums[0 .. N) = the sum of acc over the correspondences: <false> thread 0 has them all; <true> the workgroup sum of fixed shape
template <bool BLOCK, int N>
__device__ inline void pnp_sum(double (&acc)[N], PnpShared& S) {
  if (!BLOCK) {
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < N; ++k) S.sums[k] = acc[k];
    }
    return;
  }
  wg_sum(acc, S.red, S.sums);
}

template <bool BLOCK>
__device__ inline void pnp_sync() {
  if (BLOCK) asd_syncthreads();
}

// LDS written by one lane of a wave is read by the others: nothing may move across this point (a wave's LDS operations complete in order)
__device__ inline void pnp_wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// eigen-decomposition of the symmetric n x n matrix a (full storage, row stride n, n <= 12) by cyclic Jacobi: rotations (p, q) in row order,
// each annihilating a[p][q] with the smaller of the two angles; ends when every off-diagonal element is zero or at the sweep cap.  The
// eigenvalues are left on a's diagonal, the eigenvectors in the columns of v.  Called by EVERY lane of one wave: each lane evaluates the
// rotation (the same values from the same LDS words, so every branch is uniform), lane k < n updates row / column k of a and row k of v.
// Every element goes through the arithmetic a single lane would apply to it: the result does not depend on the spreading.
__device__ inline void pnp_jacobi_sym(double* a, double* v, const int n, const int lane) {
  if (lane < n)
    for (int j = 0; j < n; ++j) v[lane * n + j] = lane == j ? 1.0 : 0.0;
  pnp_wave_fence();
  for (int sweep = 0; sweep < kPnpSymSweeps; ++sweep) {
    bool zero = true;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = a[p * n + q];
        if (apq != apq) return;   // a NaN never leaves: nothing behind it is an inlier
        zero = zero && apq == 0.0;
      }
    if (zero) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = a[p * n + q];
        if (apq == 0.0) continue;
        const double app = a[p * n + p], aqq = a[q * n + q];
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        double akp = 0.0, akq = 0.0, vkp = 0.0, vkq = 0.0;
        if (lane < n) { akp = a[lane * n + p]; akq = a[lane * n + q]; vkp = v[lane * n + p]; vkq = v[lane * n + q]; }
        pnp_wave_fence();   // every lane has read what it needs of the matrix as it was
        if (lane < n) {
          if (lane != p && lane != q) {
            const double np = c * akp - s * akq, nq = s * akp + c * akq;
            a[lane * n + p] = np; a[p * n + lane] = np;
            a[lane * n + q] = nq; a[q * n + lane] = nq;
          }
          v[lane * n + p] = c * vkp - s * vkq;
          v[lane * n + q] = s * vkp + c * vkq;
        }
        if (lane == 0) {
          a[p * n + p] = app - t * apq;
          a[q * n + q] = aqq + t * apq;
          a[p * n + q] = 0.0;
          a[q * n + p] = 0.0;
        }
        pnp_wave_fence();
      }
  }
}

__device__ inline double pnp_svd_threshold(const double* sig, const int n) {
  double sum = 0.0;
  for (int j = 0; j < n; ++j) sum += sig[j];
  return 2.0 * DBL_EPSILON * sum;
}

// cvSolve(A, b, x, CV_SVD): the minimum-norm least-squares solution of the 6 x n system whose columns are cols[] of L_6x10.  w: 30 + 25 + 5
__device__ inline void pnp_solve_svd(const double* L, const int* cols, const int n, const double* rho, double* x, double* w) {
  double *W = w, *V = w + 30, *sig = w + 55;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < n; ++j) W[i * n + j] = L[10 * i + cols[j]];
  jacobi_svd<false>(W, V, sig, 6, n, kPnpSvdSweeps);
  const double thr = pnp_svd_threshold(sig, n);
  for (int k = 0; k < n; ++k) x[k] = 0.0;
  for (int j = 0; j < n; ++j) {
    if (!(sig[j] > thr)) continue;
    double ub = 0.0;
    for (int i = 0; i < 6; ++i) ub += W[i * n + j] * rho[i];
    const double f = ub / (sig[j] * sig[j]);
    for (int k = 0; k < n; ++k) x[k] += V[k * n + j] * f;
  }
}

// qr_solve (:860-950) of the 6x4 system, literally; returns false at the zero column of :887-891 (X is not written)
__device__ inline bool pnp_qr_solve(double* pA, double* pb, double* pX, double* A1, double* A2) {
  const int nr = 6, nc = 4;
  for (int k = 0; k < nc; ++k) {
    double eta = fabs(pA[k * nc + k]);
    for (int i = k + 1; i < nr; ++i) {   // (the reference reads row i - 1 here: ppAik is advanced after the comparison, :881-885)
      const double elt = fabs(pA[(i - 1) * nc + k]);
      if (eta < elt) eta = elt;
    }
    if (eta == 0) {
      A1[k] = A2[k] = 0.0;
      return false;
    }
    double sum = 0.0;
    const double inv_eta = 1. / eta;
    for (int i = k; i < nr; ++i) {
      pA[i * nc + k] *= inv_eta;
      sum += pA[i * nc + k] * pA[i * nc + k];
    }
    double sigma = sqrt(sum);
    if (pA[k * nc + k] < 0) sigma = -sigma;
    pA[k * nc + k] += sigma;
    A1[k] = sigma * pA[k * nc + k];
    A2[k] = -eta * sigma;
    for (int j = k + 1; j < nc; ++j) {
      double s = 0;
      for (int i = k; i < nr; ++i) s += pA[i * nc + k] * pA[i * nc + j];
      const double tau = s / A1[k];
      for (int i = k; i < nr; ++i) pA[i * nc + j] -= tau * pA[i * nc + k];
    }
  }
  for (int j = 0; j < nc; ++j) {   // b <- Qt b
    double tau = 0;
    for (int i = j; i < nr; ++i) tau += pA[i * nc + j] * pb[i];
    tau /= A1[j];
    for (int i = j; i < nr; ++i) pb[i] -= tau * pA[i * nc + j];
  }
  pX[nc - 1] = pb[nc - 1] / A2[nc - 1];   // X = R-1 b
  for (int i = nc - 2; i >= 0; --i) {
    double sum = 0;
    for (int j = i + 1; j < nc; ++j) sum += pA[i * nc + j] * pX[j];
    pX[i] = (pb[i] - sum) / A2[i];
  }
  return true;
}

// gauss_newton (:840-858) with compute_A_and_b_gauss_newton (:812-838).  w: 24 + 6 + 4 + 4 + 4
__device__ inline void pnp_gauss_newton(const double* L, const double* rho, double* betas, double* w) {
  double *a = w, *b = w + 24, *x = w + 30, *A1 = w + 34, *A2 = w + 38;
  for (int it = 0; it < 5; ++it) {
    for (int i = 0; i < 6; ++i) {
      const double* rowL = L + i * 10;
      double* rowA = a + i * 4;
      rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
      rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
      rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
      rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
      b[i] = rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] +
                       rowL[3] * betas[0] * betas[2] + rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] +
                       rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] + rowL[8] * betas[2] * betas[3] +
                       rowL[9] * betas[3] * betas[3]);
    }
    if (!pnp_qr_solve(a, b, x, A1, A2)) continue;   // the library's rule for :887-891: x = 0 for this step
    for (int i = 0; i < 4; ++i) betas[i] += x[i];
  }
}

// compute_barycentric_coordinates (:423-433) of one point, from the f32 point widened
__device__ inline void pnp_alphas(const PnpShared& S, const float* P3D, const int i, double (&a)[4], double (&p)[3]) {
  p[0] = (double)P3D[3 * i]; p[1] = (double)P3D[3 * i + 1]; p[2] = (double)P3D[3 * i + 2];
  const double d0 = p[0] - S.cws[0][0], d1 = p[1] - S.cws[0][1], d2 = p[2] - S.cws[0][2];
#pragma unroll
  for (int j = 0; j < 3; ++j) a[1 + j] = S.ci[3 * j] * d0 + S.ci[3 * j + 1] * d1 + S.ci[3 * j + 2] * d2;
  a[0] = 1.0 - a[1] - a[2] - a[3];
}

// thread 0 behind the PW0^T PW0 sums: choose_control_points' PCA (:399-408) and the inverse of :413-421
__device__ inline void pnp_control_points_matrix(PnpShared& S) {
  double* a = S.A;
  a[0] = S.sums[0]; a[1] = S.sums[1]; a[2] = S.sums[2];
  a[3] = S.sums[1]; a[4] = S.sums[3]; a[5] = S.sums[4];
  a[6] = S.sums[2]; a[7] = S.sums[4]; a[8] = S.sums[5];
}
__device__ inline void pnp_control_points(PnpShared& S, const int m) {
  double* a = S.A;
  int o0 = 0, o1 = 1, o2 = 2;   // descending, the first of equal ones first
  if (a[4 * o1] > a[4 * o0]) { const int x = o0; o0 = o1; o1 = x; }
  if (a[4 * o2] > a[4 * o1]) { const int x = o1; o1 = o2; o2 = x; }
  if (a[4 * o1] > a[4 * o0]) { const int x = o0; o0 = o1; o1 = x; }
  const int ord[3] = {o0, o1, o2};
  for (int i = 1; i < 4; ++i) {
    const int o = i == 1 ? ord[0] : (i == 2 ? ord[1] : ord[2]);
    const double k = sqrt(a[4 * o] / m);
    for (int j = 0; j < 3; ++j) S.cws[i][j] = S.cws[0][j] + k * S.V[3 * j + o];
  }
  double *W = S.w, *V = S.w + 9, *sig = S.w + 18;
  for (int i = 0; i < 3; ++i)
    for (int j = 1; j < 4; ++j) W[3 * i + j - 1] = S.cws[j][i] - S.cws[0][i];
  jacobi_svd<false>(W, V, sig, 3, 3, kPnpSvdSweeps);
  const double thr = pnp_svd_threshold(sig, 3);
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 3; ++i) {
      double s = 0.0;
      for (int j = 0; j < 3; ++j)
        if (sig[j] > thr) s += V[3 * k + j] * W[3 * i + j] / (sig[j] * sig[j]);
      S.ci[3 * k + i] = s;
    }
}

// thread 0 behind the M^T M sums: the basis (:493), compute_L_6x10 (:760-800), compute_rho (:802-810), the three approximations with their
// Gauss-Newton steps (:506-515), compute_ccs (:453-464) and solve_for_sign (:636-649) of each candidate
__device__ inline void pnp_betas_matrix(PnpShared& S) {
  int k = 0;
  for (int r = 0; r < 12; ++r)
    for (int c = r; c < 12; ++c) { S.A[12 * r + c] = S.sums[k]; S.A[12 * c + r] = S.sums[k]; ++k; }
}
__device__ inline void pnp_betas(PnpShared& S, const PnpPts& pts) {
  // the four smallest eigenvalues ascending (the first of equal ones first): ut rows 11, 10, 9, 8
  unsigned taken = 0;
  for (int i = 0; i < 4; ++i) {
    int best = -1;
    for (int j = 0; j < 12; ++j) {
      if (taken & (1u << j)) continue;
      if (best < 0 || S.A[13 * j] < S.A[13 * best]) best = j;
    }
    taken |= 1u << best;
    S.lam[i] = S.A[13 * best];
    for (int r = 0; r < 12; ++r) S.v[i][r] = S.V[12 * r + best];
  }
  double* dv = S.w;   // [4][6][3]
  for (int i = 0; i < 4; ++i) {
    int a = 0, b = 1;
    for (int j = 0; j < 6; ++j) {
      for (int c = 0; c < 3; ++c) dv[(i * 6 + j) * 3 + c] = S.v[i][3 * a + c] - S.v[i][3 * b + c];
      b++;
      if (b > 3) { a++; b = a + 1; }
    }
  }
  auto dot = [&](int i0, int i1, int j) {
    const double *x = dv + (i0 * 6 + j) * 3, *y = dv + (i1 * 6 + j) * 3;
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2];
  };
  for (int i = 0; i < 6; ++i) {
    double* row = S.L + 10 * i;
    row[0] = dot(0, 0, i);
    row[1] = 2.0 * dot(0, 1, i);
    row[2] = dot(1, 1, i);
    row[3] = 2.0 * dot(0, 2, i);
    row[4] = 2.0 * dot(1, 2, i);
    row[5] = dot(2, 2, i);
    row[6] = 2.0 * dot(0, 3, i);
    row[7] = 2.0 * dot(1, 3, i);
    row[8] = 2.0 * dot(2, 3, i);
    row[9] = dot(3, 3, i);
  }
  auto dist2 = [&](int i0, int i1) {
    const double d0 = S.cws[i0][0] - S.cws[i1][0], d1 = S.cws[i0][1] - S.cws[i1][1], d2 = S.cws[i0][2] - S.cws[i1][2];
    return d0 * d0 + d1 * d1 + d2 * d2;
  };
  S.rho[0] = dist2(0, 1); S.rho[1] = dist2(0, 2); S.rho[2] = dist2(0, 3);
  S.rho[3] = dist2(1, 2); S.rho[4] = dist2(1, 3); S.rho[5] = dist2(2, 3);
  double* b5 = S.w + 64;
  {   // find_betas_approx_1 (:667-694)
    const int cols[4] = {0, 1, 3, 6};
    pnp_solve_svd(S.L, cols, 4, S.rho, b5, S.w);
    double* be = S.betas[0];
    if (b5[0] < 0) { be[0] = sqrt(-b5[0]); be[1] = -b5[1] / be[0]; be[2] = -b5[2] / be[0]; be[3] = -b5[3] / be[0]; }
    else { be[0] = sqrt(b5[0]); be[1] = b5[1] / be[0]; be[2] = b5[2] / be[0]; be[3] = b5[3] / be[0]; }
  }
  {   // find_betas_approx_2 (:699-726)
    const int cols[3] = {0, 1, 2};
    pnp_solve_svd(S.L, cols, 3, S.rho, b5, S.w);
    double* be = S.betas[1];
    if (b5[0] < 0) { be[0] = sqrt(-b5[0]); be[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0; }
    else { be[0] = sqrt(b5[0]); be[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0; }
    if (b5[1] < 0) be[0] = -be[0];
    be[2] = 0.0; be[3] = 0.0;
  }
  {   // find_betas_approx_3 (:731-758)
    const int cols[5] = {0, 1, 2, 3, 4};
    pnp_solve_svd(S.L, cols, 5, S.rho, b5, S.w);
    double* be = S.betas[2];
    if (b5[0] < 0) { be[0] = sqrt(-b5[0]); be[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0; }
    else { be[0] = sqrt(b5[0]); be[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0; }
    if (b5[1] < 0) be[0] = -be[0];
    be[2] = b5[3] / be[0];
    be[3] = 0.0;
  }
  double a[4], p[3];
  pnp_alphas(S, pts.P3D, S.first, a, p);
  for (int c = 0; c < 3; ++c) {
    pnp_gauss_newton(S.L, S.rho, S.betas[c], S.w);
    for (int j = 0; j < 4; ++j)
      for (int x = 0; x < 3; ++x) S.ccs[c][j][x] = 0.0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j)
        for (int x = 0; x < 3; ++x) S.ccs[c][j][x] += S.betas[c][i] * S.v[i][3 * j + x];
    // solve_for_sign looks at pcs[2] of the first correspondence only; negating ccs negates every pc exactly
    const double pcz = a[0] * S.ccs[c][0][2] + a[1] * S.ccs[c][1][2] + a[2] * S.ccs[c][2][2] + a[3] * S.ccs[c][3][2];
    if (pcz < 0.0)
      for (int j = 0; j < 4; ++j)
        for (int x = 0; x < 3; ++x) S.ccs[c][j][x] = -S.ccs[c][j][x];
  }
}

// thread 0 behind the ABt sums: the tail of estimate_R_and_t (:608-626) for candidate c
__device__ inline void pnp_procrustes(PnpShared& S, const int c) {
  double *W = S.w, *V = S.w + 9, *sig = S.w + 18, *U = S.w + 24;
  for (int i = 0; i < 9; ++i) W[i] = S.sums[9 * c + i];
  jacobi_svd<false>(W, V, sig, 3, 3, kPnpSvdSweeps);
  const double thr = pnp_svd_threshold(sig, 3);
  for (int j = 0; j < 3; ++j)
    for (int i = 0; i < 3; ++i) U[3 * i + j] = sig[j] > thr ? W[3 * i + j] / sig[j] : 0.0;
  for (int j = 0; j < 3; ++j)
    if (!(sig[j] > thr)) {   // the library's rule for a vanishing singular value: the cross product of the other two left vectors
      const int a = (j + 1) % 3, b = (j + 2) % 3;
      U[0 + j] = U[3 + a] * U[6 + b] - U[6 + a] * U[3 + b];
      U[3 + j] = U[6 + a] * U[0 + b] - U[0 + a] * U[6 + b];
      U[6 + j] = U[0 + a] * U[3 + b] - U[3 + a] * U[0 + b];
    }
  double* R = S.Rs[c];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + U[3 * i + 2] * V[3 * j + 2];
  const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
  if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
  for (int i = 0; i < 3; ++i) S.ts[c][i] = S.pc0[c][i] - (R[3 * i] * S.pw0[0] + R[3 * i + 1] * S.pw0[1] + R[3 * i + 2] * S.pw0[2]);
}

// compute_pose (:477-525).  <false>: called by the first wave, whose lane 0 has the four sampled points; <true>: called by the whole
// workgroup, the points of pts.mask.  The single-thread algebra is thread 0's; the two symmetric Jacobis are its wave's.  Leaves S.R, S.t,
// S.N and the intermediate results the record takes.
template <bool BLOCK>
__device__ inline void pnp_compute_pose(const PnpPts& pts, PnpShared& S) {
  const bool leader = threadIdx.x == 0, wave0 = threadIdx.x < 64;
  const int lane = threadIdx.x & 63;
  const int m = pts.m;
  if (leader) {
    int first = 0;
    if (BLOCK) {
      first = pts.n;
      for (int w = 0; w < (pts.n + 63) / 64; ++w)
        if (pts.mask[w]) { first = 64 * w + __builtin_ctzll(pts.mask[w]); break; }
      if (first >= pts.n) first = 0;   // (an empty mask never gets here: Refine follows a count >= 1)
    } else {
      first = pts.idx[0];
    }
    S.first = first;
    S.m = m;
  }
  {   // choose_control_points: the centroid (:378-384)
    double acc[3] = {0.0, 0.0, 0.0};
    pnp_for_each<BLOCK>(pts, [&](int i) {
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += (double)pts.P3D[3 * i + c];
    });
    pnp_sum<BLOCK, 3>(acc, S);
    if (leader)
      for (int c = 0; c < 3; ++c) S.cws[0][c] = S.sums[c] / m;
    pnp_sync<BLOCK>();
  }
  {   // PW0^T PW0 (:395-399), upper triangle
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double c0 = S.cws[0][0], c1 = S.cws[0][1], c2 = S.cws[0][2];
    pnp_for_each<BLOCK>(pts, [&](int i) {
      const double d0 = (double)pts.P3D[3 * i] - c0, d1 = (double)pts.P3D[3 * i + 1] - c1, d2 = (double)pts.P3D[3 * i + 2] - c2;
      acc[0] += d0 * d0; acc[1] += d0 * d1; acc[2] += d0 * d2; acc[3] += d1 * d1; acc[4] += d1 * d2; acc[5] += d2 * d2;
    });
    pnp_sum<BLOCK, 6>(acc, S);
    if (wave0) {
      if (leader) pnp_control_points_matrix(S);
      pnp_wave_fence();
      pnp_jacobi_sym(S.A, S.V, 3, lane);
      if (leader) pnp_control_points(S, m);
      pnp_wave_fence();
    }
    pnp_sync<BLOCK>();
  }
  {   // M^T M (:484-492): the 78 entries of the upper triangle
    double acc[78];
#pragma unroll
    for (int k = 0; k < 78; ++k) acc[k] = 0.0;
    pnp_for_each<BLOCK>(pts, [&](int i) {
      double a[4], p[3], M1[12], M2[12];
      pnp_alphas(S, pts.P3D, i, a, p);
      const double u = (double)pts.P2D[2 * i], v = (double)pts.P2D[2 * i + 1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {   // fill_M (:436-451)
        M1[3 * j] = a[j] * pts.fu; M1[3 * j + 1] = 0.0; M1[3 * j + 2] = a[j] * (pts.uc - u);
        M2[3 * j] = 0.0; M2[3 * j + 1] = a[j] * pts.fv; M2[3 * j + 2] = a[j] * (pts.vc - v);
      }
      int k = 0;
#pragma unroll
      for (int r = 0; r < 12; ++r)
#pragma unroll
        for (int c = r; c < 12; ++c) { acc[k] += M1[r] * M1[c] + M2[r] * M2[c]; ++k; }
    });
    pnp_sum<BLOCK, 78>(acc, S);
    if (wave0) {
      if (leader) pnp_betas_matrix(S);
      pnp_wave_fence();
      pnp_jacobi_sym(S.A, S.V, 12, lane);
      if (leader) pnp_betas(S, pts);
      pnp_wave_fence();
    }
    pnp_sync<BLOCK>();
  }
  {   // estimate_R_and_t: pc0 of each candidate and pw0 (:571-588)
    double acc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0;
    pnp_for_each<BLOCK>(pts, [&](int i) {
      double a[4], p[3];
      pnp_alphas(S, pts.P3D, i, a, p);
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int x = 0; x < 3; ++x) acc[3 * c + x] += a[0] * S.ccs[c][0][x] + a[1] * S.ccs[c][1][x] + a[2] * S.ccs[c][2][x] + a[3] * S.ccs[c][3][x];
#pragma unroll
      for (int x = 0; x < 3; ++x) acc[9 + x] += p[x];
    });
    pnp_sum<BLOCK, 12>(acc, S);
    if (leader) {
      for (int c = 0; c < 3; ++c)
        for (int x = 0; x < 3; ++x) S.pc0[c][x] = S.sums[3 * c + x] / m;
      for (int x = 0; x < 3; ++x) S.pw0[x] = S.sums[9 + x] / m;
    }
    pnp_sync<BLOCK>();
  }
  {   // ABt of each candidate (:596-606)
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    pnp_for_each<BLOCK>(pts, [&](int i) {
      double a[4], p[3];
      pnp_alphas(S, pts.P3D, i, a, p);
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double pc = a[0] * S.ccs[c][0][j] + a[1] * S.ccs[c][1][j] + a[2] * S.ccs[c][2][j] + a[3] * S.ccs[c][3][j];
          const double d = pc - S.pc0[c][j];
          acc[9 * c + 3 * j] += d * (p[0] - S.pw0[0]);
          acc[9 * c + 3 * j + 1] += d * (p[1] - S.pw0[1]);
          acc[9 * c + 3 * j + 2] += d * (p[2] - S.pw0[2]);
        }
    });
    pnp_sum<BLOCK, 27>(acc, S);
    if (leader)
      for (int c = 0; c < 3; ++c) pnp_procrustes(S, c);
    pnp_sync<BLOCK>();
  }
  {   // reprojection_error of each candidate (:550-567)
    double acc[3] = {0.0, 0.0, 0.0};
    pnp_for_each<BLOCK>(pts, [&](int i) {
      const double p0 = (double)pts.P3D[3 * i], p1 = (double)pts.P3D[3 * i + 1], p2 = (double)pts.P3D[3 * i + 2];
      const double u = (double)pts.P2D[2 * i], v = (double)pts.P2D[2 * i + 1];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double* R = S.Rs[c];
        const double Xc = (R[0] * p0 + R[1] * p1 + R[2] * p2) + S.ts[c][0];
        const double Yc = (R[3] * p0 + R[4] * p1 + R[5] * p2) + S.ts[c][1];
        const double inv_Zc = 1.0 / ((R[6] * p0 + R[7] * p1 + R[8] * p2) + S.ts[c][2]);
        const double ue = pts.uc + pts.fu * Xc * inv_Zc, ve = pts.vc + pts.fv * Yc * inv_Zc;
        acc[c] += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
      }
    });
    pnp_sum<BLOCK, 3>(acc, S);
    if (leader) {
      for (int c = 0; c < 3; ++c) S.rep[c] = S.sums[c] / m;
      int N = 1;   // :518-520
      if (S.rep[1] < S.rep[0]) N = 2;
      if (S.rep[2] < S.rep[N - 1]) N = 3;
      S.N = N;
      for (int i = 0; i < 9; ++i) S.R[i] = S.Rs[N - 1][i];
      for (int i = 0; i < 3; ++i) S.t[i] = S.ts[N - 1][i];
    }
    pnp_sync<BLOCK>();
  }
}

// thread 0: what the compute_pose that just ended leaves for the host
__device__ inline void pnp_record(const PnpShared& S, PnpRec& r, const int* idx, const int count, const int hypothesis) {
  for (int i = 0; i < 9; ++i) r.R[i] = S.R[i];
  for (int i = 0; i < 3; ++i) { r.t[i] = S.t[i]; r.rep[i] = S.rep[i]; }
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 3; ++j) r.cws[3 * i + j] = S.cws[i][j];
    for (int j = 0; j < 12; ++j) r.v[12 * i + j] = S.v[i][j];
    r.eig[i] = S.lam[i];
    r.betas[i] = S.betas[S.N - 1][i];
    r.idx[i] = idx ? idx[i] : -1;
  }
  r.count = count; r.N = S.N; r.hypothesis = hypothesis; r.pad = 0;
}

// CheckInliers (:308-339) by the whole workgroup on S.R, S.t: ballot words into mask, the count returned to every thread
__device__ inline int pnp_check_inliers(const PnpRansacProb& P, const PnpShared& S, unsigned long long* mask, int* s_cnt) {
  double R[9], tt[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = S.R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) tt[i] = S.t[i];
  const double fu = (double)P.K[0], fv = (double)P.K[1], uc = (double)P.K[2], vc = (double)P.K[3];
  return ransac_score(P.n, P.words, mask, s_cnt, [&](const int i) {
    const double x = (double)P.P3D[3 * i], y = (double)P.P3D[3 * i + 1], z = (double)P.P3D[3 * i + 2];
    const float Xc = (float)(R[0] * x + R[1] * y + R[2] * z + tt[0]);           // :317-319
    const float Yc = (float)(R[3] * x + R[4] * y + R[5] * z + tt[1]);
    const float invZc = (float)(1.0 / (R[6] * x + R[7] * y + R[8] * z + tt[2]));
    const double ue = uc + fu * (double)Xc * (double)invZc;                      // :321-322
    const double ve = vc + fv * (double)Yc * (double)invZc;
    const float distX = (float)((double)P.P2D[2 * i] - ue);                      // :324-325
    const float distY = (float)((double)P.P2D[2 * i + 1] - ve);
    const float error2 = distX * distX + distY * distY;                          // :327
    return error2 < P.maxe[i];                                                   // :329
  });
}

__global__ __launch_bounds__(kPnpThreads) void k_pnp_hyp(const PnpRansacProb* probs, const int32_t* hyp_prob, PnpRec* recs) {
  __shared__ PnpShared S;
  __shared__ int s_cnt[kPnpWaves];
  __shared__ int s_idx[4];
  const int h = blockIdx.x, t = threadIdx.x;
  const PnpRansacProb P = probs[hyp_prob[h]];
  const int k = h - P.hyp_first;
  if (t < 64) {   // (every lane of the wave replays the sampling: the same values, no hand-over)
    PnpPts pts;
    ransac_sample<4>(P.draws + 4 * k, P.n, pts.idx);
    pts.P3D = P.P3D; pts.P2D = P.P2D; pts.n = P.n; pts.m = 4; pts.mask = nullptr;
    pts.fu = (double)P.K[0]; pts.fv = (double)P.K[1]; pts.uc = (double)P.K[2]; pts.vc = (double)P.K[3];
    if (t == 0)
      for (int i = 0; i < 4; ++i) s_idx[i] = pts.idx[i];
    pnp_compute_pose<false>(pts, S);
  }
  asd_syncthreads();
  const int c = pnp_check_inliers(P, S, P.masks + (size_t)k * P.words, s_cnt);
  if (t == 0) pnp_record(S, recs[h], s_idx, c, k);
}

__global__ __launch_bounds__(kPnpThreads) void k_pnp_select(const PnpRansacProb* probs, PnpRec* recs, const int total) {
  __shared__ PnpShared S;
  __shared__ int s_cnt[kPnpWaves];
  const PnpRansacProb P = probs[blockIdx.x];
  const int t = threadIdx.x;
  if (P.n_iter == 0) return;   // a problem that runs nothing (the whole workgroup leaves: no barrier is skipped by a part of it)
  // every value the walk branches on is the same in every thread: the counts are read from memory, a Refine's count comes from LDS
  int best = P.best_in, best_h = -1, found = 0, done = P.n_iter, n_ref = 0, ref_count = 0;
  for (int k = 0; k < P.n_iter; ++k) {
    const int c = recs[P.hyp_first + k].count;
    if (c < P.min_inliers) continue;                         // :209
    if (c > best) {                                          // :212
      best = c;
      best_h = k;
      PnpPts pts;
      pts.P3D = P.P3D; pts.P2D = P.P2D; pts.n = P.n; pts.m = c; pts.mask = P.masks + (size_t)k * P.words;
      pts.fu = (double)P.K[0]; pts.fv = (double)P.K[1]; pts.uc = (double)P.K[2]; pts.vc = (double)P.K[3];
      for (int i = 0; i < 4; ++i) pts.idx[i] = -1;
      pnp_compute_pose<true>(pts, S);                        // Refine (:260-305)
      ref_count = pnp_check_inliers(P, S, P.refmask, s_cnt);
      if (t == 0) pnp_record(S, recs[total + P.hyp_first + n_ref], nullptr, ref_count, k);
      ++n_ref;
    }
    if (n_ref > 0 && ref_count > P.min_inliers) { found = 1; done = k + 1; break; }   // :292
  }
  if (t == 0) {
    P.result[0] = best; P.result[1] = best_h >= 0; P.result[2] = best_h; P.result[3] = found; P.result[4] = done;
    P.result[5] = found ? ref_count : 0; P.result[6] = n_ref; P.result[7] = 0;
  }
  asd_syncthreads();   // the last Refine's ballot words are in memory
  const unsigned long long* const bm = best_h >= 0 ? P.masks + (size_t)best_h * P.words : nullptr;
  for (int i = t; i < P.n; i += kPnpThreads) {
    P.best_mask[i] = bm ? ransac_mask_bit(bm, i) : (uint8_t)0;
    P.inliers[i] = found ? ransac_mask_bit(P.refmask, i) : (uint8_t)0;
  }
}

struct PnpRansacState {
  RansacRecords<PnpRec> hyp;      // recs: the hypotheses of the call, then the Refine slots in the same layout
  std::vector<int32_t> n_ref;     // per problem of the last call
  size_t total = 0;
};

void pnp_tcw(const PnpRec& r, float* T) {   // Rcw.convertTo(CV_32F) into eye(4, 4) (:217-223, :294-300)
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)r.R[3 * i + j];
    T[4 * i + 3] = (float)r.t[i];
  }
  T[12] = T[13] = T[14] = 0.f;
  T[15] = 1.f;
}

}  // namespace

void pnp_ransac_free(asd_ctx* ctx) {
  delete static_cast<PnpRansacState*>(ctx->pnp_ransac);
  ctx->pnp_ransac = nullptr;
}

extern "C" {

int asd_pnp_ransac(asd_ctx* ctx, int32_t n_problems, asd_pnp_ransac_problem* p) {
  if (const int e = ransac_check_call(ctx, "asd_pnp_ransac", n_problems, p, ASD_PNP_RANSAC_MAX_PROBLEMS)) return e;
  // ---- validation: nothing is written before every problem has passed
  std::vector<int32_t> hyps(n_problems, 0);   // the iterations of a problem that runs
  size_t total = 0, up_bytes = 0, down_bytes = 0, mask_bytes = 0;
  for (int32_t j = 0; j < n_problems; ++j) {
    const asd_pnp_ransac_problem& q = p[j];
    if (q.n < 0 || q.n_iter < 0) { ctx->set_error("asd_pnp_ransac: problem %d: negative n or n_iter", j); return ASD_ERR_INVALID; }
    if (q.n < q.min_inliers || q.n_iter == 0) continue;   // :173-177; no iteration to run: nothing to launch
    if (q.n > ASD_PNP_RANSAC_MAX_N) {
      ctx->set_error("asd_pnp_ransac: problem %d: %d correspondences, the limit is %d", j, q.n, ASD_PNP_RANSAC_MAX_N);
      return ASD_ERR_CAPACITY;
    }
    if (q.n < ASD_PNP_MIN_SET) { ctx->set_error("asd_pnp_ransac: problem %d: n = %d, an iteration samples four correspondences", j, q.n); return ASD_ERR_INVALID; }
    if (!q.P3Dw || !q.P2D || !q.max_err || !q.draws || !q.best_mask || !q.inliers) {
      ctx->set_error("asd_pnp_ransac: problem %d: null array", j);
      return ASD_ERR_INVALID;
    }
    if (!ransac_check_draws(ctx, "asd_pnp_ransac", j, q.draws, q.n_iter, ASD_PNP_MIN_SET, q.n)) return ASD_ERR_INVALID;
    hyps[j] = q.n_iter;
    total += (size_t)q.n_iter;
    if (total > ASD_PNP_RANSAC_MAX_HYPOTHESES) {
      ctx->set_error("asd_pnp_ransac: problem %d brings the call to %zu iterations, the limit is %d", j, total, ASD_PNP_RANSAC_MAX_HYPOTHESES);
      return ASD_ERR_CAPACITY;
    }
    up_bytes += (size_t)q.n * 24 + (size_t)q.n_iter * 16 + 8 * 256;
    down_bytes += (size_t)q.n * 2 + 32 + 3 * 256;
    const size_t word_bytes = (((size_t)q.n + 63) / 64) * 8;
    mask_bytes += AsdDevBuf::padded((size_t)q.n_iter * word_bytes) + AsdDevBuf::padded(word_bytes);
  }
  if (!ctx->pnp_ransac) ctx->pnp_ransac = new PnpRansacState();
  PnpRansacState* S = static_cast<PnpRansacState*>(ctx->pnp_ransac);
  S->hyp.reset(n_problems);
  S->total = total;
  S->n_ref.assign(n_problems, 0);
  for (int32_t j = 0; j < n_problems; ++j)
    if (!hyps[j]) ransac_runs_nothing(p[j]);   // :173-177, or no iteration to run (:182)
  ctx->ms_pnp_ransac = 0;
  if (total == 0) return ASD_OK;
  std::vector<size_t> off_bm(n_problems, 0), off_inl(n_problems, 0), off_res(n_problems, 0);
  hipStream_t st = ctx->stream;
  const auto pack = [&](const int32_t j, PnpRansacProb& d) {
    const asd_pnp_ransac_problem& q = p[j];
    const size_t n = (size_t)q.n;
    d.n = q.n; d.n_iter = q.n_iter; d.min_inliers = q.min_inliers; d.best_in = q.best_inliers;
    d.words = (int32_t)((n + 63) / 64);
    memcpy(d.K, q.K, 16);
    d.P3D = ctx->up.dev<float>(ctx->up.add(q.P3Dw, n * 12));
    d.P2D = ctx->up.dev<float>(ctx->up.add(q.P2D, n * 8));
    d.maxe = ctx->up.dev<float>(ctx->up.add(q.max_err, n * 4));
    d.draws = ctx->up.dev<int32_t>(ctx->up.add(q.draws, (size_t)q.n_iter * 16));
    d.masks = ctx->scratch.carve<unsigned long long>((size_t)q.n_iter * d.words);
    d.refmask = ctx->scratch.carve<unsigned long long>((size_t)d.words);
    off_bm[j] = ctx->down.reserve(n);
    off_inl[j] = ctx->down.reserve(n);
    off_res[j] = ctx->down.reserve(32);
    d.best_mask = ctx->down.dev<uint8_t>(off_bm[j]);
    d.inliers = ctx->down.dev<uint8_t>(off_inl[j]);
    d.result = ctx->down.dev<int32_t>(off_res[j]);
  };
  const int e = ransac_run<PnpRansacProb>(
      ctx, hyps, up_bytes, down_bytes, mask_bytes + 256, 2 * total, &ctx->ms_pnp_ransac, nullptr, S->hyp, pack,
      [&](unsigned grid, const PnpRansacProb* probs, const int32_t* map, PnpRec* recs) {
        hipLaunchKernelGGL(k_pnp_hyp, dim3(grid), dim3(kPnpThreads), 0, st, probs, map, recs);
      },
      [&](unsigned grid, const PnpRansacProb* probs, PnpRec* recs) {
        hipLaunchKernelGGL(k_pnp_select, dim3(grid), dim3(kPnpThreads), 0, st, probs, recs, (int)total);
      });
  if (e != ASD_OK) return e;
  const std::vector<PnpRec>& recs = S->hyp.recs;
  for (int32_t j = 0; j < n_problems; ++j) {
    if (!hyps[j]) continue;
    const size_t first = (size_t)S->hyp.first[j];
    asd_pnp_ransac_problem& q = p[j];
    const int32_t* r = ctx->down.host<int32_t>(off_res[j]);
    S->n_ref[j] = r[6];
    q.best_inliers = r[0];
    q.best_updated = r[1];
    if (r[1]) {   // :214-223
      pnp_tcw(recs[first + r[2]], q.best_Tcw);
      memcpy(q.best_mask, ctx->down.host<uint8_t>(off_bm[j]), (size_t)q.n);
    }
    q.found = r[3];
    q.iterations_done = r[4];
    q.n_inliers = r[5];
    if (r[3]) pnp_tcw(recs[total + first + r[6] - 1], q.Tcw);   // the Refine that returned is the last one the walk ran
    memcpy(q.inliers, ctx->down.host<uint8_t>(off_inl[j]), (size_t)q.n);
  }
  return ASD_OK;
}

int32_t asd_debug_pnp_ransac(const asd_ctx* ctx, int32_t problem, int32_t which, asd_pnp_ransac_debug* out) {
  if (!ctx || !out) return ASD_ERR_INVALID;
  const PnpRansacState* S = static_cast<const PnpRansacState*>(ctx->pnp_ransac);
  if (!S || problem < 0 || problem >= (int32_t)S->hyp.count.size()) return ASD_ERR_INVALID;
  size_t at;
  if (which >= 0) {
    if (which >= S->hyp.count[problem]) return ASD_ERR_INVALID;
    at = (size_t)S->hyp.first[problem] + which;
  } else {
    const int32_t r = -1 - which;
    if (r >= S->n_ref[problem]) return ASD_ERR_INVALID;
    at = S->total + (size_t)S->hyp.first[problem] + r;
  }
  const PnpRec& r = S->hyp.recs[at];
  memcpy(out->idx, r.idx, sizeof out->idx);
  out->count = r.count;
  out->n_refines = S->n_ref[problem];
  out->N = r.N;
  out->hypothesis = r.hypothesis;
  memcpy(out->R, r.R, sizeof out->R);
  memcpy(out->t, r.t, sizeof out->t);
  memcpy(out->cws, r.cws, sizeof out->cws);
  memcpy(out->v, r.v, sizeof out->v);
  memcpy(out->eig, r.eig, sizeof out->eig);
  memcpy(out->rep_errors, r.rep, sizeof out->rep_errors);
  memcpy(out->betas, r.betas, sizeof out->betas);
  return ASD_OK;
}

}  // extern "C"
