// gba.hip -- the reduced pose system of Optimizer::BundleAdjustment (Optimizer.cc:51-237) at map scale, on gfx950, fp64.
//
// asd_bundle_adjustment (ba.hip) shares LocalBA's edge, reduction, Schur, step and Levenberg-control kernels.  What it cannot share
// is the dense solve: LocalBA's window has a dozen free keyframes and its solvers are ONE workgroup (k_ba_solve_lds / k_ba_chol_lds
// in LDS up to 32 pose blocks, k_ba_chol out of global memory beyond).  A map has hundreds of free keyframes: n = 6 nPf rows.
//
// Here: a right-looking tiled Cholesky of A + lambda I over the whole chip.  Tiles are kGbaTile = 96 rows (16 pose blocks, 6 x 16 MFMA
// rows).  Per tile column k:
//   k_gba_potrf   one workgroup: the diagonal tile factored in LDS
//   k_gba_trsm    one workgroup per tile below: X = A(i,k) L(k,k)^-T, a row per thread, both tiles in LDS
//   k_gba_syrk    one workgroup per lower tile (i >= j > k): A(i,j) -= L(i,k) L(j,k)^T -- the O(n^3) part, on v_mfma_f64_16x16x4_f64
//                 (or plain FMA: the A/B form the timing tool measures)
// then k_gba_fwd / k_gba_bwd, one launch per tile column each: the workgroup of tile row i takes the contribution of the column
// solved by the launch before, the workgroup of the diagonal tile then solves its 96 unknowns in LDS.
// Ordering between all of these is by launches on one stream: no workgroup waits for another, no grid barrier.  Every sum has a
// fixed shape and order (no float atomics): two runs of one problem give the same bits.
// A pivot that is not positive clears *chol_ok (and is replaced by 1 so that nothing downstream divides by zero); the Levenberg
// control then rejects the trial, as g2o does for a failed solve() (optimization_algorithm_levenberg.cpp:126-127).
#include "gba.h"

namespace {

constexpr int TS = kGbaTile;      // rows of a tile
constexpr int LDT = TS + 1;       // LDS row stride of a whole tile (odd: a column walk hits every bank)
constexpr int KC = 48;            // k-chunk of the trailing update
constexpr int LDK = KC + 1;

typedef double v4d __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_gba_clear(double* __restrict__ A, size_t count, const int* __restrict__ done) {
  if (*done) return;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) A[i] = 0.0;
}

// the diagonal tile (k, k): L L^T = A, column by column in LDS.  dynamic LDS: Ls[TS][LDT], dg[TS], one int
__global__ __launch_bounds__(256) void k_gba_potrf(double* __restrict__ A, int n, int k, const int* __restrict__ done, int* __restrict__ chol_ok) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* Ls = sm;
  double* dg = sm + TS * LDT;
  int* bad = reinterpret_cast<int*>(dg + TS);
  if (*done) return;
  const int t = threadIdx.x;
  const int k0 = k * TS, tk = min(TS, n - k0);
  for (int idx = t; idx < tk * tk; idx += 256) {
    const int r = idx / tk, c = idx % tk;
    if (c <= r) Ls[r * LDT + c] = A[(size_t)(k0 + r) * n + k0 + c];
  }
  if (t == 0) *bad = 0;
  asd_syncthreads();
  for (int j = 0; j < tk; ++j) {
    const double p = Ls[j * LDT + j];
    const bool neg = !(p > 0.0);
    const double d = sqrt(neg ? 1.0 : p);
    if (t == 0) {
      dg[j] = d;
      if (neg) *bad = 1;
    }
    for (int i = j + 1 + t; i < tk; i += 256) Ls[i * LDT + j] /= d;
    asd_syncthreads();
    const int m = tk - j - 1;
    for (int idx = t; idx < m * m; idx += 256) {
      const int i = j + 1 + idx / m, c = j + 1 + idx % m;
      if (c <= i) Ls[i * LDT + c] -= Ls[i * LDT + j] * Ls[c * LDT + j];
    }
    asd_syncthreads();
  }
  for (int idx = t; idx < tk * tk; idx += 256) {
    const int r = idx / tk, c = idx % tk;
    if (c <= r) A[(size_t)(k0 + r) * n + k0 + c] = c == r ? dg[r] : Ls[r * LDT + c];
  }
  if (t == 0) {
    if (k == 0) *chol_ok = *bad ? 0 : 1;
    else if (*bad) *chol_ok = 0;
  }
}

// tile (i, k), i = k + 1 + blockIdx.x: X L(k,k)^T = A(i,k), one row of X per thread.  dynamic LDS: Ls[TS][LDT], Xs[TS][LDT]
__global__ __launch_bounds__(128) void k_gba_trsm(double* __restrict__ A, int n, int k, const int* __restrict__ done) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* Ls = sm;
  double* Xs = sm + TS * LDT;
  if (*done) return;
  const int t = threadIdx.x;
  const int k0 = k * TS, i0 = (k + 1 + (int)blockIdx.x) * TS, ti = min(TS, n - i0);   // (a tile below exists: column k is TS wide)
  for (int idx = t; idx < TS * TS; idx += 128) {
    const int r = idx / TS, c = idx % TS;
    Ls[r * LDT + c] = A[(size_t)(k0 + r) * n + k0 + c];
    Xs[r * LDT + c] = r < ti ? A[(size_t)(i0 + r) * n + k0 + c] : 0.0;
  }
  asd_syncthreads();
  if (t < ti) {
    double* xr = Xs + t * LDT;
    for (int c = 0; c < TS; ++c) {
      double s = xr[c];
      const double* lc = Ls + c * LDT;
      for (int m = 0; m < c; ++m) s -= xr[m] * lc[m];
      xr[c] = s / lc[c];
    }
  }
  asd_syncthreads();
  for (int idx = t; idx < ti * TS; idx += 128) {
    const int r = idx / TS, c = idx % TS;
    A[(size_t)(i0 + r) * n + k0 + c] = Xs[r * LDT + c];
  }
}

// trailing update of the lower tile (i, j), k < j <= i: A(i,j) -= L(i,k) L(j,k)^T.  blockIdx.x numbers the lower triangle of the
// trailing tiles row by row.  dynamic LDS: Pi[TS][LDK], Pj[TS][LDK] -- the two panels, a chunk of KC columns at a time.
// MFMA: the tile is 6 x 6 blocks of 16 x 16, nine per wave; v_mfma_f64_16x16x4_f64 takes A[row = lane & 15][k = lane >> 4] and
// B[k = lane >> 4][col = lane & 15], one double per lane each, and leaves D[row = (lane >> 4) + 4 reg][col = lane & 15].
// Plain FMA: a 6 x 6 micro-tile per thread.
template <bool MFMA>
__global__ __launch_bounds__(256) void k_gba_syrk(double* __restrict__ A, int n, int k, const int* __restrict__ done) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* Pi = sm;
  double* Pj = sm + TS * LDK;
  if (*done) return;
  const int t = threadIdx.x;
  int a = (int)((sqrtf(8.f * (float)blockIdx.x + 1.f) - 1.f) * 0.5f);
  while ((a + 1) * (a + 2) / 2 <= (int)blockIdx.x) ++a;
  while (a * (a + 1) / 2 > (int)blockIdx.x) --a;
  const int b = (int)blockIdx.x - a * (a + 1) / 2;
  const int k0 = k * TS, i0 = (k + 1 + a) * TS, j0 = (k + 1 + b) * TS;
  const int ti = min(TS, n - i0), tj = min(TS, n - j0);
  const bool diag = a == b;
  const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);   // (scalar: the block tests below are branches, not masks)
  v4d accm[9];
  double accf[36];
  if constexpr (MFMA) {
#pragma unroll
    for (int u = 0; u < 9; ++u) accm[u] = v4d{0.0, 0.0, 0.0, 0.0};
  } else {
#pragma unroll
    for (int q = 0; q < 36; ++q) accf[q] = 0.0;
  }
  for (int kc = 0; kc < TS; kc += KC) {
    if (kc) asd_syncthreads();
    for (int idx = t; idx < TS * KC; idx += 256) {
      const int r = idx / KC, c = idx % KC;
      Pi[r * LDK + c] = r < ti ? A[(size_t)(i0 + r) * n + k0 + kc + c] : 0.0;
      Pj[r * LDK + c] = r < tj ? A[(size_t)(j0 + r) * n + k0 + kc + c] : 0.0;
    }
    asd_syncthreads();
    if constexpr (MFMA) {
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        const int q = wave + 4 * u, rb = q / 6, cb = q % 6;
        if (rb * 16 >= ti || cb * 16 >= tj || (diag && cb > rb)) continue;   // (uniform over the wave)
        const double* pa = Pi + (rb * 16 + (lane & 15)) * LDK + (lane >> 4);
        const double* pb = Pj + (cb * 16 + (lane & 15)) * LDK + (lane >> 4);
#pragma unroll
        for (int s = 0; s < KC / 4; ++s) accm[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[4 * s], pb[4 * s], accm[u], 0, 0, 0);
      }
    } else {
      const int ty = t >> 4, tx = t & 15;
      for (int kk = 0; kk < KC; ++kk) {
        double av[6], bv[6];
#pragma unroll
        for (int r = 0; r < 6; ++r) { av[r] = Pi[(ty * 6 + r) * LDK + kk]; bv[r] = Pj[(tx * 6 + r) * LDK + kk]; }
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int c = 0; c < 6; ++c) accf[r * 6 + c] += av[r] * bv[c];
      }
    }
  }
  if constexpr (MFMA) {
#pragma unroll
    for (int u = 0; u < 9; ++u) {
      const int q = wave + 4 * u, rb = q / 6, cb = q % 6;
      if (rb * 16 >= ti || cb * 16 >= tj || (diag && cb > rb)) continue;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int gi = rb * 16 + (lane >> 4) + 4 * reg, gj = cb * 16 + (lane & 15);
        if (gi < ti && gj < tj) A[(size_t)(i0 + gi) * n + j0 + gj] -= accm[u][reg];
      }
    }
  } else {
    const int ty = t >> 4, tx = t & 15;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const int gi = ty * 6 + r, gj = tx * 6 + c;
        if (gi < ti && gj < tj && !(diag && gj > gi)) A[(size_t)(i0 + gi) * n + j0 + gj] -= accf[r * 6 + c];
      }
  }
}

// forward substitution L y = b, launch k = 0 .. nt - 1 with nt - k workgroups: the workgroup of tile row i = k + blockIdx.x takes
// y_i -= L(i, k-1) y_(k-1) (launch 0: y_i = b_i), the first one then solves L(k,k) y_k = y_k in LDS.
// dynamic LDS: Ls[TS][LDT], xs[TS], ys[TS], out[TS]
__global__ __launch_bounds__(384) void k_gba_fwd(const double* __restrict__ A, const double* __restrict__ b, double* __restrict__ x, int n,
                                                 int k, const int* __restrict__ done) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* Ls = sm;
  double* xs = Ls + TS * LDT;
  double* ys = xs + TS;
  double* out = ys + TS;
  if (*done) return;
  const int t = threadIdx.x;
  const int i0 = (k + (int)blockIdx.x) * TS, ti = min(TS, n - i0);
  if (k == 0) {
    if (t < ti) ys[t] = b[i0 + t];
  } else {
    const int kp0 = (k - 1) * TS;   // (column k - 1 is TS wide: tile row k exists)
    if (t < TS) xs[t] = x[kp0 + t];
    asd_syncthreads();
    const int g = t >> 4, l16 = t & 15;   // sixteen lanes walk a row
    for (int rr = 0; rr < 4; ++rr) {
      const int r = rr * 24 + g;
      double s = 0.0;
      if (r < ti) {
        const double* row = A + (size_t)(i0 + r) * n + kp0;
#pragma unroll
        for (int cc = 0; cc < 6; ++cc) s += row[cc * 16 + l16] * xs[cc * 16 + l16];
      }
      s += __shfl_xor(s, 8);
      s += __shfl_xor(s, 4);
      s += __shfl_xor(s, 2);
      s += __shfl_xor(s, 1);
      if (l16 == 0 && r < ti) ys[r] = x[i0 + r] - s;
    }
  }
  asd_syncthreads();
  if (blockIdx.x != 0) {
    if (t < ti) x[i0 + t] = ys[t];
    return;
  }
  for (int idx = t; idx < ti * ti; idx += 384) {
    const int r = idx / ti, c = idx % ti;
    if (c <= r) Ls[r * LDT + c] = A[(size_t)(i0 + r) * n + i0 + c];
  }
  asd_syncthreads();
  for (int j = 0; j < ti; ++j) {
    const double yj = ys[j] / Ls[j * LDT + j];
    if (t == j) out[j] = yj;
    if (t > j && t < ti) ys[t] -= Ls[t * LDT + j] * yj;
    asd_syncthreads();
  }
  if (t < ti) x[i0 + t] = out[t];
}

// backward substitution L^T x = y, launch k = nt - 1 .. 0 with k + 1 workgroups: the workgroup of tile row i = k - blockIdx.x takes
// x_i -= L(k+1, i)^T x_(k+1), the first one then solves L(k,k)^T x_k = x_k in LDS.
// dynamic LDS: Ls[TS][LDT], xs[TS], ys[TS], out[TS], part[4][TS]
__global__ __launch_bounds__(384) void k_gba_bwd(const double* __restrict__ A, double* __restrict__ x, int n, int k, int nt,
                                                 const int* __restrict__ done) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* Ls = sm;
  double* xs = Ls + TS * LDT;
  double* ys = xs + TS;
  double* out = ys + TS;
  double* part = out + TS;
  if (*done) return;
  const int t = threadIdx.x;
  const int i0 = (k - (int)blockIdx.x) * TS, ti = min(TS, n - i0);
  if (k == nt - 1) {
    if (blockIdx.x != 0) return;
    if (t < ti) ys[t] = x[i0 + t];
  } else {
    const int k1 = (k + 1) * TS, tk1 = min(TS, n - k1);   // (tile rows <= k < nt - 1 are TS high)
    if (t < tk1) xs[t] = x[k1 + t];
    asd_syncthreads();
    const int r = t % TS, seg = t / TS;
    double s = 0.0;
    for (int c = seg * 24; c < min(seg * 24 + 24, tk1); ++c) s += A[(size_t)(k1 + c) * n + i0 + r] * xs[c];
    part[seg * TS + r] = s;
    asd_syncthreads();
    if (t < TS) ys[t] = x[i0 + t] - (((part[t] + part[TS + t]) + part[2 * TS + t]) + part[3 * TS + t]);
  }
  asd_syncthreads();
  if (blockIdx.x != 0) {
    if (t < ti) x[i0 + t] = ys[t];
    return;
  }
  for (int idx = t; idx < ti * ti; idx += 384) {
    const int r = idx / ti, c = idx % ti;
    if (c <= r) Ls[r * LDT + c] = A[(size_t)(i0 + r) * n + i0 + c];
  }
  asd_syncthreads();
  for (int j = ti - 1; j >= 0; --j) {
    const double xj = ys[j] / Ls[j * LDT + j];
    if (t == j) out[j] = xj;
    if (t < j) ys[t] -= Ls[j * LDT + t] * xj;
    asd_syncthreads();
  }
  if (t < ti) x[i0 + t] = out[t];
}

constexpr size_t kPotrfLds = ((size_t)TS * LDT + TS) * sizeof(double) + 16;
constexpr size_t kTrsmLds = (size_t)2 * TS * LDT * sizeof(double);
constexpr size_t kSyrkLds = (size_t)2 * TS * LDK * sizeof(double);
constexpr size_t kFwdLds = ((size_t)TS * LDT + 3 * TS) * sizeof(double);
constexpr size_t kBwdLds = ((size_t)TS * LDT + 7 * TS) * sizeof(double);
static_assert(kTrsmLds <= 160 * 1024, "two whole tiles fit the LDS of a CU");

}  // namespace

int gba_clear_enqueue(asd_ctx* ctx, hipStream_t st, double* A, int n, const int* done) {
  const size_t count = (size_t)n * (size_t)n;
  if (!count) return ASD_OK;
  const unsigned grid = (unsigned)std::min<size_t>((count + 255) / 256, 8192);
  hipLaunchKernelGGL(k_gba_clear, dim3(grid), dim3(256), 0, st, A, count, done);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  return ASD_OK;
}

int gba_solve_enqueue(asd_ctx* ctx, hipStream_t st, double* A, const double* b, double* x, int n, const int* done, int* chol_ok, bool mfma) {
  if (n <= 0) { ctx->set_error("gba_solve_enqueue: n = %d is not positive", n); return ASD_ERR_INVALID; }
  static AsdPerDeviceOnce attr_set;   // the dynamic-LDS attribute is per device
  if (attr_set.need(ctx->cfg.device)) {
    ASD_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_gba_potrf), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPotrfLds));
    ASD_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_gba_trsm), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTrsmLds));
    ASD_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_gba_syrk<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSyrkLds));
    ASD_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_gba_syrk<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSyrkLds));
    ASD_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_gba_fwd), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFwdLds));
    ASD_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_gba_bwd), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBwdLds));
    attr_set.done(ctx->cfg.device);
  }
  const int nt = (n + TS - 1) / TS;
  for (int k = 0; k < nt; ++k) {
    hipLaunchKernelGGL(k_gba_potrf, dim3(1), dim3(256), kPotrfLds, st, A, n, k, done, chol_ok);
    const int m = nt - k - 1;
    if (m > 0) {
      hipLaunchKernelGGL(k_gba_trsm, dim3(m), dim3(128), kTrsmLds, st, A, n, k, done);
      if (mfma) hipLaunchKernelGGL(k_gba_syrk<true>, dim3(m * (m + 1) / 2), dim3(256), kSyrkLds, st, A, n, k, done);
      else hipLaunchKernelGGL(k_gba_syrk<false>, dim3(m * (m + 1) / 2), dim3(256), kSyrkLds, st, A, n, k, done);
    }
  }
  for (int k = 0; k < nt; ++k) hipLaunchKernelGGL(k_gba_fwd, dim3(nt - k), dim3(384), kFwdLds, st, A, b, x, n, k, done);
  for (int k = nt - 1; k >= 0; --k) hipLaunchKernelGGL(k_gba_bwd, dim3(k + 1), dim3(384), kBwdLds, st, A, x, n, k, nt, done);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  return ASD_OK;
}
