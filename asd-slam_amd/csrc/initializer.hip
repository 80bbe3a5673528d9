// initializer.hip -- Initializer (reference src/vslam/src/Initializer.cc) on the device: asd_initialize.
//
// Initializer::Initialize (:43-120) is two RANSACs over the same minimal sets -- FindHomography (:123-171) and FindFundamental (:174-222),
// each iteration a small SVD and one pass over all matches -- followed by ReconstructH (:583-749) or ReconstructF (:482-581), which
// triangulate every inlier under 8 or 4 motion hypotheses (CheckRT, :840-949).  The two halves are the two kernels:
//  * k_init_hyp, one workgroup per (problem, iteration, model).  Thread 0 replays the sampling (ransac_sample), builds A from the normalised
//    points (every entry the f32 product the reference forms), takes its null vector by a one-sided Jacobi (jacobi_svd) in f64 and forms H21i / H12i or
//    F21i in the rules the header states; the workgroup then evaluates CheckHomography / CheckFundamental for all matches in the reference's
//    f32 operations (this file is compiled with -ffp-contract=off).  The per-match terms are computed in parallel and added by one lane in
//    match order, test 1 before test 2: the score is the reference's sequential f32 sum.  Each wave stores its 64 decisions as a ballot word.
//  * k_init_reconstruct, one workgroup per problem.  Thread 0 walks the scores (strict >, from 0.0f), chooses the model and derives the
//    motion hypotheses; the workgroup runs CheckRT for every (hypothesis, inlier match) pair; each wave then counts the good points of its
//    hypotheses and selects vCosParallax[min(50, size - 1)] by a bitwise search over order-preserving keys (no sort); thread 0 applies the
//    acceptance rule literally, and the workgroup scatters the winner's points to the keypoints of frame 1.
//    (The reconstruction stays one launch: its pairs are spread over the whole workgroup whatever the hypothesis count, so a launch per
//    hypothesis would add launches without shortening the longest lane.)
// Normalize (:791-837) runs on the host in front of the upload (asd_initializer_normalize: sequential f32 sums).  No atomics; everything the
// host reads travels in the context's one result block.  The small matrices live in LDS: no dynamically indexed private array.
// The sampling, the one-sided Jacobi SVD, the ballot words and the host half of the call are ransac.h's.
#include "ctx.h"
#include "ransac.h"
#include "svd4.h"

#include <cfloat>
#include <cmath>

namespace {

constexpr int kInitThreads = kRansacThreads, kInitWaves = kRansacWaves;
constexpr int kInitSvdSweeps = 60;   // one-sided Jacobi on at most 16x9: done after 6-10 sweeps; the cap bounds a NaN input
constexpr unsigned kKeyNaN = 0xfffffffeu, kKeyNone = 0xffffffffu;

// what one (iteration, model) leaves (result block; asd_debug_initialize reads the host copy)
struct InitHypRec {
  double nullv[9], U[9], w[3], Vt[9];
  float M1[9], M2[9], score;
  int32_t idx[8], pad;
};
static_assert(sizeof(InitHypRec) == 30 * 8 + 19 * 4 + 36, "InitHypRec is laid out without holes");

// what the reconstruction of one problem leaves
struct InitReconRec {
  double U[9], w[3], Vt[9];
  float R[8][9], t[8][3], parallax[8], cos_sel[8];
  int32_t n_good[8];
  int32_t best_H, best_F, n_inliers, n_hyp, winner, second_good, model, ok;
  float SH, SF, R21[9], t21[3], pad[2];
};
static_assert(sizeof(InitReconRec) == 21 * 8 + 112 * 4 + 32 + 32 + 64, "InitReconRec is laid out without holes");

// one problem as the kernels see it (upload block); every pointer is device memory
struct InitProb {
  int32_t n1, n2, N, n_iter, hyp_first, words, min_tri, pad0;
  float K[4], sigma, min_parallax;
  float T1[9], T2[9], T2inv[9], pad1[3];
  const float *keys1, *keys2, *pn1, *pn2;   // [n][2] each: mvKeys, vPn
  const int32_t *m1, *m2, *draws;           // mvMatches12 [N] first / second; [n_iter][8]
  unsigned long long* masks;                // [2 n_iter][words]: iteration k of model m at 2 k + m
  float* pts;                               // [8][N][3]
  uint8_t* flags;                           // [8][N]
  unsigned* keys;                           // [8][N] (scratch): the cosines as order-preserving keys
  float* P3D;                               // [n1][3] out
  uint8_t *tri, *inl_H, *inl_F;             // [n1], [N], [N] out
  InitReconRec* rec;
};

// C = A * B (3x3): f64 on the widened elements, terms in index order, one rounding per element
__host__ __device__ inline void init_mul33(const float* A, const float* B, float* C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = (double)A[3 * i] * (double)B[j];
      s += (double)A[3 * i + 1] * (double)B[3 + j];
      s += (double)A[3 * i + 2] * (double)B[6 + j];
      C[3 * i + j] = (float)s;
    }
}
__host__ __device__ inline double init_det33(const float* M) {
  const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
  return a * (e * i - f * h) + b * (f * g - d * i) + c * (d * h - e * g);
}
// inv(): adjugate over determinant in f64, one rounding; a zero determinant gives the zero matrix
__host__ __device__ inline void init_inv33(const float* M, float* out) {
  const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
  const double c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
  const double det = a * c00 + b * c01 + c * c02;
  if (det == 0.0) {
    for (int k = 0; k < 9; ++k) out[k] = 0.f;
    return;
  }
  out[0] = (float)(c00 / det); out[1] = (float)((c * h - b * i) / det); out[2] = (float)((b * f - c * e) / det);
  out[3] = (float)(c01 / det); out[4] = (float)((a * i - c * g) / det); out[5] = (float)((c * d - a * f) / det);
  out[6] = (float)(c02 / det); out[7] = (float)((b * g - a * h) / det); out[8] = (float)((a * e - b * d) / det);
}

// the 3x3 decomposition of the f32 matrix M by the header's rule: U, w (descending), Vt in f64.  ws: 9 + 9 + 3
__device__ inline void init_svd3(const float* M, double* U, double* w, double* Vt, double* ws) {
  double *W = ws, *V = ws + 9, *sig = ws + 18;
  for (int i = 0; i < 9; ++i) W[i] = (double)M[i];
  jacobi_svd<true>(W, V, sig, 3, 3, kInitSvdSweeps);
  int o0 = 0, o1 = 1, o2 = 2;   // descending, the first of equal ones first
  if (sig[o1] > sig[o0]) { const int x = o0; o0 = o1; o1 = x; }
  if (sig[o2] > sig[o1]) { const int x = o1; o1 = o2; o2 = x; }
  if (sig[o1] > sig[o0]) { const int x = o0; o0 = o1; o1 = x; }
  const double thr = 2.0 * DBL_EPSILON * (sig[0] + sig[1] + sig[2]);
  for (int j = 0; j < 3; ++j) {
    const int o = j == 0 ? o0 : (j == 1 ? o1 : o2);
    w[j] = sig[o];
    for (int i = 0; i < 3; ++i) {
      U[3 * i + j] = sig[o] > thr ? W[3 * i + o] / sig[o] : 0.0;
      Vt[3 * j + i] = V[3 * i + o];
    }
  }
  for (int j = 0; j < 3; ++j) {   // the sign convention: the component of v_j of largest magnitude (the first of equal ones) is positive
    int big = 0;
    if (fabs(Vt[3 * j + 1]) > fabs(Vt[3 * j + big])) big = 1;
    if (fabs(Vt[3 * j + 2]) > fabs(Vt[3 * j + big])) big = 2;
    if (Vt[3 * j + big] < 0.0)
      for (int i = 0; i < 3; ++i) { Vt[3 * j + i] = -Vt[3 * j + i]; U[3 * i + j] = -U[3 * i + j]; }
  }
  for (int j = 0; j < 3; ++j)
    if (!(w[j] > thr)) {   // a vanishing singular value: the cross product of the other two left vectors
      const int a = (j + 1) % 3, b = (j + 2) % 3;
      U[0 + j] = U[3 + a] * U[6 + b] - U[6 + a] * U[3 + b];
      U[3 + j] = U[6 + a] * U[0 + b] - U[0 + a] * U[6 + b];
      U[6 + j] = U[0 + a] * U[3 + b] - U[3 + a] * U[0 + b];
    }
}

struct InitHypShared {
  double W[16 * 9], V[81], sig[9];
  double ws[21], U[9], w[3], Vt[9], nullv[9];
  float Hn[9], A[9], B[9], D[9], M1[9], M2[9];
  float terms[2 * kInitThreads];
  int idx[8];
};

__global__ __launch_bounds__(kInitThreads) void k_init_hyp(const InitProb* probs, const int32_t* hyp_prob, InitHypRec* recs) {
  __shared__ InitHypShared S;
  const int h = blockIdx.x, t = threadIdx.x;
  const InitProb& P = probs[hyp_prob[h]];
  const int local = h - P.hyp_first, k = local >> 1, model = local & 1;
  const int N = P.N;
  if (t == 0) {
    ransac_sample<8>(P.draws + 8 * k, N, S.idx);
    const int rows = model == 0 ? 16 : 8;
    for (int j = 0; j < 8; ++j) {
      const int i1 = P.m1[S.idx[j]], i2 = P.m2[S.idx[j]];
      const float u1 = P.pn1[2 * i1], v1 = P.pn1[2 * i1 + 1], u2 = P.pn2[2 * i2], v2 = P.pn2[2 * i2 + 1];
      if (model == 0) {   // ComputeH21 (:238-256)
        double* a = S.W + 18 * j;
        a[0] = 0.0; a[1] = 0.0; a[2] = 0.0; a[3] = (double)-u1; a[4] = (double)-v1; a[5] = -1.0;
        a[6] = (double)(v2 * u1); a[7] = (double)(v2 * v1); a[8] = (double)v2;
        a[9] = (double)u1; a[10] = (double)v1; a[11] = 1.0; a[12] = 0.0; a[13] = 0.0; a[14] = 0.0;
        a[15] = (double)(-u2 * u1); a[16] = (double)(-u2 * v1); a[17] = (double)-u2;
      } else {            // ComputeF21 (:288-296)
        double* a = S.W + 9 * j;
        a[0] = (double)(u2 * u1); a[1] = (double)(u2 * v1); a[2] = (double)u2;
        a[3] = (double)(v2 * u1); a[4] = (double)(v2 * v1); a[5] = (double)v2;
        a[6] = (double)u1; a[7] = (double)v1; a[8] = 1.0;
      }
    }
    jacobi_svd<true>(S.W, S.V, S.sig, rows, 9, kInitSvdSweeps);
    int best = 0;
    for (int j = 1; j < 9; ++j)
      if (S.sig[j] <= S.sig[best]) best = j;
    double n2 = 0.0;
    for (int i = 0; i < 9; ++i) n2 += S.V[9 * i + best] * S.V[9 * i + best];
    int big = 0;   // the sign convention: the component of largest magnitude (the first of equal ones) is positive
    for (int i = 1; i < 9; ++i)
      if (fabs(S.V[9 * i + best]) > fabs(S.V[9 * big + best])) big = i;
    const double nrm = S.V[9 * big + best] < 0.0 ? -sqrt(n2) : sqrt(n2);
    for (int i = 0; i < 9; ++i) {
      S.nullv[i] = S.V[9 * i + best] / nrm;
      S.Hn[i] = (float)S.nullv[i];   // vt.row(8).reshape(0, 3) is CV_32F
    }
    if (model == 0) {
      init_mul33(P.T2inv, S.Hn, S.A);      // H21i = T2inv * Hn * T1 (:159)
      init_mul33(S.A, P.T1, S.M1);
      init_inv33(S.M1, S.M2);              // H12i = H21i.inv() (:160)
      for (int i = 0; i < 9; ++i) { S.U[i] = 0.0; S.Vt[i] = 0.0; }
      for (int i = 0; i < 3; ++i) S.w[i] = 0.0;
    } else {
      init_svd3(S.Hn, S.U, S.w, S.Vt, S.ws);   // :305
      for (int i = 0; i < 9; ++i) { S.A[i] = (float)S.U[i]; S.B[i] = (float)S.Vt[i]; S.D[i] = 0.f; }
      S.D[0] = (float)S.w[0]; S.D[4] = (float)S.w[1]; S.D[8] = 0.f;   // w.at<float>(2) = 0 (:307)
      init_mul33(S.A, S.D, S.M2);          // u * diag(w) * vt (:309)
      init_mul33(S.M2, S.B, S.Hn);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) S.A[3 * i + j] = P.T2[3 * j + i];   // T2t (:184)
      init_mul33(S.A, S.Hn, S.B);          // F21i = T2t * Fn * T1 (:211)
      init_mul33(S.B, P.T1, S.M1);
      for (int i = 0; i < 9; ++i) S.M2[i] = 0.f;
    }
  }
  asd_syncthreads();
  float m[9], mi[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) { m[i] = S.M1[i]; mi[i] = S.M2[i]; }
  const float sigma = P.sigma;
  const float invSigmaSquare = (float)(1.0 / (double)(sigma * sigma));   // :342, :418
  const float thH = (float)5.991, thF = (float)3.841, thScore = (float)5.991;
  unsigned long long* mask = P.masks + (size_t)local * P.words;
  float score = 0.f;
  for (int base = 0; base < N; base += kInitThreads) {   // (uniform trip count: every lane reaches the ballot and the barriers)
    const int i = base + t;
    bool in = false;
    float term1 = 0.f, term2 = 0.f;   // a test that fails adds nothing: score + (+0) is score
    if (i < N) {
      const int i1 = P.m1[i], i2 = P.m2[i];
      const float u1 = P.keys1[2 * i1], v1 = P.keys1[2 * i1 + 1], u2 = P.keys2[2 * i2], v2 = P.keys2[2 * i2 + 1];
      in = true;
      if (model == 0) {   // CheckHomography (:359-386)
        const float w2in1inv = (float)(1.0 / (double)(mi[6] * u2 + mi[7] * v2 + mi[8]));
        const float u2in1 = (mi[0] * u2 + mi[1] * v2 + mi[2]) * w2in1inv;
        const float v2in1 = (mi[3] * u2 + mi[4] * v2 + mi[5]) * w2in1inv;
        const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
        const float chiSquare1 = squareDist1 * invSigmaSquare;
        if (chiSquare1 > thH) in = false; else term1 = thH - chiSquare1;
        const float w1in2inv = (float)(1.0 / (double)(m[6] * u1 + m[7] * v1 + m[8]));
        const float u1in2 = (m[0] * u1 + m[1] * v1 + m[2]) * w1in2inv;
        const float v1in2 = (m[3] * u1 + m[4] * v1 + m[5]) * w1in2inv;
        const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
        const float chiSquare2 = squareDist2 * invSigmaSquare;
        if (chiSquare2 > thH) in = false; else term2 = thH - chiSquare2;
      } else {            // CheckFundamental (:439-470)
        const float a2 = m[0] * u1 + m[1] * v1 + m[2];
        const float b2 = m[3] * u1 + m[4] * v1 + m[5];
        const float c2 = m[6] * u1 + m[7] * v1 + m[8];
        const float num2 = a2 * u2 + b2 * v2 + c2;
        const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
        const float chiSquare1 = squareDist1 * invSigmaSquare;
        if (chiSquare1 > thF) in = false; else term1 = thScore - chiSquare1;
        const float a1 = m[0] * u2 + m[3] * v2 + m[6];
        const float b1 = m[1] * u2 + m[4] * v2 + m[7];
        const float c1 = m[2] * u2 + m[5] * v2 + m[8];
        const float num1 = a1 * u1 + b1 * v1 + c1;
        const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
        const float chiSquare2 = squareDist2 * invSigmaSquare;
        if (chiSquare2 > thF) in = false; else term2 = thScore - chiSquare2;
      }
    }
    S.terms[2 * t] = term1;
    S.terms[2 * t + 1] = term2;
    ransac_ballot_word(in, base, P.words, mask);
    asd_syncthreads();
    if (t == 0) {
      const int cnt = 2 * min(kInitThreads, N - base);
      for (int j = 0; j < cnt; ++j) score += S.terms[j];   // the reference's order: match by match, test 1 before test 2
    }
    asd_syncthreads();
  }
  if (t == 0) {
    InitHypRec& r = recs[h];
    for (int i = 0; i < 9; ++i) { r.nullv[i] = S.nullv[i]; r.U[i] = S.U[i]; r.Vt[i] = S.Vt[i]; r.M1[i] = S.M1[i]; r.M2[i] = S.M2[i]; }
    for (int i = 0; i < 3; ++i) r.w[i] = S.w[i];
    for (int i = 0; i < 8; ++i) r.idx[i] = S.idx[i];
    r.score = score;
    r.pad = 0;
  }
}

struct InitReconShared {
  double ws[21], U[9], w[3], Vt[9];
  float Uf[9], Vtf[9], Kf[9], A[9], B[9], M[9];
  float R[8][9], t[8][3], P2[8][12], O2[8][3];
  float parallax[8], cos_sel[8], SH, SF, R21[9], t21[3];
  int n_good[8];
  int nh, model, best_H, best_F, n_inl, winner, second, ok, best;
};

// t / cv::norm(t): each element divided by the f64 norm
__device__ inline void init_unit3(const float* v, float* out) {
  const double n = sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]);
  for (int i = 0; i < 3; ++i) out[i] = (float)((double)v[i] / n);
}
__device__ inline void init_matvec3(const float* A, const float* x, float* y) {
  for (int i = 0; i < 3; ++i) {
    double s = (double)A[3 * i] * (double)x[0];
    s += (double)A[3 * i + 1] * (double)x[1];
    s += (double)A[3 * i + 2] * (double)x[2];
    y[i] = (float)s;
  }
}

// thread 0: the eight hypotheses of ReconstructH (:595-697) from S.M = H21; leaves S.nh = 0 at the return of :607-611
__device__ inline void init_hypotheses_H(InitReconShared& S) {
  init_inv33(S.Kf, S.A);                 // invK (:595)
  init_mul33(S.A, S.M, S.B);             // A = invK * H21 * K (:596)
  init_mul33(S.B, S.Kf, S.A);
  init_svd3(S.A, S.U, S.w, S.Vt, S.ws);  // :599
  for (int i = 0; i < 9; ++i) { S.Uf[i] = (float)S.U[i]; S.Vtf[i] = (float)S.Vt[i]; }
  const float s = (float)(init_det33(S.Uf) * init_det33(S.Vtf));   // :602
  const float d1 = (float)S.w[0], d2 = (float)S.w[1], d3 = (float)S.w[2];
  if ((double)(d1 / d2) < 1.0000001 || (double)(d2 / d3) < 1.0000001) { S.nh = 0; return; }   // :607
  const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));   // :619-620
  const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);   // :625
  const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);                                    // :627
  const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);     // :662
  const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);                                      // :664
  for (int i = 0; i < 9; ++i) S.M[i] = (float)((double)s * (double)S.Uf[i]);   // s * U
  // tp = (x1, 0, -+x3) * (d1 -+ d3) (:641-645, :679-683): the four products once; a sign in front of a factor is the sign of the product
  const float km = d1 - d3, kp = d1 + d3;
  const float a1m = aux1 * km, a3m = aux3 * km, zm = 0.f * km, a1p = aux1 * kp, a3p = aux3 * kp, zp = 0.f * kp;
  for (int h = 0; h < 8; ++h) {
    const int i = h & 3;
    const bool neg1 = i >= 2, neg3 = (i & 1) != 0;                                 // x1[] and x3[] (:621-622)
    const float sg = (i == 0 || i == 3) ? 1.f : -1.f;                              // :628, :665
    float* Rp = S.A;
    for (int q = 0; q < 9; ++q) Rp[q] = 0.f;
    float tp[3];
    if (h < 4) {
      const float st = sg * aux_stheta;
      Rp[0] = ctheta; Rp[2] = -st; Rp[4] = 1.f; Rp[6] = st; Rp[8] = ctheta;     // :632-636
      tp[0] = neg1 ? -a1m : a1m; tp[1] = zm; tp[2] = neg3 ? a3m : -a3m;
    } else {
      const float sp = sg * aux_sphi;
      Rp[0] = cphi; Rp[2] = sp; Rp[4] = -1.f; Rp[6] = sp; Rp[8] = -cphi;         // :669-674
      tp[0] = neg1 ? -a1p : a1p; tp[1] = zp; tp[2] = neg3 ? -a3p : a3p;
    }
    init_mul33(S.M, Rp, S.B);            // R = s * U * Rp * Vt (:638, :676)
    init_mul33(S.B, S.Vtf, S.R[h]);
    float tt[3];
    init_matvec3(S.Uf, tp, tt);          // t = U * tp (:647, :685)
    init_unit3(tt, S.t[h]);              // t / cv::norm(t) (:648, :686)
  }
  S.nh = 8;
}

// thread 0: the four hypotheses of ReconstructF (:491-509) with DecomposeE (:951-971) from S.M = F21
__device__ inline void init_hypotheses_F(InitReconShared& S) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) S.A[3 * i + j] = S.Kf[3 * j + i];
  init_mul33(S.A, S.M, S.B);             // E21 = K.t() * F21 * K (:491)
  init_mul33(S.B, S.Kf, S.A);
  init_svd3(S.A, S.U, S.w, S.Vt, S.ws);  // :954
  for (int i = 0; i < 9; ++i) { S.Uf[i] = (float)S.U[i]; S.Vtf[i] = (float)S.Vt[i]; }
  const float u2[3] = {S.Uf[2], S.Uf[5], S.Uf[8]};
  float tt[3];
  init_unit3(u2, tt);                    // :956-957
  for (int r = 0; r < 2; ++r) {
    float* W = S.A;
    for (int q = 0; q < 9; ++q) W[q] = 0.f;
    if (r == 0) { W[1] = -1.f; W[3] = 1.f; W[8] = 1.f; }   // W (:959-962)
    else { W[1] = 1.f; W[3] = -1.f; W[8] = 1.f; }          // W.t() (:968)
    init_mul33(S.Uf, W, S.B);
    init_mul33(S.B, S.Vtf, S.R[r]);
    if (init_det33(S.R[r]) < 0)                             // :965, :969
      for (int q = 0; q < 9; ++q) S.R[r][q] = -S.R[r][q];
  }
  for (int q = 0; q < 9; ++q) { S.R[2][q] = S.R[0][q]; S.R[3][q] = S.R[1][q]; }   // (R1, t1), (R2, t1), (R1, t2), (R2, t2) (:506-509)
  for (int i = 0; i < 3; ++i) { S.t[0][i] = tt[i]; S.t[1][i] = tt[i]; S.t[2][i] = -tt[i]; S.t[3][i] = -tt[i]; }
  S.nh = 4;
}

// the body of CheckRT's loop (:877-935) for one inlier match under one hypothesis.  flags: bit 0 = counted in nGood, bit 1 = vbGood
__device__ inline void init_check_rt(const float* K, const float* Rl, const float* tl, const float* P2l, const float* O2l, const float x1,
                                     const float y1, const float x2, const float y2, const float th2, float (&X)[3], float& cosParallax,
                                     unsigned& flags) {
  float R[9], t[3], P2[12], O2[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = Rl[i];
#pragma unroll
  for (int i = 0; i < 12; ++i) P2[i] = P2l[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) { t[i] = tl[i]; O2[i] = O2l[i]; }
  const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  const float P1[12] = {fx, 0.f, cx, 0.f, 0.f, fy, cy, 0.f, 0.f, 0.f, 1.f, 0.f};   // K [I | 0] (:857-858)
  flags = 0;
  cosParallax = 0.f;
  float A[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {   // Triangulate (:778-781)
    A[0][k] = scaled_minus(x1, P1[8 + k], P1[0 + k]);
    A[1][k] = scaled_minus(y1, P1[8 + k], P1[4 + k]);
    A[2][k] = scaled_minus(x2, P2[8 + k], P2[0 + k]);
    A[3][k] = scaled_minus(y2, P2[8 + k], P2[4 + k]);
  }
  const Row4 c0{{A[0][0], A[1][0], A[2][0], A[3][0]}}, c1{{A[0][1], A[1][1], A[2][1], A[3][1]}},
      c2{{A[0][2], A[1][2], A[2][2], A[3][2]}}, c3{{A[0][3], A[1][3], A[2][3], A[3][3]}};
  const Row4 v = svd4_last_vt(c0, c1, c2, c3);
  const float inv = (float)(1.0 / (double)v.v[3]);   // :786
  X[0] = v.v[0] * inv + 0.0f; X[1] = v.v[1] * inv + 0.0f; X[2] = v.v[2] * inv + 0.0f;
  if (!isfinite(X[0]) || !isfinite(X[1]) || !isfinite(X[2])) return;   // :883
  const float dist1 = (float)sqrt((double)X[0] * X[0] + (double)X[1] * X[1] + (double)X[2] * X[2]);   // normal1 = p3dC1 - O1, O1 = 0 (:890-891)
  const float n2[3] = {X[0] - O2[0], X[1] - O2[1], X[2] - O2[2]};                                      // :893
  const float dist2 = (float)sqrt((double)n2[0] * n2[0] + (double)n2[1] * n2[1] + (double)n2[2] * n2[2]);
  double dot = (double)X[0] * (double)n2[0];
  dot += (double)X[1] * (double)n2[1];
  dot += (double)X[2] * (double)n2[2];
  cosParallax = (float)(dot / (double)(dist1 * dist2));   // :896
  const bool low = (double)cosParallax < 0.99998;
  if (X[2] <= 0 && low) return;                           // :899
  float p2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {                           // p3dC2 = R * p3dC1 + t (:903)
    double s = (double)R[3 * i] * (double)X[0];
    s += (double)R[3 * i + 1] * (double)X[1];
    s += (double)R[3 * i + 2] * (double)X[2];
    s += (double)t[i];
    p2[i] = (float)s;
  }
  if (p2[2] <= 0 && low) return;                          // :905
  const float invZ1 = (float)(1.0 / (double)X[2]);        // :910-914
  const float im1x = fx * X[0] * invZ1 + cx, im1y = fy * X[1] * invZ1 + cy;
  const float squareError1 = (im1x - x1) * (im1x - x1) + (im1y - y1) * (im1y - y1);
  if (squareError1 > th2) return;                         // :916
  const float invZ2 = (float)(1.0 / (double)p2[2]);       // :921-925
  const float im2x = fx * p2[0] * invZ2 + cx, im2y = fy * p2[1] * invZ2 + cy;
  const float squareError2 = (im2x - x2) * (im2x - x2) + (im2y - y2) * (im2y - y2);
  if (squareError2 > th2) return;                         // :927
  flags = low ? 3u : 1u;                                  // :930-935
}

// an order-preserving key of a cosine: -0 and +0 are one key, a NaN orders after every number
__device__ inline unsigned init_key(const float c) {
  if (c != c) return kKeyNaN;
  const unsigned u = __float_as_uint(c + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float init_unkey(const unsigned k) {
  if (k == kKeyNaN) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(kInitThreads) void k_init_reconstruct(const InitProb* probs, const InitHypRec* recs) {
  __shared__ InitReconShared S;
  const InitProb& P = probs[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int N = P.N;
  if (t == 0) {
    float SH = 0.0f, SF = 0.0f;   // :136, :187
    int bH = -1, bF = -1;
    for (int k = 0; k < P.n_iter; ++k) {
      const float sh = recs[P.hyp_first + 2 * k].score, sf = recs[P.hyp_first + 2 * k + 1].score;
      if (sh > SH) { SH = sh; bH = k; }   // :164
      if (sf > SF) { SF = sf; bF = k; }   // :215
    }
    const float RH = SH / (SH + SF);      // :113
    S.model = (double)RH > 0.40 ? 0 : 1;  // :114
    S.SH = SH; S.SF = SF; S.best_H = bH; S.best_F = bF;
    S.best = S.model == 0 ? bH : bF;
    S.nh = 0;
    S.Kf[0] = P.K[0]; S.Kf[1] = 0.f; S.Kf[2] = P.K[2]; S.Kf[3] = 0.f; S.Kf[4] = P.K[1]; S.Kf[5] = P.K[3]; S.Kf[6] = 0.f; S.Kf[7] = 0.f; S.Kf[8] = 1.f;
    for (int i = 0; i < 9; ++i) { S.U[i] = 0.0; S.Vt[i] = 0.0; }
    for (int i = 0; i < 3; ++i) S.w[i] = 0.0;
    for (int h = 0; h < 8; ++h) {
      for (int i = 0; i < 9; ++i) S.R[h][i] = 0.f;
      for (int i = 0; i < 3; ++i) S.t[h][i] = 0.f;
      S.n_good[h] = 0; S.parallax[h] = 0.f; S.cos_sel[h] = __uint_as_float(0x7fc00000u);
    }
    if (S.best >= 0) {
      const InitHypRec& r = recs[P.hyp_first + 2 * S.best + S.model];
      for (int i = 0; i < 9; ++i) S.M[i] = r.M1[i];
      if (S.model == 0) init_hypotheses_H(S); else init_hypotheses_F(S);
    }
    for (int h = 0; h < S.nh; ++h) {
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 4; ++j) {   // P2 = K * [R | t] (:863-866)
          double s = (double)S.Kf[3 * i] * (double)(j < 3 ? S.R[h][j] : S.t[h][0]);
          s += (double)S.Kf[3 * i + 1] * (double)(j < 3 ? S.R[h][3 + j] : S.t[h][1]);
          s += (double)S.Kf[3 * i + 2] * (double)(j < 3 ? S.R[h][6 + j] : S.t[h][2]);
          S.P2[h][4 * i + j] = (float)s;
        }
        double s = (double)S.R[h][i] * (double)S.t[h][0];   // O2 = -R.t() * t (:868)
        s += (double)S.R[h][3 + i] * (double)S.t[h][1];
        s += (double)S.R[h][6 + i] * (double)S.t[h][2];
        S.O2[h][i] = (float)-s;
      }
    }
  }
  asd_syncthreads();
  const int nh = S.nh, best = S.best, model = S.model;
  const unsigned long long* bm = best >= 0 ? P.masks + (size_t)(2 * best + model) * P.words : nullptr;
  const float th2 = (float)(4.0 * (double)(P.sigma * P.sigma));   // 4.0 * mSigma2 (:506, :714)
  const float qnan = __uint_as_float(0x7fc00000u);
  for (int p = t; p < nh * N; p += kInitThreads) {
    const int h = p / N, i = p - h * N;
    float X[3] = {qnan, qnan, qnan}, c = 0.f;
    unsigned fl = 0;
    if (ransac_mask_bit(bm, i)) {   // :874
      const int i1 = P.m1[i], i2 = P.m2[i];
      init_check_rt(P.K, S.R[h], S.t[h], S.P2[h], S.O2[h], P.keys1[2 * i1], P.keys1[2 * i1 + 1], P.keys2[2 * i2], P.keys2[2 * i2 + 1], th2, X, c, fl);
    }
    P.pts[3 * (size_t)p] = X[0]; P.pts[3 * (size_t)p + 1] = X[1]; P.pts[3 * (size_t)p + 2] = X[2];
    P.flags[p] = (uint8_t)fl;
    P.keys[p] = (fl & 1u) ? init_key(c) : kKeyNone;
  }
  asd_syncthreads();   // the keys and flags are in memory
  for (int h = wave; h < nh; h += kInitWaves) {   // one wave per hypothesis: shuffles only
    const unsigned* keys = P.keys + (size_t)h * N;
    int good = 0;
    for (int i = lane; i < N; i += 64) good += keys[i] != kKeyNone;
    for (int off = 32; off >= 1; off >>= 1) good += __shfl_xor(good, off);
    float cs = qnan, par = 0.f;   // :946
    if (good > 0) {               // :938-944
      const int idx = min(50, good - 1);
      unsigned key = 0;           // the largest key with at most idx keys below it = the idx-th smallest key
      for (int b = 31; b >= 0; --b) {
        const unsigned trial = key | (1u << b);
        int below = 0;
        for (int i = lane; i < N; i += 64) below += keys[i] < trial;
        for (int off = 32; off >= 1; off >>= 1) below += __shfl_xor(below, off);
        if (below <= idx) key = trial;
      }
      cs = init_unkey(key);
      par = (float)(acos((double)cs) * 180 / 3.1415926535897932384626433832795);
    }
    if (lane == 0) { S.n_good[h] = good; S.cos_sel[h] = cs; S.parallax[h] = par; }
  }
  asd_syncthreads();
  if (t == 0) {
    int n_inl = 0;
    if (bm)
      for (int w = 0; w < P.words; ++w) n_inl += __popcll(bm[w]);   // :485-488, :586-589
    int winner = -1, second = 0, ok = 0;
    if (nh == 4) {
      const int g0 = S.n_good[0], g1 = S.n_good[1], g2 = S.n_good[2], g3 = S.n_good[3];
      const int maxGood = max(g0, max(g1, max(g2, g3)));                 // :510
      const int nMinGood = max((int)(0.9 * n_inl), P.min_tri);          // :515
      int nsimilar = 0;
      if (g0 > 0.7 * maxGood) nsimilar++;                                // :518-525
      if (g1 > 0.7 * maxGood) nsimilar++;
      if (g2 > 0.7 * maxGood) nsimilar++;
      if (g3 > 0.7 * maxGood) nsimilar++;
      if (!(maxGood < nMinGood || nsimilar > 1)) {                       // :528
        const int c = maxGood == g0 ? 0 : (maxGood == g1 ? 1 : (maxGood == g2 ? 2 : 3));   // :534-567: the first that holds, no other is tried
        if (S.parallax[c] > P.min_parallax) { winner = c; ok = 1; }
      }
    } else if (nh == 8) {
      int bestGood = 0, bestIdx = -1;
      float bestParallax = -1;
      for (int h = 0; h < 8; ++h) {                                      // :709-731
        const int g = S.n_good[h];
        if (g > bestGood) { second = bestGood; bestGood = g; bestIdx = h; bestParallax = S.parallax[h]; }
        else if (g > second && g < bestGood) second = g;
      }
      if (second < 0.75 * bestGood && bestParallax >= P.min_parallax && bestGood > P.min_tri && bestGood > 0.9 * n_inl) {   // :738
        winner = bestIdx; ok = 1;
      }
    }
    S.n_inl = n_inl; S.winner = winner; S.second = second; S.ok = ok;
    InitReconRec& r = *P.rec;
    for (int i = 0; i < 9; ++i) { r.U[i] = S.U[i]; r.Vt[i] = S.Vt[i]; }
    for (int i = 0; i < 3; ++i) r.w[i] = S.w[i];
    for (int h = 0; h < 8; ++h) {
      for (int i = 0; i < 9; ++i) r.R[h][i] = S.R[h][i];
      for (int i = 0; i < 3; ++i) r.t[h][i] = S.t[h][i];
      r.parallax[h] = S.parallax[h]; r.cos_sel[h] = S.cos_sel[h]; r.n_good[h] = S.n_good[h];
    }
    r.best_H = S.best_H; r.best_F = S.best_F; r.n_inliers = n_inl; r.n_hyp = nh; r.winner = winner; r.second_good = second;
    r.model = model; r.ok = ok; r.SH = S.SH; r.SF = S.SF;
    for (int i = 0; i < 9; ++i) r.R21[i] = ok ? S.R[winner][i] : 0.f;
    for (int i = 0; i < 3; ++i) r.t21[i] = ok ? S.t[winner][i] : 0.f;
    r.pad[0] = r.pad[1] = 0.f;
  }
  asd_syncthreads();
  const unsigned long long* mH = S.best_H >= 0 ? P.masks + (size_t)(2 * S.best_H) * P.words : nullptr;
  const unsigned long long* mF = S.best_F >= 0 ? P.masks + (size_t)(2 * S.best_F + 1) * P.words : nullptr;
  for (int i = t; i < N; i += kInitThreads) {
    P.inl_H[i] = mH ? ransac_mask_bit(mH, i) : (uint8_t)0;
    P.inl_F[i] = mF ? ransac_mask_bit(mF, i) : (uint8_t)0;
  }
  for (int i = t; i < P.n1; i += kInitThreads) {   // vP3D.resize / vbGood(false) (:850-851)
    P.P3D[3 * i] = 0.f; P.P3D[3 * i + 1] = 0.f; P.P3D[3 * i + 2] = 0.f;
    P.tri[i] = 0;
  }
  asd_syncthreads();
  if (S.ok) {
    const size_t o = (size_t)S.winner * N;
    for (int i = t; i < N; i += kInitThreads) {
      const unsigned fl = P.flags[o + i];
      if (!(fl & 1u)) continue;
      const int i1 = P.m1[i];   // (a keypoint of frame 1 has at most one match: no two lanes write one slot)
      P.P3D[3 * i1] = P.pts[3 * (o + i)]; P.P3D[3 * i1 + 1] = P.pts[3 * (o + i) + 1]; P.P3D[3 * i1 + 2] = P.pts[3 * (o + i) + 2];   // :931
      P.tri[i1] = (uint8_t)((fl >> 1) & 1u);                                                                                       // :934-935
    }
  }
}

struct InitProbState {
  int32_t N = 0, words = 0;
  InitReconRec rec;
  std::vector<unsigned long long> masks;
  std::vector<float> pts;
  std::vector<uint8_t> flags;
};
struct InitState {
  RansacRecords<InitHypRec> hyp;   // per problem 2 n_iter records: iteration k of model m at 2 k + m
  std::vector<InitProbState> probs;
};

void init_normalize(const int N, const float* keys, float* pts, float* T) {   // Initializer::Normalize (:791-837), literally
  float meanX = 0, meanY = 0;
  for (int i = 0; i < N; i++) {
    meanX += keys[2 * i];
    meanY += keys[2 * i + 1];
  }
  meanX = meanX / N;
  meanY = meanY / N;
  float meanDevX = 0, meanDevY = 0;
  for (int i = 0; i < N; i++) {
    pts[2 * i] = keys[2 * i] - meanX;
    pts[2 * i + 1] = keys[2 * i + 1] - meanY;
    meanDevX += fabsf(pts[2 * i]);
    meanDevY += fabsf(pts[2 * i + 1]);
  }
  meanDevX = meanDevX / N;
  meanDevY = meanDevY / N;
  const float sX = (float)(1.0 / meanDevX);
  const float sY = (float)(1.0 / meanDevY);
  for (int i = 0; i < N; i++) {
    pts[2 * i] = pts[2 * i] * sX;
    pts[2 * i + 1] = pts[2 * i + 1] * sY;
  }
  T[0] = sX; T[1] = 0.f; T[2] = -meanX * sX;
  T[3] = 0.f; T[4] = sY; T[5] = -meanY * sY;
  T[6] = 0.f; T[7] = 0.f; T[8] = 1.f;
}

}  // namespace

void initializer_free(asd_ctx* ctx) {
  delete static_cast<InitState*>(ctx->initializer);
  ctx->initializer = nullptr;
}

extern "C" {

int asd_initializer_normalize(int32_t n, const float* keys, float* pts_out, float* T_out) {
  if (n < 0 || !T_out || (n > 0 && (!keys || !pts_out))) return ASD_ERR_INVALID;
  init_normalize(n, keys, pts_out, T_out);
  return ASD_OK;
}

int asd_initialize(asd_ctx* ctx, int32_t n_problems, asd_initializer_problem* p) {
  if (const int e = ransac_check_call(ctx, "asd_initialize", n_problems, p, ASD_INIT_MAX_PROBLEMS)) return e;
  // ---- validation: nothing is written before every problem has passed
  std::vector<int32_t> Ns(n_problems, 0), hyps(n_problems, 0);   // matches; (iteration, model) pairs
  size_t total = 0, up_bytes = 0, down_bytes = 0, key_count = 0;
  for (int32_t j = 0; j < n_problems; ++j) {
    const asd_initializer_problem& q = p[j];
    if (q.n1 < 0 || q.n2 < 0 || q.n_iter < 1) { ctx->set_error("asd_initialize: problem %d: negative n1 / n2 or n_iter < 1", j); return ASD_ERR_INVALID; }
    if (q.n1 > ASD_INIT_MAX_KEYS || q.n2 > ASD_INIT_MAX_KEYS) {
      ctx->set_error("asd_initialize: problem %d: %d / %d keypoints, the limit is %d", j, q.n1, q.n2, ASD_INIT_MAX_KEYS);
      return ASD_ERR_CAPACITY;
    }
    if (q.n_iter > ASD_INIT_MAX_ITERATIONS) {
      ctx->set_error("asd_initialize: problem %d: %d iterations, the limit is %d", j, q.n_iter, ASD_INIT_MAX_ITERATIONS);
      return ASD_ERR_CAPACITY;
    }
    if (!q.keys1 || !q.keys2 || !q.matches12 || !q.draws || !q.P3D || !q.triangulated || !q.inliers_H || !q.inliers_F) {
      ctx->set_error("asd_initialize: problem %d: null array", j);
      return ASD_ERR_INVALID;
    }
    int32_t N = 0;
    for (int32_t i = 0; i < q.n1; ++i) {
      const int32_t m = q.matches12[i];
      if (m < -1 || m >= q.n2) { ctx->set_error("asd_initialize: problem %d: matches12[%d] = %d is outside [-1, %d)", j, i, m, q.n2); return ASD_ERR_INVALID; }
      N += m >= 0;
    }
    if (N < 8) { ctx->set_error("asd_initialize: problem %d: %d matches, an iteration samples eight", j, N); return ASD_ERR_INVALID; }
    if (!ransac_check_draws(ctx, "asd_initialize", j, q.draws, q.n_iter, 8, N)) return ASD_ERR_INVALID;
    Ns[j] = N;
    hyps[j] = 2 * q.n_iter;
    const size_t words = ((size_t)N + 63) / 64;
    total += 2 * (size_t)q.n_iter;
    up_bytes += ((size_t)q.n1 + q.n2) * 16 + (size_t)N * 8 + (size_t)q.n_iter * 32 + 8 * 256;
    down_bytes += 2 * (size_t)q.n_iter * words * 8 + (size_t)N * (96 + 8 + 2) + (size_t)q.n1 * 13 + sizeof(InitReconRec) + 8 * 256;
    key_count += 8 * (size_t)N + 64;
  }
  if (!ctx->initializer) ctx->initializer = new InitState();
  InitState* S = static_cast<InitState*>(ctx->initializer);
  S->hyp.reset(n_problems);
  S->probs.clear();
  ctx->ms_initializer = ctx->ms_initializer_hyp = 0;
  if (n_problems == 0) return ASD_OK;
  struct Offs { size_t masks, pts, flags, P3D, tri, inlH, inlF, rec; };
  std::vector<Offs> offs(n_problems);
  hipStream_t st = ctx->stream;
  const auto pack = [&](const int32_t j, InitProb& d) {
    const asd_initializer_problem& q = p[j];
    const size_t N = (size_t)Ns[j], n1 = (size_t)q.n1, n2 = (size_t)q.n2;
    d.n1 = q.n1; d.n2 = q.n2; d.N = Ns[j]; d.n_iter = q.n_iter;
    d.words = (int32_t)((N + 63) / 64);
    d.min_tri = q.min_triangulated;
    memcpy(d.K, q.K, 16);
    d.sigma = q.sigma; d.min_parallax = q.min_parallax;
    d.keys1 = ctx->up.dev<float>(ctx->up.add(q.keys1, n1 * 8));
    d.keys2 = ctx->up.dev<float>(ctx->up.add(q.keys2, n2 * 8));
    const size_t o_pn1 = ctx->up.reserve(n1 * 8), o_pn2 = ctx->up.reserve(n2 * 8);
    init_normalize(q.n1, q.keys1, ctx->up.host<float>(o_pn1), d.T1);   // :131-132, :182-183: over all keys of the frame
    init_normalize(q.n2, q.keys2, ctx->up.host<float>(o_pn2), d.T2);
    init_inv33(d.T2, d.T2inv);                                         // :133
    d.pn1 = ctx->up.dev<float>(o_pn1);
    d.pn2 = ctx->up.dev<float>(o_pn2);
    const size_t o_m1 = ctx->up.reserve(N * 4), o_m2 = ctx->up.reserve(N * 4);
    int32_t *m1 = ctx->up.host<int32_t>(o_m1), *m2 = ctx->up.host<int32_t>(o_m2);
    for (int32_t i = 0, k = 0; i < q.n1; ++i)   // mvMatches12 (:55-64)
      if (q.matches12[i] >= 0) { m1[k] = i; m2[k] = q.matches12[i]; ++k; }
    d.m1 = ctx->up.dev<int32_t>(o_m1);
    d.m2 = ctx->up.dev<int32_t>(o_m2);
    d.draws = ctx->up.dev<int32_t>(ctx->up.add(q.draws, (size_t)q.n_iter * 32));
    Offs& o = offs[j];
    o.masks = ctx->down.reserve(2 * (size_t)q.n_iter * d.words * 8);
    o.pts = ctx->down.reserve(8 * N * 12);
    o.flags = ctx->down.reserve(8 * N);
    o.P3D = ctx->down.reserve(n1 * 12);
    o.tri = ctx->down.reserve(n1);
    o.inlH = ctx->down.reserve(N);
    o.inlF = ctx->down.reserve(N);
    o.rec = ctx->down.reserve(sizeof(InitReconRec));
    d.masks = ctx->down.dev<unsigned long long>(o.masks);
    d.pts = ctx->down.dev<float>(o.pts);
    d.flags = ctx->down.dev<uint8_t>(o.flags);
    d.keys = ctx->scratch.carve<unsigned>(8 * N);
    d.P3D = ctx->down.dev<float>(o.P3D);
    d.tri = ctx->down.dev<uint8_t>(o.tri);
    d.inl_H = ctx->down.dev<uint8_t>(o.inlH);
    d.inl_F = ctx->down.dev<uint8_t>(o.inlF);
    d.rec = ctx->down.dev<InitReconRec>(o.rec);
  };
  const int e = ransac_run<InitProb>(
      ctx, hyps, up_bytes, down_bytes, key_count * 4 + 256 * (size_t)n_problems + 256, total, &ctx->ms_initializer, &ctx->ms_initializer_hyp,
      S->hyp, pack,
      [&](unsigned grid, const InitProb* probs, const int32_t* map, InitHypRec* recs) {
        hipLaunchKernelGGL(k_init_hyp, dim3(grid), dim3(kInitThreads), 0, st, probs, map, recs);
      },
      [&](unsigned grid, const InitProb* probs, const InitHypRec* recs) {
        hipLaunchKernelGGL(k_init_reconstruct, dim3(grid), dim3(kInitThreads), 0, st, probs, recs);
      });
  if (e != ASD_OK) return e;
  const std::vector<InitHypRec>& recs = S->hyp.recs;
  S->probs.resize(n_problems);
  for (int32_t j = 0; j < n_problems; ++j) {
    asd_initializer_problem& q = p[j];
    const Offs& o = offs[j];
    const size_t N = (size_t)Ns[j], first = (size_t)S->hyp.first[j];
    InitProbState& ps = S->probs[j];
    ps.N = Ns[j]; ps.words = (int32_t)((N + 63) / 64);
    ps.rec = *ctx->down.host<InitReconRec>(o.rec);
    const unsigned long long* mk = ctx->down.host<unsigned long long>(o.masks);
    ps.masks.assign(mk, mk + 2 * (size_t)q.n_iter * ps.words);
    const float* pts = ctx->down.host<float>(o.pts);
    ps.pts.assign(pts, pts + 8 * N * 3);
    const uint8_t* fl = ctx->down.host<uint8_t>(o.flags);
    ps.flags.assign(fl, fl + 8 * N);
    const InitReconRec& r = ps.rec;
    q.n_matches = Ns[j];
    q.SH = r.SH; q.SF = r.SF; q.model = r.model; q.ok = r.ok;
    if (r.best_H >= 0) memcpy(q.H21, recs[first + 2 * r.best_H].M1, 36);       // :166
    if (r.best_F >= 0) memcpy(q.F21, recs[first + 2 * r.best_F + 1].M1, 36);   // :217
    memcpy(q.inliers_H, ctx->down.host<uint8_t>(o.inlH), N);
    memcpy(q.inliers_F, ctx->down.host<uint8_t>(o.inlF), N);
    if (r.ok) {
      memcpy(q.R21, r.R21, 36);
      memcpy(q.t21, r.t21, 12);
      memcpy(q.P3D, ctx->down.host<float>(o.P3D), (size_t)q.n1 * 12);
      memcpy(q.triangulated, ctx->down.host<uint8_t>(o.tri), (size_t)q.n1);
    }
  }
  return ASD_OK;
}

int32_t asd_debug_initialize(const asd_ctx* ctx, int32_t problem, int32_t which, asd_initializer_debug* out) {
  if (!ctx || !out) return ASD_ERR_INVALID;
  const InitState* S = static_cast<const InitState*>(ctx->initializer);
  if (!S || problem < 0 || problem >= (int32_t)S->probs.size()) return ASD_ERR_INVALID;
  const InitProbState& ps = S->probs[problem];
  const InitReconRec& rr = ps.rec;
  if (which >= 0) {
    if (which >= S->hyp.count[problem]) return ASD_ERR_INVALID;
    const InitHypRec& r = S->hyp.recs[(size_t)S->hyp.first[problem] + which];
    memcpy(out->idx, r.idx, sizeof out->idx);
    memcpy(out->nullv, r.nullv, sizeof out->nullv);
    memcpy(out->U, r.U, sizeof out->U);
    memcpy(out->w, r.w, sizeof out->w);
    memcpy(out->Vt, r.Vt, sizeof out->Vt);
    memcpy(out->M1, r.M1, sizeof out->M1);
    memcpy(out->M2, r.M2, sizeof out->M2);
    out->score = r.score;
    if (out->mask) {
      const unsigned long long* m = ps.masks.data() + (size_t)which * ps.words;
      for (int32_t i = 0; i < ps.N; ++i) out->mask[i] = ransac_mask_bit(m, i);
    }
  } else {
    const int32_t h = -2 - which;
    if (which < -1 && h >= rr.n_hyp) return ASD_ERR_INVALID;
    memcpy(out->U, rr.U, sizeof out->U);
    memcpy(out->w, rr.w, sizeof out->w);
    memcpy(out->Vt, rr.Vt, sizeof out->Vt);
    memcpy(out->R, rr.R, sizeof out->R);
    memcpy(out->t, rr.t, sizeof out->t);
    memcpy(out->parallax, rr.parallax, sizeof out->parallax);
    memcpy(out->cos_sel, rr.cos_sel, sizeof out->cos_sel);
    memcpy(out->n_good, rr.n_good, sizeof out->n_good);
    if (which < -1) {
      if (out->points) memcpy(out->points, ps.pts.data() + (size_t)h * ps.N * 3, (size_t)ps.N * 12);
      if (out->flags) memcpy(out->flags, ps.flags.data() + (size_t)h * ps.N, (size_t)ps.N);
    }
  }
  out->best_H = rr.best_H; out->best_F = rr.best_F; out->n_inliers = rr.n_inliers; out->n_hyp = rr.n_hyp; out->winner = rr.winner;
  out->second_good = rr.second_good;
  return ASD_OK;
}

}  // extern "C"
