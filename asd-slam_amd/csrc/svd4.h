// svd4.h -- the 4x4 null vector of the linear triangulations, shared by mapping.hip (LocalMapping::CreateNewMapPoints) and
// initializer.hip (Initializer::Triangulate): both call cv::SVD::compute on the same kind of 4x4 f32 matrix and keep vt.row(3).
// The arithmetic is OpenCV 3.2.0's JacobiSVDImpl_ on f32 data with its f64 accumulators; compile with -ffp-contract=off.
#pragma once
#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
namespace {

__device__ __forceinline__ float scaled_minus(float alpha, float a, float b) {
  if (alpha == 1.0f) return a - b;  // MatOp_AddEx::assign: plain subtract when the scale is 1
  return (float)((double)a * (double)alpha + (double)b * -1.0 + 0.0);
}

// One-sided Jacobi on the rows of At (= columns of A), rotations accumulated in Vt; returns the row of Vt
// belonging to the smallest singular value.  Registers only: every index is a compile-time constant.
struct Row4 { float v[4]; };

__device__ __forceinline__ void rot_pair(Row4& Ai, Row4& Aj, Row4& Vi, Row4& Vj, double& Wi, double& Wj, bool& changed) {
  const float eps = FLT_EPSILON * 2;
  double a = Wi, p = 0, b = Wj;
#pragma unroll
  for (int k = 0; k < 4; ++k) p += (double)Ai.v[k] * Aj.v[k];
  if (fabs(p) <= eps * sqrt(a * b)) return;
  p *= 2;
  const double beta = a - b, gamma = hypot(p, beta);
  float c, s;
  if (beta < 0) {
    const double delta = (gamma - beta) * 0.5;
    s = (float)sqrt(delta / gamma);
    c = (float)(p / (gamma * s * 2));
  } else {
    c = (float)sqrt((gamma + beta) / (gamma * 2));
    s = (float)(p / (gamma * c * 2));
  }
  a = b = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float t0 = c * Ai.v[k] + s * Aj.v[k];
    const float t1 = -s * Ai.v[k] + c * Aj.v[k];
    Ai.v[k] = t0; Aj.v[k] = t1;
    a += (double)t0 * t0; b += (double)t1 * t1;
  }
  Wi = a; Wj = b;
  changed = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float t0 = c * Vi.v[k] + s * Vj.v[k];
    const float t1 = -s * Vi.v[k] + c * Vj.v[k];
    Vi.v[k] = t0; Vj.v[k] = t1;
  }
}

__device__ __forceinline__ double rownorm2(const Row4& r) {
  double sd = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) sd += (double)r.v[k] * r.v[k];
  return sd;
}

__device__ inline Row4 svd4_last_vt(Row4 A0, Row4 A1, Row4 A2, Row4 A3) {
  Row4 V0{{1, 0, 0, 0}}, V1{{0, 1, 0, 0}}, V2{{0, 0, 1, 0}}, V3{{0, 0, 0, 1}};
  double W0 = rownorm2(A0), W1 = rownorm2(A1), W2 = rownorm2(A2), W3 = rownorm2(A3);
  for (int iter = 0; iter < 30; ++iter) {
    bool changed = false;
    rot_pair(A0, A1, V0, V1, W0, W1, changed);
    rot_pair(A0, A2, V0, V2, W0, W2, changed);
    rot_pair(A0, A3, V0, V3, W0, W3, changed);
    rot_pair(A1, A2, V1, V2, W1, W2, changed);
    rot_pair(A1, A3, V1, V3, W1, W3, changed);
    rot_pair(A2, A3, V2, V3, W2, W3, changed);
    if (!changed) break;
  }
  W0 = sqrt(rownorm2(A0)); W1 = sqrt(rownorm2(A1)); W2 = sqrt(rownorm2(A2)); W3 = sqrt(rownorm2(A3));
  // selection sort, descending, first maximum wins (lapack.cpp JacobiSVDImpl_): only the last slot is needed.
  // Replay it on (W, V) pairs.
#define ASD_SWAP_IF(Wa, Va, Wb, Vb) { const double tw = Wa; Wa = Wb; Wb = tw; const Row4 tv = Va; Va = Vb; Vb = tv; }
  {  // i = 0
    int j = 0; double wj = W0;
    if (wj < W1) { j = 1; wj = W1; }
    if (wj < W2) { j = 2; wj = W2; }
    if (wj < W3) { j = 3; wj = W3; }
    if (j == 1) ASD_SWAP_IF(W0, V0, W1, V1) else if (j == 2) ASD_SWAP_IF(W0, V0, W2, V2) else if (j == 3) ASD_SWAP_IF(W0, V0, W3, V3)
  }
  {  // i = 1
    int j = 1; double wj = W1;
    if (wj < W2) { j = 2; wj = W2; }
    if (wj < W3) { j = 3; wj = W3; }
    if (j == 2) ASD_SWAP_IF(W1, V1, W2, V2) else if (j == 3) ASD_SWAP_IF(W1, V1, W3, V3)
  }
  if (W2 < W3) ASD_SWAP_IF(W2, V2, W3, V3)
#undef ASD_SWAP_IF
  return V3;
}

}  // namespace
#endif
