// sim3_math.h -- g2o's Sim3 (reference src/g2o_catkin/include/g2o/types/sim3.h:41-296) and the two projection edges of
// Optimizer::OptimizeSim3 (types_seven_dof_expmap.h:152-193), fp64, host + device.  Every expression keeps the reference's order of
// operations with IEEE division and square root: OptimizeSim3 differentiates these functions numerically with delta = 1e-9, so their
// rounding IS the optimiser's noise floor (see sim3.hip).  sim3.o is built with -ffp-contract=off, like the reference's x86-64 build.
#pragma once
#include "se3.h"

struct Sim3d {  // quaternion (x,y,z,w) -- NOT renormalised, as in the reference --, translation, scale
  double qx, qy, qz, qw, tx, ty, tz, s;
};

// Eigen::Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other,3,3>), R row-major.
// kEigen: mat.trace() in Eigen's own order -- an unrolled reduction over three elements splits in halves, R00 + (R11 + R22) (see s3_mul)
template <bool kEigen = false>
ASD_HD void s3_quat_of_rot(const double R[9], double& x, double& y, double& z, double& w) {
  double t = kEigen ? R[0] + (R[4] + R[8]) : R[0] + R[4] + R[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    w = 0.5 * t;
    t = 0.5 / t;
    x = (R[7] - R[5]) * t; y = (R[2] - R[6]) * t; z = (R[3] - R[1]) * t;
  } else {   // largest diagonal element first; written out per case so that every index is static
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > (i == 0 ? R[0] : R[4])) i = 2;
    if (i == 0) {
      t = sqrt(R[0] - R[4] - R[8] + 1.0);
      x = 0.5 * t; t = 0.5 / t;
      w = (R[7] - R[5]) * t; y = (R[3] + R[1]) * t; z = (R[6] + R[2]) * t;
    } else if (i == 1) {
      t = sqrt(R[4] - R[8] - R[0] + 1.0);
      y = 0.5 * t; t = 0.5 / t;
      w = (R[2] - R[6]) * t; z = (R[7] + R[5]) * t; x = (R[1] + R[3]) * t;
    } else {
      t = sqrt(R[8] - R[0] - R[4] + 1.0);
      z = 0.5 * t; t = 0.5 / t;
      w = (R[3] - R[1]) * t; x = (R[2] + R[6]) * t; y = (R[5] + R[7]) * t;
    }
  }
}

// Sim3(const Vector7d& update) (sim3.h:70-142): update = (omega, upsilon, sigma), with the eps = 1e-5 branches as written there.
// kEigen: the sums in the order the reference's Eigen takes them (see s3_mul): omega.norm() of a Vector3d is an unrolled, unvectorised
// reduction that splits in halves, x^2 + (y^2 + z^2)
template <bool kEigen = false>
ASD_HD Sim3d s3_exp(const double u[7]) {
  const double wx = u[0], wy = u[1], wz = u[2], sigma = u[6];
  const double theta = kEigen ? sqrt(wx * wx + (wy * wy + wz * wz)) : sqrt(wx * wx + wy * wy + wz * wz);
  const double O[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
  double O2[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) O2[i * 3 + j] = O[i * 3] * O[j] + O[i * 3 + 1] * O[3 + j] + O[i * 3 + 2] * O[6 + j];
  Sim3d o;
  o.s = exp(sigma);
  const double eps = 0.00001;
  double A, B, Cc, ra, rb;   // R = I + ra Omega + rb Omega^2
  if (fabs(sigma) < eps) {
    Cc = 1;
    if (theta < eps) {
      A = 1. / 2.; B = 1. / 6.;
      ra = 1; rb = 1;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cos(theta)) / (theta2);
      B = (theta - sin(theta)) / (theta2 * theta);
      ra = sin(theta) / theta; rb = (1 - cos(theta)) / (theta * theta);
    }
  } else {
    Cc = (o.s - 1) / sigma;
    if (theta < eps) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * o.s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * o.s) / (sigma2 * sigma);
      ra = 1; rb = 1;
    } else {
      ra = sin(theta) / theta; rb = (1 - cos(theta)) / (theta * theta);
      const double a = o.s * sin(theta);
      const double b = o.s * cos(theta);
      const double theta2 = theta * theta;
      const double sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (Cc - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  double R[9], W[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const double I = (i % 4 == 0) ? 1.0 : 0.0;
    R[i] = (theta < eps) ? (I + O[i]) + O2[i] : (I + ra * O[i]) + rb * O2[i];
    W[i] = (A * O[i] + B * O2[i]) + Cc * I;
  }
  s3_quat_of_rot<kEigen>(R, o.qx, o.qy, o.qz, o.qw);
  o.tx = W[0] * u[3] + W[1] * u[4] + W[2] * u[5];
  o.ty = W[3] * u[3] + W[4] * u[4] + W[5] * u[5];
  o.tz = W[6] * u[3] + W[7] * u[4] + W[8] * u[5];
  return o;
}

// Sim3::operator* (sim3.h:270-276): r = a.r * b.r (Eigen's quaternion product), t = a.s * (a.r * b.t) + a.t, s = a.s * b.s.
// kEigen: the quaternion product with the association of Eigen's SSE2 kernel for doubles (Geometry_SSE.h:60-109), which is what the
// reference's x86-64 build runs -- the same eight products, paired differently.  The essential graph differentiates through this
// product with delta = 1e-9 and then compares chi2 of rejected trials to 1e-7: there the pairing shows (essgraph.hip).
// OptimizeSim3 (sim3.hip) keeps the plain form it was pinned with.
template <bool kEigen = false>
ASD_HD Sim3d s3_mul(const Sim3d& a, const Sim3d& b) {
  Sim3d o;
  if (kEigen) {
    o.qx = (a.qw * b.qx + a.qy * b.qz) - (a.qz * b.qy - a.qx * b.qw);
    o.qy = (a.qw * b.qy + a.qy * b.qw) + (a.qz * b.qx - a.qx * b.qz);
    o.qz = (a.qw * b.qz - a.qy * b.qx) + (a.qz * b.qw + a.qx * b.qy);
    o.qw = (a.qw * b.qw - a.qy * b.qy) - (a.qz * b.qz + a.qx * b.qx);
  } else {
    o.qw = a.qw * b.qw - a.qx * b.qx - a.qy * b.qy - a.qz * b.qz;
    o.qx = a.qw * b.qx + a.qx * b.qw + a.qy * b.qz - a.qz * b.qy;
    o.qy = a.qw * b.qy + a.qy * b.qw + a.qz * b.qx - a.qx * b.qz;
    o.qz = a.qw * b.qz + a.qz * b.qw + a.qx * b.qy - a.qy * b.qx;
  }
  const double bt[3] = {b.tx, b.ty, b.tz};
  double r[3];
  quat_rotate(a.qx, a.qy, a.qz, a.qw, bt, r);
  o.tx = a.s * r[0] + a.tx; o.ty = a.s * r[1] + a.ty; o.tz = a.s * r[2] + a.tz;
  o.s = a.s * b.s;
  return o;
}

// Sim3::inverse (sim3.h:237-240)
ASD_HD Sim3d s3_inverse(const Sim3d& a) {
  Sim3d o;
  o.qx = -a.qx; o.qy = -a.qy; o.qz = -a.qz; o.qw = a.qw;
  const double k = -1. / a.s;
  const double v[3] = {k * a.tx, k * a.ty, k * a.tz};
  double r[3];
  quat_rotate(o.qx, o.qy, o.qz, o.qw, v, r);
  o.tx = r[0]; o.ty = r[1]; o.tz = r[2];
  o.s = 1. / a.s;
  return o;
}

// Sim3::map (sim3.h:144-146): s * (r * xyz) + t
ASD_HD void s3_map(const Sim3d& S, const double v[3], double out[3]) {
  double r[3];
  quat_rotate(S.qx, S.qy, S.qz, S.qw, v, r);
  out[0] = S.s * r[0] + S.tx; out[1] = S.s * r[1] + S.ty; out[2] = S.s * r[2] + S.tz;
}

// Eigen::Quaterniond::toRotationMatrix (the quaternion as it is, not renormalised), R row-major
ASD_HD void s3_rot_of_quat(const Sim3d& S, double R[9]) {
  const double tx = 2 * S.qx, ty = 2 * S.qy, tz = 2 * S.qz;
  const double twx = tx * S.qw, twy = ty * S.qw, twz = tz * S.qw;
  const double txx = tx * S.qx, txy = ty * S.qx, txz = tz * S.qx, tyy = ty * S.qy, tyz = tz * S.qy, tzz = tz * S.qz;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

// W.lu().solve(t) for a 3x3 W (Eigen's PartialPivLU, unblocked: the largest |entry| of the column at or below the diagonal is the
// pivot, the first one on a tie), W row-major.  Written with static indices only: rows are swapped by value.  As Eigen 3.2.10 does it:
// `col /= pivot` is a true division (scalar_quotient_op), and the unrolled triangular solves subtract the SUM of a row's products
// (triangular_solver_unroller), where a hand-written substitution would subtract them one by one.
ASD_HD void s3_lu_solve3(const double W[9], const double t[3], double x[3]) {
  double a0[3] = {W[0], W[1], W[2]}, a1[3] = {W[3], W[4], W[5]}, a2[3] = {W[6], W[7], W[8]};
  double b0 = t[0], b1 = t[1], b2 = t[2];
#define S3_SWAP_ROWS(p, q, bp, bq) do { for (int c_ = 0; c_ < 3; ++c_) { const double h_ = p[c_]; p[c_] = q[c_]; q[c_] = h_; } const double g_ = bp; bp = bq; bq = g_; } while (0)
  {
    int piv = 0;
    double big = fabs(a0[0]);
    if (fabs(a1[0]) > big) { big = fabs(a1[0]); piv = 1; }
    if (fabs(a2[0]) > big) { piv = 2; }
    if (piv == 1) S3_SWAP_ROWS(a0, a1, b0, b1);
    if (piv == 2) S3_SWAP_ROWS(a0, a2, b0, b2);
  }
  a1[0] /= a0[0]; a2[0] /= a0[0];
  a1[1] -= a1[0] * a0[1]; a1[2] -= a1[0] * a0[2];
  a2[1] -= a2[0] * a0[1]; a2[2] -= a2[0] * a0[2];
  if (fabs(a2[1]) > fabs(a1[1])) S3_SWAP_ROWS(a1, a2, b1, b2);
#undef S3_SWAP_ROWS
  a2[1] /= a1[1];
  a2[2] -= a2[1] * a1[2];
  // L y = P b (unit lower), U x = y
  const double y0 = b0;
  const double y1 = b1 - a1[0] * y0;
  const double y2 = b2 - (a2[0] * y0 + a2[1] * y1);
  x[2] = y2 / a2[2];
  x[1] = (y1 - a1[2] * x[2]) / a1[1];
  x[0] = (y0 - (a0[1] * x[1] + a0[2] * x[2])) / a0[0];
}

// Sim3::log (sim3.h:152-234), with the eps = 1e-5 branches as written there: res = (omega, upsilon, sigma)
ASD_HD void s3_log(const Sim3d& S, double res[7]) {
  const double sigma = log(S.s);
  double R[9];
  s3_rot_of_quat(S, R);
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};   // deltaR (se3_ops.hpp)
  const double eps = 0.00001;
  double A, B, Cc, k;
  if (fabs(sigma) < eps) {
    Cc = 1;
    if (d > 1 - eps) {
      k = 0.5; A = 1. / 2.; B = 1. / 6.;
    } else {
      const double theta = acos(d);
      const double theta2 = theta * theta;
      k = theta / (2 * sqrt(1 - d * d));
      A = (1 - cos(theta)) / (theta2);
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    Cc = (S.s - 1) / sigma;
    if (d > 1 - eps) {
      const double sigma2 = sigma * sigma;
      k = 0.5;
      A = ((sigma - 1) * S.s + 1) / (sigma2);
      B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
    } else {
      const double theta = acos(d);
      k = theta / (2 * sqrt(1 - d * d));
      const double theta2 = theta * theta;
      const double a = S.s * sin(theta);
      const double b = S.s * cos(theta);
      const double c = theta2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (Cc - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  const double wx = k * dR[0], wy = k * dR[1], wz = k * dR[2];
  const double O[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
  double W[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      // B * Omega * Omega is (B * Omega) * Omega in the reference's expression
      const double bo2 = (B * O[i * 3]) * O[j] + (B * O[i * 3 + 1]) * O[3 + j] + (B * O[i * 3 + 2]) * O[6 + j];
      W[i * 3 + j] = (A * O[i * 3 + j] + bo2) + Cc * (i == j ? 1.0 : 0.0);
    }
  const double t[3] = {S.tx, S.ty, S.tz};
  double ups[3];
  s3_lu_solve3(W, t, ups);
  res[0] = wx; res[1] = wy; res[2] = wz; res[3] = ups[0]; res[4] = ups[1]; res[5] = ups[2]; res[6] = sigma;
}

// EdgeSim3::computeError (types_seven_dof_expmap.h:106-114): log(C * S_i * S_j^-1)
ASD_HD void s3_edge_error(const Sim3d& C, const Sim3d& Si, const Sim3d& Sj, double e[7]) {
  s3_log(s3_mul<true>(s3_mul<true>(C, Si), s3_inverse(Sj)), e);
}

// VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69)
template <bool kEigen = false>
ASD_HD Sim3d s3_oplus(const Sim3d& est, const double u[7], bool fix_scale) {
  double v[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) v[k] = u[k];
  if (fix_scale) v[6] = 0;
  return s3_mul<kEigen>(s3_exp<kEigen>(v), est);
}

// obs - cam_map(project(S.map(X))): the error of EdgeSim3ProjectXYZ with (S, X = P2c, K1, obs1) and of EdgeInverseSim3ProjectXYZ with
// (S.inverse(), X = P1c, K2, obs2) (types_seven_dof_expmap.h:160-167, :182-189)
ASD_HD void s3_project_error(const Sim3d& S, double X, double Y, double Z, double ou, double ov, double fx, double fy, double cx, double cy,
                             double& e0, double& e1) {
  const double v[3] = {X, Y, Z};
  double r[3];
  quat_rotate(S.qx, S.qy, S.qz, S.qw, v, r);
  const double x = S.s * r[0] + S.tx, y = S.s * r[1] + S.ty, z = S.s * r[2] + S.tz;
  e0 = ou - ((x / z) * fx + cx);
  e1 = ov - ((y / z) * fy + cy);
}

// BaseEdge::chi2() with information = inv_sigma2 * I: e . (Omega e)
ASD_HD double s3_chi2(double e0, double e1, double isg) { return e0 * (isg * e0) + e1 * (isg * e1); }

// Dense solve of the 7x7 system (H + lambda I) x = b, H symmetric (upper triangle read), by Cholesky; false where a pivot is not
// positive.  Fully unrolled: every index is static.
// NOT the reference's factorisation: g2o's LinearSolverDense takes Eigen's pivoted LDL^T (linear_solver_dense.h) and fails where
// that is not positive; L L^T without pivoting gives the same x up to rounding (far inside the optimiser's noise floor) and fails on
// the same matrices up to rounding.  On a failed solve g2o still applies the x of the previous solve before it rejects the trial
// (levenberg.cpp:110-127: update() is not guarded by ok2); sim3_next_trial applies nothing.  Either way the trial is rejected and
// the estimate popped, so the results agree; what differs is the estimate the stored errors of such a trial refer to.  No
// generator input makes the damped system fail (lambda >= 1e-5 max diag H keeps it positive definite).
ASD_HD bool s3_solve7(const double* H, double lambda, const double* b, double* x) {
  double L[28];   // row-major lower triangle: L[r (r + 1) / 2 + c]
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    double d = H[j * 7 + j] + lambda;
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
    if (!(d > 0)) ok = false;
    const double ljj = sqrt(d);
    L[j * (j + 1) / 2 + j] = ljj;
#pragma unroll
    for (int i = j + 1; i < 7; ++i) {
      double v = H[j * 7 + i];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
      L[i * (i + 1) / 2 + j] = v / ljj;
    }
  }
  double y[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    double v = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= L[i * (i + 1) / 2 + k] * y[k];
    y[i] = v / L[i * (i + 1) / 2 + i];
  }
#pragma unroll
  for (int i = 6; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < 7; ++k) v -= L[k * (k + 1) / 2 + i] * x[k];
    x[i] = v / L[i * (i + 1) / 2 + i];
  }
  return ok;
}
