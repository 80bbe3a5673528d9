// normal_depth.h -- the arithmetic of MapPoint::UpdateNormalAndDepth (reference src/vslam/src/MapPoint.cc:384-405) as the library states it
// (include/asd_slam.h, "MapPoint::UpdateNormalAndDepth over the tables"), once, for the kernel of localmap.hip and for
// asd_normal_and_depth_point of capi.cpp: the CPU tests of the host function pin the device's rule.  Both units are built with
// -ffp-contract=off; the only products are formed in f64 from f32 factors and are exact, so contraction could not change them anyway.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define ASD_ND_FN __host__ __device__ inline
#else
#define ASD_ND_FN inline
#endif

// one observer: unit = (Pos - Ow) / |Pos - Ow| (:390-391); returns |Pos - Ow| in f64 (cv::norm)
ASD_ND_FN double asd_nd_unit(const float* Pos, const float* Ow, float unit[3]) {
  const float dx = Pos[0] - Ow[0], dy = Pos[1] - Ow[1], dz = Pos[2] - Ow[2];
  const double nrm = sqrt(((double)dx * (double)dx + (double)dy * (double)dy) + (double)dz * (double)dz);
  const double inv = 1.0 / nrm;
  unit[0] = (float)((double)dx * inv);
  unit[1] = (float)((double)dy * inv);
  unit[2] = (float)((double)dz * inv);
  return nrm;
}
// normal = normal + unit (:391), f32, one observer after the other
ASD_ND_FN void asd_nd_add(float sum[3], const float unit[3]) {
  sum[0] = sum[0] + unit[0];
  sum[1] = sum[1] + unit[1];
  sum[2] = sum[2] + unit[2];
}
// mNormalVector = normal / n, mfMaxDistance, mfMinDistance (:395-405); nrm_ref = |Pos - Ow| of the reference keyframe.  The division is
// formed in f64 and rounded once: correctly rounded for f32 operands, whatever the build does to an f32 division
ASD_ND_FN void asd_nd_finish(const float sum[3], int n_obs, double nrm_ref, float scale_level, float scale_top, float normal[3], float* min_dist,
                             float* max_dist) {
  const double inv = 1.0 / (double)n_obs;
  normal[0] = (float)((double)sum[0] * inv);
  normal[1] = (float)((double)sum[1] * inv);
  normal[2] = (float)((double)sum[2] * inv);
  const float dist = (float)nrm_ref;
  const float mx = dist * scale_level;
  *max_dist = mx;
  *min_dist = (float)((double)mx / (double)scale_top);
}
