// undistort.hip -- cv::undistort in front of the extractor (Tracking::GrabImageMonocular / Tracking::Loc, Tracking.cc:104,125).
//
// The reference undistorts every image before its Frame is built: cv::undistort(im, mImGray, mK, mDistCoef) with
// newCameraMatrix empty, then Frame gets distCoefZero (Frame::UndistortKeyPoints is the identity).  OpenCV 3.2.0's
// undistort is initUndistortRectifyMap into a CV_16SC2 + CV_16UC1 map pair, stripe by stripe, then remap with INTER_LINEAR and
// BORDER_CONSTANT 0.  The map is built once on the host (asd_undistort_map, below: the CPU tests pin it) and kept in HBM;
// k_undistort is the remap, integer-exact, and writes level 0 of the pyramid in place of k_copy_image.
//
// What decides bits (recalled from OpenCV 3.2.0 undistort.cpp / imgwarp.cpp / lapack.cpp; tests/undistort_ref.py restates it):
//  * mK and mDistCoef are CV_32F (Tracking.cc:59-72): the coefficients are the float values widened to double; four are given,
//    so k3..k6, s1..s4 and tau are 0 (no tilt: computeTiltProjectionMatrix(0, 0) is the identity and invProj = 1);
//  * undistort builds the map in stripes of min(max(1, 4096 / cols), rows) rows and sets Ar(1,2) = cy - y0 for each stripe:
//    every stripe's row terms start from their own double;
//  * iR = Ar.inv() (R = I) is cv::invert's closed-form 3x3 path for doubles (det3 and the cofactors times 1/det), not an
//    elimination: ir[0] = fy * (1 / (fx * fy)), and ir[8] = (fx * fy) * (1 / (fx * fy)), which need not be 1;
//  * along a row _x, _y and _w are accumulated one column at a time (_x += ir[0]);
//  * kr = 1 + ((k3 r2 + k2) r2 + k1) r2 (its divisor 1 + ((k6 r2 + k5) r2 + k4) r2 is exactly 1), u = fx xd + u0, v = fy yd + v0;
//  * iu = saturate_cast<int>(u * 32) = cvRound: half to even (cvtsd2si), INT_MIN where the value does not fit;
//    map1 = (short)(iu >> 5, iv >> 5), map2 = (iv & 31) * 32 + (iu & 31);
//  * remap's fixed-point weights for fractions a = iu & 31, b = iv & 31 are (32-a)(32-b)*32, a(32-b)*32, (32-a)b*32, ab*32 (they
//    sum to 2^15) and the result is (sum w p + 2^14) >> 15.  At a = b = 0 OpenCV's table saturates the first weight to 32767
//    (saturate_cast<short>(32768.f)) and may add the missing 1 to a neighbour's weight 0: (32767 p + q + 2^14) >> 15 = p for all
//    bytes p, q, exactly what 32768 gives -- the source pixel;
//  * a neighbour outside the image contributes the border value 0; a pixel whose whole 2x2 neighbourhood is outside is 0.
// The host code of this file is compiled with -ffp-contract=off (Makefile): no FMA changes a rounding of the map.
#include <algorithm>
#include <cmath>
#include <climits>
#include <vector>

#include "ctx.h"

namespace {

// saturate_cast<int>(double) of OpenCV 3.2 on x86-64: cvRound = cvtsd2si under the default rounding mode (half to even), which
// returns INT_MIN (the "integer indefinite" value) for NaN and for values outside the int range
inline int cv_round_sat(double v) {
  const double r = std::nearbyint(v);
  if (!(r >= (double)INT_MIN && r <= (double)INT_MAX)) return INT_MIN;
  return (int)r;
}

// cv::invert, DECOMP_LU, 3x3 CV_64F: the closed form of lapack.cpp (det3, cofactors, one reciprocal)
bool invert3(const double S[3][3], double t[9]) {
  double d = S[0][0] * (S[1][1] * S[2][2] - S[1][2] * S[2][1]) - S[0][1] * (S[1][0] * S[2][2] - S[1][2] * S[2][0]) +
             S[0][2] * (S[1][0] * S[2][1] - S[1][1] * S[2][0]);
  if (d == 0.) return false;
  d = 1. / d;
  t[0] = (S[1][1] * S[2][2] - S[1][2] * S[2][1]) * d;
  t[1] = (S[0][2] * S[2][1] - S[0][1] * S[2][2]) * d;
  t[2] = (S[0][1] * S[1][2] - S[0][2] * S[1][1]) * d;
  t[3] = (S[1][2] * S[2][0] - S[1][0] * S[2][2]) * d;
  t[4] = (S[0][0] * S[2][2] - S[0][2] * S[2][0]) * d;
  t[5] = (S[0][2] * S[1][0] - S[0][0] * S[1][2]) * d;
  t[6] = (S[1][0] * S[2][1] - S[1][1] * S[2][0]) * d;
  t[7] = (S[0][1] * S[2][0] - S[0][0] * S[2][1]) * d;
  t[8] = (S[0][0] * S[1][1] - S[0][1] * S[1][0]) * d;
  return true;
}

// remap (imgwarp.cpp remapBilinear, FixedPtCast<int, uchar, 15>) on the map pair, four output pixels of a row per thread and
// one dword store into the pitched destination (pitch % 64 == 0), like k_copy_image.  The map is stored pitched (mpitch % 4 == 0
// pixels): a thread reads its four (x, y) pairs as one 16-B load and its four fractions as one 8-B load.  src is DEVICE memory
// (the caller stages host images first): the four neighbours are byte gathers.
__global__ __launch_bounds__(256) void k_undistort(const uint8_t* __restrict__ src, int stride, int width, int height,
                                                   const short2* __restrict__ xy, const uint16_t* __restrict__ frac, int mpitch,
                                                   uint8_t* __restrict__ dst, int pitch) {
  const int x4 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x4 >= width || y >= height) return;
  const size_t m = (size_t)y * mpitch + x4;
  const int4 q = *reinterpret_cast<const int4*>(xy + m);
  const uint2 f = *reinterpret_cast<const uint2*>(frac + m);
  const int qs[4] = {q.x, q.y, q.z, q.w};
  const unsigned fs[4] = {f.x & 0xffffu, f.x >> 16, f.y & 0xffffu, f.y >> 16};
  uint32_t packed = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (x4 + k >= width) break;   // (bytes beyond `width` inside the pitch are never read as image)
    const int sx = (int)(short)(qs[k] & 0xffff), sy = qs[k] >> 16;   // short2 (x, y): x in the low half
    const int a = (int)(fs[k] & 31u), b = (int)((fs[k] >> 5) & 31u);
    const bool x0 = (unsigned)sx < (unsigned)width, x1 = (unsigned)(sx + 1) < (unsigned)width;
    const bool y0 = (unsigned)sy < (unsigned)height, y1 = (unsigned)(sy + 1) < (unsigned)height;
    const uint8_t* r0 = src + (ptrdiff_t)sy * stride;   // (dereferenced only where the row is inside)
    const uint8_t* r1 = r0 + stride;
    const int p00 = (y0 && x0) ? r0[sx] : 0, p10 = (y0 && x1) ? r0[sx + 1] : 0;
    const int p01 = (y1 && x0) ? r1[sx] : 0, p11 = (y1 && x1) ? r1[sx + 1] : 0;
    const int s = ((32 - a) * (32 - b) * 32) * p00 + (a * (32 - b) * 32) * p10 + ((32 - a) * b * 32) * p01 + (a * b * 32) * p11;
    packed |= (uint32_t)(((s + (1 << 14)) >> 15) & 255) << (8 * k);
  }
  *reinterpret_cast<uint32_t*>(dst + (size_t)y * pitch + x4) = packed;
}

}  // namespace

int undistort_launch(asd_ctx* ctx, const UndistortMap& U, hipStream_t st, const uint8_t* src, int stride, uint8_t* dst, int pitch) {
  hipLaunchKernelGGL(k_undistort, dim3((U.w + 255) / 256, (U.h + 3) / 4), dim3(256), 0, st, src, stride, U.w, U.h, U.d_xy, U.d_frac,
                     U.mpitch, dst, pitch);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  return ASD_OK;
}

void undistort_free(asd_ctx* ctx) {
  UndistortMap* U = ctx->und;
  if (!U) return;
  for (void* p : {(void*)U->d_xy, (void*)U->d_frac, (void*)U->d_io}) if (p) (void)hipFree(p);
  delete U;
  ctx->und = nullptr;
}

extern "C" {

int asd_undistort_map(const float K[4], const float dist[4], int32_t width, int32_t height, int16_t* xy, uint16_t* frac) {
  if (!K || !xy || !frac || width <= 0 || height <= 0) return ASD_ERR_INVALID;
  // A = mK and the coefficients as the CV_32F matrices hold them, widened to double (undistort's convertTo / Mat_<double>)
  const double fx = K[0], fy = K[1], u0 = K[2], v0 = K[3];
  const double k1 = dist ? dist[0] : 0., k2 = dist ? dist[1] : 0., p1 = dist ? dist[2] : 0., p2 = dist ? dist[3] : 0.;
  const double k3 = 0.;
  const int stripe0 = std::min(std::max(1, 4096 / width), height);
  for (int ys = 0; ys < height; ys += stripe0) {
    const int rows = std::min(stripe0, height - ys);
    const double Ar[3][3] = {{fx, 0., u0}, {0., fy, v0 - ys}, {0., 0., 1.}};   // Ar * R with R = I is Ar exactly
    double ir[9];
    if (!invert3(Ar, ir)) return ASD_ERR_INVALID;
    for (int i = 0; i < rows; ++i) {
      int16_t* m1 = xy + ((size_t)(ys + i) * width) * 2;
      uint16_t* m2 = frac + (size_t)(ys + i) * width;
      double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
      for (int j = 0; j < width; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
        const double w = 1. / _w, x = _x * w, y = _y * w;
        const double x2 = x * x, y2 = y * y;
        const double r2 = x2 + y2, _2xy = 2 * x * y;
        const double kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2;
        const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2);
        const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
        const double u = fx * xd + u0, v = fy * yd + v0;
        const int iu = cv_round_sat(u * 32), iv = cv_round_sat(v * 32);
        m1[j * 2] = (int16_t)(iu >> 5);
        m1[j * 2 + 1] = (int16_t)(iv >> 5);
        m2[j] = (uint16_t)((iv & 31) * 32 + (iu & 31));
      }
    }
  }
  return ASD_OK;
}

int asd_set_undistortion(asd_ctx* ctx, const float K[4], const float dist[4], int32_t width, int32_t height) {
  if (!ctx) return ASD_ERR_INVALID;
  if (asd_extractor_busy(ctx, "asd_set_undistortion")) return ASD_ERR_INVALID;
  const bool none = !dist || (dist[0] == 0.f && dist[1] == 0.f && dist[2] == 0.f && dist[3] == 0.f);
  (void)hipSetDevice(ctx->cfg.device);
  if (none) { undistort_free(ctx); return ASD_OK; }   // no map, no extra launch: k_copy_image as without distortion
  if (!K || width <= 0 || height <= 0) { ctx->set_error("asd_set_undistortion: K and a positive size are required"); return ASD_ERR_INVALID; }
  if (width > ctx->cfg.max_width || height > ctx->cfg.max_height) {
    ctx->set_error("asd_set_undistortion: image %dx%d exceeds ctx capacity %dx%d", width, height, ctx->cfg.max_width, ctx->cfg.max_height);
    return ASD_ERR_CAPACITY;
  }
  std::vector<int16_t> m1((size_t)width * height * 2);
  std::vector<uint16_t> m2((size_t)width * height);
  if (asd_undistort_map(K, dist, width, height, m1.data(), m2.data()) != ASD_OK) {
    ctx->set_error("asd_set_undistortion: singular camera matrix (fx = %g, fy = %g)", (double)K[0], (double)K[1]);
    return ASD_ERR_INVALID;
  }
  undistort_free(ctx);
  UndistortMap* U = new UndistortMap();
  ctx->und = U;
  U->w = width; U->h = height;
  U->mpitch = (width + 3) / 4 * 4;
  auto fail = [&](int rc) { undistort_free(ctx); return rc; };
  int rc;
  if ((rc = [&]() -> int {
        ASD_HIP_CHECK(ctx, hipMalloc(&U->d_xy, (size_t)U->mpitch * height * sizeof(short2)));
        ASD_HIP_CHECK(ctx, hipMalloc(&U->d_frac, (size_t)U->mpitch * height * sizeof(uint16_t)));
        ASD_HIP_CHECK(ctx, hipMemcpy2D(U->d_xy, (size_t)U->mpitch * sizeof(short2), m1.data(), (size_t)width * sizeof(short2),
                                       (size_t)width * sizeof(short2), height, hipMemcpyHostToDevice));
        ASD_HIP_CHECK(ctx, hipMemcpy2D(U->d_frac, (size_t)U->mpitch * sizeof(uint16_t), m2.data(), (size_t)width * sizeof(uint16_t),
                                       (size_t)width * sizeof(uint16_t), height, hipMemcpyHostToDevice));
        return ASD_OK;
      }()) != ASD_OK)
    return fail(rc);
  return ASD_OK;
}

int asd_undistort(asd_ctx* ctx, const uint8_t* src, int32_t device_resident, int32_t width, int32_t height, int32_t stride,
                  uint8_t* dst, int32_t dst_stride) {
  if (!ctx || !src || !dst || width <= 0 || height <= 0 || stride < width || dst_stride < width) return ASD_ERR_INVALID;
  UndistortMap* U = ctx->und;
  if (!U) { ctx->set_error("asd_undistort: no undistortion map is set (asd_set_undistortion)"); return ASD_ERR_INVALID; }
  if (width != U->w || height != U->h) {
    ctx->set_error("asd_undistort: image %dx%d, the undistortion map is %dx%d", width, height, U->w, U->h);
    return ASD_ERR_INVALID;
  }
  (void)hipSetDevice(ctx->cfg.device);
  const int pitch = (width + 63) / 64 * 64;
  if (!U->d_io) ASD_HIP_CHECK(ctx, hipMalloc(&U->d_io, (size_t)pitch * height * 2));   // input staging + output, this call's own
  uint8_t* d_in = U->d_io;
  uint8_t* d_out = U->d_io + (size_t)pitch * height;
  const uint8_t* s = src;
  int ss = stride;
  int rc;
  if (!device_resident) {
    if ((rc = frontend_image_to_device(ctx, src, false, width, height, stride, d_in, pitch, ctx->stream)) != ASD_OK) return rc;
    s = d_in; ss = pitch;
  }
  if ((rc = undistort_launch(ctx, *U, ctx->stream, s, ss, d_out, pitch)) != ASD_OK) return rc;
  ASD_HIP_CHECK(ctx, hipMemcpy2DAsync(dst, dst_stride, d_out, pitch, width, height, hipMemcpyDeviceToHost, ctx->stream));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return ASD_OK;
}

}  // extern "C"
