// prim_debug.hip -- asd_debug_prim: ONE call of one fp64 primitive of se3.h / sim3_math.h per input item, on the device (one lane per
// item) or on the host (the same header functions through ASD_HD).  A test aid (tests/test_prims.py, tests/test_prims_ref.py): the
// optimisers show these functions only behind several Levenberg iterations.
//
// The headers are compiled under two flag sets in the library -- -ffp-contract=off (sim3.o, essgraph.o) and contraction allowed
// (ba.o, gba.o) -- so this file is compiled twice: as itself with the default flags (every op), and through prim_debug_fused.hip,
// which defines ASD_PRIM_FUSED, with the flags of ba.o (the se3.h ops only).
//
// What this instantiation does NOT show: inside the production kernels the same functions are inlined into other code, and where
// contraction is allowed the compiler may pair multiplies and adds differently there than here.  The tests therefore assert error
// bounds, and bits only where IEEE arithmetic without contraction fixes them (the contract-off unit).
#include "ctx.h"
#include "se3.h"
#ifndef ASD_PRIM_FUSED
#include "sim3_math.h"
#define PRIM_NS prim_plain
#else
#define PRIM_NS prim_fused
#endif

#include <vector>

// every name of this file lives in a namespace of its unit: the two units instantiate the same templates under different flags
namespace PRIM_NS {
namespace {

// doubles per item, by op (include/asd_slam.h, asd_debug_prim)
constexpr int kIn[ASD_PRIM_OPS] = {1, 4, 7, 10, 13, 9, 2, 5, 7, 7, 8, 16, 16, 8, 11, 16, 16, 9, 9, 8, 12, 24, 17, 3, 57};
constexpr int kOut[ASD_PRIM_OPS] = {1, 4, 3, 3, 7, 4, 2, 12, 8, 8, 7, 8, 8, 8, 3, 8, 8, 4, 4, 9, 3, 7, 2, 1, 8};
#ifndef ASD_PRIM_FUSED
constexpr int kOps = ASD_PRIM_OPS;
#else
constexpr int kOps = ASD_PRIM_SE3_OPS;
#endif

ASD_HD Pose7 load_pose(const double* x) { return Pose7{x[0], x[1], x[2], x[3], x[4], x[5], x[6]}; }
#ifndef ASD_PRIM_FUSED
ASD_HD Sim3d load_sim3(const double* x) { return Sim3d{x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]}; }
ASD_HD void store_sim3(const Sim3d& s, double* y) {
  y[0] = s.qx; y[1] = s.qy; y[2] = s.qz; y[3] = s.qw; y[4] = s.tx; y[5] = s.ty; y[6] = s.tz; y[7] = s.s;
}
#endif

template <int OP>
ASD_HD void prim_one(const double* x, double* y) {
  if constexpr (OP == ASD_PRIM_RSQRT) {
    y[0] = asd_rsqrt(x[0]);
  } else if constexpr (OP == ASD_PRIM_QUAT_NORMALIZE) {
    y[0] = x[0]; y[1] = x[1]; y[2] = x[2]; y[3] = x[3];
    quat_normalize(y[0], y[1], y[2], y[3]);
  } else if constexpr (OP == ASD_PRIM_QUAT_ROTATE) {
    quat_rotate(x[0], x[1], x[2], x[3], x + 4, y);
  } else if constexpr (OP == ASD_PRIM_POSE_MAP) {
    pose_map(load_pose(x), x + 7, y);
  } else if constexpr (OP == ASD_PRIM_POSE_OPLUS) {
    const Pose7 o = pose_oplus(load_pose(x), x + 7);
    y[0] = o.qx; y[1] = o.qy; y[2] = o.qz; y[3] = o.qw; y[4] = o.tx; y[5] = o.ty; y[6] = o.tz;
  } else if constexpr (OP == ASD_PRIM_ROT_TO_QUAT_EIGEN) {
    rot_to_quat_eigen(x, y[0], y[1], y[2], y[3]);
  } else if constexpr (OP == ASD_PRIM_HUBER) {
    huber(x[0], x[1], y[0], y[1]);
  } else if constexpr (OP == ASD_PRIM_JAC_POSE) {
    jac_pose(x[0], x[1], x[2], x[3], x[4], y);
  }
#ifndef ASD_PRIM_FUSED
  else if constexpr (OP == ASD_PRIM_S3_EXP) {
    store_sim3(s3_exp<false>(x), y);
  } else if constexpr (OP == ASD_PRIM_S3_EXP_EIGEN) {
    store_sim3(s3_exp<true>(x), y);
  } else if constexpr (OP == ASD_PRIM_S3_LOG) {
    s3_log(load_sim3(x), y);
  } else if constexpr (OP == ASD_PRIM_S3_MUL) {
    store_sim3(s3_mul<false>(load_sim3(x), load_sim3(x + 8)), y);
  } else if constexpr (OP == ASD_PRIM_S3_MUL_EIGEN) {
    store_sim3(s3_mul<true>(load_sim3(x), load_sim3(x + 8)), y);
  } else if constexpr (OP == ASD_PRIM_S3_INVERSE) {
    store_sim3(s3_inverse(load_sim3(x)), y);
  } else if constexpr (OP == ASD_PRIM_S3_MAP) {
    s3_map(load_sim3(x), x + 8, y);
  } else if constexpr (OP == ASD_PRIM_S3_OPLUS) {
    store_sim3(s3_oplus<false>(load_sim3(x), x + 8, x[15] != 0), y);
  } else if constexpr (OP == ASD_PRIM_S3_OPLUS_EIGEN) {
    store_sim3(s3_oplus<true>(load_sim3(x), x + 8, x[15] != 0), y);
  } else if constexpr (OP == ASD_PRIM_S3_QUAT_OF_ROT) {
    s3_quat_of_rot<false>(x, y[0], y[1], y[2], y[3]);
  } else if constexpr (OP == ASD_PRIM_S3_QUAT_OF_ROT_EIGEN) {
    s3_quat_of_rot<true>(x, y[0], y[1], y[2], y[3]);
  } else if constexpr (OP == ASD_PRIM_S3_ROT_OF_QUAT) {
    s3_rot_of_quat(load_sim3(x), y);
  } else if constexpr (OP == ASD_PRIM_S3_LU_SOLVE3) {
    s3_lu_solve3(x, x + 9, y);
  } else if constexpr (OP == ASD_PRIM_S3_EDGE_ERROR) {
    s3_edge_error(load_sim3(x), load_sim3(x + 8), load_sim3(x + 16), y);
  } else if constexpr (OP == ASD_PRIM_S3_PROJECT_ERROR) {
    s3_project_error(load_sim3(x), x[8], x[9], x[10], x[11], x[12], x[13], x[14], x[15], x[16], y[0], y[1]);
  } else if constexpr (OP == ASD_PRIM_S3_CHI2) {
    y[0] = s3_chi2(x[0], x[1], x[2]);
  } else if constexpr (OP == ASD_PRIM_S3_SOLVE7) {
    y[0] = s3_solve7(x, x[49], x + 50, y + 1) ? 1.0 : 0.0;
  }
#endif
}

// one lane per item; the item's doubles go through registers (static indices), as the production kernels hold them
template <int OP>
__global__ __launch_bounds__(64) void k_prim(int n, const double* __restrict__ in, double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double x[kIn[OP]], y[kOut[OP]];
#pragma unroll
  for (int k = 0; k < kIn[OP]; ++k) x[k] = in[(size_t)i * kIn[OP] + k];
  prim_one<OP>(x, y);
#pragma unroll
  for (int k = 0; k < kOut[OP]; ++k) out[(size_t)i * kOut[OP] + k] = y[k];
}

template <int OP>
void host_all(int n, const double* in, double* out) {
  for (int i = 0; i < n; ++i) prim_one<OP>(in + (size_t)i * kIn[OP], out + (size_t)i * kOut[OP]);
}

template <int OP>
void launch(hipStream_t st, int n, const double* d_in, double* d_out) {
  hipLaunchKernelGGL(k_prim<OP>, dim3((n + 63) / 64), dim3(64), 0, st, n, d_in, d_out);
}

template <int OP = 0>
void dispatch(int op, bool host, hipStream_t st, int n, const double* in, double* out) {
  if constexpr (OP < kOps) {
    if (op != OP) return dispatch<OP + 1>(op, host, st, n, in, out);
    if (host) host_all<OP>(n, in, out);
    else launch<OP>(st, n, in, out);
  }
}

}  // namespace

// arguments checked by asd_debug_prim; ctx is read on the device path only
int run(asd_ctx* ctx, int op, bool host, int n, const double* in, double* out) {
  if (op < 0 || op >= kOps) return ASD_ERR_INVALID;
  if (host) {
    dispatch(op, true, nullptr, n, in, out);
    return ASD_OK;
  }
  (void)hipSetDevice(ctx->cfg.device);
  hipStream_t st = ctx->stream;
  const size_t szi = AsdDevBuf::padded((size_t)n * kIn[op] * sizeof(double)), szo = AsdDevBuf::padded((size_t)n * kOut[op] * sizeof(double));
  char* dev = nullptr;
  ASD_HIP_CHECK(ctx, hipMalloc(&dev, szi + szo));
  double* d_in = reinterpret_cast<double*>(dev);
  double* d_out = reinterpret_cast<double*>(dev + szi);
  auto body = [&]() -> int {
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(d_in, in, (size_t)n * kIn[op] * sizeof(double), hipMemcpyHostToDevice, st));
    dispatch(op, false, st, n, d_in, d_out);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(out, d_out, (size_t)n * kOut[op] * sizeof(double), hipMemcpyDeviceToHost, st));
    ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return ASD_OK;
  };
  const int rc = body();
  if (rc != ASD_OK) (void)hipStreamSynchronize(st);
  (void)hipFree(dev);
  return rc;
}

}  // namespace PRIM_NS

#ifndef ASD_PRIM_FUSED
namespace prim_fused {
int run(asd_ctx* ctx, int op, bool host, int n, const double* in, double* out);   // prim_debug_fused.hip
}

int32_t asd_debug_prim(asd_ctx* ctx, int32_t op, int32_t flags, int32_t n, const double* in, double* out) {
  const bool host = (flags & ASD_PRIM_HOST) != 0, fused = (flags & ASD_PRIM_FUSED_BUILD) != 0;
  if (!ctx && !host) return ASD_ERR_INVALID;
  auto fail = [&](const char* what) {
    if (ctx) ctx->set_error("asd_debug_prim: %s (op %d, flags %d, n %d)", what, op, flags, n);
    return (int32_t)ASD_ERR_INVALID;
  };
  if (flags & ~(ASD_PRIM_HOST | ASD_PRIM_FUSED_BUILD)) return fail("unknown flag bits");
  if (op < 0 || op >= (fused ? ASD_PRIM_SE3_OPS : ASD_PRIM_OPS)) return fail(fused ? "the contracted unit holds the se3.h ops only" : "unknown op");
  if (n < 0) return fail("n is negative");
  if (!in || !out) return fail("null argument");
  if (n == 0) return ASD_OK;
  return fused ? prim_fused::run(ctx, op, host, n, in, out) : prim_plain::run(ctx, op, host, n, in, out);
}
#endif
