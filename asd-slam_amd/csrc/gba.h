// gba.h -- the map-scale dense solve of asd_bundle_adjustment (gba.hip), as ba.hip's entry point enqueues it
#pragma once
#include <hip/hip_runtime.h>

#include "ctx.h"

// a tile of the tiled Cholesky: 16 pose blocks = 96 rows = 6 x 16 MFMA rows; a pose block never straddles a tile
constexpr int kGbaTilePoses = 16;
constexpr int kGbaTile = 6 * kGbaTilePoses;
inline int gba_tile_count(int n_free_poses) { return (n_free_poses + kGbaTilePoses - 1) / kGbaTilePoses; }

// A (n x n, row-major, n = 6 nPf) <- 0, unless *done
int gba_clear_enqueue(asd_ctx* ctx, hipStream_t st, double* A, int n, const int* done);
// Cholesky of A (the lower triangle is read and overwritten by L; the strict upper triangle outside the diagonal tiles is not
// touched) and x = A^-1 b, unless *done.  *chol_ok <- 1, or 0 when a pivot was not positive (x is then meaningless).
// n: any positive size -- every tile edge is clipped (bundle adjustment passes multiples of 6, the essential graph multiples of 7).
// Ordering between the steps is by launches on `st` only.  mfma: the trailing update on v_mfma_f64_16x16x4_f64, else plain FMA.
int gba_solve_enqueue(asd_ctx* ctx, hipStream_t st, double* A, const double* b, double* x, int n, const int* done, int* chol_ok, bool mfma);
// true (+ error message) while a run of asd_local_ba_submit is outstanding on this context (ba.hip)
bool ba_lane_busy(asd_ctx* ctx, const char* who);
