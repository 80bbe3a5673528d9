// matcher.hip -- Frame grid (G1), every kernel of the ORBmatcher searches and the per-frame tracking stages (M0-M2).  The searches that
// replay the reference's logic on the host (M4, M5, loop closing) are in matcher_replay.cpp, the banks in matcher_banks.cpp (matcher.h).
//
// Reference (src/vslam/src): Frame.cc:123-138,219-286 (grid), Frame.cc:160-217 (isInFrustum),
// ORBmatcher.cc:1629-1650 (DescriptorDistance), :44-122, :1318-1452 (the tracking searches), :825-936 (Fuse),
// MapPoint.cc:271-338 (ComputeDistinctiveDescriptors).
//
// Split of work.  The reference's searches are order-dependent: a keypoint claimed by an earlier
// map point is skipped by later ones, best/second-best use strict '<' so the first candidate in
// grid order wins ties.  What is data parallel is DescriptorDistance itself, which the
// reference calls ~10^4-10^5 times per frame with two Mat conversions and two heap vectors per
// call.  So: the host only projects the queries (u, v, radius, level range); ONE kernel
// (k_window_search, a wave per query) walks the frame's 64x48 CSR grid in the reference's visiting
// order (Frame::GetFeaturesInArea: ix outer, iy inner, insertion order inside a cell), compacts the
// accepted candidates by ballot/prefix in that order and evaluates each candidate's squared L2 in
// the reference's exact summation order (sequential f32, no FMA: -ffp-contract=off) from
// descriptors resident in HBM; the claim / ratio / rotation-histogram logic is then replayed over the
// per-query (index, distance) lists: by k_resolve2 for the tracking stages, on the host (matcher_replay.cpp) elsewhere.
// The all-pairs matrix (asd_dist_matrix) uses the same exact summation, tiled through LDS.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <array>
#include <functional>
#include <memory>

#include "matcher.h"
#include "resolve2.h"

namespace {

// (TH_HIGH, TH_LOW, HISTO, kTop: resolve2.h)
constexpr int GC = ASD_GRID_COLS, GR = ASD_GRID_ROWS;

struct GridDev {
  const float4* kp;        // (x, y, octave as int bits, angle) per keypoint
  const int* cell_start;   // [64*48+1], cell = ix*48 + iy
  const int* cell_items;
  float min_x, min_y, inv_w, inv_h;
};

// one wave per query: pass 1 counts the candidates, one atomicAdd reserves the query's segment
// (segments may land in any order, each query's own list is in reference order), pass 2 writes
// (candidate index, distance).  Arithmetic of the cell range / distance tests is the float
// arithmetic of Frame.cc:226-265 verbatim.
//
// SORT = true (the device claim replay, k_resolve2; round 4): the query's list leaves the kernel in PREFERENCE order instead -- ascending
// (distance bits, position in Frame::GetFeaturesInArea order), which is the order the reference's strict `<` walks settle ties in
// (ORBmatcher.cc:86-104, :1392-1404: the first candidate in visiting order wins among equal distances) -- with its four best entries
// also in a compact per-query table.  The replay then needs the head of each list only: "best candidate no earlier map point holds"
// is the first entry of the sorted list without such a claim, the second best the next one.  A wave ranks its list by counting
// (rank of p = number of entries with a smaller key; keys are distinct because positions are): O(n^2 / 64) LDS broadcast reads for
// lists of 6 entries on average.  Entries the replay can never pick are left out here: keypoints that hold a map point on entry
// (`occ`, ORBmatcher.cc:84-88) and, with th_cut = TH_HIGH, candidates beyond it (frame-to-frame search: best-only, :1406).
#ifndef ASD_SEARCH_WAVES
#define ASD_SEARCH_WAVES 8
#endif
constexpr int kSearchWaves = ASD_SEARCH_WAVES;   // queries (waves) per workgroup
constexpr int kSearchCols = 16;                  // fast path: windows of up to this many grid columns ...
constexpr int kSearchList = 128;                 // ... and up to this many candidates per query
struct SortArgs {
  const uint8_t* occ;      // [n_cur] or null: keypoints that cannot be matched (occupied on entry)
  float th_cut;            // q_cnt counts the entries with distance <= th_cut (they are the list's head); +inf = all
  uint16_t* top_idx;       // [nq][kTop] keypoint (0xffff = no entry)
};
template <bool SORT>
__global__ __launch_bounds__(64 * kSearchWaves) void k_window_search(GridDev G, const WinQuery* __restrict__ queries, int nq,
                                                       const float* __restrict__ qdesc, const float* __restrict__ cdesc,
                                                       int* __restrict__ q_off, int* __restrict__ q_cnt,
                                                       int* __restrict__ total, int cap, int* __restrict__ out_idx,
                                                       float* __restrict__ out_dist, SortArgs S) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x * kSearchWaves + wave;
  // the waves of a workgroup reserve their segments with ONE atomicAdd (2000 same-address atomics, one per query, were a
  // serial chain through one L2 channel): every wave stays alive up to the barriers below, a query beyond nq counts as empty
  __shared__ int wg_cnt[kSearchWaves], wg_base;
  __shared__ int cand_l[kSearchWaves][kSearchList];
  __shared__ unsigned dist_l[SORT ? kSearchWaves : 1][kSearchList];
  const bool live = q < nq;
  const WinQuery Q = live ? queries[q] : WinQuery{0.f, 0.f, 0.f, 0, 0, -1};
  int cnt = 0, off = 0;
  bool empty = Q.qrow < 0;
  const int nMinCellX = max(0, (int)floorf((Q.x - G.min_x - Q.r) * G.inv_w));
  const int nMaxCellX = min(ASD_GRID_COLS - 1, (int)ceilf((Q.x - G.min_x + Q.r) * G.inv_w));
  const int nMinCellY = max(0, (int)floorf((Q.y - G.min_y - Q.r) * G.inv_h));
  const int nMaxCellY = min(ASD_GRID_ROWS - 1, (int)ceilf((Q.y - G.min_y + Q.r) * G.inv_h));
  if (nMinCellX >= ASD_GRID_COLS || nMaxCellX < 0 || nMinCellY >= ASD_GRID_ROWS || nMaxCellY < 0) empty = true;
  const bool check = (Q.min_level > 0) || (Q.max_level >= 0);
  auto accept = [&](const float4& kp) {
    const int oct = __float_as_int(kp.z);
    bool ok = true;
    if (check) {
      if (oct < Q.min_level) ok = false;
      if (Q.max_level >= 0 && oct > Q.max_level) ok = false;
    }
    const float dx = kp.x - Q.x, dy = kp.y - Q.y;
    if (!(fabsf(dx) < Q.r && fabsf(dy) < Q.r)) ok = false;
    return ok;
  };
  // the query's row is the same for the whole wave: read through the scalar cache (no vector registers, no address per lane), which leaves
  // room for sixteen candidate quads in flight per lane -- two dependent round trips per distance instead of four (beside the ASDNet
  // grids a dependent read takes 2-3 us, and this kernel's time is its waves' chains of them)
  const int qrow_u = __builtin_amdgcn_readfirstlane(Q.qrow < 0 ? 0 : Q.qrow);
  auto distance = [&](int idx) {   // exact summation order of DescriptorDistance (sequential f32)
    const float4* a = reinterpret_cast<const float4*>(qdesc + (size_t)qrow_u * 128);
    const float4* bb = reinterpret_cast<const float4*>(cdesc + (size_t)idx * 128);
    float sqd = 0.f;
#pragma unroll 16
    for (int k = 0; k < 32; ++k) {
      const float4 x = a[k], y = bb[k];
      float d;
      d = x.x - y.x; sqd = sqd + d * d;
      d = x.y - y.y; sqd = sqd + d * d;
      d = x.z - y.z; sqd = sqd + d * d;
      d = x.w - y.w; sqd = sqd + d * d;
    }
    return sqd;
  };
  auto score = [&](int idx, int p) {   // candidate p of the list, in list order
    const float sqd = distance(idx);
    out_idx[off + p] = idx;
    out_dist[off + p] = sqd;
  };
  // the general walk (any window, any list length): one dependent chain cell range -> items -> keypoints per column and pass
  auto walk = [&](int pass) {
    int pos = 0;
    for (int ix = nMinCellX; ix <= nMaxCellX; ++ix) {
      const int b = G.cell_start[ix * ASD_GRID_ROWS + nMinCellY], e = G.cell_start[ix * ASD_GRID_ROWS + nMaxCellY + 1];
      for (int base = b; base < e; base += 64) {
        const int it = base + lane;
        bool ok = false;
        int idx = 0;
        if (it < e) {
          idx = G.cell_items[it];
          ok = accept(G.kp[idx]);
          if (SORT && ok && S.occ && S.occ[idx]) ok = false;
        }
        const unsigned long long m = __ballot(ok);
        if (pass == 1 && ok) {
          const int p = pos + __popcll(m & ((1ull << lane) - 1));
          if (off + p < cap) score(idx, p);
        }
        pos += __popcll(m);
      }
    }
    return pos;
  };
  // Fast path (wave-uniform choice): the window's columns fit kSearchCols register slots and no column holds more than 64 items.
  // All column ranges are fetched together, then all item lists, then all keypoints -- three round trips instead of three per
  // column -- and the accepted keypoints are parked in LDS in list order, so that the second pass is one distance per lane
  // instead of a second walk.  Same visiting order (columns ascending, items in cell order), same arithmetic.
  const int ncol = nMaxCellX - nMinCellX + 1;
  bool fast = !empty && ncol <= kSearchCols;
  int cb[kSearchCols], ce[kSearchCols];
  if (fast) {
#pragma unroll
    for (int c = 0; c < kSearchCols; ++c) {
      const int ix = min(nMinCellX + c, nMaxCellX);
      cb[c] = G.cell_start[ix * ASD_GRID_ROWS + nMinCellY];
      ce[c] = G.cell_start[ix * ASD_GRID_ROWS + nMaxCellY + 1];
    }
#pragma unroll
    for (int c = 0; c < kSearchCols; ++c) {
      if (c >= ncol) ce[c] = cb[c];                 // unused slot: empty range
      if (ce[c] - cb[c] > 64) fast = false;
    }
  }
  if (fast) {
    int idxc[kSearchCols];
#pragma unroll
    for (int c = 0; c < kSearchCols; ++c) idxc[c] = cb[c] + lane < ce[c] ? G.cell_items[cb[c] + lane] : -1;
    float4 kpc[kSearchCols];
#pragma unroll
    for (int c = 0; c < kSearchCols; ++c) kpc[c] = idxc[c] >= 0 ? G.kp[idxc[c]] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (SORT && S.occ) {   // keypoints occupied on entry never enter a list (one more batch of loads, in flight with the keypoints)
      uint8_t oc[kSearchCols];
#pragma unroll
      for (int c = 0; c < kSearchCols; ++c) oc[c] = idxc[c] >= 0 ? S.occ[idxc[c]] : (uint8_t)0;
#pragma unroll
      for (int c = 0; c < kSearchCols; ++c) if (oc[c]) idxc[c] = -1;
    }
    int pos = 0;
#pragma unroll
    for (int c = 0; c < kSearchCols; ++c) {
      const bool ok = idxc[c] >= 0 && accept(kpc[c]);
      const unsigned long long m = __ballot(ok);
      if (ok) {
        const int p = pos + __popcll(m & ((1ull << lane) - 1));
        if (p < kSearchList) cand_l[wave][p] = idxc[c];
      }
      pos += __popcll(m);
    }
    cnt = pos;
    if (cnt > kSearchList) fast = false;            // (the list did not fit: the second pass walks again)
  } else if (!empty) {
    cnt = walk(0);
  }
  if (lane == 0) wg_cnt[wave] = cnt;
  asd_syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int w = 0; w < kSearchWaves; ++w) sum += wg_cnt[w];
    wg_base = sum ? atomicAdd(total, sum) : 0;
  }
  asd_syncthreads();
  off = wg_base;
  for (int w = 0; w < wave; ++w) off += wg_cnt[w];
  if (!SORT) {
    if (cnt > 0) {
      if (fast) {
        for (int p = lane; p < cnt; p += 64)
          if (off + p < cap) score(cand_l[wave][p], p);
      } else {
        (void)walk(1);
      }
    }
    if (lane == 0 && live) { q_cnt[q] = cnt; q_off[q] = cnt ? off : 0; }
    return;
  }
  // ---- SORT: the list in preference order + the compact head table
  if (!live) return;
  const bool fits = off + cnt <= cap;   // (an overflowing search is run again by the host: nothing of it is read)
  int n_keep = 0, s_off = off;
  auto put = [&](int base, int rank, int idx, float d) {
    out_idx[base + rank] = idx;
    out_dist[base + rank] = d;
    if (rank < kTop) S.top_idx[(size_t)q * kTop + rank] = (uint16_t)idx;
  };
  if (cnt > 0 && fits) {
    if (fast) {   // at most two candidates per lane, every key of the list in LDS
      const bool v0 = lane < cnt, v1 = lane + 64 < cnt;
      const int i0 = v0 ? cand_l[wave][lane] : 0, i1 = v1 ? cand_l[wave][lane + 64] : 0;
      const float d0 = v0 ? distance(i0) : 0.f, d1 = v1 ? distance(i1) : 0.f;
      const unsigned b0 = __float_as_uint(d0), b1 = __float_as_uint(d1);
      if (v0) dist_l[wave][lane] = b0;
      if (v1) dist_l[wave][lane + 64] = b1;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      int r0 = 0, r1 = 0;
      for (int i = 0; i < cnt; ++i) {
        const unsigned di = dist_l[wave][i];
        r0 += (di < b0) || (di == b0 && i < lane);
        r1 += (di < b1) || (di == b1 && i < lane + 64);
      }
      if (v0) put(off, r0, i0, d0);
      if (v1) put(off, r1, i1, d1);
      n_keep = __popcll(__ballot(v0 && d0 <= S.th_cut)) + __popcll(__ballot(v1 && d1 <= S.th_cut));
    } else {      // any length: the list is written in visiting order first, then ranked from there in chunks of kSearchList keys
      (void)walk(1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      s_off = cap + off;   // the sorted copy lives in the buffers' second half
      constexpr int R = 4;
      for (int pb = 0; pb < cnt; pb += 64 * R) {
        int pi[R], ii[R], rk[R]; unsigned bi[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          pi[r] = pb + 64 * r + lane;
          const int pc = min(pi[r], cnt - 1);
          ii[r] = __hip_atomic_load(out_idx + off + pc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          bi[r] = __float_as_uint(__hip_atomic_load(out_dist + off + pc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
          rk[r] = 0;
        }
        for (int cbase = 0; cbase < cnt; cbase += kSearchList) {
          __builtin_amdgcn_wave_barrier();
          for (int i = lane; i < kSearchList; i += 64)
            dist_l[wave][i] = cbase + i < cnt ? __float_as_uint(__hip_atomic_load(out_dist + off + cbase + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : 0xffffffffu;
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          __builtin_amdgcn_wave_barrier();
          const int m = min(kSearchList, cnt - cbase);
          for (int i = 0; i < m; ++i) {
            const unsigned di = dist_l[wave][i];
#pragma unroll
            for (int r = 0; r < R; ++r) rk[r] += (di < bi[r]) || (di == bi[r] && cbase + i < pi[r]);
          }
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const bool v = pi[r] < cnt;
          if (v) put(s_off, rk[r], ii[r], __uint_as_float(bi[r]));
          n_keep += __popcll(__ballot(v && __uint_as_float(bi[r]) <= S.th_cut));
        }
      }
    }
  }
  if (lane < kTop && lane >= (fits ? cnt : 0)) S.top_idx[(size_t)q * kTop + lane] = 0xffffu;
  if (lane == 0) { q_cnt[q] = n_keep; q_off[q] = cnt ? s_off : 0; }
}

// Node-restricted search (BoW-guided matchers): query q is matched against the explicit candidate list
// cand[cbeg[q] .. cend[q]) (the frame-2 members of the query's vocabulary node); distances land at
// out[ooff[q] + t] in list order.  One wave per query, lanes over candidates.
__global__ __launch_bounds__(256) void k_list_dist(const ListQuery* __restrict__ queries, int nq,
                                                   const int* __restrict__ cand, const float* __restrict__ qdesc,
                                                   const float* __restrict__ cdesc, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  const ListQuery Q = queries[q];
  const float4* a = reinterpret_cast<const float4*>(qdesc + (size_t)Q.qrow * 128);
  for (int t = Q.cbeg + lane; t < Q.cend; t += 64) {
    const float4* b = reinterpret_cast<const float4*>(cdesc + (size_t)cand[t] * 128);
    float sqd = 0.f;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) {
      const float4 x = a[k], y = b[k];
      float d;
      d = x.x - y.x; sqd = sqd + d * d;
      d = x.y - y.y; sqd = sqd + d * d;
      d = x.z - y.z; sqd = sqd + d * d;
      d = x.w - y.w; sqd = sqd + d * d;
    }
    out[Q.ooff + (t - Q.cbeg)] = sqd;
  }
}

// MapPoint::ComputeDistinctiveDescriptors for many map points at once: one workgroup per map point (<= 64
// observations), descriptors staged in LDS, all-pairs distances in the exact summation order, then the row medians by
// rank counting (the k-th order statistic is the element that k others precede; ties ordered by index, which does not
// change the VALUE found) and the first row with the smallest median (strict `<`, MapPoint.cc:318-331).
constexpr int kDistinctMax = 64;
__global__ __launch_bounds__(256) void k_distinctive(const float* __restrict__ desc, const int* __restrict__ set_start, int* __restrict__ best_out) {
  extern __shared__ __attribute__((aligned(16))) float smem_d[];
  const int s0 = set_start[blockIdx.x], n = set_start[blockIdx.x + 1] - s0;
  float* sd = smem_d;                       // [n][132] (padded rows)
  float* D = smem_d + kDistinctMax * 132;   // [n][n + 1]
  float* med = D + kDistinctMax * (kDistinctMax + 1);
  const int t = threadIdx.x;
  for (int idx = t; idx < n * 32; idx += 256) {
    const int r = idx >> 5, c = idx & 31;
    *reinterpret_cast<float4*>(sd + r * 132 + c * 4) = reinterpret_cast<const float4*>(desc + (size_t)(s0 + r) * 128)[c];
  }
  asd_syncthreads();
  for (int p = t; p < n * n; p += 256) {
    const int i = p / n, j = p % n;
    float acc = 0.f;
    if (i != j) {
      const float4* x = reinterpret_cast<const float4*>(sd + i * 132);
      const float4* y = reinterpret_cast<const float4*>(sd + j * 132);
      for (int k = 0; k < 32; ++k) {
        const float4 a = x[k], b = y[k];
        float d;
        d = a.x - b.x; acc = acc + d * d;
        d = a.y - b.y; acc = acc + d * d;
        d = a.z - b.z; acc = acc + d * d;
        d = a.w - b.w; acc = acc + d * d;
      }
    }
    D[i * (n + 1) + j] = acc;
  }
  asd_syncthreads();
  const int kth = (int)(0.5 * (n - 1));
  for (int p = t; p < n * n; p += 256) {
    const int i = p / n, j = p % n;
    const float v = D[i * (n + 1) + j];
    int rank = 0;
    for (int l = 0; l < n; ++l) {
      const float u = D[i * (n + 1) + l];
      rank += (u < v || (u == v && l < j)) ? 1 : 0;
    }
    if (rank == kth) med[i] = v;  // exactly one j per row has this rank
  }
  asd_syncthreads();
  if (t == 0) {
    float best_median = 100;
    int best = 0;
    for (int i = 0; i < n; ++i)
      if (med[i] < best_median) { best_median = med[i]; best = i; }
    best_out[blockIdx.x] = best;
  }
}

// all-pairs: block = 256 columns (b rows) x 16 a rows; a tile broadcast from LDS, b row in VGPRs.
__global__ __launch_bounds__(256) void k_dist_matrix(const float* __restrict__ a, int na, const float* __restrict__ b,
                                                     int nb, float* __restrict__ out) {
  __shared__ float4 sa[16][32];
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int i0 = blockIdx.y * 16;
  for (int idx = threadIdx.x; idx < 16 * 32; idx += 256) {
    const int r = idx >> 5, c = idx & 31;
    const int ia = min(i0 + r, na - 1);
    sa[r][c] = reinterpret_cast<const float4*>(a + (size_t)ia * 128)[c];
  }
  asd_syncthreads();
  const float4* brow = reinterpret_cast<const float4*>(b + (size_t)min(j, nb - 1) * 128);
  float acc[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k = 0; k < 32; ++k) {
    const float4 y = brow[k];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float4 x = sa[r][k];
      float d;
      d = x.x - y.x; acc[r] = acc[r] + d * d;
      d = x.y - y.y; acc[r] = acc[r] + d * d;
      d = x.z - y.z; acc[r] = acc[r] + d * d;
      d = x.w - y.w; acc[r] = acc[r] + d * d;
    }
  }
  if (j < nb)
    for (int r = 0; r < 16; ++r)
      if (i0 + r < na) out[(size_t)(i0 + r) * nb + j] = acc[r];
}


// device-to-device copy of descriptor rows as a plain kernel: a hipMemcpyAsync costs the host 15-25 us per call on this
// stream, a launch ~5 (frame_set's adoption of the extractor's descriptors, asd_bank_put_from_frame)
__global__ __launch_bounds__(256) void k_copy16(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
hipError_t copy_rows(hipStream_t st, void* dst, const void* src, size_t bytes) {   // bytes % 16 == 0, 16-B aligned
  const size_t n16 = bytes / 16;
  if (!n16) return hipSuccess;
  hipLaunchKernelGGL(k_copy16, dim3((unsigned)std::min<size_t>((n16 + 255) / 256, 1024)), dim3(256), 0, st, static_cast<const uint4*>(src),
                     static_cast<uint4*>(dst), n16);
  return hipGetLastError();
}

// ---- claim / ratio / rotation-histogram replay on the device ------------------------------------------------------
// The searches are order dependent: map point q (in input order) takes the best candidate that no EARLIER map point with
// Observations() > 0 holds (ORBmatcher.cc:86-88, :1392-1395).  Written as a recurrence, pick(q) = g(picks of all q' < q):
// a triangular system with exactly one solution, the serial walk's.  A serial walk is ~100 dependent LDS / L2 round trips
// per map point, so the system is solved by fixed-point iteration instead: every map point recomputes its pick in parallel
// from the claims of the previous iteration ("keypoint j is taken for q iff the smallest claimant of j is < q") until an
// iteration changes nothing.  Correctness propagates upward from q = 0 (after k iterations the first k map points are
// final), and a state that one more iteration leaves unchanged IS the solution of the recurrence; real frames settle in
// 4-13 iterations of one barrier each (13: 2000 frame-to-frame queries with every candidate eligible and random distances).
// Claims live in LDS as two tables used alternately; an entry is (iterations-left << 16 | q) so that atomicMin lets the
// current iteration's posts overrule stale ones and nothing has to be cleared.  A keypoint held by a map point without
// observations stays available (mp_obs_positive): such map points post no claim, and the keypoint's final holder is the
// LAST writer = the largest q picking it.
// KIND 0 = SearchByProjection(frame, frame) (:1318-1452): best only, TH_HIGH, rotation histogram over every write.
// KIND 1 = SearchByProjection(frame, points) (:44-122): best / second best with levels and the ratio test; counts twice.
// Round 2-3 solved the recurrence with every candidate bidding for its query in every iteration (historical, removed: `k_resolve`, 86-91 us for the frame-to-frame
// search); since round 4 the search hands its lists over in preference order and the replay walks their heads (resolve2.h: 33-40 us) --
// the bidding kernel was removed in round 5 (DESIGN.md section 4.0c keeps its numbers).
// (the claim replay over sorted lists -- Resolve2Args, resolve2_body -- lives in resolve2.h: ba.hip runs it inside k_resolve_pose)
template <int KIND, int QPT>
__global__ __launch_bounds__(kResolve2Threads) void k_resolve2(Resolve2Args a) {
  resolve2_body<KIND, QPT, kResolve2Threads>(a);
}

// Frame::isInFrustum (Frame.cc:160-217) + MapPoint::PredictScale (MapPoint.cc:438-453) + the search window of
// ORBmatcher::SearchByProjection(F, vpMapPoints, th) (:60-70), one thread per map point, straight into the query table of
// k_window_search.  The arithmetic is asd_frustum's, operation for operation (f32 with the two double accumulations of the
// reference; -ffp-contract=off; IEEE division and square root), and the level comes from comparisons with thresholds that the
// host derived from its own logf (ctx.h, level_thr), so the queries are the ones the host would have written.
// The upload of a fused chain rides in its first kernel: the blocks behind the query blocks copy the chain's pinned upload block to its
// device twin (everything but the query table at its head, which the query blocks write), the query blocks read their own inputs from
// the PINNED block.  One launch and ~10 us of dependent copy kernel less per stage; the kernels behind this one read the device twin.
struct UploadTail {
  const uint4* src; uint4* dst;   // pinned block, device twin
  size_t first16, n16;            // 16-B words [first16, n16) are copied
  int q_blocks;                   // blocks [0, q_blocks) make queries, the rest copy
};
__device__ inline bool upload_tail_block(const UploadTail& u) {
  if ((int)blockIdx.x < u.q_blocks) return false;
  const size_t nb = gridDim.x - u.q_blocks;
  for (size_t i = u.first16 + (size_t)(blockIdx.x - u.q_blocks) * 256 + threadIdx.x; i < u.n16; i += nb * 256) u.dst[i] = u.src[i];
  return true;
}
constexpr int kUploadTailBlocks = 64;

struct FrustumArgs {
  int n, n_levels, bfactor;
  const float* Xw; const float* normal; const float* min_dist; const float* max_dist;
  const int* rows;          // bank row per map point, or null: descriptor row = map point index
  float T[16], Ow[3];
  float fx, fy, cx, cy, min_x, max_x, min_y, max_y, cos_limit, th;
  float level_thr[ASD_MAX_LEVELS], scale[ASD_MAX_LEVELS];
  WinQuery* queries;
  UploadTail up;
  // asd_track_frame (the stage behind another one, nothing from the host in between): the frame pose comes from device memory
  // (T_dev[16] + Ow[3], written by k_between), the map points are rows of the attribute bank (attr[row][8] = position, normal,
  // min / max distance), candidates flagged in `skip` are in the frame already (Tracking.cc:811-823) and make no query, and every
  // candidate's position is also written to xw_out[q] for the edges of the pose solver behind the search
  const float* T_dev; const float* attr; const uint8_t* skip; float* xw_out;
};
__global__ __launch_bounds__(256) void k_frustum_queries(FrustumArgs a) {
  if (upload_tail_block(a.up)) return;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= a.n) return;
  WinQuery Q{0.f, 0.f, 0.f, 0, 0, -1};
  if (a.attr) {   // bank form: the map points are rows of the attribute bank (the per-candidate arithmetic lives in ctx.h)
    if (a.T_dev) asd_frustum_bank_point(a, a.T_dev, a.skip, q);   // asd_track_frame: pose and skip flags from the stage in front
    else {                                                        // asd_track_local_points_rows: pose from the host, by value
      float Tl[19];
      for (int i = 0; i < 16; ++i) Tl[i] = a.T[i];
      for (int i = 0; i < 3; ++i) Tl[16 + i] = a.Ow[i];
      asd_frustum_bank_point(a, Tl, a.skip, q);
    }
    return;
  }
  const float* P = a.Xw + 3 * (size_t)q;
  float Pc[3];
  for (int r = 0; r < 3; ++r) {
    const float t0 = a.T[r * 4 + 0] * P[0] + a.T[r * 4 + 1] * P[1] + a.T[r * 4 + 2] * P[2];
    Pc[r] = (float)((double)t0 + (double)a.T[r * 4 + 3]);
  }
  bool ok = !(Pc[2] < 0.0f);
  const float invz = 1.0f / Pc[2];
  const float u = a.fx * Pc[0] * invz + a.cx, v = a.fy * Pc[1] * invz + a.cy;
  if (u < a.min_x || u > a.max_x || v < a.min_y || v > a.max_y) ok = false;
  const float maxD = 1.2f * a.max_dist[q], minD = 0.8f * a.min_dist[q];
  const float PO[3] = {P[0] - a.Ow[0], P[1] - a.Ow[1], P[2] - a.Ow[2]};
  const double nn = (double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2];
  const float dist = (float)sqrt(nn);
  if (dist < minD || dist > maxD) ok = false;
  const float* Pn = a.normal + 3 * (size_t)q;
  const double dot = (double)PO[0] * Pn[0] + (double)PO[1] * Pn[1] + (double)PO[2] * Pn[2];
  const float vc = (float)(dot / dist);
  if (vc < a.cos_limit) ok = false;
  if (ok) {
    const float ratio = a.max_dist[q] / dist;
    int lvl = 0;
    for (int k = 1; k < a.n_levels; ++k) lvl += ratio >= a.level_thr[k];
    float r = vc > 0.998 ? 2.5f : 4.0f;  // RadiusByViewingCos (:126-132)
    if (a.bfactor) r *= a.th;
    Q = WinQuery{u, v, r * a.scale[lvl], lvl - 1, lvl, a.rows ? a.rows[q] : q};
  }
  a.queries[q] = Q;
}

// The projection loop of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th) (ORBmatcher.cc:1343-1368), one thread per
// map point of the last frame, straight into the query table of k_window_search: the same f32 operations in the same order as
// the host loop of match_project_frame_impl (-ffp-contract=off, the reciprocal as a double division rounded to float), the
// octave from the last frame's device keypoints.
struct ProjectArgs {
  int n;
  const uint8_t* has_mp; const float* Xw; const int* rows; const float4* kp_last;
  float T[16];
  float fx, fy, cx, cy, min_x, max_x, min_y, max_y, th;
  float scale[ASD_MAX_LEVELS];
  WinQuery* queries;
  UploadTail up;
};
__global__ __launch_bounds__(256) void k_project_queries(ProjectArgs a) {
  if (upload_tail_block(a.up)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  WinQuery Q{0.f, 0.f, 0.f, 0, 0, -1};
  if (a.has_mp[i]) {
    const float* X = a.Xw + 3 * (size_t)i;
    float Xc[3];
    for (int r = 0; r < 3; ++r) {
      const float t0 = a.T[r * 4 + 0] * X[0] + a.T[r * 4 + 1] * X[1] + a.T[r * 4 + 2] * X[2];
      Xc[r] = (float)((double)t0 + (double)a.T[r * 4 + 3]);
    }
    const float invzc = (float)(1.0 / (double)Xc[2]);
    if (!(invzc < 0)) {
      const float u = a.fx * Xc[0] * invzc + a.cx;
      const float v = a.fy * Xc[1] * invzc + a.cy;
      if (!(u < a.min_x || u > a.max_x) && !(v < a.min_y || v > a.max_y)) {
        const int oct = __float_as_int(a.kp_last[i].z);
        Q = WinQuery{u, v, a.th * a.scale[oct], oct - 1, oct + 1, a.rows ? a.rows[i] : i};
      }
    }
  }
  a.queries[i] = Q;
}

// (k_between's body lives in ctx.h: asd_between_body -- it runs as the tail of the motion-model stage's k_pose_opt)
// ---- host helpers -------------------------------------------------------------------------
// device candidate buffers (k_window_search's output, k_resolve2's input): 8 B per candidate, twice over
int ensure_cands_dev(asd_ctx* ctx, MatcherState* m, size_t n) {
  if (n <= (size_t)m->cand_cap) return ASD_OK;
  if (n > ((size_t)1 << 30)) { ctx->set_error("candidate buffers: %zu entries asked for", n); return ASD_ERR_CAPACITY; }
  const size_t cap = std::max(n + n / 2, (size_t)1 << 18);
  if (m->d_idx) { (void)hipFree(m->d_idx); (void)hipFree(m->d_dist); }
  m->d_idx = nullptr; m->d_dist = nullptr;
  m->cand_cap = 0;
  // idx / dist twice over: k_window_search<true> writes the sorted copy of a list that took its slow path into the second half
  ASD_HIP_CHECK(ctx, hipMalloc(&m->d_idx, 2 * cap * sizeof(int)));
  ASD_HIP_CHECK(ctx, hipMalloc(&m->d_dist, 2 * cap * sizeof(float)));
  m->cand_cap = (int)std::min(cap, (size_t)0x7fffffff);
  return ASD_OK;
}
// ... and their pinned host twins, which only the host replay (matcher_window_search) reads
int ensure_cands(asd_ctx* ctx, MatcherState* m, int n) {
  int rc = ensure_cands_dev(ctx, m, (size_t)n);
  if (rc != ASD_OK) return rc;
  if (m->cand_cap <= m->h_cand_cap) return ASD_OK;
  if (m->h_idx) { (void)hipHostFree(m->h_idx); (void)hipHostFree(m->h_dist); }
  m->h_idx = nullptr; m->h_dist = nullptr;
  m->h_cand_cap = 0;
  ASD_HIP_CHECK(ctx, hipHostMalloc(&m->h_idx, (size_t)m->cand_cap * sizeof(int)));
  ASD_HIP_CHECK(ctx, hipHostMalloc(&m->h_dist, (size_t)m->cand_cap * sizeof(float)));
  m->h_cand_cap = m->cand_cap;
  return ASD_OK;
}
}  // namespace

// ---- what matcher_replay.cpp and matcher_banks.cpp call (matcher.h) -----------------------------------------------------------------
MatcherState* matcher_state(asd_ctx* ctx) {
  if (!ctx->matcher) {
    MatcherState* m = new MatcherState();
    m->replay_host = ctx->match_replay_host;
    ctx->matcher = m;
  }
  return static_cast<MatcherState*>(ctx->matcher);
}

int matcher_ensure_queries(asd_ctx* ctx, MatcherState* m, int nq) {
  if (nq <= m->q_cap) return ASD_OK;
  const int cap = std::max(nq * 3 / 2, 8192);
  if (m->d_queries) { (void)hipFree(m->d_queries); (void)hipHostFree(m->h_queries); (void)hipFree(m->d_q_off); (void)hipHostFree(m->h_q); }
  m->q_cap = 0;
  ASD_HIP_CHECK(ctx, hipMalloc(&m->d_queries, (size_t)cap * sizeof(WinQuery)));
  ASD_HIP_CHECK(ctx, hipHostMalloc(&m->h_queries, (size_t)cap * sizeof(WinQuery)));
  ASD_HIP_CHECK(ctx, hipMalloc(&m->d_q_off, ((size_t)2 * cap + 4) * sizeof(int)));  // off | cnt | total
  ASD_HIP_CHECK(ctx, hipHostMalloc(&m->h_q, ((size_t)2 * cap + 4) * sizeof(int)));
  m->q_cap = cap;
  return ASD_OK;
}
int matcher_ensure_qdesc(asd_ctx* ctx, MatcherState* m, int n) {
  if (n <= m->qdesc_cap) return ASD_OK;
  const int cap = std::max(n * 3 / 2, 8192);
  if (m->d_qdesc) { (void)hipFree(m->d_qdesc); (void)hipHostFree(m->h_qdesc); }
  m->qdesc_cap = 0;
  ASD_HIP_CHECK(ctx, hipMalloc(&m->d_qdesc, (size_t)cap * 512));
  ASD_HIP_CHECK(ctx, hipHostMalloc(&m->h_qdesc, (size_t)cap * 512));
  m->qdesc_cap = cap;
  return ASD_OK;
}

int matcher_upload_qdesc(asd_ctx* ctx, MatcherState* m, const float* desc, int n) {
  int rc = matcher_ensure_qdesc(ctx, m, n);
  if (rc != ASD_OK) return rc;
  memcpy(m->h_qdesc, desc, (size_t)n * 512);
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(m->d_qdesc, m->h_qdesc, (size_t)n * 512, hipMemcpyHostToDevice, ctx->stream));
  return ASD_OK;
}

AsdFrameSlot* matcher_slot(asd_ctx* ctx, int s) {
  if (!ctx || s < 0 || s >= ASD_MAX_FRAMES) return nullptr;
  return &ctx->frames[s];
}

int matcher_window_search(asd_ctx* ctx, MatcherState* m, const AsdFrameSlot& F, int nq, const float* d_q, SearchResult* res, int kind) {
  if (asd_track_busy(ctx, "matcher call")) return ASD_ERR_INVALID;
  static const bool timing = getenv("ASD_TIMING") != nullptr;   // per-kind host-side split, printed every 200 searches
  static double tacc[4][3]; static long tcalls[4];
  const auto tw0 = std::chrono::steady_clock::now();
  auto tw1 = tw0;
  int rc = ensure_cands(ctx, m, 1);
  if (rc != ASD_OK) return rc;
  hipStream_t st = ctx->stream;
  // off | cnt | total packed for THIS query count, so one small copy brings all three back
  int* d_off = m->d_q_off;
  int* d_cnt = m->d_q_off + nq;
  int* d_total = m->d_q_off + 2 * nq;
  // candidates copied back together with the counts: a little more than the last search produced
  const int optimistic = std::min(m->cand_cap, std::max(4096, m->last_total[kind] + m->last_total[kind] / 4));
  for (int attempt = 0; attempt < 2; ++attempt) {
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(m->d_queries, m->h_queries, (size_t)nq * sizeof(WinQuery), hipMemcpyHostToDevice, st));
    ASD_HIP_CHECK(ctx, hipMemsetAsync(d_total, 0, sizeof(int), st));
    GridDev G{F.d_kp, F.d_cell_start, F.d_cell_items, F.min_x, F.min_y, F.inv_w, F.inv_h};
    ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, st));
    hipLaunchKernelGGL(k_window_search<false>, dim3((nq + kSearchWaves - 1) / kSearchWaves), dim3(64 * kSearchWaves), 0, st, G, m->d_queries, nq, d_q, F.d_desc, d_off, d_cnt,
                       d_total, m->cand_cap, m->d_idx, m->d_dist, SortArgs{});
    ASD_HIP_CHECK(ctx, hipGetLastError());
    ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, st));
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(m->h_q, d_off, ((size_t)2 * nq + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(m->h_idx, m->d_idx, (size_t)optimistic * sizeof(int), hipMemcpyDeviceToHost, st));
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(m->h_dist, m->d_dist, (size_t)optimistic * sizeof(float), hipMemcpyDeviceToHost, st));
    tw1 = std::chrono::steady_clock::now();
    ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
    const int total = m->h_q[2 * nq];
    m->last_total[kind] = total;
    if (total > m->cand_cap) {  // segment reservation overflowed the buffers: grow and run again
      if ((rc = ensure_cands(ctx, m, total)) != ASD_OK) return rc;
      continue;
    }
    if (total > optimistic) {
      ASD_HIP_CHECK(ctx, hipMemcpyAsync(m->h_idx + optimistic, m->d_idx + optimistic, (size_t)(total - optimistic) * sizeof(int), hipMemcpyDeviceToHost, st));
      ASD_HIP_CHECK(ctx, hipMemcpyAsync(m->h_dist + optimistic, m->d_dist + optimistic, (size_t)(total - optimistic) * sizeof(float), hipMemcpyDeviceToHost, st));
      ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    break;
  }
  ASD_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->ms_match, ctx->ev0, ctx->ev1));
  if (timing) {
    const auto tw2 = std::chrono::steady_clock::now();
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    tacc[kind][0] += ms(tw0, tw1); tacc[kind][1] += ms(tw1, tw2); tacc[kind][2] += ctx->ms_match;
    if (++tcalls[kind] % 200 == 0)
      fprintf(stderr, "[window_search kind %d] enqueue %.3f sync %.3f kernel %.3f ms, %d candidates copied (last total %d)\n", kind,
              tacc[kind][0] / tcalls[kind], tacc[kind][1] / tcalls[kind], tacc[kind][2] / tcalls[kind], optimistic, m->last_total[kind]);
  }
  res->off = m->h_q;
  res->cnt = m->h_q + nq;
  res->idx = m->h_idx;
  res->dist = m->h_dist;
  return ASD_OK;
}

namespace {
// where the claim / ratio / histogram replay runs: on the device (k_resolve2, default) or on the host over the copied-back
// candidate lists (ASD_MATCH_REPLAY=host in the environment of asd_ctx_create; also taken when the tables would
// not fit the workgroup's LDS or there are more than 4096 queries)
size_t resolve_lds_bytes(int kind, int n_cur, int nq) {
  // k_resolve2: the two claim tables, angle / octave table, last-writer table, (local map) the compacted list of map points with candidates
  return resolve2_fixed_lds(kind, n_cur) + (size_t)n_cur * 4 + (kind == 1 ? ((size_t)nq * 2 + 15) / 16 * 16 : 0);
}
bool replay_on_device(const MatcherState* m, int kind, int n_cur, int nq) {
  // kind 0 (frame to frame): every last-frame point is a slot of the replay workgroup; kind 1 (local map): the map points that HAVE candidates are
  // replayed in chunks (resolve2.h), so the count of candidates is bounded only by the compaction's rounds and the 16-bit indices
  const int max_q = kind == 0 ? kResolve2Threads * 4 : std::min(kResolve2MaxRounds * 512, 65535);
  return !m->replay_host && n_cur > 0 && n_cur < 65536 && nq <= max_q && resolve_lds_bytes(kind, n_cur, nq) <= 96 * 1024;
}

// ---- one tracking stage ------------------------------------------------------------------------------------------------------------
// [query kernel] -> k_window_search<true> -> claim replay -> [PoseOptimization], described by ONE struct and enqueued by ONE function
// (enqueue_stage).  asd_match_project_* and the single-stage asd_track_* chains run one stage behind one synchronisation
// (search_and_resolve: with a second search after a candidate overflow, or deferred); asd_track_frame runs two with the between-stage
// block and no second search.  Every pointer of a description is final when it is built -- device memory, or the context's pinned upload /
// result blocks, which do not move after AsdXfer::begin -- so a stage can be enqueued a second time from the same description.
struct StageSolver {               // PoseOptimization behind the replay, on the match table it wrote (pose_chain_enqueue)
  const float* d_points;           // [.][3] world positions the match table names
  const uint8_t* d_hold;           // [n_cur] or null: keypoints that held a map point on entry ...
  const float* d_own;              // [n_cur][3] or null: ... and that point's position
  double pose0[7];                 // the start pose, unless
  const double* d_pose0;           // non-null: it is read from the device (the stage in front wrote it)
  double K[4];
  double* io;                      // the solver's reservation in the result block (pinned: the kernel stores there directly)
  double* d_io_dev;                // optional: a second copy in device memory for the stage behind
  const AsdBetweenArgs* d_between; // optional: the work between two stages as the solver's tail
};
enum QuerySource { kQueriesUploaded, kQueriesProject, kQueriesFrustum };   // the host's table inside the upload block, or the kernel that writes it
enum StageUpload { kUploadElsewhere, kUploadCopy, kUploadCarried };       // the upload block: an earlier stage's business / a copy in front of
                                                                           // the stage / carried by the tail blocks of the stage's query kernel
struct TrackStage {
  int kind, nq;                    // 0 frame to frame, 1 local map; number of queries
  const AsdFrameSlot* F;           // the current frame
  QuerySource source;
  ProjectArgs project;             // kQueriesProject
  FrustumArgs frustum;             // kQueriesFrustum
  StageUpload upload;
  const WinQuery* d_queries;
  const float* d_qdesc;            // the queries' descriptor table (m->d_qdesc or m->d_bank)
  const float4* kp_last;           // kind 0: the last frame's keypoints
  const uint8_t* d_obs_pos;        // [nq] or null: Observations() > 0 per query
  const uint8_t* d_occupied;       // [n_cur] or null: keypoints that hold a map point on entry (kind 1)
  int check_ori;
  float nn_ratio;
  int *d_off, *d_cnt;              // [nq] each: the lists' offsets and pickable heads
  int* d_total;                    // the candidate counter (a zeroed word of the upload block)
  uint16_t* d_top;                 // [nq][kTop]
  int *d_out, *h_out;              // match table [n_cur] + counters: the result block's reservation on the device and its pinned twin
  bool timed;                      // ASD_TIMING: event records around search + replay (the "match" clock of asd_last_stage_ms)
  bool has_solver;
  StageSolver solver;
};

// the copy of the upload block that a query kernel's tail blocks carry (the query table is the block's first reservation: the copy starts
// behind it); not carried: the kernel has query blocks only
UploadTail upload_tail(const AsdXfer& up, int nq, bool carried) {
  return UploadTail{reinterpret_cast<const uint4*>(up.h), reinterpret_cast<uint4*>(up.d), carried ? ((size_t)nq * sizeof(WinQuery) + 255) / 256 * 16 : 0,
                    carried ? (up.used + 15) / 16 : 0, (nq + 255) / 256};
}

// k_project_queries' constants (the tables, the query table and the upload tail belong to the stage that owns them)
ProjectArgs project_args(const asd_ctx* ctx, const AsdFrameSlot& C, const AsdFrameSlot& L, const float* Tcw, const float* K, float th) {
  ProjectArgs pa{};
  pa.n = L.n; pa.kp_last = L.d_kp;
  memcpy(pa.T, Tcw, sizeof pa.T);
  pa.fx = K[0]; pa.fy = K[1]; pa.cx = K[2]; pa.cy = K[3];
  pa.min_x = C.min_x; pa.max_x = C.max_x; pa.min_y = C.min_y; pa.max_y = C.max_y; pa.th = th;
  for (int l = 0; l < ASD_MAX_LEVELS; ++l) pa.scale[l] = l < ctx->cfg.n_levels ? ctx->scale[l] : 0.f;
  return pa;
}
// k_frustum_queries' constants.  The frame pose by value (Tcw, host) or from device memory (T_dev[19]: Tcw + Ow, written by the stage in front)
FrustumArgs frustum_args(const asd_ctx* ctx, const AsdFrameSlot& F, int n, const float* Tcw, const float* T_dev, const float* K, float cos_limit, float th) {
  FrustumArgs fa{};
  fa.n = n; fa.n_levels = ctx->cfg.n_levels; fa.bfactor = th != 1.0;
  if (Tcw) {
    memcpy(fa.T, Tcw, sizeof fa.T);
    matcher_camera_centre(Tcw, 4, Tcw + 3, 4, fa.Ow);
  }
  fa.T_dev = T_dev;
  fa.fx = K[0]; fa.fy = K[1]; fa.cx = K[2]; fa.cy = K[3];
  fa.min_x = F.min_x; fa.max_x = F.max_x; fa.min_y = F.min_y; fa.max_y = F.max_y;
  fa.cos_limit = cos_limit; fa.th = th;
  for (int l = 0; l < ASD_MAX_LEVELS; ++l) { fa.level_thr[l] = ctx->level_thr[l]; fa.scale[l] = l < ctx->cfg.n_levels ? ctx->scale[l] : 0.f; }
  return fa;
}
// the replay's argument block of a stage; returns the dynamic LDS it needs
size_t resolve2_args(const MatcherState* m, const TrackStage& s, Resolve2Args* out) {
  const int n_cur = s.F->n;
  Resolve2Args a{};
  a.nq = s.nq; a.n_cur = n_cur;
  a.q_off = s.d_off; a.q_cnt = s.d_cnt; a.idx = m->d_idx; a.dist = m->d_dist; a.top_idx = s.d_top;
  a.total = s.d_total; a.cap = m->cand_cap;
  a.obs_pos = s.d_obs_pos;
  a.kp_cur = s.F->d_kp; a.kp_last = s.kp_last;
  a.check_ori = s.check_ori; a.nn_ratio = s.nn_ratio;
  a.match_cur = s.d_out; a.n_matches = s.d_out + n_cur; a.mirror = s.h_out;
  // the sorted lists' copy in LDS (for queries whose four best are all held): what the previous search of this kind produced and
  // a quarter on top, as far as the 96 KB this kernel may ask for allow; entries beyond it are read from global memory
  const size_t fixed = resolve_lds_bytes(s.kind, n_cur, s.nq), per = s.kind == 1 ? 6 : 2;
  a.stage_cap = (int)std::min<size_t>(((size_t)m->last_total[s.kind] * 5 / 4 + 1023) / 1024 * 1024, ((size_t)96 * 1024 - fixed) / per / 8 * 8);
  *out = a;
  return fixed + (size_t)a.stage_cap * per;
}
// more than 64 KB of dynamic LDS has to be asked for once per kernel and device: a runtime request, made ahead of a chain's first launch
int resolve2_attributes(asd_ctx* ctx) {
  static AsdPerDeviceOnce attrs;
  if (!attrs.need(ctx->cfg.device)) return ASD_OK;
  const void* ks[] = {reinterpret_cast<const void*>(k_resolve2<0, 2>), reinterpret_cast<const void*>(k_resolve2<0, 4>),
                      reinterpret_cast<const void*>(k_resolve2<1, 2>), reinterpret_cast<const void*>(k_resolve2<1, 4>)};
  for (const void* k : ks) ASD_HIP_CHECK(ctx, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
  attrs.done(ctx->cfg.device);
  return ASD_OK;
}
hipError_t launch_resolve2(hipStream_t st, int kind, const Resolve2Args& a, size_t lds) {
  auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(1), dim3(kResolve2Threads), lds, st, a); };
  const bool two = a.nq <= 2 * kResolve2Threads;   // queries per thread
  if (kind == 0) { if (two) go(k_resolve2<0, 2>); else go(k_resolve2<0, 4>); }
  else { if (two) go(k_resolve2<1, 2>); else go(k_resolve2<1, 4>); }
  return hipGetLastError();
}
// With a PoseOptimization behind the search, replay and solver are ONE workgroup (k_resolve_pose: resolve2_body on the solver's threads, then
// the solver) where the stage's tables fit: as two kernels the solver waits 35-55 us for a CU of its own behind the replay, beside the
// extractor's ASDNet workgroups
bool stage_fuses(const asd_ctx* ctx, const MatcherState* m, const TrackStage& s) {
  Resolve2Args a;
  return s.has_solver && pose_chain_fused_ok(ctx, s.kind, s.nq, s.F->n, resolve2_args(m, s, &a));
}

// Enqueues one stage on the context's stream: [upload copy] [query kernel] search, then the replay as k_resolve2 [and the solver], or -- with
// `fuse` (stage_fuses) -- replay and solver as one workgroup.  Launches only: every allocation and attribute was asked for by the caller.
int enqueue_stage(asd_ctx* ctx, const MatcherState* m, const TrackStage& s, bool fuse) {
  hipStream_t st = ctx->stream;
  const AsdFrameSlot& F = *s.F;
  int rc;
  if (s.upload == kUploadCopy) ASD_HIP_CHECK(ctx, ctx->up.upload(st));
  if (s.source == kQueriesProject) {
    const UploadTail& t = s.project.up;
    hipLaunchKernelGGL(k_project_queries, dim3(t.q_blocks + (t.n16 ? kUploadTailBlocks : 0)), dim3(256), 0, st, s.project);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  } else if (s.source == kQueriesFrustum) {
    const UploadTail& t = s.frustum.up;
    hipLaunchKernelGGL(k_frustum_queries, dim3(t.q_blocks + (t.n16 ? kUploadTailBlocks : 0)), dim3(256), 0, st, s.frustum);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  // (two timed event records per chain, each a barrier packet on the stream -- only when somebody asked for timings)
  if (s.timed) ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, st));
  // the lists in preference order (k_window_search<true>), the replay over their heads
  const GridDev G{F.d_kp, F.d_cell_start, F.d_cell_items, F.min_x, F.min_y, F.inv_w, F.inv_h};
  const SortArgs sa{s.d_occupied, s.kind == 0 ? TH_HIGH : __builtin_huge_valf(), s.d_top};
  hipLaunchKernelGGL(k_window_search<true>, dim3((s.nq + kSearchWaves - 1) / kSearchWaves), dim3(64 * kSearchWaves), 0, st, G, s.d_queries, s.nq, s.d_qdesc, F.d_desc, s.d_off,
                     s.d_cnt, s.d_total, m->cand_cap, m->d_idx, m->d_dist, sa);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  Resolve2Args ra;
  const size_t lds = resolve2_args(m, s, &ra);
  if (!fuse) {
    ASD_HIP_CHECK(ctx, launch_resolve2(st, s.kind, ra, lds));
    if (s.timed) ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, st));
  }
  if (s.has_solver) {
    const StageSolver& v = s.solver;
    const AsdFusedReplay fr{&ra, s.kind, s.nq, lds};
    AsdPoseChainArgs c{};
    c.n_cur = F.n; c.d_match = s.d_out; c.d_kp = F.d_kp;
    c.d_points = v.d_points; c.d_hold = v.d_hold; c.d_own = v.d_own;
    c.pose7 = v.d_pose0 ? nullptr : v.pose0; c.K = v.K;
    c.d_io = v.io; c.d_pose0 = v.d_pose0; c.d_io_dev = v.d_io_dev; c.between = v.d_between;
    c.fused = fuse ? &fr : nullptr;
    if ((rc = pose_chain_enqueue(ctx, c)) != ASD_OK) return rc;
  }
  if (fuse && s.timed) ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, st));   // (the "match" clock then covers the solver too)
  return ASD_OK;
}
// the one event record at a chain's end.  The completion waits for THIS point of the stream, not for the stream: a split-phase caller
// enqueues the next frame's grid and descriptor copies behind the chain, and they are not part of its result
int record_chain_end(asd_ctx* ctx) {
  if (!ctx->ev_chain) ASD_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_chain, hipEventDisableTiming));
  ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_chain, ctx->stream));
  return ASD_OK;
}

// A solver's result block -- pose[7], n_bad, flags, edge count -- into the caller's arrays.  kp_flags (pose_chain_lds_form): the flags
// come per keypoint with the edge count behind them; otherwise per edge, edges in keypoint order: keypoint j carries one when it held a
// map point on entry (hold) or was matched.  Fewer than 3 edges leave the pose as it started (Optimizer.cc:323-324; the kernel cleared the flags).
void unpack_solver_block(const double* h_io, int n_cur, bool kp_flags, const int32_t* match, const uint8_t* hold, const double* pose_start, double* pose,
                         uint8_t* outlier, int32_t* n_inliers) {
  int ne = 0;
  if (kp_flags) {
    ne = (int)(h_io[8 + (n_cur + 7) / 8] + 0.5);
    memcpy(outlier, h_io + 8, (size_t)n_cur);
  } else {
    auto edge = [&](int j) { return (hold && hold[j]) || match[j] >= 0; };
    for (int j = 0; j < n_cur; ++j) ne += edge(j);
    const uint8_t* flags = reinterpret_cast<const uint8_t*>(h_io + 8);
    for (int j = 0, e = 0; j < n_cur; ++j) outlier[j] = edge(j) && ne >= 3 ? flags[e++] : 0;
  }
  memcpy(pose, ne < 3 ? pose_start : h_io, 56);
  *n_inliers = ne < 3 ? 0 : ne - (int)(h_io[7] + 0.5);
}

// What the host hands a single stage (search_and_resolve copies the tables into the upload block, in the order of the fields below; a null
// table takes no room).  The search's own inputs first, then what a chain adds: the query kernel's tables and the solver's.
struct StageInputs {
  int kind = 0, nq = 0;
  const float* d_qdesc = nullptr;
  const float4* kp_last = nullptr;
  const uint8_t* obs_pos = nullptr;     // [nq] or null
  const uint8_t* occupied = nullptr;    // [n_cur] (kind 1)
  int check_ori = 0;
  float nn_ratio = 0.f;
  QuerySource source = kQueriesUploaded;   // kQueriesUploaded: m->h_queries[0..nq)
  ProjectArgs project{};                // constants (project_args / frustum_args); search_and_resolve points them at the tables
  FrustumArgs frustum{};
  bool has_solver = false;
  double pose0[7] = {}, K[4] = {};
  const float* points = nullptr;        // [n_points][3] positions the match table names, or
  int n_points = 0;
  const float* d_points = nullptr;      // ... the table on the device already
  const uint8_t* has_mp = nullptr;      // [nq] k_project_queries
  const float* own = nullptr;           // [n_cur][3] the solver's d_own
  const uint8_t* hold = nullptr;        // [n_cur] the solver's d_hold (its own copy of `occupied`)
  const float* normal = nullptr;        // [nq][3], [nq], [nq]: k_frustum_queries, with `points`
  const float* min_dist = nullptr;
  const float* max_dist = nullptr;
  const int32_t* rows = nullptr;        // [nq] bank rows of the queries' descriptors, or null: row = query index
  const int32_t* d_rows = nullptr;      // ... the same table on the device already (asd_track_local_points_map): `rows` is not uploaded then
};

// One stage behind one synchronisation: one upload block (queries, the zeroed candidate counter, flags, the chain's tables), the kernels back
// to back, one result block (match table, counters, the solver's results): a copy costs 15-25 us on this stream whatever its size
// (rocprof timeline), five of them per call were a third of the call.
// Split in two: `attempt` enqueues everything (inputs are consumed: they live in the pinned upload block from then on), `complete`
// synchronises, handles a candidate-buffer overflow (grow, enqueue again from the same description) and unpacks match_cur[n_cur] / *n_matches.
// With `defer` the caller gets `complete` back instead of having it run (asd_track_async / asd_track_finish).  *solver_io: where the
// solver's result block will be on the host.
int search_and_resolve(asd_ctx* ctx, MatcherState* m, const AsdFrameSlot& F, const StageInputs& in, int32_t* match_cur, int32_t* n_matches,
                       const double** solver_io = nullptr, std::function<int()>* defer = nullptr) {
  if (asd_track_busy(ctx, "matcher call")) return ASD_ERR_INVALID;
  static const bool timing = getenv("ASD_TIMING") != nullptr;
  static const bool tail_upload = getenv("ASD_UPLOAD_COPY") == nullptr;   // ASD_UPLOAD_COPY=1 (copy commands instead of copy kernels) makes the upload a command of its own
  const int n_cur = F.n, nq = in.nq, kind = in.kind;
  // A deferred completion (asd_track_async) runs after the caller may have rewritten bank rows and other frame slots
  // (include/asd_slam.h allows asd_bank_put* / asd_frame_set in between), so it must never have to search again: the candidate
  // buffers are sized for the worst case up front -- a query's list holds at most every keypoint of the frame -- and an
  // overflow at completion is an error, not a retry.  (16 B x nq x n_cur: 128 MB at 4000 x 2000; 288 GB of HBM make that a non-issue.)
  const bool deferred = defer != nullptr;
  int rc = ensure_cands_dev(ctx, m, deferred ? std::max((size_t)nq * (size_t)std::max(n_cur, 1), (size_t)1) : (size_t)1);
  if (rc != ASD_OK) return rc;
  hipStream_t st = ctx->stream;
  AsdXfer &up = ctx->up, &down = ctx->down;
  const size_t io_bytes = in.has_solver ? pose_chain_io_bytes(n_cur) : 0;
  ASD_HIP_CHECK(ctx, up.begin(st, (size_t)nq * (sizeof(WinQuery) + 1 + 12 + 12 + 4 + 4 + 4) + (size_t)in.n_points * 12 + (size_t)n_cur * (1 + 12 + 1) + 16 * 256));
  ASD_HIP_CHECK(ctx, down.begin(st, ((size_t)n_cur + 16) * sizeof(int) + 256 + io_bytes));
  ASD_HIP_CHECK(ctx, ctx->scratch.reserve(AsdDevBuf::padded((size_t)nq * kTop * 2)));
  // every runtime request of the chain that is not a launch happens here, before the first kernel goes out
  if ((rc = resolve2_attributes(ctx)) != ASD_OK || (in.has_solver && (rc = pose_chain_reserve(ctx, n_cur)) != ASD_OK)) return rc;

  TrackStage s{};
  s.kind = kind; s.nq = nq; s.F = &F;
  s.source = in.source;
  s.upload = in.source != kQueriesUploaded && tail_upload ? kUploadCarried : kUploadCopy;
  s.d_qdesc = in.d_qdesc; s.kp_last = in.kp_last; s.check_ori = in.check_ori; s.nn_ratio = in.nn_ratio;
  s.d_off = m->d_q_off; s.d_cnt = m->d_q_off + nq;
  s.d_top = ctx->scratch.carve<uint16_t>((size_t)nq * kTop);
  s.timed = timing;
  // the upload block: the query table first (a query kernel writes the device twin, the tail blocks copy what lies behind it)
  const size_t o_q = in.source == kQueriesUploaded ? up.add(m->h_queries, (size_t)nq * sizeof(WinQuery)) : up.reserve((size_t)nq * sizeof(WinQuery));
  const size_t o_total = up.zeros(sizeof(int));
  s.d_queries = up.dev<WinQuery>(o_q);
  s.d_total = up.dev<int>(o_total);
  if (in.obs_pos) s.d_obs_pos = up.dev<uint8_t>(up.add(in.obs_pos, nq));
  if (kind == 1) s.d_occupied = up.dev<uint8_t>(up.add(in.occupied, n_cur));
  // a query kernel that carries the upload reads its tables from the PINNED block, the kernels behind it the device twin
  const bool carried = s.upload == kUploadCarried;
  const void *q_points = nullptr, *q_has = nullptr, *q_normal = nullptr, *q_min = nullptr, *q_max = nullptr, *q_rows = nullptr;
  auto table = [&](const void* src, size_t bytes, const void** for_query) -> const void* {
    if (!src) return nullptr;
    const size_t o = up.add(src, bytes);
    if (for_query) *for_query = carried ? up.host<void>(o) : up.dev<void>(o);
    return up.dev<void>(o);
  };
  const void* d_points = table(in.points, (size_t)in.n_points * 12, &q_points);
  (void)table(in.has_mp, nq, &q_has);
  const void* d_own = table(in.own, (size_t)n_cur * 12, nullptr);
  const void* d_hold = table(in.hold, n_cur, nullptr);
  (void)table(in.normal, (size_t)nq * 12, &q_normal);
  (void)table(in.min_dist, (size_t)nq * 4, &q_min);
  (void)table(in.max_dist, (size_t)nq * 4, &q_max);
  if (in.d_rows) q_rows = in.d_rows;
  else (void)table(in.rows, (size_t)nq * 4, &q_rows);
  if (in.source == kQueriesProject) {
    s.project = in.project;
    s.project.Xw = static_cast<const float*>(q_points); s.project.has_mp = static_cast<const uint8_t*>(q_has); s.project.rows = static_cast<const int*>(q_rows);
    s.project.queries = up.dev<WinQuery>(o_q);
    s.project.up = upload_tail(up, nq, carried);
  } else if (in.source == kQueriesFrustum) {
    s.frustum = in.frustum;
    s.frustum.Xw = static_cast<const float*>(q_points); s.frustum.normal = static_cast<const float*>(q_normal);
    s.frustum.min_dist = static_cast<const float*>(q_min); s.frustum.max_dist = static_cast<const float*>(q_max);
    s.frustum.rows = static_cast<const int*>(q_rows);
    s.frustum.queries = up.dev<WinQuery>(o_q);
    s.frustum.up = upload_tail(up, nq, carried);
  }
  // the result block: results stored by the kernels straight into the pinned block
  const size_t o_out = down.reserve(((size_t)n_cur + 16) * sizeof(int));
  s.d_out = down.dev<int>(o_out); s.h_out = down.host<int>(o_out);
  s.has_solver = in.has_solver;
  if (in.has_solver) {
    StageSolver& v = s.solver;
    v.d_points = in.d_points ? in.d_points : static_cast<const float*>(d_points);
    v.d_hold = static_cast<const uint8_t*>(d_hold); v.d_own = static_cast<const float*>(d_own);
    memcpy(v.pose0, in.pose0, sizeof v.pose0); memcpy(v.K, in.K, sizeof v.K);
    v.io = down.host<double>(down.reserve(io_bytes));
    if (solver_io) *solver_io = v.io;
  }
  int* const h_total = up.host<int>(o_total);
  const int* const h_out = s.h_out;

  auto attempt = [ctx, m, s]() -> int {
    const int rc = enqueue_stage(ctx, m, s, stage_fuses(ctx, m, s));
    return rc != ASD_OK ? rc : record_chain_end(ctx);
  };

  auto complete = [=]() -> int {
    int rc;
    for (int round = 0;; ++round) {
      ASD_HIP_CHECK(ctx, hipEventSynchronize(ctx->ev_chain));
      const int total = h_out[n_cur + 1];
      m->last_total[kind] = total;
      if (total > m->cand_cap && deferred) {   // cannot happen with the worst-case sizing above; never search again over state the caller may have changed
        ctx->set_error("asd_track_finish: %d candidates overflowed the %d-entry buffers of a deferred stage", total, m->cand_cap);
        return ASD_ERR_CAPACITY;
      }
      if (total > m->cand_cap && round == 0) {  // the candidate buffers overflowed (the replay did not run): grow and search again
        if ((rc = ensure_cands_dev(ctx, m, (size_t)total)) != ASD_OK) return rc;
        *h_total = 0;
        if ((rc = attempt()) != ASD_OK) return rc;
        continue;
      }
      break;
    }
    if (timing) ASD_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->ms_match, ctx->ev0, ctx->ev1));
    else ctx->ms_match = 0.f;
    memcpy(match_cur, h_out, (size_t)n_cur * sizeof(int));
    *n_matches = h_out[n_cur];
    if (timing) {
      static double acc[2]; static long calls[2]; static long rounds[2]; static double st_us[2][8];
      acc[kind] += ctx->ms_match; rounds[kind] += h_out[n_cur + 2];
      for (int i = 0; i < 8; ++i) st_us[kind][i] += 0.01 * h_out[n_cur + 3 + i];
      if (++calls[kind] % 200 == 0)
        fprintf(stderr, "[search+resolve kind %d] device %.3f ms, %.1f iterations, %d candidates; replay: staging %.1f us, iterations %.1f us (the first %.1f; thread 0 work %.1f, barrier + verdict %.1f), outputs %.1f us\n", kind,
                acc[kind] / calls[kind], (double)rounds[kind] / calls[kind], h_out[n_cur + 1], st_us[kind][0] / calls[kind], st_us[kind][1] / calls[kind],
                st_us[kind][3] / calls[kind], st_us[kind][4] / calls[kind], st_us[kind][5] / calls[kind], st_us[kind][2] / calls[kind]);
    }
    return ASD_OK;
  };

  if ((rc = attempt()) != ASD_OK) return rc;
  if (defer) { *defer = complete; return ASD_OK; }
  return complete();
}

}  // namespace

hipError_t asd_copy_rows(hipStream_t st, void* dst, const void* src, size_t bytes) { return copy_rows(st, dst, src, bytes); }

void matcher_free(asd_ctx* ctx) {
  if (ctx->matcher && static_cast<MatcherState*>(ctx->matcher)->d_cxw) (void)hipFree(static_cast<MatcherState*>(ctx->matcher)->d_cxw);
  for (auto& f : ctx->frames) {
    if (f.d_desc) (void)hipFree(f.d_desc);
    if (f.d_fv) (void)hipFree(f.d_fv);
    f.d_fv = nullptr;
    if (f.d_kp) (void)hipFree(f.d_kp);   // one block: keypoints, cell offsets, cell items
    if (f.h_stage) (void)hipHostFree(f.h_stage);
    if (f.ev_staged) (void)hipEventDestroy(f.ev_staged);
    f.ev_staged = nullptr;
    f.d_desc = nullptr; f.d_kp = nullptr; f.d_cell_start = nullptr; f.d_cell_items = nullptr; f.h_stage = nullptr;
  }
  if (ctx->matcher) {
    MatcherState* m = static_cast<MatcherState*>(ctx->matcher);
    void* dev[] = {m->d_queries, m->d_q_off, m->d_idx, m->d_dist, m->d_qdesc, m->d_bank, m->d_attr};
    for (void* p : dev) if (p) (void)hipFree(p);
    void* host[] = {m->h_queries, m->h_q, m->h_idx, m->h_dist, m->h_qdesc, m->h_attr[0], m->h_attr[1]};
    for (void* p : host) if (p) (void)hipHostFree(p);
    for (hipEvent_t e : m->ev_attr) if (e) (void)hipEventDestroy(e);
    delete m;
    ctx->matcher = nullptr;
  }
}

extern "C" {

static int frame_set_impl(asd_ctx* ctx, int32_t slot, const asd_keypoint* kps, const float* desc, int32_t n, float min_x,
                          float max_x, float min_y, float max_y, asd_ctx* src);
int asd_frame_set(asd_ctx* ctx, int32_t slot, const asd_keypoint* kps, const float* desc, int32_t n, float min_x,
                  float max_x, float min_y, float max_y) {
  return frame_set_impl(ctx, slot, kps, desc, n, min_x, max_x, min_y, max_y, ctx);
}
// the frame's descriptors adopted from ANOTHER context's last extraction (same device): the right image of a stereo pair is extracted by
// its own context (the reference keeps two extractors) and matched inside the left one's
int asd_frame_set_from_ctx(asd_ctx* ctx, int32_t slot, const asd_keypoint* kps, int32_t n, float min_x, float max_x, float min_y, float max_y,
                           asd_ctx* src) {
  if (!ctx || !src || src->cfg.device != ctx->cfg.device) return ASD_ERR_INVALID;
  return frame_set_impl(ctx, slot, kps, nullptr, n, min_x, max_x, min_y, max_y, src);
}
static int frame_set_impl(asd_ctx* ctx, int32_t slot, const asd_keypoint* kps, const float* desc, int32_t n, float min_x,
                          float max_x, float min_y, float max_y, asd_ctx* src) {
  AsdFrameSlot* F = matcher_slot(ctx, slot);
  if (!F || n < 0 || (n > 0 && !kps) || !(max_x > min_x) || !(max_y > min_y)) return ASD_ERR_INVALID;
  if (n > ctx->cfg.max_patches) { ctx->set_error("frame has %d keypoints, capacity %d", n, ctx->cfg.max_patches); return ASD_ERR_CAPACITY; }
  if (!desc && !src->d_desc_last) { ctx->set_error("desc == NULL: no extraction has completed on the source context yet"); return ASD_ERR_INVALID; }
  if (!desc && n != src->last_n) { ctx->set_error("desc == NULL adopts the last extract (%d keypoints), got n=%d", src->last_n, n); return ASD_ERR_INVALID; }
  (void)hipSetDevice(ctx->cfg.device);
  const size_t cap = ctx->cfg.max_patches;
  if (!F->d_desc) {
    ASD_HIP_CHECK(ctx, hipMalloc(&F->d_desc, cap * 128 * sizeof(float)));
    // keypoints, cell offsets and cell items in ONE device block laid out like the pinned staging buffer: one copy per frame
    char* blk = nullptr;
    ASD_HIP_CHECK(ctx, hipMalloc(&blk, cap * (sizeof(float4) + sizeof(int)) + (GC * GR + 1) * sizeof(int) + 16));
    F->d_kp = reinterpret_cast<float4*>(blk);
    F->d_cell_start = reinterpret_cast<int32_t*>(blk + cap * sizeof(float4));
    F->d_cell_items = F->d_cell_start + (GC * GR + 1);
    ASD_HIP_CHECK(ctx, hipHostMalloc(&F->h_stage, cap * (sizeof(float4) + sizeof(int)) + (GC * GR + 1) * sizeof(int) + 16));
    ASD_HIP_CHECK(ctx, hipEventCreateWithFlags(&F->ev_staged, hipEventDisableTiming));
  } else {
    // the slot's pinned staging buffer is about to be rewritten: its previous copies (a frame or more ago) must have left it
    ASD_HIP_CHECK(ctx, hipEventSynchronize(F->ev_staged));
  }
  hipStream_t st = asd_prep_stream(ctx);
  if (n > 0) {
    if (desc) ASD_HIP_CHECK(ctx, hipMemcpyAsync(F->d_desc, desc, (size_t)n * 128 * sizeof(float), hipMemcpyHostToDevice, st));
    else ASD_HIP_CHECK(ctx, copy_rows(st, F->d_desc, src->d_desc_last, (size_t)n * 128 * sizeof(float)));
  }
  F->n = n;
  F->min_x = min_x; F->max_x = max_x; F->min_y = min_y; F->max_y = max_y;
  F->inv_w = static_cast<float>(GC) / static_cast<float>(max_x - min_x);  // Frame.cc:106-107
  F->inv_h = static_cast<float>(GR) / static_cast<float>(max_y - min_y);
  F->kps.assign(kps, kps + n);
  // AssignFeaturesToGrid (Frame.cc:123-138): stable counting sort into CSR, cell = ix*48 + iy
  std::vector<int> cell(n);
  F->cell_start.assign(GC * GR + 1, 0);
  for (int i = 0; i < n; ++i) {
    const int px = (int)std::round((kps[i].x - min_x) * F->inv_w);  // PosInGrid uses round (Frame.cc:278-279)
    const int py = (int)std::round((kps[i].y - min_y) * F->inv_h);
    if (px < 0 || px >= GC || py < 0 || py >= GR) { cell[i] = -1; continue; }
    cell[i] = px * GR + py;
    ++F->cell_start[cell[i] + 1];
  }
  for (int c = 0; c < GC * GR; ++c) F->cell_start[c + 1] += F->cell_start[c];
  F->cell_items.assign(F->cell_start[GC * GR], 0);
  std::vector<int> cur(F->cell_start.begin(), F->cell_start.end() - 1);
  for (int i = 0; i < n; ++i)
    if (cell[i] >= 0) F->cell_items[cur[cell[i]]++] = i;
  // device mirror of keypoints + grid (pinned staging, three small async copies)
  float4* hk = reinterpret_cast<float4*>(F->h_stage);
  int* hs = reinterpret_cast<int*>(F->h_stage + cap * sizeof(float4));
  int* hi = hs + (GC * GR + 1);
  for (int i = 0; i < n; ++i) {
    float ob;
    memcpy(&ob, &kps[i].octave, sizeof ob);  // octave travels as raw int bits in .z
    hk[i] = make_float4(kps[i].x, kps[i].y, ob, kps[i].angle);  // .w = angle (rotation histogram of k_resolve2)
  }
  memcpy(hs, F->cell_start.data(), (GC * GR + 1) * sizeof(int));
  if (!F->cell_items.empty()) memcpy(hi, F->cell_items.data(), F->cell_items.size() * sizeof(int));
  // one copy for the three arrays (the block up to the last cell item in use; unused keypoint rows travel along: 16 B each)
  {
    static const bool by_kernel = getenv("ASD_UPLOAD_COPY") == nullptr;   // ASD_UPLOAD_COPY=1: copy commands instead
    const size_t bytes = cap * sizeof(float4) + (GC * GR + 1 + F->cell_items.size()) * sizeof(int);
    if (by_kernel) ASD_HIP_CHECK(ctx, copy_rows(st, F->d_kp, hk, (bytes + 15) / 16 * 16));
    else ASD_HIP_CHECK(ctx, hipMemcpyAsync(F->d_kp, hk, bytes, hipMemcpyHostToDevice, st));
  }
  // desc == NULL (the per-frame path): no synchronisation -- every consumer of the slot is enqueued on this stream behind the
  // copies; ev_staged guards the slot's pinned staging buffer, ev_adopt the extraction buffer the descriptors are copied
  // out of (asd_extract_submit waits for it before the worker may reuse that buffer on its own streams).
  // desc != NULL: the caller's buffer is ordinary host memory and may be freed or rewritten as soon as we return.
  ASD_HIP_CHECK(ctx, hipEventRecord(F->ev_staged, st));
  if (!desc && n > 0) {   // (the SOURCE context's extractor must not reuse that buffer before the copy has left it)
    if (!src->ev_adopt) ASD_HIP_CHECK(ctx, hipEventCreateWithFlags(&src->ev_adopt, hipEventDisableTiming));
    ASD_HIP_CHECK(ctx, hipEventRecord(src->ev_adopt, st));
    src->adopt_pending = true;
  } else {
    ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  return ASD_OK;
}

int asd_dist_matrix(asd_ctx* ctx, const float* a, int32_t na, const float* b, int32_t nb, float* out) {
  if (!ctx || na < 0 || nb < 0 || ((na > 0 && nb > 0) && (!a || !b || !out))) return ASD_ERR_INVALID;
  if (na == 0 || nb == 0) return ASD_OK;
  if (asd_track_busy(ctx, "asd_dist_matrix")) return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  float *da = nullptr, *db = nullptr, *dout = nullptr;
  hipStream_t st = ctx->stream;
  ASD_HIP_CHECK(ctx, ctx->scratch.reserve(AsdDevBuf::padded((size_t)na * 512) + AsdDevBuf::padded((size_t)nb * 512) +
                                          AsdDevBuf::padded((size_t)na * nb * sizeof(float))));
  da = ctx->scratch.carve<float>((size_t)na * 128);
  db = ctx->scratch.carve<float>((size_t)nb * 128);
  dout = ctx->scratch.carve<float>((size_t)na * nb);
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(da, a, (size_t)na * 512, hipMemcpyHostToDevice, st));
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(db, b, (size_t)nb * 512, hipMemcpyHostToDevice, st));
  ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, st));
  hipLaunchKernelGGL(k_dist_matrix, dim3((nb + 255) / 256, (na + 15) / 16), dim3(256), 0, st, da, na, db, nb, dout);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, st));
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(out, dout, (size_t)na * nb * sizeof(float), hipMemcpyDeviceToHost, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  ASD_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->ms_match, ctx->ev0, ctx->ev1));
  return ASD_OK;
}

int asd_distinctive_descriptor(asd_ctx* ctx, const float* desc, int32_t n, int32_t* best_idx) {
  if (!ctx || !desc || !best_idx || n < 1) return ASD_ERR_INVALID;
  std::vector<float> D((size_t)n * n);
  int rc = asd_dist_matrix(ctx, desc, n, desc, n, D.data());
  if (rc != ASD_OK) return rc;
  // MapPoint.cc:305-331: the reference fills the upper triangle and mirrors it; (a-b)^2 == (b-a)^2
  // term by term, so the full matrix is already symmetric bit for bit.  Diagonal = 0.
  float best_median = 100;
  int best = 0;
  std::vector<float> row(n);
  for (int i = 0; i < n; ++i) {
    std::copy(D.begin() + (size_t)i * n, D.begin() + (size_t)(i + 1) * n, row.begin());
    row[i] = 0;
    std::sort(row.begin(), row.end());
    const float median = row[(size_t)(0.5 * (n - 1))];
    if (median < best_median) { best_median = median; best = i; }
  }
  *best_idx = best;
  return ASD_OK;
}

int asd_distinctive_descriptor_batch(asd_ctx* ctx, int32_t n_sets, const int32_t* set_start, const float* desc, int32_t* best_idx) {
  if (!ctx || n_sets < 0 || (n_sets > 0 && (!set_start || !desc || !best_idx))) return ASD_ERR_INVALID;
  if (n_sets == 0) return ASD_OK;
  if (set_start[0] != 0) { ctx->set_error("asd_distinctive_descriptor_batch: set_start[0] must be 0"); return ASD_ERR_INVALID; }
  bool any_big = false;
  for (int s = 0; s < n_sets; ++s) {
    const int n = set_start[s + 1] - set_start[s];
    if (n < 1) { ctx->set_error("asd_distinctive_descriptor_batch: set %d is empty", s); return ASD_ERR_INVALID; }
    any_big |= n > kDistinctMax;
  }
  (void)hipSetDevice(ctx->cfg.device);
  hipStream_t st = ctx->stream;
  const int total = set_start[n_sets];
  hipError_t e = ctx->scratch.reserve(AsdDevBuf::padded((size_t)total * 512) + 2 * AsdDevBuf::padded((size_t)(n_sets + 1) * sizeof(int)));
  float* dd = ctx->scratch.carve<float>((size_t)total * 128);
  int* ds = ctx->scratch.carve<int>((size_t)n_sets + 1);
  int* db = ctx->scratch.carve<int>((size_t)n_sets + 1);
  if (e == hipSuccess) e = hipMemcpyAsync(dd, desc, (size_t)total * 512, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(ds, set_start, (size_t)(n_sets + 1) * sizeof(int), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(db, 0, (size_t)n_sets * sizeof(int), st);
  if (e == hipSuccess) {
    static AsdPerDeviceOnce attr;
    const size_t lds = (size_t)(kDistinctMax * 132 + kDistinctMax * (kDistinctMax + 1) + kDistinctMax) * sizeof(float);
    if (attr.need(ctx->cfg.device)) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_distinctive), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); attr.done(ctx->cfg.device); }
    // one launch per run of map points that fit a workgroup (normally a single launch over all of them)
    for (int s = 0; s < n_sets;) {
      if (set_start[s + 1] - set_start[s] > kDistinctMax) { ++s; continue; }
      int r = s;
      while (r < n_sets && set_start[r + 1] - set_start[r] <= kDistinctMax) ++r;
      hipLaunchKernelGGL(k_distinctive, dim3(r - s), dim3(256), lds, st, dd, ds + s, db + s);
      s = r;
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(best_idx, db, (size_t)n_sets * sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { ctx->set_error("asd_distinctive_descriptor_batch: %s", hipGetErrorString(e)); return ASD_ERR_HIP; }
  if (any_big)  // map points with more observations than one workgroup stages: through the all-pairs kernel, one by one
    for (int s = 0; s < n_sets; ++s) {
      const int n = set_start[s + 1] - set_start[s];
      if (n <= kDistinctMax) continue;
      const int rc = asd_distinctive_descriptor(ctx, desc + (size_t)set_start[s] * 128, n, best_idx + s);
      if (rc != ASD_OK) return rc;
    }
  return ASD_OK;
}

}  // extern "C"

// mp_desc: host table indexed like the last frame's keypoints, or NULL with mp_rows = bank rows
static int match_project_frame_impl(asd_ctx* ctx, int32_t slot_cur, int32_t slot_last, const uint8_t* has_mp, const float* Xw,
                            const float* mp_desc, const int32_t* mp_rows, const float* Tcw, const float* K, float th,
                            int32_t check_orientation, int32_t* match_cur, int32_t* n_matches, const uint8_t* obs_pos,
                            StageInputs* chain = nullptr, const double** solver_io = nullptr, std::function<int()>* defer = nullptr) {
  // chain: what asd_track_motion_model adds to the stage (query kernel, solver); *solver_io stays null when the stage was not chained --
  // nothing to search, or the replay ran on the host
  AsdFrameSlot *C = matcher_slot(ctx, slot_cur), *L = matcher_slot(ctx, slot_last);
  if (!C || !L || !has_mp || !Xw || (!mp_desc && !mp_rows) || !Tcw || !K || !match_cur || !n_matches) return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  std::fill(match_cur, match_cur + C->n, -1);
  *n_matches = 0;
  if (L->n == 0 || C->n == 0) return ASD_OK;
  int rc = matcher_ensure_queries(ctx, m, L->n);
  if (rc != ASD_OK) return rc;
  if (mp_desc) { if ((rc = matcher_upload_qdesc(ctx, m, mp_desc, L->n)) != ASD_OK) return rc; }
  else if ((rc = matcher_check_bank_rows(ctx, m, mp_rows, has_mp, L->n, false)) != ASD_OK) return rc;
  const auto tm0 = std::chrono::steady_clock::now();
  const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  const bool on_device = replay_on_device(m, 0, C->n, L->n);
  auto project = [&](int i, WinQuery& Q) {  // projection, ORBmatcher.cc:1343-1368
    if (!has_mp[i]) return;
    float Xc[3];
    matcher_transform(Tcw, Xw + 3 * i, Xc);
    const float invzc = 1.0 / Xc[2];  // double division, rounded to float (:1352)
    if (invzc < 0) return;
    const float u = fx * Xc[0] * invzc + cx;
    const float v = fy * Xc[1] * invzc + cy;
    if (u < C->min_x || u > C->max_x) return;
    if (v < C->min_y || v > C->max_y) return;
    const int oct = L->kps[i].octave;
    Q = WinQuery{u, v, th * ctx->scale[oct], oct - 1, oct + 1, mp_desc ? i : mp_rows[i]};
  };
  // (on the device with a chain's query kernel: k_project_queries writes them there, asd_track_motion_model)
  if (!(on_device && chain && chain->source == kQueriesProject) && (rc = matcher_fill_queries(ctx, m, L->n, project)) != ASD_OK) return rc;
  if (on_device)   // search + claims + rotation histogram on the device, one synchronisation, 4 B per keypoint back
  {
    StageInputs plain;
    StageInputs& in = chain ? *chain : plain;
    in.kind = 0; in.nq = L->n;
    in.d_qdesc = mp_desc ? m->d_qdesc : m->d_bank; in.kp_last = L->d_kp;
    in.obs_pos = obs_pos; in.check_ori = check_orientation;
    return search_and_resolve(ctx, m, *C, in, match_cur, n_matches, solver_io, defer);
  }
  return matcher_replay_frame(ctx, m, *C, *L, mp_desc ? m->d_qdesc : m->d_bank, obs_pos, check_orientation, match_cur, n_matches, tm0);
}

static int match_project_points_impl(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const uint8_t* in_view, const float* proj,
                             const int32_t* level, const float* view_cos, const float* desc, const int32_t* rows,
                             const uint8_t* occupied, float th, float nn_ratio, int32_t* match_cur, int32_t* n_matches,
                             const uint8_t* obs_pos, StageInputs* chain = nullptr, const double** solver_io = nullptr, std::function<int()>* defer = nullptr) {
  AsdFrameSlot* F = matcher_slot(ctx, slot_cur);
  if (!F || n_mp < 0 || !match_cur || !n_matches || (n_mp > 0 && (!in_view || !proj || !level || !view_cos || (!desc && !rows))) ||
      (F->n > 0 && !occupied))
    return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  std::fill(match_cur, match_cur + F->n, -1);
  *n_matches = 0;
  if (n_mp == 0 || F->n == 0) return ASD_OK;
  const bool bFactor = th != 1.0;
  int bad = ASD_OK;   // the first map point the table cannot take ends the call
  int rc = matcher_fill_queries(ctx, m, n_mp, [&](int q, WinQuery& Q) {
    if (bad != ASD_OK || !in_view[q]) return;
    const int lvl = level[q];
    if (lvl < 0 || lvl >= ctx->cfg.n_levels) { ctx->set_error("map point %d: level %d out of range", q, lvl); bad = ASD_ERR_INVALID; return; }
    float r = view_cos[q] > 0.998 ? 2.5f : 4.0f;  // RadiusByViewingCos (:126-132)
    if (bFactor) r *= th;
    if (!desc && (bad = matcher_check_bank_rows(ctx, m, rows + q, nullptr, 1, false)) != ASD_OK) return;
    Q = WinQuery{proj[2 * q], proj[2 * q + 1], r * ctx->scale[lvl], lvl - 1, lvl, desc ? q : rows[q]};
  });
  if (rc != ASD_OK || (rc = bad) != ASD_OK) return rc;
  if (desc && (rc = matcher_upload_qdesc(ctx, m, desc, n_mp)) != ASD_OK) return rc;
  if (replay_on_device(m, 1, F->n, n_mp)) {
    StageInputs plain;
    StageInputs& in = chain ? *chain : plain;
    in.kind = 1; in.nq = n_mp;
    in.d_qdesc = desc ? m->d_qdesc : m->d_bank;
    in.obs_pos = obs_pos; in.occupied = occupied; in.nn_ratio = nn_ratio;
    return search_and_resolve(ctx, m, *F, in, match_cur, n_matches, solver_io, defer);
  }
  return matcher_replay_points(ctx, m, *F, n_mp, desc ? m->d_qdesc : m->d_bank, occupied, obs_pos, nn_ratio, match_cur, n_matches);
}

extern "C" {

int asd_match_project_frame(asd_ctx* ctx, int32_t slot_cur, int32_t slot_last, const uint8_t* has_mp, const float* Xw,
                            const float* mp_desc, const float* Tcw, const float* K, float th,
                            int32_t check_orientation, int32_t* match_cur, int32_t* n_matches, const uint8_t* mp_obs_positive) {
  if (!mp_desc) return ASD_ERR_INVALID;
  return match_project_frame_impl(ctx, slot_cur, slot_last, has_mp, Xw, mp_desc, nullptr, Tcw, K, th, check_orientation, match_cur, n_matches, mp_obs_positive);
}

int asd_match_project_frame_bank(asd_ctx* ctx, int32_t slot_cur, int32_t slot_last, const uint8_t* has_mp, const float* Xw,
                                 const int32_t* mp_rows, const float* Tcw, const float* K, float th,
                                 int32_t check_orientation, int32_t* match_cur, int32_t* n_matches, const uint8_t* mp_obs_positive) {
  if (!mp_rows) return ASD_ERR_INVALID;
  return match_project_frame_impl(ctx, slot_cur, slot_last, has_mp, Xw, nullptr, mp_rows, Tcw, K, th, check_orientation, match_cur, n_matches, mp_obs_positive);
}

int asd_match_project_points(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const uint8_t* in_view, const float* proj,
                             const int32_t* level, const float* view_cos, const float* desc, const uint8_t* occupied,
                             float th, float nn_ratio, int32_t* match_cur, int32_t* n_matches, const uint8_t* mp_obs_positive) {
  if (n_mp > 0 && !desc) return ASD_ERR_INVALID;
  return match_project_points_impl(ctx, slot_cur, n_mp, in_view, proj, level, view_cos, desc, nullptr, occupied, th, nn_ratio, match_cur, n_matches, mp_obs_positive);
}

int asd_match_project_points_bank(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const uint8_t* in_view, const float* proj,
                                  const int32_t* level, const float* view_cos, const int32_t* rows, const uint8_t* occupied,
                                  float th, float nn_ratio, int32_t* match_cur, int32_t* n_matches, const uint8_t* mp_obs_positive) {
  if (n_mp > 0 && !rows) return ASD_ERR_INVALID;
  return match_project_points_impl(ctx, slot_cur, n_mp, in_view, proj, level, view_cos, nullptr, rows, occupied, th, nn_ratio, match_cur, n_matches, mp_obs_positive);
}

// ---- fused tracking chains -------------------------------------------------------------------------------------------
// The numeric bodies of Tracking::TrackWithMotionModel (Tracking.cc:664-723: SearchByProjection(cur, last) then
// Optimizer::PoseOptimization) and Tracking::TrackLocalMap (:725-736 with SearchLocalPoints' matcher call, :803-851) as ONE
// submission each: search, claim replay, edge assembly and the pose solver are enqueued back to back on the context's stream
// and the host synchronises once, instead of search -> host -> solver with two round trips.  Same kernels, same edge order
// (keypoint order, Optimizer.cc:281) as the separate calls, so the results are the same bits (tests/test_track_chain.py).
// Every chain entry point has one shape: fill the stage's inputs (StageInputs: copied into the upload block when the stage is enqueued, so
// that it can be enqueued again after a candidate overflow), call search_and_resolve, complete (finish_chain).
namespace {
// the solver's part of a chain's stage inputs
void chain_solver_inputs(StageInputs* in, const double* pose7, const float* K) {
  in->has_solver = true;
  memcpy(in->pose0, pose7, sizeof in->pose0);
  for (int i = 0; i < 4; ++i) in->K[i] = (double)K[i];
}
// The stage was not chained (nothing to search, or the matches were replayed on the host: ASD_MATCH_REPLAY=host, very large inputs): the
// whole PoseOptimization through the separate entry point.  Runs inside the call, so it may read the caller's tables: keypoint j's point is
// own[j] where hold[j], else points[match_cur[j]].
int pose_optimize_host_matches(asd_ctx* ctx, const AsdFrameSlot& C, const int32_t* match_cur, const float* points, const uint8_t* hold, const float* own,
                               const double* K, double* pose7, uint8_t* outlier, int32_t* n_inliers) {
  const int n_cur = C.n;
  auto point_of = [&](int j) -> const float* { return hold && hold[j] ? own + 3 * (size_t)j : (match_cur[j] >= 0 ? points + 3 * (size_t)match_cur[j] : nullptr); };
  std::vector<int> kp_of_edge;
  for (int j = 0; j < n_cur; ++j) { outlier[j] = 0; if (point_of(j)) kp_of_edge.push_back(j); }
  const int ne = (int)kp_of_edge.size();
  *n_inliers = 0;
  if (ne < 3) return ASD_OK;   // Optimizer.cc:323-324
  std::vector<double> Xd((size_t)3 * ne), obs((size_t)2 * ne), info(ne);
  std::vector<uint8_t> out(ne);
  for (int e = 0; e < ne; ++e) {
    const int jk = kp_of_edge[e];
    const float* X = point_of(jk);
    for (int k = 0; k < 3; ++k) Xd[3 * e + k] = (double)X[k];
    obs[2 * e] = (double)C.kps[jk].x; obs[2 * e + 1] = (double)C.kps[jk].y;
    info[e] = (double)ctx->inv_sigma2[C.kps[jk].octave];
  }
  const int rc = asd_pose_optimize(ctx, pose7, ne, Xd.data(), obs.data(), info.data(), K, out.data(), n_inliers);
  if (rc != ASD_OK) return rc;
  for (int e = 0; e < ne; ++e) outlier[kp_of_edge[e]] = out[e];
  return ASD_OK;
}
// Completes a chained stage -- the search's completion, then the solver's block into the caller's arrays -- or hands the completion to the
// caller (`defer`, asd_track_async).  The completion reads the caller's OUTPUT arrays and, of the inputs, only copies made here: the start
// pose and, where the flags come back per edge, the `hold` flags.
int finish_chain(asd_ctx* ctx, const AsdFrameSlot& F, const StageInputs& in, const std::function<int()>& search_done, const double* h_io, double* pose7,
                 int32_t* match_cur, uint8_t* outlier, int32_t* n_inliers, std::function<int()>* defer) {
  const int n_cur = F.n;
  const bool kp_flags = pose_chain_lds_form(ctx, n_cur);
  std::array<double, 7> p0;
  memcpy(p0.data(), in.pose0, sizeof in.pose0);
  std::shared_ptr<std::vector<uint8_t>> hold;
  if (in.hold && !kp_flags) hold = std::make_shared<std::vector<uint8_t>>(in.hold, in.hold + n_cur);
  auto fin = [=]() -> int {
    if (search_done) { const int r = search_done(); if (r != ASD_OK) return r; }
    unpack_solver_block(h_io, n_cur, kp_flags, match_cur, hold ? hold->data() : nullptr, p0.data(), pose7, outlier, n_inliers);
    return ASD_OK;
  };
  if (defer && search_done) { *defer = fin; return ASD_OK; }
  return fin();
}

int track_motion_model_impl(asd_ctx* ctx, int32_t slot_cur, int32_t slot_last, const uint8_t* has_mp, const float* Xw, const float* mp_desc,
                            const int32_t* mp_rows, const float* Tcw, const float* K, float th, int32_t check_orientation,
                            const uint8_t* mp_obs_positive, double* pose7, int32_t* match_cur, int32_t* n_matches, uint8_t* outlier,
                            int32_t* n_inliers, std::function<int()>* defer) {
  AsdFrameSlot *C = matcher_slot(ctx, slot_cur), *L = matcher_slot(ctx, slot_last);
  if (!C || !L || !pose7 || !outlier || !n_inliers || !K) return ASD_ERR_INVALID;
  StageInputs in;
  chain_solver_inputs(&in, pose7, K);
  in.points = Xw; in.n_points = L->n;
  if (has_mp && Xw && Tcw && L->n > 0) {   // the projection loop on the device too (2000 points: ~45 us of host time otherwise)
    in.source = kQueriesProject;
    in.project = project_args(ctx, *C, *L, Tcw, K, th);
    in.has_mp = has_mp; in.rows = mp_rows;
  }
  const double* h_io = nullptr;
  std::function<int()> search_done;
  const int rc = match_project_frame_impl(ctx, slot_cur, slot_last, has_mp, Xw, mp_desc, mp_rows, Tcw, K, th, check_orientation, match_cur, n_matches,
                                          mp_obs_positive, &in, &h_io, defer ? &search_done : nullptr);
  if (rc != ASD_OK) return rc;
  if (!h_io) return pose_optimize_host_matches(ctx, *C, match_cur, Xw, nullptr, nullptr, in.K, pose7, outlier, n_inliers);
  return finish_chain(ctx, *C, in, search_done, h_io, pose7, match_cur, outlier, n_inliers, defer);
}

int track_local_map_impl(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const uint8_t* in_view, const float* proj, const int32_t* level,
                         const float* view_cos, const float* desc, const int32_t* rows, const float* mp_Xw, const uint8_t* occupied,
                         const float* cur_Xw, float th, float nn_ratio, const uint8_t* mp_obs_positive, const float* K, double* pose7,
                         int32_t* match_cur, int32_t* n_matches, uint8_t* outlier, int32_t* n_inliers, std::function<int()>* defer) {
  AsdFrameSlot* F = matcher_slot(ctx, slot_cur);
  if (!F || !pose7 || !outlier || !n_inliers || !K || (n_mp > 0 && !mp_Xw) || (F->n > 0 && (!occupied || !cur_Xw))) return ASD_ERR_INVALID;
  StageInputs in;
  chain_solver_inputs(&in, pose7, K);
  in.points = mp_Xw; in.n_points = n_mp;
  in.own = cur_Xw; in.hold = occupied;
  const double* h_io = nullptr;
  std::function<int()> search_done;
  const int rc = match_project_points_impl(ctx, slot_cur, n_mp, in_view, proj, level, view_cos, desc, rows, occupied, th, nn_ratio, match_cur, n_matches,
                                           mp_obs_positive, &in, &h_io, defer ? &search_done : nullptr);
  if (rc != ASD_OK) return rc;
  if (!h_io) return pose_optimize_host_matches(ctx, *F, match_cur, mp_Xw, occupied, cur_Xw, in.K, pose7, outlier, n_inliers);
  return finish_chain(ctx, *F, in, search_done, h_io, pose7, match_cur, outlier, n_inliers, defer);
}

// Tracking::SearchLocalPoints (Tracking.cc:803-851: isInFrustum for every local map point, then SearchByProjection) +
// Optimizer::PoseOptimization = Tracking::TrackLocalMap's numeric body (:725-736) with the frustum test and the search windows
// made on the device too: the host uploads the map points (position, normal, distance bounds) and gets matches and pose back.
int track_local_points_impl(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const float* Xw, const float* normal, const float* min_dist,
                            const float* max_dist, const float* desc, const int32_t* rows, const float* Tcw, const float* K, float cos_limit,
                            const uint8_t* occupied, const float* cur_Xw, float th, float nn_ratio, const uint8_t* mp_obs_positive,
                            double* pose7, int32_t* match_cur, int32_t* n_matches, uint8_t* outlier, int32_t* n_inliers,
                            std::function<int()>* defer) {
  AsdFrameSlot* F = matcher_slot(ctx, slot_cur);
  if (!F || n_mp < 0 || !Tcw || !K || !pose7 || !match_cur || !n_matches || !outlier || !n_inliers ||
      (n_mp > 0 && (!Xw || !normal || !min_dist || !max_dist || (!desc && !rows))) || (F->n > 0 && (!occupied || !cur_Xw)))
    return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  if (n_mp == 0 || F->n == 0 || !replay_on_device(m, 1, F->n, n_mp)) {
    // host frustum + the chain on its outputs (also the fallback for very large maps)
    std::vector<uint8_t> in_view(std::max(n_mp, 1));
    std::vector<float> proj((size_t)2 * std::max(n_mp, 1)), vc(std::max(n_mp, 1));
    std::vector<int32_t> level(std::max(n_mp, 1));
    int rc = asd_frustum(ctx, slot_cur, n_mp, Xw, normal, min_dist, max_dist, Tcw, K, cos_limit, in_view.data(), proj.data(), level.data(), vc.data());
    if (rc != ASD_OK) return rc;
    return track_local_map_impl(ctx, slot_cur, n_mp, in_view.data(), proj.data(), level.data(), vc.data(), desc, rows, Xw, occupied, cur_Xw, th,
                                nn_ratio, mp_obs_positive, K, pose7, match_cur, n_matches, outlier, n_inliers, defer);
  }
  std::fill(match_cur, match_cur + F->n, -1);
  *n_matches = 0;
  int rc = matcher_ensure_queries(ctx, m, n_mp);
  if (rc != ASD_OK) return rc;
  if (!desc && (rc = matcher_check_bank_rows(ctx, m, rows, nullptr, n_mp, false)) != ASD_OK) return rc;
  if (desc && (rc = matcher_upload_qdesc(ctx, m, desc, n_mp)) != ASD_OK) return rc;
  StageInputs in;
  in.kind = 1; in.nq = n_mp;
  in.d_qdesc = desc ? m->d_qdesc : m->d_bank;
  in.obs_pos = mp_obs_positive; in.occupied = occupied; in.nn_ratio = nn_ratio;
  in.source = kQueriesFrustum;
  in.frustum = frustum_args(ctx, *F, n_mp, Tcw, nullptr, K, cos_limit, th);
  chain_solver_inputs(&in, pose7, K);
  in.points = Xw; in.n_points = n_mp;
  in.own = cur_Xw; in.hold = occupied;
  in.normal = normal; in.min_dist = min_dist; in.max_dist = max_dist;
  in.rows = desc ? nullptr : rows;
  const double* h_io = nullptr;
  std::function<int()> search_done;
  if ((rc = search_and_resolve(ctx, m, *F, in, match_cur, n_matches, &h_io, defer ? &search_done : nullptr)) != ASD_OK) return rc;
  return finish_chain(ctx, *F, in, search_done, h_io, pose7, match_cur, outlier, n_inliers, defer);
}

// The same with the map points named by ROW of the banks (descriptor bank: MapPoint::mDescriptor, attribute bank: position, normal, distance
// range -- asd_bank_put*, asd_mpbank_put): what the host uploads per candidate shrinks from 36 bytes (position, normal, distances, row) to 4,
// and it gathers nothing.  Same kernels as asd_track_frame's local-map stage (k_frustum_queries' bank form), same results as
// asd_track_local_points_bank given the same attributes.
int track_local_points_rows_impl(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const int32_t* rows, const float* Tcw, const float* K, float cos_limit,
                                 const uint8_t* occupied, const float* cur_Xw, float th, float nn_ratio, const uint8_t* mp_obs_positive,
                                 double* pose7, int32_t* match_cur, int32_t* n_matches, uint8_t* outlier, int32_t* n_inliers, std::function<int()>* defer,
                                 const int32_t* d_rows = nullptr) {
  AsdFrameSlot* F = matcher_slot(ctx, slot_cur);
  if (!F || n_mp < 1 || !rows || !Tcw || !K || !pose7 || !match_cur || !n_matches || !outlier || !n_inliers || F->n < 1 || !occupied || !cur_Xw) return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  if (!replay_on_device(m, 1, F->n, n_mp)) {
    ctx->set_error("asd_track_local_points_rows: %d map points / %d keypoints are outside the device replay (use asd_track_local_points_bank)", n_mp, F->n);
    return ASD_ERR_CAPACITY;
  }
  int rc = matcher_check_bank_rows(ctx, m, rows, nullptr, n_mp, true);
  if (rc != ASD_OK) return rc;
  std::fill(match_cur, match_cur + F->n, -1);
  *n_matches = 0;
  if ((rc = matcher_ensure_queries(ctx, m, n_mp)) != ASD_OK) return rc;
  if (m->cxw_cap < (size_t)n_mp * 3) {
    if (m->d_cxw) { ASD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(m->d_cxw); m->d_cxw = nullptr; m->cxw_cap = 0; }
    const size_t want = (size_t)n_mp * 3 + (size_t)n_mp / 2 * 3 + 3072;
    ASD_HIP_CHECK(ctx, hipMalloc(&m->d_cxw, want * sizeof(float)));
    m->cxw_cap = want;
  }
  StageInputs in;
  in.kind = 1; in.nq = n_mp;
  in.d_qdesc = m->d_bank;
  in.obs_pos = mp_obs_positive; in.occupied = occupied; in.nn_ratio = nn_ratio;
  in.source = kQueriesFrustum;
  in.frustum = frustum_args(ctx, *F, n_mp, Tcw, nullptr, K, cos_limit, th);
  in.frustum.attr = m->d_attr; in.frustum.xw_out = m->d_cxw;   // the bank form: positions are read from the attribute bank and written out for the solver
  chain_solver_inputs(&in, pose7, K);
  in.d_points = m->d_cxw;
  in.own = cur_Xw; in.hold = occupied;
  in.rows = rows; in.d_rows = d_rows;
  const double* h_io = nullptr;
  std::function<int()> search_done;
  if ((rc = search_and_resolve(ctx, m, *F, in, match_cur, n_matches, &h_io, defer ? &search_done : nullptr)) != ASD_OK) return rc;
  return finish_chain(ctx, *F, in, search_done, h_io, pose7, match_cur, outlier, n_inliers, defer);
}

// asd_track_async / asd_track_finish: run an asd_track_* entry point split in two
extern "C++" {
template <typename Impl>
int run_track(asd_ctx* ctx, Impl&& impl) {
  if (!ctx) return ASD_ERR_INVALID;
  if (asd_track_busy(ctx, "asd_track_*")) return ASD_ERR_INVALID;
  const bool async = ctx->track_async_armed;
  ctx->track_async_armed = false;
  std::function<int()> fin;
  const int rc = impl(async ? &fin : nullptr);
  if (!async || rc != ASD_OK) return rc;
  ctx->track_pending = fin ? std::move(fin) : std::function<int()>([] { return (int)ASD_OK; });   // finished on the host already
  ctx->track_has_pending = true;
  return ASD_OK;
}
}  // extern "C++"
}  // namespace

int asd_track_motion_model(asd_ctx* ctx, int32_t slot_cur, int32_t slot_last, const uint8_t* has_mp, const float* Xw, const float* mp_desc,
                           const float* Tcw, const float* K, float th, int32_t check_orientation, const uint8_t* mp_obs_positive, double* pose7,
                           int32_t* match_cur, int32_t* n_matches, uint8_t* outlier, int32_t* n_inliers) {
  if (!mp_desc) return ASD_ERR_INVALID;
  return run_track(ctx, [&](std::function<int()>* defer) {
    return track_motion_model_impl(ctx, slot_cur, slot_last, has_mp, Xw, mp_desc, nullptr, Tcw, K, th, check_orientation, mp_obs_positive, pose7,
                                   match_cur, n_matches, outlier, n_inliers, defer); });
}
int asd_track_motion_model_bank(asd_ctx* ctx, int32_t slot_cur, int32_t slot_last, const uint8_t* has_mp, const float* Xw, const int32_t* mp_rows,
                                const float* Tcw, const float* K, float th, int32_t check_orientation, const uint8_t* mp_obs_positive,
                                double* pose7, int32_t* match_cur, int32_t* n_matches, uint8_t* outlier, int32_t* n_inliers) {
  if (!mp_rows) return ASD_ERR_INVALID;
  return run_track(ctx, [&](std::function<int()>* defer) {
    return track_motion_model_impl(ctx, slot_cur, slot_last, has_mp, Xw, nullptr, mp_rows, Tcw, K, th, check_orientation, mp_obs_positive, pose7,
                                   match_cur, n_matches, outlier, n_inliers, defer); });
}
int asd_track_local_map(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const uint8_t* in_view, const float* proj, const int32_t* level,
                        const float* view_cos, const float* desc, const float* mp_Xw, const uint8_t* occupied, const float* cur_Xw, float th,
                        float nn_ratio, const uint8_t* mp_obs_positive, const float* K, double* pose7, int32_t* match_cur, int32_t* n_matches,
                        uint8_t* outlier, int32_t* n_inliers) {
  if (n_mp > 0 && !desc) return ASD_ERR_INVALID;
  return run_track(ctx, [&](std::function<int()>* defer) {
    return track_local_map_impl(ctx, slot_cur, n_mp, in_view, proj, level, view_cos, desc, nullptr, mp_Xw, occupied, cur_Xw, th, nn_ratio,
                                mp_obs_positive, K, pose7, match_cur, n_matches, outlier, n_inliers, defer); });
}
int asd_track_local_map_bank(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const uint8_t* in_view, const float* proj, const int32_t* level,
                             const float* view_cos, const int32_t* rows, const float* mp_Xw, const uint8_t* occupied, const float* cur_Xw,
                             float th, float nn_ratio, const uint8_t* mp_obs_positive, const float* K, double* pose7, int32_t* match_cur,
                             int32_t* n_matches, uint8_t* outlier, int32_t* n_inliers) {
  if (n_mp > 0 && !rows) return ASD_ERR_INVALID;
  return run_track(ctx, [&](std::function<int()>* defer) {
    return track_local_map_impl(ctx, slot_cur, n_mp, in_view, proj, level, view_cos, nullptr, rows, mp_Xw, occupied, cur_Xw, th, nn_ratio,
                                mp_obs_positive, K, pose7, match_cur, n_matches, outlier, n_inliers, defer); });
}
int asd_track_local_points(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const float* Xw, const float* normal, const float* min_dist,
                           const float* max_dist, const float* desc, const float* Tcw, const float* K, float viewing_cos_limit,
                           const uint8_t* occupied, const float* cur_Xw, float th, float nn_ratio, const uint8_t* mp_obs_positive, double* pose7,
                           int32_t* match_cur, int32_t* n_matches, uint8_t* outlier, int32_t* n_inliers) {
  if (n_mp > 0 && !desc) return ASD_ERR_INVALID;
  return run_track(ctx, [&](std::function<int()>* defer) {
    return track_local_points_impl(ctx, slot_cur, n_mp, Xw, normal, min_dist, max_dist, desc, nullptr, Tcw, K, viewing_cos_limit, occupied, cur_Xw, th,
                                   nn_ratio, mp_obs_positive, pose7, match_cur, n_matches, outlier, n_inliers, defer); });
}
int asd_track_local_points_bank(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const float* Xw, const float* normal, const float* min_dist,
                                const float* max_dist, const int32_t* rows, const float* Tcw, const float* K, float viewing_cos_limit,
                                const uint8_t* occupied, const float* cur_Xw, float th, float nn_ratio, const uint8_t* mp_obs_positive,
                                double* pose7, int32_t* match_cur, int32_t* n_matches, uint8_t* outlier, int32_t* n_inliers) {
  if (n_mp > 0 && !rows) return ASD_ERR_INVALID;
  return run_track(ctx, [&](std::function<int()>* defer) {
    return track_local_points_impl(ctx, slot_cur, n_mp, Xw, normal, min_dist, max_dist, nullptr, rows, Tcw, K, viewing_cos_limit, occupied, cur_Xw, th,
                                   nn_ratio, mp_obs_positive, pose7, match_cur, n_matches, outlier, n_inliers, defer); });

}

int asd_track_local_points_rows(asd_ctx* ctx, int32_t slot_cur, int32_t n_mp, const int32_t* rows, const float* Tcw, const float* K, float viewing_cos_limit,
                                const uint8_t* occupied, const float* cur_Xw, float th, float nn_ratio, const uint8_t* mp_obs_positive,
                                double* pose7, int32_t* match_cur, int32_t* n_matches, uint8_t* outlier, int32_t* n_inliers) {
  return run_track(ctx, [&](std::function<int()>* defer) {
    return track_local_points_rows_impl(ctx, slot_cur, n_mp, rows, Tcw, K, viewing_cos_limit, occupied, cur_Xw, th, nn_ratio, mp_obs_positive, pose7, match_cur,
                                        n_matches, outlier, n_inliers, defer); });
}

// asd_track_local_points_rows over the search list that the last asd_update_local_map left on the device (localmap.hip): the same stage from
// the same description, with the row table already where k_frustum_queries reads it -- nothing per candidate is uploaded
int asd_track_local_points_map(asd_ctx* ctx, int32_t slot_cur, const float* Tcw, const float* K, float viewing_cos_limit, const uint8_t* occupied,
                               const float* cur_Xw, float th, float nn_ratio, const uint8_t* mp_obs_positive, double* pose7, int32_t* match_cur,
                               int32_t* n_matches, uint8_t* outlier, int32_t* n_inliers) {
  return run_track(ctx, [&](std::function<int()>* defer) {
    const int32_t *h_rows = nullptr, *d_rows = nullptr;
    int n_mp = 0;
    const int rc = localmap_search_list(ctx, "asd_track_local_points_map", &h_rows, &d_rows, &n_mp);
    if (rc != ASD_OK) return rc;
    return track_local_points_rows_impl(ctx, slot_cur, n_mp, h_rows, Tcw, K, viewing_cos_limit, occupied, cur_Xw, th, nn_ratio, mp_obs_positive, pose7, match_cur,
                                        n_matches, outlier, n_inliers, defer, d_rows); });
}


namespace {
int track_frame_impl(asd_ctx* ctx, const asd_track_frame_args& A, std::function<int()>* defer) {
  AsdFrameSlot *C = matcher_slot(ctx, A.slot_cur), *L = matcher_slot(ctx, A.slot_last);
  if (!C || !L || !A.has_mp || !A.Xw_last || !A.last_rows || !A.Tcw || !A.K || !A.cand_rows || A.n_cand < 1 || !A.pose7 || !A.pose1 || !A.match1 ||
      !A.n_matches1 || !A.outlier1 || !A.n_inliers1 || !A.match2 || !A.n_matches2 || !A.outlier2 || !A.n_inliers2)
    return ASD_ERR_INVALID;
  if (asd_track_busy(ctx, "asd_track_frame")) return ASD_ERR_INVALID;
  static const bool timing = getenv("ASD_TIMING") != nullptr;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  const int nl = L->n, nc = C->n, ncand = A.n_cand;
  if (nl < 1 || nc < 1 || !replay_on_device(m, 0, nc, nl) || !replay_on_device(m, 1, nc, ncand) || !pose_chain_lds_form(ctx, nc)) {
    ctx->set_error("asd_track_frame: %d / %d keypoints, %d candidates are outside what the one-submission form handles (empty frame, more than "
                   "%d last-frame points or %d candidates, or tables beyond the workgroup's LDS): use asd_track_motion_model_bank + asd_track_local_points_bank", nc, nl, ncand,
                   kResolve2Threads * 4, kResolve2MaxRounds * 512);
    return ASD_ERR_CAPACITY;
  }
  int rc;
  if ((rc = matcher_check_bank_rows(ctx, m, A.last_rows, A.has_mp, nl, false)) != ASD_OK || (rc = matcher_check_bank_rows(ctx, m, A.cand_rows, nullptr, ncand, true)) != ASD_OK) return rc;
  // nothing is searched twice here: the candidate buffers take the worst case up front (a list holds at most every keypoint)
  if ((rc = ensure_cands_dev(ctx, m, (size_t)std::max(nl, ncand) * (size_t)nc)) != ASD_OK) return rc;
  hipStream_t st = ctx->stream;
  AsdXfer &up = ctx->up, &down = ctx->down;
  const size_t io_bytes = pose_chain_io_bytes(nc);
  ASD_HIP_CHECK(ctx, up.begin(st, (size_t)nl * sizeof(WinQuery) + (size_t)nl * (1 + 1 + 12 + 4 + 4) + (size_t)ncand * 5 + 16 * 256));
  ASD_HIP_CHECK(ctx, down.begin(st, 2 * (((size_t)nc + 16) * sizeof(int) + 256 + io_bytes + 256)));
  size_t need = 0;
  auto pad = [](size_t b) { return AsdDevBuf::padded(b); };
  need += pad((size_t)ncand * sizeof(WinQuery)) + 2 * pad((size_t)nl * 4) + 2 * pad((size_t)ncand * 4) + pad((size_t)nl * kTop * 2) + pad((size_t)ncand * kTop * 2) +
          pad(nc) + pad((size_t)nc * 12) + pad(ncand) + pad((size_t)ncand * 12) + pad(32 * 4) + pad(io_bytes);
  ASD_HIP_CHECK(ctx, ctx->scratch.reserve(need));
  // every runtime request of the chain that is not a launch happens here, before the first kernel goes out
  if ((rc = pose_chain_reserve(ctx, nc)) != ASD_OK || (rc = resolve2_attributes(ctx)) != ASD_OK) return rc;
  TrackStage s1{}, s2{};
  s1.kind = 0; s1.nq = nl; s2.kind = 1; s2.nq = ncand;
  s1.F = s2.F = C;
  s1.d_qdesc = s2.d_qdesc = m->d_bank;
  WinQuery* d_q2 = ctx->scratch.carve<WinQuery>(ncand);
  s1.d_off = ctx->scratch.carve<int>(nl); s1.d_cnt = ctx->scratch.carve<int>(nl); s2.d_off = ctx->scratch.carve<int>(ncand); s2.d_cnt = ctx->scratch.carve<int>(ncand);
  s1.d_top = ctx->scratch.carve<uint16_t>((size_t)nl * kTop); s2.d_top = ctx->scratch.carve<uint16_t>((size_t)ncand * kTop);
  uint8_t* d_occ = ctx->scratch.carve<uint8_t>(nc);
  float* d_curXw = ctx->scratch.carve<float>((size_t)nc * 3);
  uint8_t* d_skip = ctx->scratch.carve<uint8_t>(ncand);
  float* d_cXw = ctx->scratch.carve<float>((size_t)ncand * 3);
  float* d_T1 = ctx->scratch.carve<float>(32);
  double* d_io1 = reinterpret_cast<double*>(ctx->scratch.carve<char>(io_bytes));
  // one upload block: the motion-model stage's query table (written on the device) first, the copy its query kernel carries behind it
  const size_t o_q1 = up.reserve((size_t)nl * sizeof(WinQuery));
  s1.d_total = up.dev<int>(up.zeros(sizeof(int))); s2.d_total = up.dev<int>(up.zeros(sizeof(int)));
  if (A.last_obs_positive) s1.d_obs_pos = up.dev<uint8_t>(up.add(A.last_obs_positive, nl));
  if (A.cand_obs_positive) s2.d_obs_pos = up.dev<uint8_t>(up.add(A.cand_obs_positive, ncand));
  const size_t o_has = up.add(A.has_mp, nl), o_Xw = up.add(A.Xw_last, (size_t)nl * 12), o_rows1 = up.add(A.last_rows, (size_t)nl * 4);
  const size_t o_lc = A.last_cand ? up.add(A.last_cand, (size_t)nl * 4) : 0, o_crows = up.add(A.cand_rows, (size_t)ncand * 4);
  const size_t o_btw = up.reserve(sizeof(AsdBetweenArgs));
  const size_t o_out1 = down.reserve(((size_t)nc + 16) * sizeof(int)), o_res1 = down.reserve(io_bytes);
  const size_t o_out2 = down.reserve(((size_t)nc + 16) * sizeof(int)), o_res2 = down.reserve(io_bytes);
  s1.d_out = down.dev<int>(o_out1); s1.h_out = down.host<int>(o_out1);
  s2.d_out = down.dev<int>(o_out2); s2.h_out = down.host<int>(o_out2);
  {   // what happens between the stages is the tail of the motion-model stage's solver (the workgroup that has just written the flags and
      // the pose: no launch, no second read of them); its arguments travel in the upload block
    AsdBetweenArgs b{};
    b.n_cur = nc; b.n_last = nl; b.n_cand = ncand;
    b.match1 = s1.d_out; b.io1 = d_io1; b.Xw_last = up.dev<float>(o_Xw); b.last_cand = A.last_cand ? up.dev<int>(o_lc) : nullptr;
    memcpy(b.T_pred, A.Tcw, sizeof b.T_pred);
    b.occ = d_occ; b.cur_Xw = d_curXw; b.skip = d_skip; b.T1 = d_T1;
    memcpy(up.host<char>(o_btw), &b, sizeof b);
  }
  // ---- motion-model stage: its query kernel reads the pinned block and carries the upload
  s1.source = kQueriesProject; s1.upload = kUploadCarried;
  s1.project = project_args(ctx, *C, *L, A.Tcw, A.K, A.th);
  s1.project.Xw = up.host<float>(o_Xw); s1.project.has_mp = up.host<uint8_t>(o_has); s1.project.rows = up.host<int>(o_rows1);
  s1.project.queries = up.dev<WinQuery>(o_q1);
  s1.project.up = upload_tail(up, nl, true);
  s1.d_queries = up.dev<WinQuery>(o_q1);
  s1.kp_last = L->d_kp; s1.check_ori = A.check_orientation;
  s1.has_solver = true;
  s1.solver.d_points = up.dev<float>(o_Xw);
  memcpy(s1.solver.pose0, A.pose7, sizeof s1.solver.pose0);
  for (int i = 0; i < 4; ++i) s1.solver.K[i] = s2.solver.K[i] = (double)A.K[i];
  s1.solver.io = down.host<double>(o_res1); s1.solver.d_io_dev = d_io1; s1.solver.d_between = up.dev<AsdBetweenArgs>(o_btw);
  // ---- local-map stage: everything it reads was left on the device by the stage in front (pose, occupied keypoints, candidates to skip)
  s2.source = kQueriesFrustum; s2.upload = kUploadElsewhere;
  s2.frustum = frustum_args(ctx, *C, ncand, nullptr, d_T1, A.K, A.viewing_cos_limit, A.th_local);
  s2.frustum.rows = up.dev<int>(o_crows); s2.frustum.queries = d_q2;
  s2.frustum.up = upload_tail(up, ncand, false);
  s2.frustum.attr = m->d_attr; s2.frustum.skip = d_skip; s2.frustum.xw_out = d_cXw;
  s2.d_queries = d_q2;
  s2.d_occupied = d_occ; s2.nn_ratio = A.nn_ratio;
  s2.has_solver = true;
  s2.solver.d_points = d_cXw; s2.solver.d_hold = d_occ; s2.solver.d_own = d_curXw;
  s2.solver.d_pose0 = d_io1; s2.solver.io = down.host<double>(o_res2);
  // replay + solver of a stage as ONE workgroup where both stages' tables fit (k_resolve_pose); two kernels each otherwise
  const bool fuse = stage_fuses(ctx, m, s1) && stage_fuses(ctx, m, s2);
  if ((rc = enqueue_stage(ctx, m, s1, fuse)) != ASD_OK || (rc = enqueue_stage(ctx, m, s2, fuse)) != ASD_OK || (rc = record_chain_end(ctx)) != ASD_OK) return rc;

  asd_track_frame_args O = A;   // (only the output pointers are used below)
  std::array<double, 7> p_in;
  memcpy(p_in.data(), A.pose7, 56);
  auto complete = [=]() -> int {
    ASD_HIP_CHECK(ctx, hipEventSynchronize(ctx->ev_chain));
    const int *h1 = ctx->down.host<int>(o_out1), *h2 = ctx->down.host<int>(o_out2);
    m->last_total[0] = h1[nc + 1]; m->last_total[1] = h2[nc + 1];
    if (h1[nc + 1] > m->cand_cap || h2[nc + 1] > m->cand_cap) {   // cannot happen with the worst-case sizing above
      ctx->set_error("asd_track_frame: %d / %d candidates overflowed the %d-entry buffers", h1[nc + 1], h2[nc + 1], m->cand_cap);
      return ASD_ERR_CAPACITY;
    }
    auto unpack = [&](const int* h_out, const double* h_io, const double* p_start, int32_t* match, int32_t* n_matches, uint8_t* outlier, double* pose, int32_t* n_inl) {
      memcpy(match, h_out, (size_t)nc * sizeof(int));
      *n_matches = h_out[nc];
      unpack_solver_block(h_io, nc, true, match, nullptr, p_start, pose, outlier, n_inl);   // (pose_chain_lds_form holds: checked on entry)
    };
    unpack(h1, ctx->down.host<double>(o_res1), p_in.data(), O.match1, O.n_matches1, O.outlier1, O.pose1, O.n_inliers1);
    double p1[7];
    memcpy(p1, O.pose1, 56);
    unpack(h2, ctx->down.host<double>(o_res2), p1, O.match2, O.n_matches2, O.outlier2, O.pose7, O.n_inliers2);
    ctx->ms_match = 0.f;
    if (timing) {   // k_resolve2's own stamps (10 ns units), averaged over 200 frames
      static double acc[2][5], tl[8]; static long calls;
      const int* hh[2] = {h1, h2};
      for (int k = 0; k < 2; ++k) { acc[k][0] += hh[k][nc + 2]; for (int i = 0; i < 4; ++i) acc[k][1 + i] += 0.01 * hh[k][nc + 3 + i]; }
      // the chain on the device's own 100 MHz clock: resolve 1 [start, end], pose 1 [start, end], resolve 2, pose 2
      const double* io[2] = {ctx->down.host<double>(o_res1), ctx->down.host<double>(o_res2)};
      const int nw = (nc + 7) / 8;
      double st[8];
      for (int k = 0; k < 2; ++k) {
        st[4 * k] = hh[k][nc + 9]; st[4 * k + 1] = hh[k][nc + 10];
        st[4 * k + 2] = (double)((long long)io[k][8 + nw + 1] & 0x7fffffff); st[4 * k + 3] = (double)((long long)io[k][8 + nw + 2] & 0x7fffffff);
      }
      auto d = [](double a, double b) { double x = b - a; if (x < 0) x += 2147483648.0; return 0.01 * x; };
      tl[0] += d(st[0], st[1]); tl[1] += d(st[1], st[2]); tl[2] += d(st[2], st[3]); tl[3] += d(st[3], st[4]);
      tl[4] += d(st[4], st[5]); tl[5] += d(st[5], st[6]); tl[6] += d(st[6], st[7]); tl[7] += d(st[0], st[7]);
      if (++calls % 200 == 0) {
        for (int k = 0; k < 2; ++k)
          fprintf(stderr, "[track_frame resolve kind %d] %.1f iterations, %d candidates; staging %.1f us, iterations %.1f us (the first %.1f), outputs %.1f us; last frame: thread 0 work %.1f us, barrier + verdict %.1f us\n", k,
                  acc[k][0] / calls, hh[k][nc + 1], acc[k][1] / calls, acc[k][2] / calls, acc[k][4] / calls, acc[k][3] / calls, 0.01 * hh[k][nc + 7], 0.01 * hh[k][nc + 8]);
        fprintf(stderr, "[track_frame device clock] resolve1 %.1f | -> pose1 %.1f | pose1 %.1f | -> (frustum, search) resolve2 %.1f | resolve2 %.1f | -> pose2 %.1f | pose2 %.1f | resolve1 start -> pose2 end %.1f us\n",
                tl[0] / calls, tl[1] / calls, tl[2] / calls, tl[3] / calls, tl[4] / calls, tl[5] / calls, tl[6] / calls, tl[7] / calls);
      }
    }
    return ASD_OK;
  };
  if (defer) { *defer = complete; return ASD_OK; }
  return complete();
}
}  // namespace

int asd_track_frame(asd_ctx* ctx, const asd_track_frame_args* args) {
  if (!args) return ASD_ERR_INVALID;
  return run_track(ctx, [&](std::function<int()>* defer) { return track_frame_impl(ctx, *args, defer); });
}

int asd_track_async(asd_ctx* ctx) {
  if (!ctx) return ASD_ERR_INVALID;
  if (asd_track_busy(ctx, "asd_track_async")) return ASD_ERR_INVALID;
  ctx->track_async_armed = true;
  return ASD_OK;
}

int asd_track_finish(asd_ctx* ctx) {
  if (!ctx) return ASD_ERR_INVALID;
  if (!ctx->track_has_pending) { ctx->set_error("asd_track_finish: no asd_track_* call is outstanding (asd_track_async arms the next one)"); return ASD_ERR_INVALID; }
  (void)hipSetDevice(ctx->cfg.device);
  std::function<int()> fin = std::move(ctx->track_pending);
  ctx->track_pending = nullptr;
  ctx->track_has_pending = false;
  return fin();
}

// ---- asd_fuse_search_batch: every (keyframe, map point list) pair of SearchInNeighbors in one launch ------------------------------
// One wave per candidate map point.  The gates of ORBmatcher::Fuse (ORBmatcher.cc:850-895) are evaluated by the wave (uniformly: every
// lane the same f32 / f64 operations asd_fuse_search's host loop performs, -ffp-contract=off; the predicted level from the thresholds the
// host derived from its own logf), the window is walked in KeyFrame::GetFeaturesInArea order (no level filter), a lane takes a
// candidate -- level gate (:905-906), 5.99 chi2 gate (:909-916), DescriptorDistance in the reference's summation order -- and the wave
// keeps the smallest distance, the FIRST such candidate among equals (`dist < bestDist`, :927).
struct FuseCallDev {
  GridDev G;
  const float* desc;         // the keyframe's descriptors
  float T[16], Ow[3], K[4];
  float min_x, max_x, min_y, max_y;
  int first, n;
};
struct FuseBatchArgs {
  const FuseCallDev* calls; const int* call_of;   // [n_total]
  int n_total, n_levels;
  const uint8_t* valid; const float* Xw; const float* normal; const float* min_dist; const float* max_dist; const float* desc;
  const int* desc_rows;      // null: desc is [n_total][128]; else desc = the descriptor bank and desc_rows[i] the map point's row
  float th, level_thr[ASD_MAX_LEVELS], scale[ASD_MAX_LEVELS], inv_sigma2[ASD_MAX_LEVELS];
  int* best_idx; float* best_dist;
};
__global__ __launch_bounds__(256) void k_fuse_batch(FuseBatchArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n_total) return;
  int out_idx = -1;
  float out_dist = 256.f;
  do {
    if (!a.valid[i]) break;
    const FuseCallDev& Cc = a.calls[a.call_of[i]];
    const float* P = a.Xw + 3 * (size_t)i;
    float Pc[3];
    for (int r = 0; r < 3; ++r) {
      const float t0 = Cc.T[r * 4 + 0] * P[0] + Cc.T[r * 4 + 1] * P[1] + Cc.T[r * 4 + 2] * P[2];
      Pc[r] = (float)((double)t0 + (double)Cc.T[r * 4 + 3]);
    }
    if (Pc[2] < 0.0f) break;
    const float invz = 1 / Pc[2];
    const float u = Cc.K[0] * (Pc[0] * invz) + Cc.K[2], v = Cc.K[1] * (Pc[1] * invz) + Cc.K[3];
    if (!(u >= Cc.min_x && u < Cc.max_x && v >= Cc.min_y && v < Cc.max_y)) break;  // KeyFrame::IsInImage
    const float maxD = 1.2f * a.max_dist[i], minD = 0.8f * a.min_dist[i];
    const float PO[3] = {P[0] - Cc.Ow[0], P[1] - Cc.Ow[1], P[2] - Cc.Ow[2]};
    const double nn = (double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2];
    const float dist3D = (float)sqrt(nn);
    if (dist3D < minD || dist3D > maxD) break;
    const float* Pn = a.normal + 3 * (size_t)i;
    const double dot = (double)PO[0] * Pn[0] + (double)PO[1] * Pn[1] + (double)PO[2] * Pn[2];
    if (dot < 0.5 * dist3D) break;
    const float ratio = a.max_dist[i] / dist3D;
    int lvl = 0;
    for (int k = 1; k < a.n_levels; ++k) lvl += ratio >= a.level_thr[k];
    const float r = a.th * a.scale[lvl];
    const GridDev& G = Cc.G;
    const int nMinCellX = max(0, (int)floorf((u - G.min_x - r) * G.inv_w));
    const int nMaxCellX = min(ASD_GRID_COLS - 1, (int)ceilf((u - G.min_x + r) * G.inv_w));
    const int nMinCellY = max(0, (int)floorf((v - G.min_y - r) * G.inv_h));
    const int nMaxCellY = min(ASD_GRID_ROWS - 1, (int)ceilf((v - G.min_y + r) * G.inv_h));
    if (nMinCellX >= ASD_GRID_COLS || nMaxCellX < 0 || nMinCellY >= ASD_GRID_ROWS || nMaxCellY < 0) break;
    const float4* qa = reinterpret_cast<const float4*>(a.desc + (size_t)(a.desc_rows ? a.desc_rows[i] : i) * 128);
    unsigned long long best = ~0ull;
    int pos = 0;   // position in GetFeaturesInArea order (ties: the first wins)
    for (int ix = nMinCellX; ix <= nMaxCellX; ++ix) {
      const int b = G.cell_start[ix * ASD_GRID_ROWS + nMinCellY], e = G.cell_start[ix * ASD_GRID_ROWS + nMaxCellY + 1];
      for (int base = b; base < e; base += 64) {
        const int it = base + lane;
        bool in = false;
        int idx = 0;
        float4 kp = make_float4(0.f, 0.f, 0.f, 0.f);
        if (it < e) {
          idx = G.cell_items[it];
          kp = G.kp[idx];
          const float dx = kp.x - u, dy = kp.y - v;
          in = fabsf(dx) < r && fabsf(dy) < r;
        }
        const unsigned long long m = __ballot(in);
        unsigned long long key = ~0ull;
        if (in) {
          const int p = pos + __popcll(m & ((1ull << lane) - 1));
          const int oct = __float_as_int(kp.z);
          bool ok = !(oct < lvl - 1 || oct > lvl);
          const float ex = u - kp.x, ey = v - kp.y;
          const float e2 = ex * ex + ey * ey;
          if ((double)(e2 * a.inv_sigma2[oct]) > 5.99) ok = false;
          if (ok) {
            const float4* qb = reinterpret_cast<const float4*>(Cc.desc + (size_t)idx * 128);
            float sqd = 0.f;
#pragma unroll 8
            for (int k = 0; k < 32; ++k) {
              const float4 x = qa[k], y = qb[k];
              float d;
              d = x.x - y.x; sqd = sqd + d * d;
              d = x.y - y.y; sqd = sqd + d * d;
              d = x.z - y.z; sqd = sqd + d * d;
              d = x.w - y.w; sqd = sqd + d * d;
            }
            if (sqd < 256.f) key = ((unsigned long long)__float_as_uint(sqd) << 32) | ((unsigned long long)(unsigned)p << 16) | (unsigned)idx;
          }
        }
        for (int off = 32; off >= 1; off >>= 1) {
          const unsigned long long o = __shfl_xor(key, off);
          key = o < key ? o : key;
        }
        best = key < best ? key : best;
        pos += __popcll(m);
      }
    }
    if (best != ~0ull) {
      const float d = __uint_as_float((unsigned)(best >> 32));
      if (d <= TH_LOW) { out_idx = (int)(best & 0xffffu); out_dist = d; }
    }
  } while (false);
  if (lane == 0) { a.best_idx[i] = out_idx; a.best_dist[i] = out_dist; }
}

int asd_fuse_search_batch(asd_ctx* ctx, int32_t n_calls, const asd_fuse_call* calls, int32_t n_total, const uint8_t* valid, const float* Xw,
                          const float* normal, const float* min_dist, const float* max_dist, const float* desc, const int32_t* desc_rows, float th,
                          int32_t* best_idx, float* best_dist) {
  if (!ctx || n_calls < 0 || n_total < 0 || (n_calls > 0 && !calls) ||
      (n_total > 0 && (!valid || !Xw || !normal || !min_dist || !max_dist || (!desc && !desc_rows) || !best_idx || !best_dist)))
    return ASD_ERR_INVALID;
  if (asd_track_busy(ctx, "asd_fuse_search_batch")) return ASD_ERR_INVALID;
  for (int i = 0; i < n_total; ++i) { best_idx[i] = -1; best_dist[i] = 256.f; }
  if (n_calls == 0 || n_total == 0) return ASD_OK;
  (void)hipSetDevice(ctx->cfg.device);
  std::vector<FuseCallDev> cd(n_calls);
  std::vector<int> call_of(n_total, -1);
  for (int c = 0; c < n_calls; ++c) {
    const asd_fuse_call& A = calls[c];
    AsdFrameSlot* KF = matcher_slot(ctx, A.slot_kf);
    if (!KF || !KF->d_kp || A.first < 0 || A.n < 0 || A.first + A.n > n_total) { ctx->set_error("asd_fuse_search_batch: call %d: slot %d / rows [%d, %d) of %d", c, A.slot_kf, A.first, A.first + A.n, n_total); return ASD_ERR_INVALID; }
    if (KF->n >= 65536) { ctx->set_error("asd_fuse_search_batch: keyframe of %d keypoints", KF->n); return ASD_ERR_CAPACITY; }
    FuseCallDev& D = cd[c];
    D.G = GridDev{KF->d_kp, KF->d_cell_start, KF->d_cell_items, KF->min_x, KF->min_y, KF->inv_w, KF->inv_h};
    D.desc = KF->d_desc;
    memcpy(D.T, A.Tcw, sizeof D.T);
    matcher_keyframe_centre(A.Tcw, D.Ow);   // (as asd_fuse_search)
    memcpy(D.K, A.K, sizeof D.K);
    D.min_x = KF->min_x; D.max_x = KF->max_x; D.min_y = KF->min_y; D.max_y = KF->max_y;
    D.first = A.first; D.n = A.n;
    for (int i = A.first; i < A.first + A.n; ++i) {
      if (call_of[i] >= 0) { ctx->set_error("asd_fuse_search_batch: rows of calls %d and %d overlap", call_of[i], c); return ASD_ERR_INVALID; }
      call_of[i] = c;
    }
  }
  std::vector<uint8_t> val(valid, valid + n_total);
  for (int i = 0; i < n_total; ++i) if (call_of[i] < 0) { val[i] = 0; call_of[i] = 0; }   // rows no call covers: nothing to search
  MatcherState* mst = matcher_state(ctx);
  if (!desc)
    for (int i = 0; i < n_total; ++i)
      if (val[i] && (desc_rows[i] < 0 || desc_rows[i] >= mst->bank_cap)) { ctx->set_error("asd_fuse_search_batch: bank row %d out of range", desc_rows[i]); return ASD_ERR_INVALID; }
  hipStream_t st = ctx->stream;
  AsdXfer &up = ctx->up, &down = ctx->down;
  ASD_HIP_CHECK(ctx, up.begin(st, (size_t)n_total * (1 + 12 + 12 + 4 + 4 + 512 + 4) + (size_t)n_calls * sizeof(FuseCallDev) + 16 * 256));
  ASD_HIP_CHECK(ctx, down.begin(st, (size_t)n_total * 8 + 1024));
  FuseBatchArgs a{};
  a.calls = up.dev<FuseCallDev>(up.add(cd.data(), cd.size() * sizeof(FuseCallDev)));
  a.call_of = up.dev<int>(up.add(call_of.data(), (size_t)n_total * 4));
  a.n_total = n_total; a.n_levels = ctx->cfg.n_levels;
  a.valid = up.dev<uint8_t>(up.add(val.data(), n_total));
  a.Xw = up.dev<float>(up.add(Xw, (size_t)n_total * 12));
  a.normal = up.dev<float>(up.add(normal, (size_t)n_total * 12));
  a.min_dist = up.dev<float>(up.add(min_dist, (size_t)n_total * 4));
  a.max_dist = up.dev<float>(up.add(max_dist, (size_t)n_total * 4));
  if (desc) { a.desc = up.dev<float>(up.add(desc, (size_t)n_total * 512)); a.desc_rows = nullptr; }
  else { a.desc = mst->d_bank; a.desc_rows = up.dev<int>(up.add(desc_rows, (size_t)n_total * 4)); }
  a.th = th;
  for (int l = 0; l < ASD_MAX_LEVELS; ++l) {
    a.level_thr[l] = ctx->level_thr[l];
    a.scale[l] = l < ctx->cfg.n_levels ? ctx->scale[l] : 0.f;
    a.inv_sigma2[l] = l < ctx->cfg.n_levels ? ctx->inv_sigma2[l] : 0.f;
  }
  const size_t o_i = down.reserve((size_t)n_total * 4), o_d = down.reserve((size_t)n_total * 4);
  a.best_idx = down.dev<int>(o_i); a.best_dist = down.dev<float>(o_d);
  ASD_HIP_CHECK(ctx, up.upload(st));
  hipLaunchKernelGGL(k_fuse_batch, dim3((n_total + 3) / 4), dim3(256), 0, st, a);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, down.download(st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  memcpy(best_idx, down.host<int>(o_i), (size_t)n_total * 4);
  memcpy(best_dist, down.host<float>(o_d), (size_t)n_total * 4);
  return ASD_OK;
}

}  // extern "C"

// merge-join of two DBoW2 feature vectors (std::map iteration + lower_bound, ORBmatcher.cc:183-278):
// calls fn(a, b) for every node present in both
template <typename Fn>
static void node_join(const asd_feature_vector* A, const asd_feature_vector* B, Fn fn) {
  int a = 0, b = 0;
  while (a < A->n_nodes && b < B->n_nodes) {
    if (A->node_id[a] == B->node_id[b]) { fn(a, b); ++a; ++b; }
    else if (A->node_id[a] < B->node_id[b]) a = (int)(std::lower_bound(A->node_id, A->node_id + A->n_nodes, B->node_id[b]) - A->node_id);
    else b = (int)(std::lower_bound(B->node_id, B->node_id + B->n_nodes, A->node_id[a]) - B->node_id);
  }
}

int matcher_list_search(asd_ctx* ctx, MatcherState* m, const AsdFrameSlot& A, const AsdFrameSlot& B, const asd_feature_vector* fvA,
                        const asd_feature_vector* fvB, const uint8_t* skipA, bool skip_if_set, std::vector<ListQuery>& lq, const float** dist_out) {
  lq.clear();
  int total = 0;
  node_join(fvA, fvB, [&](int a, int b) {
    const int cb = fvB->start[b], ce = fvB->start[b + 1];
    for (int t = fvA->start[a]; t < fvA->start[a + 1]; ++t) {
      const int i = fvA->idx[t];
      if ((skipA[i] != 0) == skip_if_set) continue;
      lq.push_back(ListQuery{i, cb, ce, total});
      total += ce - cb;
    }
  });
  *dist_out = nullptr;
  if (lq.empty() || total == 0) return ASD_OK;
  int rc;
  if ((rc = ensure_cands(ctx, m, std::max(total, fvB->start[fvB->n_nodes]))) != ASD_OK) return rc;
  if ((rc = matcher_ensure_queries(ctx, m, (int)lq.size())) != ASD_OK) return rc;
  static_assert(sizeof(ListQuery) <= sizeof(WinQuery), "query staging is shared");
  hipStream_t st = ctx->stream;
  memcpy(m->h_queries, lq.data(), lq.size() * sizeof(ListQuery));
  const int ncand = fvB->start[fvB->n_nodes];
  memcpy(m->h_idx, fvB->idx, (size_t)ncand * sizeof(int));
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(m->d_queries, m->h_queries, lq.size() * sizeof(ListQuery), hipMemcpyHostToDevice, st));
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(m->d_idx, m->h_idx, (size_t)ncand * sizeof(int), hipMemcpyHostToDevice, st));
  ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev0, st));
  hipLaunchKernelGGL(k_list_dist, dim3(((int)lq.size() + 3) / 4), dim3(256), 0, st, reinterpret_cast<const ListQuery*>(m->d_queries),
                     (int)lq.size(), m->d_idx, A.d_desc, B.d_desc, m->d_dist);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev1, st));
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(m->h_dist, m->d_dist, (size_t)total * sizeof(float), hipMemcpyDeviceToHost, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  ASD_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->ms_match, ctx->ev0, ctx->ev1));
  *dist_out = m->h_dist;
  return ASD_OK;
}
