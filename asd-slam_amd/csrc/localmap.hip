// localmap.hip -- Tracking::UpdateLocalMap (reference src/vslam/src/Tracking.cc:871-1015) with SearchLocalPoints' skip loop (:827-841), and
// the counting half of KeyFrame::UpdateConnections (src/vslam/src/KeyFrame.cc:541-573), over a resident observation table.
//
// Device layout.  The table is keyframe-major: one arena of int32 bank rows (-1 = no map point), a slot table {offset, length, id, bad,
// covisibles, parent} in front of it (a free slot has length -1; ids map to slots as in kfdb.hip), the children lists as one CSR block
// and the live ids in ascending order with their slots (both rebuilt by the next query after a call that changed them).  Three tables
// run by bank row: MapPoint::isBad() as a byte, the frame's marks (the vote multiplicity in the low bits, "carries mnLastFrameSeen" in
// bit 30) and the claim word of the ordered de-duplication.  Marks and claims are never cleared as a whole: a query undoes exactly what
// it touched (k_lm_unmark; the surviving claimant resets its claim word).
//
// A query.  k_lm_mark (integer atomics on the mark table) -> k_lm_vote (one wave per slot walks the keyframe's row with coalesced loads and
// adds the marks' multiplicities: every table entry counts, see the header's precondition) -> k_lm_decide (ONE workgroup: the voted
// keyframes in ascending id, pKFmax, the expansion :958-1008, the prefix of the row lengths over the list) -> the host reads five
// numbers and sizes the rest -> k_lm_claim (every entry of the concatenated rows claims its point with atomicMin of its global position)
// -> k_lm_count / k_lm_tilescan / k_lm_scatter (the claimants compacted in position order into mvpLocalMapPoints and the sub-list
// SearchLocalPoints does not skip).  Every decision is a minimum, a maximum or a scan over integers: the output does not depend on the
// scheduling.
//
// The ordering rule.  Where the reference walks a std::map<KeyFrame*, ...> or a std::set<KeyFrame*> in pointer order, the walk here is
// in ascending keyframe id: the vote list, the first strict maximum, GetChilds().
//
// Culling.  LocalMapping::KeyFrameCulling (reference src/vslam/src/LocalMapping.cc:739-809, monocular) and MapPoint::Observations() read the
// same table; the arena has a second plane, one byte per entry = mvKeysUn[idx].octave, that follows its row through growth and compaction.
// asd_keyframe_culling: the candidates' rows laid end to end go through the claim / count / tile-scan / scatter compaction above, which
// leaves their distinct not-bad points in order; k_cull_index writes each point's position into the mark table and zeroes its 16 int32
// counters; k_cull_count is ONE pass over every live row (one wave per slot, coalesced row and octave loads, integer atomics) that builds
// the per-octave observation counts of those points only; k_cull_walk is ONE workgroup that takes the candidates in order -- a strided
// count over the row, a workgroup reduction, the decision 10 nR > 9 nM, then over the same row the decrements, the points that fall to
// <= 2 observations (appended in keypoint order by a ballot scan) -- so a cull is seen by the next candidate without a host round trip.
// The walk changes only the call's scratch.  With apply = 1 one more pass over the live rows (k_cull_apply) empties the culled rows and
// the entries of the points that turned bad; k_cull_finish undoes the marks either way.  asd_map_observations is the same marking and the
// same pass with one counter per point.
//
// UpdateNormalAndDepth.  MapPoint::UpdateNormalAndDepth (reference src/vslam/src/MapPoint.cc:361-407) for many points at once, over this
// table, a camera centre per slot (d_center, beside d_table) and the matcher's attribute bank, which it rewrites in place.  The mean
// viewing direction is an f32 sum whose order is part of the result, so nothing is added atomically: k_nd_mark writes the points'
// positions into the mark table, k_cull_count counts their observers (ONE pass over the live rows, integer atomics), k_nd_scan gives
// every point a segment, k_nd_fill (the second pass) drops (keyframe id, slot) into the segments through an integer cursor, k_nd_order
// ranks every segment by keyframe id, and k_nd_point -- one wave per point -- adds the unit vectors one after the other in that order.
// The arithmetic itself is normal_depth.h, shared with the host function asd_normal_and_depth_point.  Nothing is sized by a typical
// observer count: the host reads the total between scan and fill and sizes the segments by it.
//
// LocalBundleAdjustment.  asd_local_ba_graph is Optimizer.cc:418-467 with the structure of :484-593: the local keyframes' rows go through
// the claim / count / tile-scan / scatter compaction (lLocalMapPoints), k_cull_count and k_nd_scan give every point its Observations() and
// a segment, k_bg_fill / k_bg_order lay (keyframe id, slot, keypoint index, octave) into it in ascending id.  An entry's position in the
// ordered segments is the moment the reference's walk meets it, so lFixedCameras is one more ordered de-duplication (a claim word per slot,
// atomicMin of the position) and one more count / tile-scan / scatter, which numbers the edges at the same time; point_rank is a scan over
// the marked rows of the row tables.  The segments and the edge -> entry map stay resident (d_bg*: storage of their own) for
// asd_local_ba_apply, which evaluates the erase policy of :652-697 per point in closed form and, with apply = 1, empties the erased
// entries THROUGH the segments, without another pass over the table.
//
// Fuse's side effects.  asd_fuse_apply is what ORBmatcher::Fuse does with bestIdx (ORBmatcher.cc:939-955, :1065-1079), the Replace loops of
// LoopClosing (LoopClosing.cc:540-555, :619-627) and MapPoint::Replace (MapPoint.cc:206-244), in the reference's order.  The points that can
// take part -- the candidates with a best_idx and what kf's row holds there -- are marked, k_cull_count counts their observers, k_nd_scan
// gives them segments, k_fa_fill lays (slot, keypoint index, point, owner) into them; k_fa_walk is ONE workgroup: thread 0 takes the
// candidates in order and stops at every Replace, which all threads do together over the two points' chains of segments.  With apply = 1
// k_fa_write rewrites the rows THROUGH the segments, without another pass over the table.
//
// Streams.  Every copy into these tables and every kernel that reads them is enqueued on ctx->stream, every entry point returns with that
// stream drained, and all of them are refused while an armed asd_track_* call is unfinished (asd_track_local_points_map reads the search
// list on that stream).  A growth therefore orders itself against the only stream that can hold a write to the old storage: the copy
// into the new block is enqueued behind them on ctx->stream, and the old block is freed after that stream has been waited for.  The
// extractor's streams and asd_prep_async's second stream never touch these tables.
#include <algorithm>
#include <climits>
#include <map>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "matcher.h"
#include "normal_depth.h"

namespace {

constexpr int kInitSlots = 64;            // slot table, arena and row tables start small and double
constexpr long long kInitEntries = 16384;
constexpr int kInitRows = 4096;
constexpr int kMaxSlots = 1 << 18;        // the "included" bit set of k_lm_decide lives in LDS: 32 KB
constexpr int kMaxKeypoints = 1 << 16;
constexpr int kMaxRow = 1 << 28;
constexpr int kMaxCov = 10;               // GetBestCovisibilityKeyFrames(10)
constexpr int kMaxLocalKfs = 1000;        // bound of max_kfs: the appended ids of the expansion are kept in LDS
constexpr int kVoteMask = 0x3fffffff, kSkipBit = 0x40000000;
constexpr int kClaimFree = 0x7f7f7f7f;    // (a byte pattern: hipMemsetAsync fills the claim table)
constexpr long long kMaxEntriesPerQuery = 0x7f000000;
constexpr int kTile = 1024;               // entries per workgroup of the compaction: 4 rounds of 256
constexpr int kLevels = ASD_MAX_LEVELS;   // counters per point of asd_keyframe_culling
constexpr int kMaxCand = 4096;
constexpr long long kMaxCullEntries = 1ll << 26;   // entries of the candidates' rows together: 16 counters each stay below 2^31 words
constexpr int kMaxNdPoints = 1 << 20;              // points of one asd_update_normal_and_depth
constexpr long long kMaxNdEntries = 1ll << 30;     // their observations together: the segment offsets are int32

struct LmSlotDev { long long off; int n; int id; int bad; int n_cov; int parent; int pad; int cov[kMaxCov]; int pad2[2]; };   // n < 0: free slot
struct LmMove { long long from, to; int n; int pad; };

struct LmDecideArgs {
  const LmSlotDev* table;
  const int* sorted_id; const int* sorted_slot; int n_live;   // the live keyframes in ascending id
  const int* cnt;                                              // [slots] votes
  const int* child_off; const int* children;                   // CSR by slot
  const int* prev; int n_prev; int max_kfs; int incl_words;
  int ids_in_lds;                                              // the ascending id list fits the LDS beside the bit set: the id -> slot searches read it there
  int* list_id; int* list_slot; long long* list_base;          // out: mvpLocalKeyFrames, their slots (-1: not in the table), prefix of the row lengths
  int* head;                                                   // out: n_list, ref_kf, any vote, longest row, entries (2 words), 0, 0, n_local, n_search
};

struct LmPointArgs {
  const LmSlotDev* table; const int* rows;
  const int* list_slot; const long long* list_base; int tiles_per_kf;
  const uint8_t* pbad; const int* mark; int* claim;
  int* tile_cnt; const int* tile_off;       // [tiles][2]: survivors of the local list and of the search list
  int* d_local; int* d_search;              // the lists on the device
  int* h_local; int cap_local; int* h_search; int cap_search;   // and in the pinned result block, as far as the caller's capacities go
};

__device__ inline int lm_lookup(const int* sorted_id, const int* sorted_slot, int n, int id) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (sorted_id[mid] < id) lo = mid + 1; else hi = mid; }
  return lo < n && sorted_id[lo] == id ? sorted_slot[lo] : -1;
}

// frame rows: cur [0, n_cur) vote (unless the point is bad) and are skipped by the search, seen [n_cur, n_cur + n_seen) are skipped only
__global__ __launch_bounds__(256) void k_lm_mark(const int* __restrict__ cur, int n_cur, const int* __restrict__ seen, int n_seen,
                                                 const uint8_t* __restrict__ pbad, int* __restrict__ mark) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_cur) {
    const int r = cur[i];
    if (r >= 0) { atomicOr(&mark[r], kSkipBit); if (!pbad[r]) atomicAdd(&mark[r], 1); }
  } else if (i < n_cur + n_seen) {
    const int r = seen[i - n_cur];
    if (r >= 0) atomicOr(&mark[r], kSkipBit);
  }
}
__global__ __launch_bounds__(256) void k_lm_unmark(const int* __restrict__ cur, int n_cur, const int* __restrict__ seen, int n_seen, int* __restrict__ mark) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_cur + n_seen) return;
  const int r = i < n_cur ? cur[i] : seen[i - n_cur];
  if (r >= 0) mark[r] = 0;
}

// one wave per slot: the sum of the marks' multiplicities over the keyframe's row
__global__ __launch_bounds__(256) void k_lm_vote(const LmSlotDev* __restrict__ table, int n_slots, const int* __restrict__ rows,
                                                 const int* __restrict__ mark, int* __restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= n_slots) return;   // whole waves leave together
  const long long off = table[slot].off;
  const int n = table[slot].n;
  int c = 0;
  for (int i = lane; i < n; i += 64) {
    const int r = rows[off + i];
    if (r >= 0) c += mark[r] & kVoteMask;
  }
  for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s, 64);
  if (lane == 0) cnt[slot] = c;
}

__global__ __launch_bounds__(256) void k_lm_set(int* __restrict__ row, const int* __restrict__ idx, const int* __restrict__ val, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) row[idx[i]] = val[i];
}
__global__ __launch_bounds__(256) void k_lm_point_bad(uint8_t* __restrict__ pbad, const int* __restrict__ rows, int n, int flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) pbad[rows[i]] = (uint8_t)flag;
}
// growth: one workgroup per live keyframe copies its row from the old arena into the new one
__global__ __launch_bounds__(256) void k_lm_move(const LmMove* __restrict__ mv, const int* __restrict__ r0, int* __restrict__ r1,
                                                 const uint8_t* __restrict__ o0, uint8_t* __restrict__ o1) {
  const LmMove m = mv[blockIdx.x];
  for (int t = threadIdx.x; t < m.n; t += 256) { r1[m.to + t] = r0[m.from + t]; o1[m.to + t] = o0[m.from + t]; }
}

// exclusive prefix of one int per thread over the workgroup (256 threads); *total = the sum
__device__ inline int lm_block_scan(int v, int* s, int* total) {
  const int t = threadIdx.x;
  s[t] = v;
  asd_syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int x = t >= d ? s[t - d] : 0;
    asd_syncthreads();
    s[t] += x;
    asd_syncthreads();
  }
  const int incl = s[t];
  *total = s[255];
  asd_syncthreads();
  return incl - v;
}
// the same for a flag per thread: ballots, and one LDS word per wave
__device__ inline int lm_block_scan_flag(bool f, int* s_wave, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long b = __ballot(f);
  if (lane == 0) s_wave[w] = __popcll(b);
  asd_syncthreads();
  int before = 0, all = 0;
  for (int k = 0; k < 4; ++k) { const int c = s_wave[k]; if (k < w) before += c; all += c; }
  *total = all;
  asd_syncthreads();
  return before + __popcll(b & ((1ull << lane) - 1));
}

// UpdateLocalKeyFrames' list decisions (:929-1008) in one workgroup
__global__ __launch_bounds__(256) void k_lm_decide(LmDecideArgs a) {
  extern __shared__ unsigned s_incl[];   // mnTrackReferenceForFrame == this frame, one bit per slot
  __shared__ int s_scan[256], s_wave[4], s_app[3 * (kMaxLocalKfs + 1)];
  __shared__ int s_n, s_any, s_napp, s_first, s_stop, s_maxn;
  __shared__ unsigned long long s_best;
  const int t = threadIdx.x;
  for (int w = t; w < a.incl_words; w += 256) s_incl[w] = 0u;
  // every id -> slot search below is a chain of dependent loads: from LDS where the list fits, from global memory otherwise
  int* const s_ids = reinterpret_cast<int*>(s_incl + a.incl_words);
  if (a.ids_in_lds) for (int i = t; i < a.n_live; i += 256) s_ids[i] = a.sorted_id[i];
  const int* const ids_sorted = a.ids_in_lds ? s_ids : a.sorted_id;
  if (t == 0) { s_n = 0; s_any = 0; s_napp = 0; s_stop = 0; s_maxn = 0; s_best = 0ull; }
  asd_syncthreads();
  // the voted keyframes in ascending id, bad ones skipped (:939-954); pKFmax = the first strictly larger count
  for (int base = 0; base < a.n_live; base += 256) {
    const int p = base + t;
    bool take = false;
    int sl = -1, c = 0;
    if (p < a.n_live) {
      sl = a.sorted_slot[p];
      c = a.cnt[sl];
      if (c > 0) { s_any = 1; take = !a.table[sl].bad; }
    }
    int total;
    const int pos = s_n + lm_block_scan_flag(take, s_wave, &total);
    if (take) {
      a.list_id[pos] = a.sorted_id[p];
      a.list_slot[pos] = sl;
      atomicOr(&s_incl[sl >> 5], 1u << (sl & 31));
      atomicMax(&s_best, ((unsigned long long)(unsigned)c << 32) | (unsigned)(0x7fffffff - p));
    }
    asd_syncthreads();
    if (t == 0) s_n += total;
    asd_syncthreads();
  }
  const int n0 = s_n;
  const bool any = s_any != 0;
  int ref = -1;
  if (any && s_best) ref = a.sorted_id[0x7fffffff - (int)(unsigned)(s_best & 0xffffffffull)];
  if (!any) {   // nobody voted (:929-930): the list stays the caller's
    for (int i = t; i < a.n_prev; i += 256) {
      const int id = a.prev[i];
      a.list_id[i] = id;
      a.list_slot[i] = lm_lookup(ids_sorted, a.sorted_slot, a.n_live, id);
    }
  }
  asd_syncthreads();
  // thread 0 appends: the keyframe becomes part of the list and is marked
  auto append = [&](int id) {
    const int sl = lm_lookup(ids_sorted, a.sorted_slot, a.n_live, id);
    const int pos = n0 + s_napp;
    a.list_id[pos] = id;
    a.list_slot[pos] = sl;
    s_app[s_napp] = id;
    s_napp = s_napp + 1;
    if (sl >= 0) s_incl[sl >> 5] |= 1u << (sl & 31);
  };
  auto included = [&](int id, int sl) -> bool {
    if (sl >= 0) return (s_incl[sl >> 5] >> (sl & 31)) & 1u;
    const int na = s_napp;   // an id that is not in the table can only have been appended
    for (int k = 0; k < na; ++k) if (s_app[k] == id) return true;
    return false;
  };
  // the first not-bad, not-yet-included of ids[0 .. count) is appended; all threads call this together
  auto first_ok = [&](const int* ids, int count) {
    for (int base = 0; base < count; base += 256) {
      if (t == 0) s_first = INT_MAX;
      asd_syncthreads();
      const int k = base + t;
      if (k < count) {
        const int id = ids[k];
        const int sl = lm_lookup(ids_sorted, a.sorted_slot, a.n_live, id);
        if (!(sl >= 0 && a.table[sl].bad) && !included(id, sl)) atomicMin(&s_first, k);
      }
      asd_syncthreads();
      const int f = s_first;
      if (f != INT_MAX && t == 0) append(ids[f]);
      asd_syncthreads();
      if (f != INT_MAX) break;
    }
  };
  if (any) {
    for (int i = 0; i < n0; ++i) {   // the end iterator was taken before anything was appended
      const int napp = s_napp;
      asd_syncthreads();   // (thread 0 appends further down: everybody has read the count first)
      if (n0 + napp > a.max_kfs) break;   // :961
      const int sl = a.list_slot[i];
      const LmSlotDev* S = a.table + sl;
      first_ok(S->cov, S->n_cov);
      first_ok(a.children + a.child_off[sl], a.child_off[sl + 1] - a.child_off[sl]);
      if (t == 0) {   // the parent has no bad test, and taking it ends the expansion (:997-1006)
        const int id = S->parent;
        if (id >= 0 && !included(id, lm_lookup(ids_sorted, a.sorted_slot, a.n_live, id))) { append(id); s_stop = 1; }
      }
      asd_syncthreads();
      if (s_stop) break;
    }
  }
  asd_syncthreads();
  const int n_list = any ? n0 + s_napp : a.n_prev;
  // the rows of the list laid end to end: the global position of an entry is the order UpdateLocalPoints meets it in
  long long run = 0;
  for (int base = 0; base < n_list; base += 256) {
    const int i = base + t;
    int n = 0;
    if (i < n_list) { const int sl = a.list_slot[i]; if (sl >= 0) n = a.table[sl].n; }
    if (n > 0) atomicMax(&s_maxn, n);
    int total;
    const int ex = lm_block_scan(n, s_scan, &total);
    if (i < n_list) a.list_base[i] = run + ex;
    run += total;
  }
  asd_syncthreads();
  if (t == 0) {
    a.head[0] = n_list; a.head[1] = ref; a.head[2] = any; a.head[3] = s_maxn;
    a.head[4] = (int)(unsigned)(run & 0xffffffffll); a.head[5] = (int)(run >> 32);
    a.head[6] = 0; a.head[7] = 0; a.head[8] = 0; a.head[9] = 0;
  }
}

// the entry of this thread in round k of its tile: row value (or -1) and global position
__device__ inline int lm_entry(const LmPointArgs& a, int k, long long* pos) {
  const int sl = a.list_slot[blockIdx.x];   // (x: the list entry, y: the tile inside its row)
  if (sl < 0) return -1;
  const LmSlotDev* S = a.table + sl;
  const int idx = blockIdx.y * kTile + k * 256 + threadIdx.x;
  if (idx >= S->n) return -1;
  *pos = a.list_base[blockIdx.x] + idx;
  const int r = a.rows[S->off + idx];
  return r >= 0 && !a.pbad[r] ? r : -1;
}
__global__ __launch_bounds__(256) void k_lm_claim(LmPointArgs a) {
  for (int k = 0; k < 4; ++k) {
    long long pos = 0;
    const int r = lm_entry(a, k, &pos);
    if (r >= 0) atomicMin(&a.claim[r], (int)pos);
  }
}
__global__ __launch_bounds__(256) void k_lm_count(LmPointArgs a) {
  __shared__ int s_wave[4];
  int nl = 0, ns = 0;
  for (int k = 0; k < 4; ++k) {
    long long pos = 0;
    const int r = lm_entry(a, k, &pos);
    if (r >= 0 && a.claim[r] == (int)pos) { ++nl; ns += !(a.mark[r] & kSkipBit); }
  }
  int packed = nl | (ns << 12);   // (a tile's sums are at most 1024 each)
  for (int s = 32; s > 0; s >>= 1) packed += __shfl_xor(packed, s, 64);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = packed;
  asd_syncthreads();
  if (threadIdx.x == 0) {
    const int sum = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    const int tile = blockIdx.x * a.tiles_per_kf + blockIdx.y;
    a.tile_cnt[2 * tile] = sum & 0xfff;
    a.tile_cnt[2 * tile + 1] = sum >> 12;
  }
}
__global__ __launch_bounds__(256) void k_lm_tilescan(const int* __restrict__ tile_cnt, int* __restrict__ tile_off, int n_tiles, int* __restrict__ head) {
  __shared__ int s_scan[256];
  int run[2] = {0, 0};
  for (int base = 0; base < n_tiles; base += 256) {
    const int i = base + threadIdx.x;
    for (int f = 0; f < 2; ++f) {
      const int v = i < n_tiles ? tile_cnt[2 * i + f] : 0;
      int total;
      const int ex = lm_block_scan(v, s_scan, &total);
      if (i < n_tiles) tile_off[2 * i + f] = run[f] + ex;
      run[f] += total;
    }
  }
  if (threadIdx.x == 0) { head[8] = run[0]; head[9] = run[1]; }
}
__global__ __launch_bounds__(256) void k_lm_scatter(LmPointArgs a) {
  __shared__ int s_wave[4];
  const int tile = blockIdx.x * a.tiles_per_kf + blockIdx.y;
  int ol = a.tile_off[2 * tile], os = a.tile_off[2 * tile + 1];
  for (int k = 0; k < 4; ++k) {
    long long pos = 0;
    const int r = lm_entry(a, k, &pos);
    const bool win = r >= 0 && a.claim[r] == (int)pos;
    const bool srch = win && !(a.mark[r] & kSkipBit);
    int tl, ts;
    const int pl = lm_block_scan_flag(win, s_wave, &tl);
    const int ps = lm_block_scan_flag(srch, s_wave, &ts);
    if (win) {
      a.d_local[ol + pl] = r;
      if (ol + pl < a.cap_local) a.h_local[ol + pl] = r;
      a.claim[r] = kClaimFree;   // every other entry of this point compares its own position, which is never this value
    }
    if (srch) {
      a.d_search[os + ps] = r;
      if (os + ps < a.cap_search) a.h_search[os + ps] = r;
    }
    ol += tl; os += ts;
  }
}

// ---- KeyFrameCulling and Observations()
struct LmCullArgs {
  const LmSlotDev* table; const int* rows; const uint8_t* oct; const uint8_t* pbad; const int* mark;
  const int* cand_slot; const uint8_t* cand_flags; int n_cand;   // slot -1: skipped (:751-754)
  int* cnt; int* gone;         // per compacted point: observations per octave [16]; 1 = EraseObservation turned it bad in this call
  int* bad_rows;               // out: those points in the order it happened
  int* culled;                 // [slots] 1 = SetBadFlag took effect
  int* out;                    // [3][n_cand]: decision, nMPs, nRedundantObservations
  int* head;                   // head[10] = number of bad_rows
};

// the compacted points get their position (+ 1) in the mark table and clean counters; head[8] = their number
__global__ __launch_bounds__(256) void k_cull_index(const int* __restrict__ pts, const int* __restrict__ head, int* __restrict__ mark,
                                                    int* __restrict__ cnt, int* __restrict__ gone) {
  const int ci = blockIdx.x * 256 + threadIdx.x;
  if (ci >= head[8]) return;
  mark[pts[ci]] = ci + 1;
  gone[ci] = 0;
  int4* q = reinterpret_cast<int4*>(cnt + (size_t)ci * kLevels);
  const int4 z = make_int4(0, 0, 0, 0);
  for (int k = 0; k < kLevels / 4; ++k) q[k] = z;
}
// ONE pass over the table, one wave per slot: every entry that names a marked point counts, at its octave (levels = 16) or at all (1)
__global__ __launch_bounds__(256) void k_cull_count(const LmSlotDev* __restrict__ table, int n_slots, const int* __restrict__ rows,
                                                    const uint8_t* __restrict__ oct, const int* __restrict__ mark, int* __restrict__ cnt, int levels) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= n_slots) return;
  const long long off = table[slot].off;
  const int n = table[slot].n;
  for (int i = lane; i < n; i += 64) {
    const int r = rows[off + i];
    if (r < 0) continue;
    const int m = mark[r];
    if (m > 0) atomicAdd(&cnt[(size_t)(m - 1) * levels + (levels > 1 ? (oct[off + i] & (kLevels - 1)) : 0)], 1);
  }
}
// the point of table entry e as the walk sees it now: its compacted position, or -1 (none, bad, or turned bad by an earlier cull)
__device__ inline int cull_point(const LmCullArgs& a, long long e) {
  const int r = a.rows[e];
  if (r < 0 || a.pbad[r]) return -1;
  const int ci = a.mark[r] - 1;
  return ci >= 0 && !a.gone[ci] ? ci : -1;
}
// the sequential part (:748-808) as ONE workgroup.  A point occurs once per row (the table's precondition), so the threads of a round
// touch different counters; the barrier at the end of a candidate orders its decrements before the next candidate's reads.
__global__ __launch_bounds__(256) void k_cull_walk(LmCullArgs a) {
  __shared__ int s_red[4][2], s_wave[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int n_bad = 0;
  for (int c = 0; c < a.n_cand; ++c) {
    const int sl = a.cand_slot[c];
    if (sl < 0) {   // (the same for every thread)
      if (t == 0) { a.out[c] = 3; a.out[a.n_cand + c] = 0; a.out[2 * a.n_cand + c] = 0; }
      continue;
    }
    const long long off = a.table[sl].off;
    const int n = a.table[sl].n;
    int nm = 0, nr = 0;
    for (int i = t; i < n; i += 256) {
      const int ci = cull_point(a, off + i);
      if (ci < 0) continue;
      ++nm;
      const int* q = a.cnt + (size_t)ci * kLevels;
      const int lim = min((a.oct[off + i] & (kLevels - 1)) + 1, kLevels - 1);
      int total = 0, upto = 0;   // Observations(), and the observations at an octave <= scaleLevel + 1 -- the keyframe's own among them
      for (int k = 0; k < kLevels; ++k) { const int v = q[k]; total += v; if (k <= lim) upto += v; }
      if (total > 3 && upto - 1 >= 3) ++nr;
    }
    for (int s = 32; s > 0; s >>= 1) { nm += __shfl_xor(nm, s, 64); nr += __shfl_xor(nr, s, 64); }
    if (lane == 0) { s_red[w][0] = nm; s_red[w][1] = nr; }
    asd_syncthreads();
    nm = s_red[0][0] + s_red[1][0] + s_red[2][0] + s_red[3][0];
    nr = s_red[0][1] + s_red[1][1] + s_red[2][1] + s_red[3][1];
    const bool cull = 10 * nr > 9 * nm;   // nRedundantObservations > 0.9 * nMPs (:805); rows hold at most 65536 entries
    const int decision = !cull ? 0 : (a.cand_flags[c] & 2) ? 2 : 1;
    if (decision == 1) {   // SetBadFlag: the observations leave in ascending keypoint index
      for (int base = 0; base < n; base += 256) {
        const int i = base + t;
        bool turned = false;
        int r = -1;
        if (i < n) {
          const int ci = cull_point(a, off + i);
          if (ci >= 0) {
            int* q = a.cnt + (size_t)ci * kLevels;
            q[a.oct[off + i] & (kLevels - 1)] -= 1;
            int total = 0;
            for (int k = 0; k < kLevels; ++k) total += q[k];
            if (total <= 2) { turned = true; a.gone[ci] = 1; r = a.rows[off + i]; }   // MapPoint.cc:136-141
          }
        }
        int round;
        const int pos = lm_block_scan_flag(turned, s_wave, &round);
        if (turned) a.bad_rows[n_bad + pos] = r;
        n_bad += round;
      }
      if (t == 0) a.culled[sl] = 1;
    }
    if (t == 0) { a.out[c] = decision; a.out[a.n_cand + c] = nm; a.out[2 * a.n_cand + c] = nr; }
    asd_syncthreads();
  }
  if (t == 0) a.head[10] = n_bad;
}
// apply = 1: the culled keyframes' rows and every entry of a point that turned bad become -1; the culled keyframes become bad
__global__ __launch_bounds__(256) void k_cull_apply(LmSlotDev* __restrict__ table, int n_slots, int* __restrict__ rows, const int* __restrict__ mark,
                                                    const int* __restrict__ gone, const int* __restrict__ culled) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= n_slots) return;
  const long long off = table[slot].off;
  const int n = table[slot].n;
  if (n < 0) return;
  const bool all = culled[slot] != 0;
  for (int i = lane; i < n; i += 64) {
    const int r = rows[off + i];
    if (r < 0) continue;
    const int m = mark[r];
    if (all || (m > 0 && gone[m - 1])) rows[off + i] = -1;
  }
  if (all && lane == 0) table[slot].bad = 1;
}
// the marks are undone; with apply the points that turned bad get their byte
__global__ __launch_bounds__(256) void k_cull_finish(const int* __restrict__ pts, const int* __restrict__ head, int* __restrict__ mark,
                                                     const int* __restrict__ gone, uint8_t* __restrict__ pbad, int apply) {
  const int ci = blockIdx.x * 256 + threadIdx.x;
  if (ci >= head[8]) return;
  const int r = pts[ci];
  mark[r] = 0;
  if (apply && gone[ci]) pbad[r] = 1;
}
// asd_map_observations: a row asked for twice shares one counter (the larger position wins, whatever the scheduling)
// (a row beyond the row tables has never been named by an entry: it counts 0 and the tables do not grow for it)
__global__ __launch_bounds__(256) void k_obs_mark(const int* __restrict__ rows, int n, int row_cap, int* __restrict__ mark) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && rows[i] < row_cap) atomicMax(&mark[rows[i]], i + 1);
}
__global__ __launch_bounds__(256) void k_obs_gather(const int* __restrict__ rows, int n, int row_cap, const int* __restrict__ mark, const int* __restrict__ cnt,
                                                    int* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = rows[i] < row_cap ? cnt[mark[rows[i]] - 1] : 0;
}
__global__ __launch_bounds__(256) void k_obs_unmark(const int* __restrict__ rows, int n, int row_cap, int* __restrict__ mark) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && rows[i] < row_cap) mark[rows[i]] = 0;
}

// ---- MapPoint::UpdateNormalAndDepth
struct LmNdArgs {
  const LmSlotDev* table; int n_slots; const int* rows; const uint8_t* oct; const uint8_t* pbad; const int* mark; int row_cap;
  const float* center;         // [slots][3]
  const int* req; const int* ref_slot; const float* xw; int n;   // the call's points: bank row, slot of mpRefKF (-1: not in the table; k_nd_mark), new position or null
  const int* cnt; int* cursor; const int* seg_off;                // per point: observers, fill cursor, start of its segment
  int* lvl;                    // per point: the octave of ref_kf's entry, -1 = its row does not name the point
  int2* seg;                   // (keyframe id, slot) per observation, segment by segment, in the order the fill met them
  int* ord;                    // the slots of a segment in ascending keyframe id
  float* attr;                 // the attribute bank
  float* res;                  // out [n][6], pinned host memory: normal, min, max, status (as int bits)
  float scale[kLevels]; float scale_top;
};

// the requested rows get their position (+ 1) in the mark table (distinct rows; a row beyond the row tables has no entry and stays unmarked)
// and mpRefKF's id becomes its slot, or -1 (the ascending id list of refresh_lists)
__global__ __launch_bounds__(256) void k_nd_mark(const int* __restrict__ req, int n, int row_cap, int* __restrict__ mark, int* __restrict__ cnt,
                                                 int* __restrict__ cursor, int* __restrict__ lvl, const int* __restrict__ ref_id,
                                                 const int* __restrict__ sorted_id, const int* __restrict__ sorted_slot, int n_live, int* __restrict__ ref_slot) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  cnt[i] = 0; cursor[i] = 0; lvl[i] = -1;
  ref_slot[i] = lm_lookup(sorted_id, sorted_slot, n_live, ref_id[i]);
  if (req[i] < row_cap) mark[req[i]] = i + 1;
}
// exclusive prefix of the counts in ONE workgroup, 16 consecutive points per thread and round; head[12..13] = the total (64 bit)
__global__ __launch_bounds__(256) void k_nd_scan(const int* __restrict__ cnt, int n, int* __restrict__ seg_off, int* __restrict__ head) {
  __shared__ int s_scan[256];
  long long run = 0;
  for (int base = 0; base < n; base += 4096) {
    const int i0 = base + threadIdx.x * 16;
    int v[16], mine = 0;
    for (int k = 0; k < 16; ++k) { v[k] = i0 + k < n ? cnt[i0 + k] : 0; mine += v[k]; }
    int total;
    int ex = lm_block_scan(mine, s_scan, &total);
    for (int k = 0; k < 16; ++k) {
      if (i0 + k < n) seg_off[i0 + k] = (int)(run + ex);   // (meaningless beyond kMaxNdEntries: the host reads the total first)
      ex += v[k];
    }
    run += total;
  }
  if (threadIdx.x == 0) { seg_off[n] = (int)run; head[12] = (int)(unsigned)(run & 0xffffffffll); head[13] = (int)(run >> 32); }   // (head: pinned host memory)
}
// the second pass over the table, one wave per slot: every entry that names a marked point drops (id, slot) into the point's segment
// through an integer cursor; the entry of mpRefKF leaves its octave.  The order inside a segment is whatever the scheduling made it:
// k_nd_order undoes that.
__global__ __launch_bounds__(256) void k_nd_fill(LmNdArgs a) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= a.n_slots) return;
  const long long off = a.table[slot].off;
  const int n = a.table[slot].n, id = a.table[slot].id;
  for (int i = lane; i < n; i += 64) {
    const int r = a.rows[off + i];
    if (r < 0) continue;
    const int m = a.mark[r];
    if (m <= 0) continue;
    const int p = atomicAdd(&a.cursor[m - 1], 1);
    if (p < a.cnt[m - 1]) a.seg[(size_t)a.seg_off[m - 1] + p] = make_int2(id, slot);   // (the count pass saw the same table: p is always inside)
    if (slot == a.ref_slot[m - 1]) a.lvl[m - 1] = a.oct[off + i] & (kLevels - 1);
  }
}
// one wave per point: the rank of every observer by comparison (the ids of a segment are distinct: a point occurs once per row), the slots
// written in that order.  Lanes read the same id together, so a segment costs len^2 / 64 broadcast loads.
__global__ __launch_bounds__(256) void k_nd_order(LmNdArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n) return;
  const int len = a.cnt[i];
  const int2* seg = a.seg + a.seg_off[i];
  int* ord = a.ord + a.seg_off[i];
  for (int e = lane; e < len; e += 64) {
    const int2 me = seg[e];
    int rank = 0;
    for (int j = 0; j < len; ++j) { const int o = seg[j].x; rank += o < me.x || (o == me.x && j < e); }   // (a table that breaks the precondition still gets a permutation)
    ord[rank] = me.y;
  }
}
// one wave per point: MapPoint.cc:361-407.  The units of up to 64 observers are computed side by side, then added one after the other in
// ascending keyframe id -- every lane forms the same f32 sum from the same values, lane 0 stores it.
__global__ __launch_bounds__(256) void k_nd_point(LmNdArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n) return;
  const int r = a.req[i];
  float* row = a.attr + 8 * (size_t)r;
  float Pos[3];
  if (a.xw) { Pos[0] = a.xw[3 * (size_t)i]; Pos[1] = a.xw[3 * (size_t)i + 1]; Pos[2] = a.xw[3 * (size_t)i + 2]; }   // SetWorldPos: no bad test
  else { Pos[0] = row[0]; Pos[1] = row[1]; Pos[2] = row[2]; }
  const int len = a.cnt[i], lvl = a.lvl[i];
  const int status = (r < a.row_cap && a.pbad[r]) ? 1 : len == 0 ? 2 : lvl < 0 ? 3 : 0;
  float out[5] = {row[3], row[4], row[5], row[6], row[7]};
  if (status == 0) {
    const int* ord = a.ord + a.seg_off[i];
    float sum[3] = {0.f, 0.f, 0.f};
    for (int base = 0; base < len; base += 64) {
      const int m = min(64, len - base);
      float u[3] = {0.f, 0.f, 0.f};
      if (lane < m) asd_nd_unit(Pos, a.center + 3 * (size_t)ord[base + lane], u);
      for (int k = 0; k < m; ++k) {
        const float v[3] = {__shfl(u[0], k, 64), __shfl(u[1], k, 64), __shfl(u[2], k, 64)};
        asd_nd_add(sum, v);
      }
    }
    float unused[3];
    const double nrm_ref = asd_nd_unit(Pos, a.center + 3 * (size_t)a.ref_slot[i], unused);
    asd_nd_finish(sum, len, nrm_ref, a.scale[lvl], a.scale_top, out, out + 3, out + 4);
  }
  if (lane == 0) {
    if (a.xw) { row[0] = Pos[0]; row[1] = Pos[1]; row[2] = Pos[2]; }
    if (status == 0) for (int k = 0; k < 5; ++k) row[3 + k] = out[k];
    float* q = a.res + 6 * (size_t)i;
    for (int k = 0; k < 5; ++k) q[k] = out[k];
    q[5] = __int_as_float(status);
  }
}
// asd_map_kf_centers: distinct slots
__global__ __launch_bounds__(256) void k_nd_set_centers(float* __restrict__ center, const int* __restrict__ slot, const float* __restrict__ val, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float* c = center + 3 * (size_t)slot[i];
  c[0] = val[3 * i]; c[1] = val[3 * i + 1]; c[2] = val[3 * i + 2];
}

// ---- Optimizer::LocalBundleAdjustment: the graph (Optimizer.cc:418-467, :534-593) and the erase policy (:652-697)
struct LmBgArgs {
  const LmSlotDev* table; const int* rows; const uint8_t* oct; const int* mark; int n_slots;
  const int* pts; int n;                          // lLocalMapPoints (the compaction's list) and their number
  const int* cnt; int* cursor; const int* seg_off;   // per point: Observations(), fill cursor, start of its segment
  int4* useg; int4* oseg;                         // (keyframe id, slot, keypoint index | octave << 16, point) as the fill met them / in ascending id
  const uint8_t* local;                           // [slots] 1 = member of lLocalKeyFrames
  int* kf_claim;                                  // [slots] the first position in the ordered segments that names a not-local, not-bad keyframe
  long long total;                                // entries of all segments
  int* tile_cnt; const int* tile_off;             // [tiles][2]: fixed keyframes first met in the tile, edges of the tile
  int* fixed; int* e_ent;                         // out: lFixedCameras as ids; edge -> position in the ordered segments
};
struct LmBgEdgeArgs {
  const int4* oseg; const int* e_ent; const int* rank; const int* pose_idx; int n_edges; int cap;
  int* e_point; int* e_pose; int* e_kf; int* e_idx; uint8_t* e_oct;   // pinned host memory, as far as the caller's capacity goes
};
struct LmBaArgs {
  LmSlotDev* table; int* rows; uint8_t* pbad;
  const int* pts; int n; const int* cnt; const int* seg_off; const int4* oseg;
  const uint8_t* flagged;      // per segment entry: its edge is in vToErase
  int* gone; const int* boff;  // per point: turned bad; its place in bad_rows
  int* new_ref; int* bad_rows; int bad_cap;   // pinned host memory
  int* head;                   // head[14] += observations erased
  int apply;
};

// the compacted points get their position (+ 1) in the mark table, a clean counter and a clean cursor
__global__ __launch_bounds__(256) void k_bg_index(const int* __restrict__ pts, int n, int* __restrict__ mark, int* __restrict__ cnt, int* __restrict__ cursor) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  mark[pts[i]] = i + 1;
  cnt[i] = 0; cursor[i] = 0;
}
// point_rank: the marked rows counted in row order -- tiles of the row tables, then k_lm_tilescan, then the ranks
__global__ __launch_bounds__(256) void k_bg_rank_count(const int* __restrict__ mark, int row_cap, int* __restrict__ tile_cnt) {
  __shared__ int s_wave[4];
  int c = 0;
  for (int k = 0; k < 4; ++k) {
    const long long r = (long long)blockIdx.x * kTile + k * 256 + threadIdx.x;
    c += r < row_cap && mark[r] > 0;
  }
  for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s, 64);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
  asd_syncthreads();
  if (threadIdx.x == 0) { tile_cnt[2 * blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]; tile_cnt[2 * blockIdx.x + 1] = 0; }
}
__global__ __launch_bounds__(256) void k_bg_rank_scatter(const int* __restrict__ mark, int row_cap, const int* __restrict__ tile_off, int* __restrict__ rank) {
  __shared__ int s_wave[4];
  int o = tile_off[2 * blockIdx.x];
  for (int k = 0; k < 4; ++k) {
    const long long r = (long long)blockIdx.x * kTile + k * 256 + threadIdx.x;
    const int m = r < row_cap ? mark[r] : 0;
    int total;
    const int p = lm_block_scan_flag(m > 0, s_wave, &total);
    if (m > 0) rank[m - 1] = o + p;
    o += total;
  }
}
// k_nd_fill with the keypoint index and the octave kept: one wave per slot, every entry that names a marked point drops into the point's
// segment through an integer cursor
__global__ __launch_bounds__(256) void k_bg_fill(LmBgArgs a) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= a.n_slots) return;
  const long long off = a.table[slot].off;
  const int n = a.table[slot].n, id = a.table[slot].id;
  for (int i = lane; i < n; i += 64) {
    const int r = a.rows[off + i];
    if (r < 0) continue;
    const int m = a.mark[r];
    if (m <= 0) continue;
    const int p = atomicAdd(&a.cursor[m - 1], 1);
    if (p < a.cnt[m - 1]) a.useg[(size_t)a.seg_off[m - 1] + p] = make_int4(id, slot, i | ((a.oct[off + i] & (kLevels - 1)) << 16), m - 1);
  }
}
// k_nd_order with the whole entry moved: one wave per point ranks its observers by keyframe id.  The position of an entry in the ordered
// segments is the moment the walk of :453-467 meets it: a keyframe that is neither local nor bad is claimed by the smallest one.
__global__ __launch_bounds__(256) void k_bg_order(LmBgArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n) return;
  const int len = a.cnt[i], base = a.seg_off[i];
  const int4* seg = a.useg + base;
  for (int e = lane; e < len; e += 64) {
    const int4 me = seg[e];
    int rank = 0;
    for (int j = 0; j < len; ++j) { const int o = seg[j].x; rank += o < me.x || (o == me.x && j < e); }
    a.oseg[base + rank] = me;
    if (!a.local[me.y] && !a.table[me.y].bad) atomicMin(&a.kf_claim[me.y], base + rank);
  }
}
// the ordered segments as one array in tiles of 1024: the claimants are lFixedCameras in order, the entries of not-bad keyframes the edges
__device__ inline void bg_entry(const LmBgArgs& a, int k, bool* win, bool* edge, long long* pos, int* id) {
  *pos = (long long)blockIdx.x * kTile + k * 256 + threadIdx.x;
  *win = false; *edge = false; *id = -1;
  if (*pos >= a.total) return;
  const int4 s = a.oseg[*pos];
  *win = a.kf_claim[s.y] == (int)*pos;
  *edge = !a.table[s.y].bad;
  *id = s.x;
}
__global__ __launch_bounds__(256) void k_bg_count(LmBgArgs a) {
  __shared__ int s_wave[4];
  int nf = 0, ne = 0;
  for (int k = 0; k < 4; ++k) {
    bool win, edge; long long pos; int id;
    bg_entry(a, k, &win, &edge, &pos, &id);
    nf += win; ne += edge;
  }
  int packed = nf | (ne << 12);
  for (int s = 32; s > 0; s >>= 1) packed += __shfl_xor(packed, s, 64);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = packed;
  asd_syncthreads();
  if (threadIdx.x == 0) {
    const int sum = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    a.tile_cnt[2 * blockIdx.x] = sum & 0xfff;
    a.tile_cnt[2 * blockIdx.x + 1] = sum >> 12;
  }
}
__global__ __launch_bounds__(256) void k_bg_scatter(LmBgArgs a) {
  __shared__ int s_wave[4];
  int of = a.tile_off[2 * blockIdx.x], oe = a.tile_off[2 * blockIdx.x + 1];
  for (int k = 0; k < 4; ++k) {
    bool win, edge; long long pos; int id;
    bg_entry(a, k, &win, &edge, &pos, &id);
    int tf, te;
    const int pf = lm_block_scan_flag(win, s_wave, &tf);
    const int pe = lm_block_scan_flag(edge, s_wave, &te);
    if (win) a.fixed[of + pf] = id;
    if (edge) a.e_ent[oe + pe] = (int)pos;
    of += tf; oe += te;
  }
}
__global__ __launch_bounds__(256) void k_bg_edges(LmBgEdgeArgs a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.n_edges || e >= a.cap) return;
  const int4 s = a.oseg[a.e_ent[e]];
  a.e_point[e] = a.rank[s.w];
  a.e_pose[e] = a.pose_idx[s.y];
  a.e_kf[e] = s.x;
  a.e_idx[e] = s.z & 0xffff;
  a.e_oct[e] = (uint8_t)(s.z >> 16);
}
// Converter::toVector3d of the points' positions, in point_rank order; a row outside the attribute bank is reported, not read
__global__ __launch_bounds__(256) void k_bg_xw(const int* __restrict__ pts, const int* __restrict__ rank, int n, const float* __restrict__ attr, int attr_cap,
                                               double* __restrict__ xw, int* __restrict__ head) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int r = pts[i];
  if (r >= attr_cap) { atomicMax(&head[15], r + 1); return; }
  double* q = xw + 3 * (size_t)rank[i];
  for (int k = 0; k < 3; ++k) q[k] = (double)attr[8 * (size_t)r + k];
}
__global__ __launch_bounds__(256) void k_ba_flag(const uint8_t* __restrict__ erase, const int* __restrict__ e_ent, int n_edges, uint8_t* __restrict__ flagged) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n_edges && erase[e]) flagged[e_ent[e]] = 1;
}
// one wave per point, the closed form of the sequential erasure: left = Observations() - flagged edges; the point turns bad when it has
// a flagged edge and left <= 2; otherwise mpRefKF's candidate is the lowest id left
__global__ __launch_bounds__(256) void k_ba_point(LmBaArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n) return;
  const int len = a.cnt[i], base = a.seg_off[i];
  int nflag = 0, first = INT_MAX;
  for (int e = lane; e < len; e += 64) {
    if (a.flagged[base + e]) ++nflag; else first = min(first, e);
  }
  for (int s = 32; s > 0; s >>= 1) { nflag += __shfl_xor(nflag, s, 64); first = min(first, __shfl_xor(first, s, 64)); }
  if (lane) return;
  const bool bad = nflag > 0 && len - nflag <= 2;
  a.gone[i] = bad;
  a.new_ref[i] = nflag > 0 && !bad ? a.oseg[base + first].x : -1;
  const int erased = nflag == 0 ? 0 : bad ? max(1, len - 2) : nflag;   // the pairs behind the one that turned the point bad are no-ops
  if (erased) atomicAdd(&a.head[14], erased);
}
// bad_rows in lLocalMapPoints order; with apply the flagged entries and every entry of a point that turned bad become -1, through the segments
__global__ __launch_bounds__(256) void k_ba_write(LmBaArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.n) return;
  const int len = a.cnt[i], base = a.seg_off[i];
  const bool g = a.gone[i] != 0;
  if (g && lane == 0) {
    if (a.boff[i] < a.bad_cap) a.bad_rows[a.boff[i]] = a.pts[i];
    if (a.apply) a.pbad[a.pts[i]] = 1;
  }
  if (!a.apply) return;
  for (int e = lane; e < len; e += 64) {
    if (!g && !a.flagged[base + e]) continue;
    const int4 s = a.oseg[base + e];
    a.rows[a.table[s.y].off + (s.z & 0xffff)] = -1;
  }
}

// ---- ORBmatcher::Fuse's side effects (ORBmatcher.cc:939-955, :1065-1079; LoopClosing.cc:540-555, :619-627) and MapPoint::Replace
// (MapPoint.cc:206-244).  The points that can take part are known at entry: the candidates that carry a best_idx (the hits; point index
// j = their place among the hits) and what kf's row holds at those keypoints (point index nh + j for the hit that claims the point).
struct LmFaArgs {
  const LmSlotDev* table; int* rows; uint8_t* pbad; int* mark; int n_slots;
  int kf_slot; long long kf_off; int mode;
  const int* cand; const int* best; int nh; int P;   // the hits: bank row and keypoint of kf; P = 2 nh points
  int* cnt; int* cursor; int* seg_off;               // per point: Observations() as the walk proceeds, fill cursor, start of its segment [P + 1]
  int* pt_row; int* gone; int* head; int* tail;      // per point: bank row (-1: unused index), replaced in this call, its chain of segments
  int* inkf; int* inkf0;                             // per point: the keypoint of kf that names it, now / at entry (-1: none)
  int* next;                                         // per segment [P + nh]: the next one of the chain; segment P + j is the spare entry of hit j
  int* oidx;                                         // per hit: pMPinKF as a point index
  int4* ent; int total;                              // (slot, keypoint index, the point the fill found there, the point that owns it now or -1)
  int* krow;                                         // kf's row as point indices, valid at the hits' keypoints
  int* stamp;                                        // [slots] the Replace that met a live entry of the winner in that keyframe last
  int* out;                                          // [6][nh]: action, other (bank row), obs_cand, obs_other, n_moved, n_dropped
  int apply;
};

__global__ __launch_bounds__(256) void k_fa_mark_cand(const int* __restrict__ cand, int nh, int* __restrict__ mark) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < nh) mark[cand[j]] = j + 1;   // (distinct rows)
}
// what kf's row holds at the hits' keypoints: a point that is no candidate belongs to the largest hit that meets it, whatever the scheduling
__global__ __launch_bounds__(256) void k_fa_mark_other(LmFaArgs a) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.nh) return;
  const int q = a.rows[a.kf_off + a.best[j]];
  if (q < 0) return;
  const int m = a.mark[q];
  if (m == 0 || m > a.nh) atomicMax(&a.mark[q], a.nh + j + 1);
}
__global__ __launch_bounds__(256) void k_fa_index(LmFaArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.P) return;
  a.cnt[i] = 0; a.cursor[i] = 0; a.gone[i] = 0; a.inkf[i] = -1; a.inkf0[i] = -1;
  const int j = i < a.nh ? i : i - a.nh;
  const int q = a.rows[a.kf_off + a.best[j]];
  if (i < a.nh) {
    a.pt_row[i] = a.cand[i];
    a.krow[a.best[j]] = q >= 0 ? a.mark[q] - 1 : -1;   // (hits that share a keypoint store the same value)
  } else {
    a.pt_row[i] = q >= 0 && a.mark[q] == i + 1 ? q : -1;
  }
}
// k_bg_fill without the octave plane; the entry of kf leaves its keypoint with the point
__global__ __launch_bounds__(256) void k_fa_fill(LmFaArgs a) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= a.n_slots) return;
  const long long off = a.table[slot].off;
  const int n = a.table[slot].n;
  for (int i = lane; i < n; i += 64) {
    const int r = a.rows[off + i];
    if (r < 0) continue;
    const int m = a.mark[r];
    if (m <= 0) continue;
    const int p = atomicAdd(&a.cursor[m - 1], 1);
    if (p < a.seg_off[m] - a.seg_off[m - 1]) a.ent[(size_t)a.seg_off[m - 1] + p] = make_int4(slot, i, m - 1, m - 1);   // (the count pass saw the same table)
    if (slot == a.kf_slot) { a.inkf[m - 1] = i; a.inkf0[m - 1] = i; }
  }
}
__device__ inline void fa_seg(const LmFaArgs& a, int s, int* base, int* len) {
  if (s < a.P) { *base = a.seg_off[s]; *len = a.seg_off[s + 1] - *base; }
  else { *base = a.total + (s - a.P); *len = 1; }
}
// The ordered walk as ONE workgroup.  Thread 0 takes the hits one after the other -- gate, empty entry, bad entry, the comparison of the
// two Observations() -- and stops at a Replace(L -> W), which all threads do together: the live entries of W's chain stamp their keyframes,
// the live entries of L's chain are re-seated on W or dropped by that stamp, L's chain is appended to W's.  The keyframes of one point are
// distinct, so the threads of a round touch different stamps and the counts are sums: nothing depends on the order inside a segment.
__global__ __launch_bounds__(256) void k_fa_walk(LmFaArgs a) {
  __shared__ int s_dec[4], s_red[4][2];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int p = t; p < a.P; p += 256) { const int h = a.cnt[p] > 0 ? p : -1; a.head[p] = h; a.tail[p] = h; }
  for (int s = t; s < a.P + a.nh; s += 256) a.next[s] = -1;
  for (int j = t; j < a.nh; j += 256) a.ent[(size_t)a.total + j] = make_int4(a.kf_slot, a.best[j], j, -1);
  asd_syncthreads();
  int* const o_act = a.out; int* const o_oth = a.out + a.nh; int* const o_oc = a.out + 2 * a.nh; int* const o_oo = a.out + 3 * a.nh;
  int* const o_mv = a.out + 4 * a.nh; int* const o_dr = a.out + 5 * a.nh;
  const int last = a.mode == 1 ? 2 * a.nh : a.nh;   // mode 1: the hits once more for SearchAndFuse's loop (LoopClosing.cc:619-627)
  int pos = 0, step = 0;                            // pos: thread 0's place in the walk
  while (true) {
    if (t == 0) {
      int kind = 0, L = -1, W = -1, hit = -1;
      for (; pos < last && !kind; ++pos) {
        const int j = pos < a.nh ? pos : pos - a.nh;
        if (pos >= a.nh) {   // pass 2: vpReplacePoint[i]->Replace(vpPoints[i]), no test at all
          if (o_act[j] != 3) continue;
          L = a.oidx[j]; W = j; hit = j; kind = 1;
          o_oc[j] = a.cnt[W]; o_oo[j] = a.cnt[L];
          continue;
        }
        const int b = a.best[j], q = a.krow[b];
        const bool cbad = a.pbad[a.pt_row[j]] || a.gone[j];
        int act, oth = -1, oc = 0, oo = 0;
        if (a.mode == 0 && (cbad || a.inkf[j] >= 0)) act = 7;         // :849, at the candidate's turn
        else if (a.mode == 1 && (cbad || a.inkf0[j] >= 0)) act = 7;   // :979, :992: spAlreadyFound is a snapshot
        else if (q < 0) {
          oc = a.cnt[j];
          if (a.mode == 2 && a.inkf[j] >= 0) act = 6;                 // not restated: the table holds a point once per row
          else {                                                      // AddObservation + AddMapPoint
            act = 1;
            a.krow[b] = j; a.inkf[j] = b; a.cnt[j] = oc + 1;
            reinterpret_cast<int*>(a.ent + (size_t)a.total + j)[3] = j;
            if (a.head[j] < 0) a.head[j] = a.P + j; else a.next[a.tail[j]] = a.P + j;
            a.tail[j] = a.P + j;
          }
        } else {
          oth = a.pt_row[q]; oc = a.cnt[j]; oo = a.cnt[q];
          a.oidx[j] = q;
          if (q == j) act = 5;
          else if (a.mode != 2 && (a.pbad[oth] || a.gone[q])) act = 4;
          else if (a.mode == 1) { act = 3; oc = 0; oo = 0; }          // noted; pass 2 fills the counts when it acts
          else if (a.mode == 0 && oo > oc) { act = 2; kind = 1; L = j; W = q; hit = j; }
          else { act = 3; kind = 1; L = q; W = j; hit = j; }
        }
        o_act[j] = act; o_oth[j] = oth; o_oc[j] = oc; o_oo[j] = oo; o_mv[j] = 0; o_dr[j] = 0;
      }
      s_dec[0] = kind; s_dec[1] = L; s_dec[2] = W; s_dec[3] = hit;
    }
    asd_syncthreads();
    if (!s_dec[0]) break;   // (the same for every thread)
    const int L = s_dec[1], W = s_dec[2], hit = s_dec[3];
    ++step;
    for (int s = a.head[W]; s >= 0; s = a.next[s]) {
      int base, len;
      fa_seg(a, s, &base, &len);
      for (int e = t; e < len; e += 256) { const int4 x = a.ent[(size_t)base + e]; if (x.w >= 0) a.stamp[x.x] = step; }
    }
    asd_syncthreads();
    int mv = 0, dr = 0;
    for (int s = a.head[L]; s >= 0; s = a.next[s]) {
      int base, len;
      fa_seg(a, s, &base, &len);
      for (int e = t; e < len; e += 256) {
        const int4 x = a.ent[(size_t)base + e];
        if (x.w < 0) continue;
        const bool in_w = a.stamp[x.x] == step;   // pMP->IsInKeyFrame(pKF)
        reinterpret_cast<int*>(a.ent + (size_t)base + e)[3] = in_w ? -1 : W;
        if (in_w) ++dr; else ++mv;
        if (x.x == a.kf_slot) { a.krow[x.y] = in_w ? -1 : W; if (!in_w) a.inkf[W] = x.y; }
      }
    }
    for (int s = 32; s > 0; s >>= 1) { mv += __shfl_xor(mv, s, 64); dr += __shfl_xor(dr, s, 64); }
    if (lane == 0) { s_red[w][0] = mv; s_red[w][1] = dr; }
    asd_syncthreads();
    if (t == 0) {
      mv = s_red[0][0] + s_red[1][0] + s_red[2][0] + s_red[3][0];
      dr = s_red[0][1] + s_red[1][1] + s_red[2][1] + s_red[3][1];
      o_mv[hit] = mv; o_dr[hit] = dr;
      a.cnt[W] += mv; a.cnt[L] = 0; a.gone[L] = 1; a.inkf[L] = -1;
      const int h = a.head[L];
      if (h >= 0) {
        if (a.head[W] < 0) a.head[W] = h; else a.next[a.tail[W]] = h;
        a.tail[W] = a.tail[L];
        a.head[L] = -1; a.tail[L] = -1;
      }
    }
    // (thread 0 goes on with the walk; everybody else waits for it at the barrier above)
  }
}
// apply = 1, THROUGH the segments: an entry of another keyframe whose owner changed is rewritten; kf's own row is written from the walk's
// view of it (its keypoints can be emptied and taken again, so several segment entries may stand for one of them)
__global__ __launch_bounds__(256) void k_fa_write(LmFaArgs a) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < a.total) {
    const int4 x = a.ent[e];
    if (x.x != a.kf_slot && x.w != x.z) a.rows[a.table[x.x].off + x.y] = x.w < 0 ? -1 : a.pt_row[x.w];
  } else if (e < (long long)a.total + a.nh) {
    const int b = a.best[e - a.total], v = a.krow[b];
    a.rows[a.kf_off + b] = v < 0 ? -1 : a.pt_row[v];
  }
}
// the marks are undone; with apply the losers get their bad byte
__global__ __launch_bounds__(256) void k_fa_finish(LmFaArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.P) return;
  const int r = a.pt_row[i];
  if (r < 0) return;
  a.mark[r] = 0;
  if (a.apply && a.gone[i]) a.pbad[r] = 1;
}

struct LmSlot {
  int kf = -1;   // -1: free slot
  int n = -1;
  long long off = 0;
  bool bad = false;
  bool has_oct = false;   // asd_map_put_octaves has filled the octave plane of this row
  bool has_center = false;   // asd_map_kf_centers has set this slot's camera centre
  int n_cov = 0, cov[kMaxCov] = {};
  int parent = -1;
  std::vector<int> children;
};

struct LocalMapState {
  std::vector<LmSlot> slots;
  std::vector<int> free_slots;
  std::map<int, int> by_kf;   // ascending id -> slot
  long long live_entries = 0;
  uint64_t version = 1;       // bumped by every call that changes what a query reads
  LmSlotDev* d_table = nullptr; size_t table_cap = 0;
  int* d_rows = nullptr; long long entry_cap = 0, entry_used = 0;
  uint8_t* d_oct = nullptr;   // the octave plane of the arena: same offsets, same capacity
  int live_without_oct = 0;   // live keyframes whose row has no octaves (asd_keyframe_culling refuses unless 0)
  float* d_center = nullptr; size_t center_cap = 0;   // KeyFrame::GetCameraCenter() per slot [3], beside d_table: grows with it
  int live_without_center = 0;   // live keyframes without a centre (asd_update_normal_and_depth refuses unless 0)
  uint8_t* d_pbad = nullptr; int* d_mark = nullptr; int* d_claim = nullptr; size_t row_cap = 0;
  bool tables_dirty = false;  // a query failed between marking and undoing
  int* d_sorted = nullptr; size_t sorted_cap = 0; bool sorted_dirty = true;   // ids [live] | slots [live]
  int* d_child = nullptr; size_t child_cap = 0; bool child_dirty = true;       // offsets [slots + 1] | children
  size_t child_off_words = 0;
  int* d_cnt = nullptr; size_t cnt_cap = 0;
  int* d_list = nullptr; size_t list_cap = 0;           // ids [cap] | slots [cap]
  long long* d_list_base = nullptr; size_t list_base_cap = 0;
  int* d_head = nullptr; size_t head_cap = 0;
  int* h_head = nullptr;   // pinned
  int* d_tile = nullptr; size_t tile_cap = 0;           // counts [tiles][2] | offsets [tiles][2]
  int* d_local = nullptr; size_t local_cap = 0;
  int* d_search = nullptr; size_t search_cap = 0;
  int* d_cull = nullptr; size_t cull_cap = 0;           // scratch of asd_keyframe_culling / asd_map_observations
  int* d_culled = nullptr; size_t culled_cap = 0;       // [slots]
  int* d_nd = nullptr; size_t nd_cap = 0;               // asd_update_normal_and_depth: the observers' segments (id, slot) | the ordered slots
  std::vector<uint32_t> nd_stamp; uint32_t nd_call = 0; // its duplicate test: the call that named a bank row last
  // asd_local_ba_graph: its own storage, because what it leaves is resident for asd_local_ba_apply
  int* d_bgp = nullptr; size_t bgp_cap = 0;             // lLocalMapPoints | the compaction's second list
  int* d_bgn = nullptr; size_t bgn_cap = 0;             // per point: Observations() | cursor | segment offsets | point_rank | gone | place in bad_rows
  int4* d_bgs = nullptr; size_t bgs_cap = 0;            // the segments as filled | in ascending keyframe id
  int* d_bge = nullptr; size_t bge_cap = 0;             // edge -> segment entry
  int* d_bgk = nullptr; size_t bgk_cap = 0;             // [slots] claim | lFixedCameras
  uint8_t* d_bgf = nullptr; size_t bgf_cap = 0;         // per segment entry: flagged by asd_local_ba_apply
  int* d_fa = nullptr; size_t fa_cap = 0;               // asd_fuse_apply: per point, per segment and per hit words | kf's row | stamps
  int4* d_fas = nullptr; size_t fas_cap = 0;            // its segments
  bool bg_valid = false; uint64_t bg_version = 0;       // the resident graph and the table version it was built from
  int bg_points = 0, bg_edges = 0; long long bg_total = 0; size_t bg_N = 0;
  AsdXfer up, down;
  int growths[3] = {0, 0, 0};   // slot table, arena, row tables
  // what the last asd_update_local_map left for asd_track_local_points_map
  bool last_valid = false;
  uint64_t last_version = 0;
  std::vector<int32_t> last_search;
};

LocalMapState* lstate(asd_ctx* ctx) {
  if (!ctx->localmap) ctx->localmap = new LocalMapState();
  return static_cast<LocalMapState*>(ctx->localmap);
}

// room for `need` elements.  keep: elements of the old block copied over; fill: byte value the new block starts with (-1: none).  The
// copy goes on ctx->stream behind every write to the old block, which is freed once that stream has drained (see the head of the file).
template <typename T>
int lm_reserve(asd_ctx* ctx, T** p, size_t* cap, size_t need, size_t keep, int fill, size_t min_cap, int* growths = nullptr) {
  if (need <= *cap) return ASD_OK;
  const size_t nc = std::max(min_cap, std::max(need, 2 * *cap));
  T* q = nullptr;
  if (hipMalloc(&q, nc * sizeof(T)) != hipSuccess) { ctx->set_error("local map: out of device memory for %zu bytes", nc * sizeof(T)); return ASD_ERR_HIP; }
  hipError_t e = hipSuccess;
  if (fill >= 0) e = hipMemsetAsync(q, fill, nc * sizeof(T), ctx->stream);
  if (e == hipSuccess && *p && keep) e = hipMemcpyAsync(q, *p, keep * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) { (void)hipFree(q); ctx->set_error("local map: growth failed: %s", hipGetErrorString(e)); return ASD_ERR_HIP; }
  if (*p) { (void)hipFree(*p); if (growths) ++*growths; }
  *p = q;
  *cap = nc;
  return ASD_OK;
}

void release_device(LocalMapState* S) {
  void* dev[] = {S->d_table, S->d_rows, S->d_pbad, S->d_mark, S->d_claim, S->d_sorted, S->d_child, S->d_cnt, S->d_list, S->d_list_base, S->d_head,
                 S->d_tile, S->d_local, S->d_search, S->d_oct, S->d_cull, S->d_culled, S->d_center, S->d_nd, S->d_bgp, S->d_bgn, S->d_bgs, S->d_bge, S->d_bgk, S->d_bgf, S->d_fa, S->d_fas};
  for (void* p : dev) if (p) (void)hipFree(p);
  S->d_table = nullptr; S->d_rows = nullptr; S->d_pbad = nullptr; S->d_mark = nullptr; S->d_claim = nullptr; S->d_sorted = nullptr; S->d_child = nullptr;
  S->d_cnt = nullptr; S->d_list = nullptr; S->d_list_base = nullptr; S->d_head = nullptr; S->d_tile = nullptr; S->d_local = nullptr; S->d_search = nullptr;
  S->d_oct = nullptr; S->d_cull = nullptr; S->d_culled = nullptr; S->cull_cap = S->culled_cap = 0;
  S->d_center = nullptr; S->d_nd = nullptr; S->center_cap = S->nd_cap = 0;
  S->d_bgp = nullptr; S->d_bgn = nullptr; S->d_bgs = nullptr; S->d_bge = nullptr; S->d_bgk = nullptr; S->d_bgf = nullptr;
  S->d_fa = nullptr; S->d_fas = nullptr; S->fa_cap = S->fas_cap = 0;
  S->bgp_cap = S->bgn_cap = S->bgs_cap = S->bge_cap = S->bgk_cap = S->bgf_cap = 0; S->bg_valid = false;
  S->table_cap = S->row_cap = S->sorted_cap = S->child_cap = S->cnt_cap = S->list_cap = S->list_base_cap = S->head_cap = S->tile_cap = S->local_cap = S->search_cap = 0;
  S->entry_cap = S->entry_used = 0;
}

LmSlotDev dev_entry(const LmSlot& s) {
  LmSlotDev e{};
  e.off = s.off; e.n = s.kf < 0 ? -1 : s.n; e.id = s.kf; e.bad = s.bad; e.n_cov = s.n_cov; e.parent = s.parent;
  for (int k = 0; k < kMaxCov; ++k) e.cov[k] = k < s.n_cov ? s.cov[k] : -1;
  return e;
}

// the three per-row tables cover rows [0, rows)
int ensure_rows(asd_ctx* ctx, LocalMapState* S, size_t rows) {
  if (rows <= S->row_cap) return ASD_OK;
  size_t c0 = S->row_cap, c1 = S->row_cap, c2 = S->row_cap;
  int rc;
  if ((rc = lm_reserve(ctx, &S->d_pbad, &c0, rows, S->row_cap, 0, kInitRows, &S->growths[2])) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_mark, &c1, c0, S->row_cap, 0, c0)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_claim, &c2, c0, S->row_cap, 0x7f, c0)) != ASD_OK) return rc;
  S->row_cap = c0;
  return ASD_OK;
}

int check_rows(asd_ctx* ctx, const char* who, const int32_t* rows, int n, int* max_row) {
  int mx = -1;
  for (int i = 0; i < n; ++i) {
    if (rows[i] < -1 || rows[i] >= kMaxRow) { ctx->set_error("%s: bank row %d at %d (rows are -1 or 0 .. %d)", who, rows[i], i, kMaxRow - 1); return rows[i] < -1 ? ASD_ERR_INVALID : ASD_ERR_CAPACITY; }
    mx = std::max(mx, rows[i]);
  }
  *max_row = mx;
  return ASD_OK;
}

// one slot's table entry to the device
int upload_entry(asd_ctx* ctx, LocalMapState* S, int slot) {
  const LmSlotDev e = dev_entry(S->slots[slot]);
  ASD_HIP_CHECK(ctx, S->up.begin(ctx->stream, sizeof e));
  const size_t o = S->up.add(&e, sizeof e);
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->d_table + slot, S->up.h + o, sizeof e, hipMemcpyHostToDevice, ctx->stream));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return ASD_OK;
}

int grow_table(asd_ctx* ctx, LocalMapState* S, size_t need) {
  const int rc = lm_reserve(ctx, &S->d_table, &S->table_cap, need, S->table_cap, 0xff, kInitSlots, &S->growths[0]);   // (0xff: n = -1, a free slot)
  if (rc != ASD_OK) return rc;
  return lm_reserve(ctx, &S->d_center, &S->center_cap, 3 * S->table_cap, S->center_cap, 0, 3 * S->table_cap);   // the centres follow their slots
}

// room for `need` more entries behind entry_used: a new arena of twice the live entries, the live rows moved into it back to back in slot
// order (this closes the holes that erase and a longer put leave)
int grow_arena(asd_ctx* ctx, LocalMapState* S, long long need) {
  if (S->entry_used + need <= S->entry_cap) return ASD_OK;
  const long long cap = std::max(kInitEntries, 2 * (S->live_entries + need));
  int* nr = nullptr;
  uint8_t* no = nullptr;
  if (hipMalloc(&nr, (size_t)cap * sizeof(int)) != hipSuccess || hipMalloc(&no, (size_t)cap) != hipSuccess) {
    if (nr) (void)hipFree(nr);
    ctx->set_error("local map: out of device memory for %lld table entries", cap);
    return ASD_ERR_HIP;
  }
  std::vector<LmMove> mv;
  std::vector<int> moved;
  long long used = 0;
  for (size_t s = 0; s < S->slots.size(); ++s) {
    LmSlot& L = S->slots[s];
    if (L.kf < 0 || L.n <= 0) continue;
    mv.push_back(LmMove{L.off, used, L.n, 0});
    moved.push_back((int)s);
    L.off = used;
    used += L.n;
  }
  hipStream_t st = ctx->stream;
  hipError_t e = hipMemsetAsync(no, 0, (size_t)cap, st);   // (rows without octaves read as level 0, never as a level outside the counters)
  if (e == hipSuccess && !mv.empty() && S->d_rows) {
    const size_t b_mv = mv.size() * sizeof(LmMove);
    e = S->up.begin(st, b_mv + moved.size() * AsdDevBuf::padded(sizeof(LmSlotDev)) + 1024);   // (every add is padded to 256 B)
    if (e == hipSuccess) {
      const size_t o = S->up.add(mv.data(), b_mv);
      e = hipMemcpyAsync(S->up.d + o, S->up.h + o, b_mv, hipMemcpyHostToDevice, st);
      if (e == hipSuccess) { hipLaunchKernelGGL(k_lm_move, dim3((unsigned)mv.size()), dim3(256), 0, st, S->up.dev<LmMove>(o), S->d_rows, nr, S->d_oct, no); e = hipGetLastError(); }
      for (size_t k = 0; k < moved.size() && e == hipSuccess; ++k) {   // the moved rows' new offsets
        const LmSlotDev d = dev_entry(S->slots[moved[k]]);
        const size_t oe = S->up.add(&d, sizeof d);
        e = hipMemcpyAsync(S->d_table + moved[k], S->up.h + oe, sizeof d, hipMemcpyHostToDevice, st);
      }
    }
  }
  const hipError_t es = hipStreamSynchronize(st);   // the old arena goes only when the stream that read and wrote it has drained
  if (e == hipSuccess) e = es;
  if (S->d_rows) { (void)hipFree(S->d_rows); (void)hipFree(S->d_oct); ++S->growths[1]; }
  S->d_rows = nr;
  S->d_oct = no;
  S->entry_cap = cap; S->entry_used = used;
  if (e != hipSuccess) { ctx->set_error("local map: arena growth failed: %s", hipGetErrorString(e)); return ASD_ERR_HIP; }
  return ASD_OK;
}

// the ascending id list and the children block, where a call since the last query changed them
int refresh_lists(asd_ctx* ctx, LocalMapState* S) {
  hipStream_t st = ctx->stream;
  const size_t live = S->by_kf.size(), n_slots = S->slots.size();
  if (S->sorted_dirty && live) {
    int rc = lm_reserve(ctx, &S->d_sorted, &S->sorted_cap, 2 * live, 0, -1, 2 * kInitSlots);
    if (rc != ASD_OK) return rc;
    std::vector<int> v(2 * live);
    size_t k = 0;
    for (const auto& kv : S->by_kf) { v[k] = kv.first; v[live + k] = kv.second; ++k; }
    ASD_HIP_CHECK(ctx, S->up.begin(st, v.size() * sizeof(int)));
    const size_t o = S->up.add(v.data(), v.size() * sizeof(int));
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->d_sorted, S->up.h + o, v.size() * sizeof(int), hipMemcpyHostToDevice, st));
    ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  S->sorted_dirty = false;
  if ((S->child_dirty || S->child_off_words != n_slots + 1) && n_slots) {
    std::vector<int> v(n_slots + 1, 0);
    for (size_t s = 0; s < n_slots; ++s) v[s + 1] = v[s] + (S->slots[s].kf >= 0 ? (int)S->slots[s].children.size() : 0);
    for (size_t s = 0; s < n_slots; ++s) if (S->slots[s].kf >= 0) v.insert(v.end(), S->slots[s].children.begin(), S->slots[s].children.end());
    int rc = lm_reserve(ctx, &S->d_child, &S->child_cap, v.size() + 1, 0, -1, 4 * kInitSlots);
    if (rc != ASD_OK) return rc;
    ASD_HIP_CHECK(ctx, S->up.begin(st, v.size() * sizeof(int)));
    const size_t o = S->up.add(v.data(), v.size() * sizeof(int));
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->d_child, S->up.h + o, v.size() * sizeof(int), hipMemcpyHostToDevice, st));
    ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S->child_off_words = n_slots + 1;
  }
  S->child_dirty = false;
  return ASD_OK;
}

// a query that failed half way may have left marks and claims behind
int clean_tables(asd_ctx* ctx, LocalMapState* S) {
  if (!S->tables_dirty || !S->row_cap) { S->tables_dirty = false; return ASD_OK; }
  ASD_HIP_CHECK(ctx, hipMemsetAsync(S->d_mark, 0, S->row_cap * sizeof(int), ctx->stream));
  ASD_HIP_CHECK(ctx, hipMemsetAsync(S->d_claim, 0x7f, S->row_cap * sizeof(int), ctx->stream));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  S->tables_dirty = false;
  return ASD_OK;
}

LmSlot* find_kf(asd_ctx* ctx, LocalMapState* S, const char* who, int32_t kf, int* slot) {
  const auto it = S->by_kf.find(kf);
  if (it == S->by_kf.end()) { ctx->set_error("%s: keyframe %d is not in the observation table", who, kf); return nullptr; }
  *slot = it->second;
  return &S->slots[it->second];
}

bool refuse(asd_ctx* ctx, const char* who) { return asd_track_busy(ctx, who); }

}  // namespace

void localmap_free(asd_ctx* ctx) {
  if (!ctx->localmap) return;
  LocalMapState* S = static_cast<LocalMapState*>(ctx->localmap);
  release_device(S);
  if (S->h_head) (void)hipHostFree(S->h_head);
  S->up.release();
  S->down.release();
  delete S;
  ctx->localmap = nullptr;
}

int localmap_search_list(asd_ctx* ctx, const char* who, const int32_t** h_rows, const int32_t** d_rows, int* n) {
  LocalMapState* S = lstate(ctx);
  if (!S->last_valid) { ctx->set_error("%s: no asd_update_local_map of this context has left a search list", who); return ASD_ERR_INVALID; }
  if (S->last_version != S->version) { ctx->set_error("%s: the observation table has changed since the last asd_update_local_map", who); return ASD_ERR_INVALID; }
  if (S->last_search.empty()) { ctx->set_error("%s: the last asd_update_local_map left an empty search list", who); return ASD_ERR_INVALID; }
  *h_rows = S->last_search.data();
  *d_rows = S->d_search;
  *n = (int)S->last_search.size();
  return ASD_OK;
}

extern "C" {

int asd_map_clear(asd_ctx* ctx) {
  if (!ctx) return ASD_ERR_INVALID;
  if (refuse(ctx, "asd_map_clear")) return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  LocalMapState* S = lstate(ctx);
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  release_device(S);
  S->slots.clear(); S->free_slots.clear(); S->by_kf.clear();
  S->live_entries = 0;
  S->live_without_oct = 0;
  S->live_without_center = 0;
  S->sorted_dirty = S->child_dirty = true; S->child_off_words = 0; S->tables_dirty = false;
  S->growths[0] = S->growths[1] = S->growths[2] = 0;
  S->last_valid = false; S->last_search.clear();
  ++S->version;
  return ASD_OK;
}

int asd_map_put(asd_ctx* ctx, int32_t kf, int32_t n, const int32_t* rows) {
  if (!ctx) return ASD_ERR_INVALID;
  if (refuse(ctx, "asd_map_put")) return ASD_ERR_INVALID;
  if (kf < 0 || n < 0 || (n > 0 && !rows)) { ctx->set_error("asd_map_put: invalid argument (keyframe %d, %d entries)", kf, n); return ASD_ERR_INVALID; }
  if (n > kMaxKeypoints) { ctx->set_error("asd_map_put: %d entries exceed the %d a keyframe's row holds", n, kMaxKeypoints); return ASD_ERR_CAPACITY; }
  int max_row = -1;
  int rc = check_rows(ctx, "asd_map_put", rows, n, &max_row);
  if (rc != ASD_OK) return rc;
  (void)hipSetDevice(ctx->cfg.device);
  LocalMapState* S = lstate(ctx);
  const auto it = S->by_kf.find(kf);
  const bool fresh = it == S->by_kf.end();
  if (fresh && S->free_slots.empty() && (int)S->slots.size() >= kMaxSlots) { ctx->set_error("asd_map_put: the table holds %d keyframes, its limit", kMaxSlots); return ASD_ERR_CAPACITY; }
  if ((rc = ensure_rows(ctx, S, (size_t)max_row + 1)) != ASD_OK) return rc;
  int slot;
  if (!fresh) slot = it->second;
  else if (!S->free_slots.empty()) { slot = S->free_slots.back(); S->free_slots.pop_back(); }
  else { slot = (int)S->slots.size(); S->slots.emplace_back(); }
  auto undo = [&]() { if (fresh) S->free_slots.push_back(slot); };
  if ((rc = grow_table(ctx, S, S->slots.size())) != ASD_OK) { undo(); return rc; }
  LmSlot& L = S->slots[slot];
  const int old_n = fresh ? -1 : L.n;
  long long off = L.off;
  if (n > old_n) {   // a new place at the end of the arena (the old one becomes a hole)
    if (!fresh) { S->live_entries -= L.n; L.n = 0; }
    if ((rc = grow_arena(ctx, S, n)) != ASD_OK) { undo(); if (!fresh) { L.n = old_n; S->live_entries += old_n; } return rc; }
    off = S->entry_used;
    S->entry_used += n;
    S->live_entries += n;
  } else {
    S->live_entries += n - old_n;
  }
  if (fresh) { L = LmSlot(); L.kf = kf; S->by_kf[kf] = slot; S->sorted_dirty = true; S->child_dirty = true; ++S->live_without_oct; ++S->live_without_center; }
  else if (n != old_n && L.has_oct) { L.has_oct = false; ++S->live_without_oct; }   // the octaves are the keypoints': another n is another set of keypoints
  L.n = n; L.off = off;
  ++S->version;
  hipStream_t st = ctx->stream;
  const LmSlotDev e = dev_entry(L);
  ASD_HIP_CHECK(ctx, S->up.begin(st, (size_t)n * sizeof(int) + sizeof e + 1024));
  const size_t o_e = S->up.add(&e, sizeof e);
  if (n > 0) {
    const size_t o_r = S->up.add(rows, (size_t)n * sizeof(int));
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->d_rows + off, S->up.h + o_r, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
  }
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->d_table + slot, S->up.h + o_e, sizeof e, hipMemcpyHostToDevice, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  return ASD_OK;
}

int asd_map_set(asd_ctx* ctx, int32_t kf, int32_t count, const int32_t* idx, const int32_t* rows) {
  if (!ctx) return ASD_ERR_INVALID;
  if (refuse(ctx, "asd_map_set")) return ASD_ERR_INVALID;
  if (count < 0 || (count > 0 && (!idx || !rows))) { ctx->set_error("asd_map_set: invalid argument"); return ASD_ERR_INVALID; }
  LocalMapState* S = lstate(ctx);
  int slot;
  LmSlot* L = find_kf(ctx, S, "asd_map_set", kf, &slot);
  if (!L) return ASD_ERR_INVALID;
  int max_row = -1;
  int rc = check_rows(ctx, "asd_map_set", rows, count, &max_row);
  if (rc != ASD_OK) return rc;
  for (int i = 0; i < count; ++i)
    if (idx[i] < 0 || idx[i] >= L->n) { ctx->set_error("asd_map_set: keypoint %d of keyframe %d, whose row has %d entries", idx[i], kf, L->n); return ASD_ERR_INVALID; }
  if (count == 0) return ASD_OK;
  (void)hipSetDevice(ctx->cfg.device);
  if ((rc = ensure_rows(ctx, S, (size_t)max_row + 1)) != ASD_OK) return rc;
  // the changes apply in the order given: of two for one keypoint the later one stays
  std::unordered_map<int, int> last;
  for (int i = 0; i < count; ++i) last[idx[i]] = rows[i];
  std::vector<int> vi, vr;
  for (const auto& kv : last) { vi.push_back(kv.first); vr.push_back(kv.second); }
  const int m = (int)vi.size();
  ++S->version;
  hipStream_t st = ctx->stream;
  ASD_HIP_CHECK(ctx, S->up.begin(st, (size_t)m * 8 + 1024));
  const size_t o_i = S->up.add(vi.data(), (size_t)m * sizeof(int)), o_r = S->up.add(vr.data(), (size_t)m * sizeof(int));
  ASD_HIP_CHECK(ctx, S->up.upload(st));
  hipLaunchKernelGGL(k_lm_set, dim3((m + 255) / 256), dim3(256), 0, st, S->d_rows + L->off, S->up.dev<int>(o_i), S->up.dev<int>(o_r), m);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  return ASD_OK;
}

int asd_map_erase(asd_ctx* ctx, int32_t kf) {
  if (!ctx) return ASD_ERR_INVALID;
  if (refuse(ctx, "asd_map_erase")) return ASD_ERR_INVALID;
  LocalMapState* S = lstate(ctx);
  const auto it = S->by_kf.find(kf);
  if (it == S->by_kf.end()) return ASD_OK;
  (void)hipSetDevice(ctx->cfg.device);
  const int slot = it->second;
  S->live_entries -= S->slots[slot].n;
  if (!S->slots[slot].has_oct) --S->live_without_oct;
  if (!S->slots[slot].has_center) --S->live_without_center;
  S->slots[slot] = LmSlot();   // its row stays in the arena until the next growth compacts it
  S->free_slots.push_back(slot);
  S->by_kf.erase(it);
  S->sorted_dirty = S->child_dirty = true;
  ++S->version;
  return upload_entry(ctx, S, slot);
}

int asd_map_kf_links(asd_ctx* ctx, int32_t kf, int32_t n_cov, const int32_t* cov, int32_t n_children, const int32_t* children, int32_t parent) {
  if (!ctx) return ASD_ERR_INVALID;
  if (refuse(ctx, "asd_map_kf_links")) return ASD_ERR_INVALID;
  if (n_cov < 0 || n_cov > kMaxCov || (n_cov > 0 && !cov) || n_children < 0 || (n_children > 0 && !children) || parent < -1) {
    ctx->set_error("asd_map_kf_links: invalid argument (%d covisibles of at most %d, %d children, parent %d)", n_cov, kMaxCov, n_children, parent);
    return ASD_ERR_INVALID;
  }
  for (int i = 0; i < n_cov; ++i) if (cov[i] < 0) { ctx->set_error("asd_map_kf_links: covisible id %d", cov[i]); return ASD_ERR_INVALID; }
  for (int i = 0; i < n_children; ++i)
    if (children[i] < 0 || (i > 0 && children[i] <= children[i - 1])) { ctx->set_error("asd_map_kf_links: children ids are not non-negative and strictly ascending at %d", i); return ASD_ERR_INVALID; }
  LocalMapState* S = lstate(ctx);
  int slot;
  LmSlot* L = find_kf(ctx, S, "asd_map_kf_links", kf, &slot);
  if (!L) return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  L->n_cov = n_cov;
  for (int i = 0; i < n_cov; ++i) L->cov[i] = cov[i];
  L->children.assign(children, children + n_children);
  L->parent = parent;
  S->child_dirty = true;
  ++S->version;
  return upload_entry(ctx, S, slot);
}

int asd_map_kf_bad(asd_ctx* ctx, int32_t kf, int32_t flag) {
  if (!ctx) return ASD_ERR_INVALID;
  if (refuse(ctx, "asd_map_kf_bad")) return ASD_ERR_INVALID;
  LocalMapState* S = lstate(ctx);
  int slot;
  LmSlot* L = find_kf(ctx, S, "asd_map_kf_bad", kf, &slot);
  if (!L) return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  L->bad = flag != 0;
  ++S->version;
  return upload_entry(ctx, S, slot);
}

int asd_map_point_bad(asd_ctx* ctx, int32_t n, const int32_t* rows, int32_t flag) {
  if (!ctx) return ASD_ERR_INVALID;
  if (refuse(ctx, "asd_map_point_bad")) return ASD_ERR_INVALID;
  if (n < 0 || (n > 0 && !rows)) { ctx->set_error("asd_map_point_bad: invalid argument"); return ASD_ERR_INVALID; }
  int max_row = -1;
  int rc = check_rows(ctx, "asd_map_point_bad", rows, n, &max_row);
  if (rc != ASD_OK) return rc;
  for (int i = 0; i < n; ++i) if (rows[i] < 0) { ctx->set_error("asd_map_point_bad: bank row %d", rows[i]); return ASD_ERR_INVALID; }
  if (n == 0) return ASD_OK;
  (void)hipSetDevice(ctx->cfg.device);
  LocalMapState* S = lstate(ctx);
  if ((rc = ensure_rows(ctx, S, (size_t)max_row + 1)) != ASD_OK) return rc;
  ++S->version;
  hipStream_t st = ctx->stream;
  ASD_HIP_CHECK(ctx, S->up.begin(st, (size_t)n * sizeof(int)));
  const size_t o = S->up.add(rows, (size_t)n * sizeof(int));
  ASD_HIP_CHECK(ctx, S->up.upload(st));
  hipLaunchKernelGGL(k_lm_point_bad, dim3((n + 255) / 256), dim3(256), 0, st, S->d_pbad, S->up.dev<int>(o), n, flag != 0);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  return ASD_OK;
}

int asd_update_local_map(asd_ctx* ctx, asd_local_map_args* A) {
  if (!ctx) return ASD_ERR_INVALID;
  if (!A || A->n_cur < 0 || A->n_seen < 0 || A->n_prev < 0 || (A->n_cur > 0 && !A->cur_rows) || (A->n_seen > 0 && !A->seen_rows) || (A->n_prev > 0 && !A->prev_kfs) ||
      A->max_kfs < 0 || A->kf_capacity < 0 || A->row_capacity < 0 || A->search_capacity < 0 || (A->kf_capacity > 0 && !A->local_kfs) ||
      (A->row_capacity > 0 && !A->local_rows) || (A->search_capacity > 0 && !A->search_rows)) {
    ctx->set_error("asd_update_local_map: invalid argument");
    return ASD_ERR_INVALID;
  }
  if (refuse(ctx, "asd_update_local_map")) return ASD_ERR_INVALID;
  if (A->max_kfs > kMaxLocalKfs) { ctx->set_error("asd_update_local_map: max_kfs = %d exceeds %d", A->max_kfs, kMaxLocalKfs); return ASD_ERR_CAPACITY; }
  if ((long long)A->n_cur + A->n_seen > kVoteMask / 2) { ctx->set_error("asd_update_local_map: %d + %d frame rows", A->n_cur, A->n_seen); return ASD_ERR_CAPACITY; }
  for (int i = 0; i < A->n_prev; ++i) if (A->prev_kfs[i] < 0) { ctx->set_error("asd_update_local_map: keyframe id %d in prev_kfs", A->prev_kfs[i]); return ASD_ERR_INVALID; }
  int mx0 = -1, mx1 = -1;
  int rc;
  if ((rc = check_rows(ctx, "asd_update_local_map", A->cur_rows, A->n_cur, &mx0)) != ASD_OK) return rc;
  if ((rc = check_rows(ctx, "asd_update_local_map", A->seen_rows, A->n_seen, &mx1)) != ASD_OK) return rc;
  (void)hipSetDevice(ctx->cfg.device);
  LocalMapState* S = lstate(ctx);
  S->last_valid = false;
  A->n_local_kfs = 0; A->ref_kf = -1; A->n_local = 0; A->n_search = 0;
  hipStream_t st = ctx->stream;
  const int n_slots = (int)S->slots.size(), n_live = (int)S->by_kf.size();
  const size_t list_need = (size_t)std::max(n_live, A->n_prev) + 3 * ((size_t)A->max_kfs + 1) + 1;
  if ((rc = ensure_rows(ctx, S, (size_t)std::max(mx0, mx1) + 1)) != ASD_OK) return rc;
  if ((rc = refresh_lists(ctx, S)) != ASD_OK) return rc;
  if ((rc = clean_tables(ctx, S)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_cnt, &S->cnt_cap, (size_t)n_slots + 1, 0, -1, kInitSlots)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_list, &S->list_cap, 2 * list_need, 0, -1, 1024)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_list_base, &S->list_base_cap, list_need, 0, -1, 512)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_head, &S->head_cap, 16, 0, 0, 16)) != ASD_OK) return rc;
  int* d_list_id = S->d_list;
  int* d_list_slot = S->d_list + S->list_cap / 2;

  const int n_frame = A->n_cur + A->n_seen;
  ASD_HIP_CHECK(ctx, S->up.begin(st, ((size_t)n_frame + A->n_prev) * sizeof(int) + 1024));
  const size_t o_cur = S->up.add(A->cur_rows, (size_t)A->n_cur * sizeof(int)), o_seen = S->up.add(A->seen_rows, (size_t)A->n_seen * sizeof(int));
  const size_t o_prev = S->up.add(A->prev_kfs, (size_t)A->n_prev * sizeof(int));
  const size_t cap_l = (size_t)A->row_capacity, cap_s = (size_t)A->search_capacity;
  ASD_HIP_CHECK(ctx, S->up.upload(st));
  S->tables_dirty = true;
  if (n_frame > 0) {
    hipLaunchKernelGGL(k_lm_mark, dim3((n_frame + 255) / 256), dim3(256), 0, st, S->up.dev<int>(o_cur), A->n_cur, S->up.dev<int>(o_seen), A->n_seen, S->d_pbad, S->d_mark);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  if (n_slots > 0) {
    hipLaunchKernelGGL(k_lm_vote, dim3((n_slots + 3) / 4), dim3(256), 0, st, S->d_table, n_slots, S->d_rows, S->d_mark, S->d_cnt);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  LmDecideArgs da{};
  da.table = S->d_table; da.sorted_id = S->d_sorted; da.sorted_slot = S->d_sorted ? S->d_sorted + n_live : nullptr; da.n_live = n_live;
  da.cnt = S->d_cnt; da.child_off = S->d_child; da.children = S->d_child ? S->d_child + S->child_off_words : nullptr;
  da.prev = S->up.dev<int>(o_prev); da.n_prev = A->n_prev; da.max_kfs = A->max_kfs; da.incl_words = (n_slots + 31) / 32;
  da.list_id = d_list_id; da.list_slot = d_list_slot; da.list_base = S->d_list_base; da.head = S->d_head;
  da.ids_in_lds = ((size_t)da.incl_words + n_live) * 4 <= 48 * 1024;   // (+ 14 KB of static LDS: inside the 64 KB a kernel gets without asking)
  hipLaunchKernelGGL(k_lm_decide, dim3(1), dim3(256), ((size_t)da.incl_words + (da.ids_in_lds ? n_live : 0)) * 4, st, da);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  if (!S->h_head) ASD_HIP_CHECK(ctx, hipHostMalloc(&S->h_head, 16 * sizeof(int)));
  int* const head = S->h_head;
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(head, S->d_head, 16 * sizeof(int), hipMemcpyDeviceToHost, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const int n_list = head[0], maxn = head[3];
  const long long entries = ((long long)head[5] << 32) | (unsigned)head[4];
  auto unmark = [&]() -> int {
    if (n_frame > 0) {
      hipLaunchKernelGGL(k_lm_unmark, dim3((n_frame + 255) / 256), dim3(256), 0, st, S->up.dev<int>(o_cur), A->n_cur, S->up.dev<int>(o_seen), A->n_seen, S->d_mark);
      ASD_HIP_CHECK(ctx, hipGetLastError());
    }
    return ASD_OK;
  };
  if (entries >= kMaxEntriesPerQuery) {
    if ((rc = unmark()) != ASD_OK) return rc;
    ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S->tables_dirty = false;
    ctx->set_error("asd_update_local_map: the %d local keyframes hold %lld table entries, more than one query collects (%lld)", n_list, entries, kMaxEntriesPerQuery);
    return ASD_ERR_CAPACITY;
  }
  const size_t give_l = std::min(cap_l, (size_t)entries), give_s = std::min(cap_s, (size_t)entries), give_k = std::min((size_t)A->kf_capacity, (size_t)n_list);
  ASD_HIP_CHECK(ctx, S->down.begin(st, (give_l + give_s + give_k) * sizeof(int) + 1024));
  const size_t o_hl = S->down.reserve(give_l * sizeof(int)), o_hs = S->down.reserve(give_s * sizeof(int)), o_hk = S->down.reserve(give_k * sizeof(int));
  if (entries > 0) {
    const int tiles_per_kf = (maxn + kTile - 1) / kTile;
    const size_t n_tiles = (size_t)tiles_per_kf * n_list;
    if ((rc = lm_reserve(ctx, &S->d_tile, &S->tile_cap, 4 * n_tiles, 0, -1, 4096)) != ASD_OK) return rc;
    if ((rc = lm_reserve(ctx, &S->d_local, &S->local_cap, (size_t)entries, 0, -1, 65536)) != ASD_OK) return rc;
    if ((rc = lm_reserve(ctx, &S->d_search, &S->search_cap, (size_t)entries, 0, -1, 65536)) != ASD_OK) return rc;
    LmPointArgs pa{};
    pa.table = S->d_table; pa.rows = S->d_rows; pa.list_slot = d_list_slot; pa.list_base = S->d_list_base; pa.tiles_per_kf = tiles_per_kf;
    pa.pbad = S->d_pbad; pa.mark = S->d_mark; pa.claim = S->d_claim;
    pa.tile_cnt = S->d_tile; pa.tile_off = S->d_tile + 2 * n_tiles;
    pa.d_local = S->d_local; pa.d_search = S->d_search;
    pa.h_local = S->down.host<int>(o_hl); pa.cap_local = (int)give_l; pa.h_search = S->down.host<int>(o_hs); pa.cap_search = (int)give_s;
    const dim3 grid((unsigned)n_list, (unsigned)tiles_per_kf);
    hipLaunchKernelGGL(k_lm_claim, grid, dim3(256), 0, st, pa);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lm_count, grid, dim3(256), 0, st, pa);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lm_tilescan, dim3(1), dim3(256), 0, st, S->d_tile, S->d_tile + 2 * n_tiles, (int)n_tiles, S->d_head);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lm_scatter, grid, dim3(256), 0, st, pa);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  if ((rc = unmark()) != ASD_OK) return rc;
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(head, S->d_head, 16 * sizeof(int), hipMemcpyDeviceToHost, st));
  if (give_k) ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->down.h + o_hk, d_list_id, give_k * sizeof(int), hipMemcpyDeviceToHost, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  S->tables_dirty = false;
  A->n_local_kfs = n_list; A->ref_kf = head[1]; A->n_local = head[8]; A->n_search = head[9];
  if (n_list > A->kf_capacity || A->n_local > A->row_capacity || A->n_search > A->search_capacity) {
    ctx->set_error("asd_update_local_map: %d keyframes, %d local points, %d points to search exceed the capacities %d, %d, %d", n_list, A->n_local, A->n_search,
                   A->kf_capacity, A->row_capacity, A->search_capacity);
    return ASD_ERR_CAPACITY;
  }
  if (n_list) memcpy(A->local_kfs, S->down.h + o_hk, (size_t)n_list * sizeof(int));
  if (A->n_local) memcpy(A->local_rows, S->down.h + o_hl, (size_t)A->n_local * sizeof(int));
  if (A->n_search) memcpy(A->search_rows, S->down.h + o_hs, (size_t)A->n_search * sizeof(int));
  S->last_search.assign(A->search_rows, A->search_rows + A->n_search);
  S->last_valid = true;
  S->last_version = S->version;
  return ASD_OK;
}

int asd_map_shared_counts(asd_ctx* ctx, int32_t kf, int32_t capacity, int32_t* kfs, int32_t* counts, int32_t* n) {
  if (!ctx) return ASD_ERR_INVALID;
  if (!n || capacity < 0 || (capacity > 0 && (!kfs || !counts))) { ctx->set_error("asd_map_shared_counts: invalid argument"); return ASD_ERR_INVALID; }
  if (refuse(ctx, "asd_map_shared_counts")) return ASD_ERR_INVALID;
  LocalMapState* S = lstate(ctx);
  int slot;
  const LmSlot* L = find_kf(ctx, S, "asd_map_shared_counts", kf, &slot);
  if (!L) return ASD_ERR_INVALID;
  *n = 0;
  (void)hipSetDevice(ctx->cfg.device);
  hipStream_t st = ctx->stream;
  const int n_slots = (int)S->slots.size();
  int rc;
  if ((rc = clean_tables(ctx, S)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_cnt, &S->cnt_cap, (size_t)n_slots + 1, 0, -1, kInitSlots)) != ASD_OK) return rc;
  if (L->n > 0) {
    ASD_HIP_CHECK(ctx, S->down.begin(st, (size_t)n_slots * sizeof(int)));
    const size_t o = S->down.reserve((size_t)n_slots * sizeof(int));
    const int* own = S->d_rows + L->off;
    S->tables_dirty = true;
    hipLaunchKernelGGL(k_lm_mark, dim3((L->n + 255) / 256), dim3(256), 0, st, own, L->n, own, 0, S->d_pbad, S->d_mark);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lm_vote, dim3((n_slots + 3) / 4), dim3(256), 0, st, S->d_table, n_slots, S->d_rows, S->d_mark, S->d_cnt);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lm_unmark, dim3((L->n + 255) / 256), dim3(256), 0, st, own, L->n, own, 0, S->d_mark);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->down.h + o, S->d_cnt, (size_t)n_slots * sizeof(int), hipMemcpyDeviceToHost, st));
    ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S->tables_dirty = false;
    const int* c = S->down.host<int>(o);
    int k = 0;
    for (const auto& kv : S->by_kf) {   // KFcounter in ascending id, the keyframe itself left out (:559-565)
      if (kv.first == kf || c[kv.second] <= 0) continue;
      if (k < capacity) { kfs[k] = kv.first; counts[k] = c[kv.second]; }
      ++k;
    }
    *n = k;
    if (k > capacity) { ctx->set_error("asd_map_shared_counts: %d keyframes exceed the capacity %d", k, capacity); return ASD_ERR_CAPACITY; }
  }
  return ASD_OK;
}

int asd_map_put_octaves(asd_ctx* ctx, int32_t kf, int32_t n, const uint8_t* octave) {
  if (!ctx) return ASD_ERR_INVALID;
  if (refuse(ctx, "asd_map_put_octaves")) return ASD_ERR_INVALID;
  if (n < 0 || (n > 0 && !octave)) { ctx->set_error("asd_map_put_octaves: invalid argument (keyframe %d, %d octaves)", kf, n); return ASD_ERR_INVALID; }
  LocalMapState* S = lstate(ctx);
  int slot;
  LmSlot* L = find_kf(ctx, S, "asd_map_put_octaves", kf, &slot);
  if (!L) return ASD_ERR_INVALID;
  if (n != L->n) { ctx->set_error("asd_map_put_octaves: %d octaves for keyframe %d, whose row has %d entries", n, kf, L->n); return ASD_ERR_INVALID; }
  for (int i = 0; i < n; ++i)
    if (octave[i] >= ASD_MAX_LEVELS) { ctx->set_error("asd_map_put_octaves: octave %d at keypoint %d of keyframe %d (levels are 0 .. %d)", (int)octave[i], i, kf, ASD_MAX_LEVELS - 1); return ASD_ERR_INVALID; }
  (void)hipSetDevice(ctx->cfg.device);
  if (n > 0) {
    hipStream_t st = ctx->stream;
    ASD_HIP_CHECK(ctx, S->up.begin(st, (size_t)n));
    const size_t o = S->up.add(octave, (size_t)n);
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->d_oct + L->off, S->up.h + o, (size_t)n, hipMemcpyHostToDevice, st));
    ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  if (!L->has_oct) { L->has_oct = true; --S->live_without_oct; }
  return ASD_OK;   // (the search list of the last asd_update_local_map stays: nothing it was built from has changed)
}

int asd_keyframe_culling(asd_ctx* ctx, asd_kf_culling_args* A) {
  if (!ctx) return ASD_ERR_INVALID;
  if (!A || A->n_cand < 0 || (A->n_cand > 0 && (!A->cand || !A->cand_flags || !A->decision || !A->n_mps || !A->n_redundant)) || A->bad_capacity < 0 ||
      (A->bad_capacity > 0 && !A->bad_rows)) {
    ctx->set_error("asd_keyframe_culling: invalid argument");
    return ASD_ERR_INVALID;
  }
  if (refuse(ctx, "asd_keyframe_culling")) return ASD_ERR_INVALID;
  A->n_bad = 0;
  const int n_cand = A->n_cand;
  if (n_cand > kMaxCand) { ctx->set_error("asd_keyframe_culling: %d candidates exceed %d", n_cand, kMaxCand); return ASD_ERR_CAPACITY; }
  LocalMapState* S = lstate(ctx);
  std::vector<int> cand_slot(n_cand);
  std::vector<long long> base(n_cand);
  long long entries = 0;
  int maxn = 0;
  {
    std::vector<int> seen(A->cand, A->cand + n_cand);
    std::sort(seen.begin(), seen.end());
    for (int i = 1; i < n_cand; ++i) if (seen[i] == seen[i - 1]) { ctx->set_error("asd_keyframe_culling: keyframe %d occurs twice among the candidates", seen[i]); return ASD_ERR_INVALID; }
  }
  for (int i = 0; i < n_cand; ++i) {
    int slot;
    const LmSlot* L = find_kf(ctx, S, "asd_keyframe_culling", A->cand[i], &slot);
    if (!L) return ASD_ERR_INVALID;
    const bool skip = (A->cand_flags[i] & 1) || A->cand[i] == 0;   // GetGlobalMapFlag(), mnId == 0 (:751-754)
    cand_slot[i] = skip ? -1 : slot;
    base[i] = entries;
    if (!skip) { entries += L->n; maxn = std::max(maxn, L->n); }
  }
  if (S->live_without_oct > 0) {
    for (const auto& kv : S->by_kf)
      if (!S->slots[kv.second].has_oct) { ctx->set_error("asd_keyframe_culling: keyframe %d has no octaves (asd_map_put_octaves); %d live keyframes have none", kv.first, S->live_without_oct); break; }
    return ASD_ERR_INVALID;
  }
  if (n_cand == 0) return ASD_OK;
  if (entries > kMaxCullEntries) { ctx->set_error("asd_keyframe_culling: the candidates' rows hold %lld entries, more than one call takes (%lld)", entries, kMaxCullEntries); return ASD_ERR_CAPACITY; }
  (void)hipSetDevice(ctx->cfg.device);
  hipStream_t st = ctx->stream;
  const int n_slots = (int)S->slots.size();
  const size_t E = ((size_t)entries + 3) / 4 * 4 + 4;   // (a multiple of 4: the counters are stored as int4)
  int rc;
  if ((rc = clean_tables(ctx, S)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_head, &S->head_cap, 16, 0, 0, 16)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_culled, &S->culled_cap, (size_t)n_slots + 1, 0, -1, kInitSlots)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_cull, &S->cull_cap, (4 + kLevels) * E + 3 * (size_t)n_cand, 0, -1, 65536)) != ASD_OK) return rc;
  // pts | the compaction's second list (unused) | counters | gone | bad rows | decision, nMPs, nRedundantObservations
  int* const d_pts = S->d_cull; int* const d_second = d_pts + E; int* const d_ccnt = d_second + E; int* const d_gone = d_ccnt + kLevels * E;
  int* const d_bad = d_gone + E; int* const d_out = d_bad + E;
  if (!S->h_head) ASD_HIP_CHECK(ctx, hipHostMalloc(&S->h_head, 16 * sizeof(int)));
  ASD_HIP_CHECK(ctx, S->up.begin(st, (size_t)n_cand * 13 + 1024));
  const size_t o_slot = S->up.add(cand_slot.data(), (size_t)n_cand * sizeof(int)), o_base = S->up.add(base.data(), (size_t)n_cand * sizeof(long long));
  const size_t o_flag = S->up.add(A->cand_flags, (size_t)n_cand);
  ASD_HIP_CHECK(ctx, S->up.upload(st));
  ASD_HIP_CHECK(ctx, hipMemsetAsync(S->d_head, 0, 16 * sizeof(int), st));
  ASD_HIP_CHECK(ctx, hipMemsetAsync(S->d_culled, 0, ((size_t)n_slots + 1) * sizeof(int), st));
  S->tables_dirty = true;
  const unsigned pt_blocks = (unsigned)((entries + 255) / 256);
  if (entries > 0) {   // the distinct not-bad points of the candidates' rows, in order
    const int tiles_per_kf = (maxn + kTile - 1) / kTile;
    const size_t n_tiles = (size_t)tiles_per_kf * n_cand;
    if ((rc = lm_reserve(ctx, &S->d_tile, &S->tile_cap, 4 * n_tiles, 0, -1, 4096)) != ASD_OK) return rc;
    LmPointArgs pa{};
    pa.table = S->d_table; pa.rows = S->d_rows; pa.list_slot = S->up.dev<int>(o_slot); pa.list_base = S->up.dev<long long>(o_base); pa.tiles_per_kf = tiles_per_kf;
    pa.pbad = S->d_pbad; pa.mark = S->d_mark; pa.claim = S->d_claim;
    pa.tile_cnt = S->d_tile; pa.tile_off = S->d_tile + 2 * n_tiles;
    pa.d_local = d_pts; pa.d_search = d_second;   // (not the resident search list: that one stays as it is)
    pa.h_local = nullptr; pa.cap_local = 0; pa.h_search = nullptr; pa.cap_search = 0;
    const dim3 grid((unsigned)n_cand, (unsigned)tiles_per_kf);
    hipLaunchKernelGGL(k_lm_claim, grid, dim3(256), 0, st, pa);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lm_count, grid, dim3(256), 0, st, pa);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lm_tilescan, dim3(1), dim3(256), 0, st, S->d_tile, S->d_tile + 2 * n_tiles, (int)n_tiles, S->d_head);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lm_scatter, grid, dim3(256), 0, st, pa);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_cull_index, dim3(pt_blocks), dim3(256), 0, st, d_pts, S->d_head, S->d_mark, d_ccnt, d_gone);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_cull_count, dim3((n_slots + 3) / 4), dim3(256), 0, st, S->d_table, n_slots, S->d_rows, S->d_oct, S->d_mark, d_ccnt, kLevels);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  LmCullArgs ca{};
  ca.table = S->d_table; ca.rows = S->d_rows; ca.oct = S->d_oct; ca.pbad = S->d_pbad; ca.mark = S->d_mark;
  ca.cand_slot = S->up.dev<int>(o_slot); ca.cand_flags = S->up.dev<uint8_t>(o_flag); ca.n_cand = n_cand;
  ca.cnt = d_ccnt; ca.gone = d_gone; ca.bad_rows = d_bad; ca.culled = S->d_culled; ca.out = d_out; ca.head = S->d_head;
  hipLaunchKernelGGL(k_cull_walk, dim3(1), dim3(256), 0, st, ca);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  const size_t give_bad = std::min((size_t)A->bad_capacity, (size_t)entries);
  ASD_HIP_CHECK(ctx, S->down.begin(st, (3 * (size_t)n_cand + give_bad) * sizeof(int) + 1024));
  const size_t o_out = S->down.reserve(3 * (size_t)n_cand * sizeof(int)), o_bad = S->down.reserve(give_bad * sizeof(int));
  int* const head = S->h_head;
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(head, S->d_head, 16 * sizeof(int), hipMemcpyDeviceToHost, st));
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->down.h + o_out, d_out, 3 * (size_t)n_cand * sizeof(int), hipMemcpyDeviceToHost, st));
  if (give_bad) ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->down.h + o_bad, d_bad, give_bad * sizeof(int), hipMemcpyDeviceToHost, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const int n_bad = head[10];
  const int* out = S->down.host<int>(o_out);
  bool any_culled = false;
  for (int i = 0; i < n_cand; ++i) any_culled = any_culled || out[i] == 1;
  const bool fits = n_bad <= A->bad_capacity;
  const bool change = fits && A->apply && any_culled;
  if (change) {
    hipLaunchKernelGGL(k_cull_apply, dim3((n_slots + 3) / 4), dim3(256), 0, st, S->d_table, n_slots, S->d_rows, S->d_mark, d_gone, S->d_culled);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  if (entries > 0) {
    hipLaunchKernelGGL(k_cull_finish, dim3(pt_blocks), dim3(256), 0, st, d_pts, S->d_head, S->d_mark, d_gone, S->d_pbad, change ? 1 : 0);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  S->tables_dirty = false;
  A->n_bad = n_bad;
  if (!fits) {
    ctx->set_error("asd_keyframe_culling: %d points turn bad, bad_capacity is %d", n_bad, A->bad_capacity);
    return ASD_ERR_CAPACITY;
  }
  for (int i = 0; i < n_cand; ++i) { A->decision[i] = (uint8_t)out[i]; A->n_mps[i] = out[n_cand + i]; A->n_redundant[i] = out[2 * n_cand + i]; }
  if (n_bad) memcpy(A->bad_rows, S->down.h + o_bad, (size_t)n_bad * sizeof(int));
  if (change) {
    for (int i = 0; i < n_cand; ++i) if (out[i] == 1) S->slots[cand_slot[i]].bad = true;   // the host mirror of what k_cull_apply wrote
    ++S->version;
  }
  return ASD_OK;
}

int asd_map_observations(asd_ctx* ctx, int32_t n, const int32_t* rows, int32_t* counts) {
  if (!ctx) return ASD_ERR_INVALID;
  if (n < 0 || (n > 0 && (!rows || !counts))) { ctx->set_error("asd_map_observations: invalid argument"); return ASD_ERR_INVALID; }
  if (refuse(ctx, "asd_map_observations")) return ASD_ERR_INVALID;
  int max_row = -1;
  int rc = check_rows(ctx, "asd_map_observations", rows, n, &max_row);
  if (rc != ASD_OK) return rc;
  for (int i = 0; i < n; ++i) if (rows[i] < 0) { ctx->set_error("asd_map_observations: bank row %d", rows[i]); return ASD_ERR_INVALID; }
  if (n == 0) return ASD_OK;
  (void)hipSetDevice(ctx->cfg.device);
  LocalMapState* S = lstate(ctx);
  hipStream_t st = ctx->stream;
  const int n_slots = (int)S->slots.size();
  const int row_cap = (int)S->row_cap;   // (at most 2^28)
  if (row_cap == 0 || n_slots == 0) { for (int i = 0; i < n; ++i) counts[i] = 0; return ASD_OK; }
  if ((rc = clean_tables(ctx, S)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_cull, &S->cull_cap, 2 * (size_t)n, 0, -1, 65536)) != ASD_OK) return rc;
  int* const d_ccnt = S->d_cull; int* const d_res = S->d_cull + n;
  ASD_HIP_CHECK(ctx, S->up.begin(st, (size_t)n * sizeof(int)));
  const size_t o = S->up.add(rows, (size_t)n * sizeof(int));
  ASD_HIP_CHECK(ctx, S->up.upload(st));
  ASD_HIP_CHECK(ctx, S->down.begin(st, (size_t)n * sizeof(int)));
  const size_t o_res = S->down.reserve((size_t)n * sizeof(int));
  ASD_HIP_CHECK(ctx, hipMemsetAsync(d_ccnt, 0, (size_t)n * sizeof(int), st));
  S->tables_dirty = true;
  const dim3 grid((n + 255) / 256);
  hipLaunchKernelGGL(k_obs_mark, grid, dim3(256), 0, st, S->up.dev<int>(o), n, row_cap, S->d_mark);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_cull_count, dim3((n_slots + 3) / 4), dim3(256), 0, st, S->d_table, n_slots, S->d_rows, S->d_oct, S->d_mark, d_ccnt, 1);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_obs_gather, grid, dim3(256), 0, st, S->up.dev<int>(o), n, row_cap, S->d_mark, d_ccnt, d_res);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_obs_unmark, grid, dim3(256), 0, st, S->up.dev<int>(o), n, row_cap, S->d_mark);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->down.h + o_res, d_res, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  S->tables_dirty = false;
  memcpy(counts, S->down.h + o_res, (size_t)n * sizeof(int));
  return ASD_OK;
}

int asd_map_kf_centers(asd_ctx* ctx, int32_t n, const int32_t* kfs, const float* Ow) {
  if (!ctx) return ASD_ERR_INVALID;
  if (refuse(ctx, "asd_map_kf_centers")) return ASD_ERR_INVALID;
  if (n < 0 || (n > 0 && (!kfs || !Ow))) { ctx->set_error("asd_map_kf_centers: invalid argument (%d keyframes)", n); return ASD_ERR_INVALID; }
  LocalMapState* S = lstate(ctx);
  std::unordered_map<int, int> last;   // slot -> the last position that names it
  for (int i = 0; i < n; ++i) {
    int slot;
    if (!find_kf(ctx, S, "asd_map_kf_centers", kfs[i], &slot)) return ASD_ERR_INVALID;
    last[slot] = i;
  }
  if (n == 0) return ASD_OK;
  (void)hipSetDevice(ctx->cfg.device);
  std::vector<int> vs;
  std::vector<float> vc;
  for (const auto& kv : last) { vs.push_back(kv.first); for (int k = 0; k < 3; ++k) vc.push_back(Ow[3 * (size_t)kv.second + k]); }
  const int m = (int)vs.size();
  hipStream_t st = ctx->stream;
  ASD_HIP_CHECK(ctx, S->up.begin(st, (size_t)m * 16 + 1024));
  const size_t o_s = S->up.add(vs.data(), (size_t)m * sizeof(int)), o_c = S->up.add(vc.data(), (size_t)m * 3 * sizeof(float));
  ASD_HIP_CHECK(ctx, S->up.upload(st));
  hipLaunchKernelGGL(k_nd_set_centers, dim3((m + 255) / 256), dim3(256), 0, st, S->d_center, S->up.dev<int>(o_s), S->up.dev<float>(o_c), m);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  for (const int slot : vs) if (!S->slots[slot].has_center) { S->slots[slot].has_center = true; --S->live_without_center; }
  return ASD_OK;   // (the search list of the last asd_update_local_map stays: nothing it was built from has changed)
}

int asd_update_normal_and_depth(asd_ctx* ctx, asd_normal_depth_args* A) {
  if (!ctx) return ASD_ERR_INVALID;
  if (!A || A->n < 0 || (A->n > 0 && (!A->rows || !A->ref_kf))) { ctx->set_error("asd_update_normal_and_depth: invalid argument"); return ASD_ERR_INVALID; }
  if (ctx->prep_on) { ctx->set_error("asd_update_normal_and_depth: an asd_prep_async bracket is open"); return ASD_ERR_INVALID; }
  if (refuse(ctx, "asd_update_normal_and_depth")) return ASD_ERR_INVALID;
  const int n = A->n;
  if (n > kMaxNdPoints) { ctx->set_error("asd_update_normal_and_depth: %d points exceed the %d one call takes", n, kMaxNdPoints); return ASD_ERR_CAPACITY; }
  if (n == 0) return ASD_OK;
  LocalMapState* S = lstate(ctx);
  MatcherState* M = matcher_state(ctx);
  for (int i = 0; i < n; ++i)
    if (A->rows[i] < 0 || A->rows[i] >= M->attr_cap) {
      ctx->set_error("asd_update_normal_and_depth: bank row %d at %d lies outside the attribute bank (%d rows): its position was never put", A->rows[i], i, M->attr_cap);
      return ASD_ERR_INVALID;
    }
  if (S->nd_stamp.size() < (size_t)M->attr_cap || S->nd_call == 0xffffffffu) { S->nd_stamp.assign((size_t)M->attr_cap, 0u); S->nd_call = 0; }
  ++S->nd_call;
  for (int i = 0; i < n; ++i) {
    uint32_t& stamp = S->nd_stamp[A->rows[i]];
    if (stamp == S->nd_call) { ctx->set_error("asd_update_normal_and_depth: bank row %d occurs twice", A->rows[i]); return ASD_ERR_INVALID; }
    stamp = S->nd_call;
  }
  if (S->live_without_oct > 0 || S->live_without_center > 0) {
    for (const auto& kv : S->by_kf) {
      const LmSlot& L = S->slots[kv.second];
      if (!L.has_oct) { ctx->set_error("asd_update_normal_and_depth: keyframe %d has no octaves (asd_map_put_octaves); %d live keyframes have none", kv.first, S->live_without_oct); break; }
      if (!L.has_center) { ctx->set_error("asd_update_normal_and_depth: keyframe %d has no camera centre (asd_map_kf_centers); %d live keyframes have none", kv.first, S->live_without_center); break; }
    }
    return ASD_ERR_INVALID;
  }
  (void)hipSetDevice(ctx->cfg.device);
  hipStream_t st = ctx->stream;
  const int n_slots = (int)S->slots.size(), n_live = (int)S->by_kf.size();
  const int row_cap = (int)S->row_cap;   // (at most 2^28)
  int rc;
  if ((rc = refresh_lists(ctx, S)) != ASD_OK) return rc;
  if ((rc = clean_tables(ctx, S)) != ASD_OK) return rc;
  // counts | cursors | levels | segment offsets [n + 1] | slots of mpRefKF
  const size_t N = ((size_t)n + 4) / 4 * 4;
  if ((rc = lm_reserve(ctx, &S->d_cull, &S->cull_cap, 5 * N, 0, -1, 65536)) != ASD_OK) return rc;
  int* const d_cnt = S->d_cull; int* const d_cursor = d_cnt + N; int* const d_lvl = d_cursor + N; int* const d_off = d_lvl + N;
  int* const d_ref = d_off + N;
  if (!S->h_head) ASD_HIP_CHECK(ctx, hipHostMalloc(&S->h_head, 16 * sizeof(int)));
  ASD_HIP_CHECK(ctx, S->up.begin(st, (size_t)n * (A->Xw ? 20 : 8) + 1024));
  const size_t o_rows = S->up.add(A->rows, (size_t)n * sizeof(int)), o_ref = S->up.add(A->ref_kf, (size_t)n * sizeof(int));
  const size_t o_xw = A->Xw ? S->up.add(A->Xw, (size_t)n * 3 * sizeof(float)) : 0;
  ASD_HIP_CHECK(ctx, S->up.upload(st));
  ASD_HIP_CHECK(ctx, S->down.begin(st, (size_t)n * 6 * sizeof(float)));
  const size_t o_res = S->down.reserve((size_t)n * 6 * sizeof(float));
  const dim3 per_point((n + 255) / 256), per_wave((n + 3) / 4), per_slot((n_slots + 3) / 4);
  S->tables_dirty = true;
  hipLaunchKernelGGL(k_nd_mark, per_point, dim3(256), 0, st, S->up.dev<int>(o_rows), n, row_cap, S->d_mark, d_cnt, d_cursor, d_lvl, S->up.dev<int>(o_ref),
                     S->d_sorted, S->d_sorted ? S->d_sorted + n_live : nullptr, n_live, d_ref);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  if (n_slots > 0 && row_cap > 0) {
    hipLaunchKernelGGL(k_cull_count, per_slot, dim3(256), 0, st, S->d_table, n_slots, S->d_rows, S->d_oct, S->d_mark, d_cnt, 1);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  int* const head = S->h_head;   // (pinned: the kernels store the total and the results there themselves, no copy commands in the call)
  hipLaunchKernelGGL(k_nd_scan, dim3(1), dim3(256), 0, st, d_cnt, n, d_off, head);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const long long entries = ((long long)head[13] << 32) | (unsigned)head[12];
  auto unmark = [&]() -> int {
    hipLaunchKernelGGL(k_obs_unmark, per_point, dim3(256), 0, st, S->up.dev<int>(o_rows), n, row_cap, S->d_mark);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    return ASD_OK;
  };
  if (entries > kMaxNdEntries) {   // nothing has been written but the marks
    if ((rc = unmark()) != ASD_OK) return rc;
    ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S->tables_dirty = false;
    ctx->set_error("asd_update_normal_and_depth: the %d points have %lld observations, more than one call takes (%lld)", n, entries, kMaxNdEntries);
    return ASD_ERR_CAPACITY;
  }
  if ((rc = lm_reserve(ctx, &S->d_nd, &S->nd_cap, 3 * (size_t)entries + 4, 0, -1, 65536)) != ASD_OK) return rc;
  LmNdArgs na{};
  na.table = S->d_table; na.n_slots = n_slots; na.rows = S->d_rows; na.oct = S->d_oct; na.pbad = S->d_pbad; na.mark = S->d_mark; na.row_cap = row_cap;
  na.center = S->d_center;
  na.req = S->up.dev<int>(o_rows); na.ref_slot = d_ref; na.xw = A->Xw ? S->up.dev<float>(o_xw) : nullptr; na.n = n;
  na.cnt = d_cnt; na.cursor = d_cursor; na.seg_off = d_off; na.lvl = d_lvl;
  na.seg = reinterpret_cast<int2*>(S->d_nd); na.ord = S->d_nd + 2 * (size_t)entries;
  na.attr = M->d_attr; na.res = S->down.host<float>(o_res);
  for (int l = 0; l < kLevels; ++l) na.scale[l] = l < ctx->cfg.n_levels ? ctx->scale[l] : 0.f;
  na.scale_top = ctx->scale[ctx->cfg.n_levels - 1];
  if (entries > 0) {
    hipLaunchKernelGGL(k_nd_fill, per_slot, dim3(256), 0, st, na);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_nd_order, per_wave, dim3(256), 0, st, na);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(k_nd_point, per_wave, dim3(256), 0, st, na);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  if ((rc = unmark()) != ASD_OK) return rc;
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  S->tables_dirty = false;
  const float* res = S->down.host<float>(o_res);
  for (int i = 0; i < n; ++i) {
    const float* q = res + 6 * (size_t)i;
    if (A->normal) { A->normal[3 * (size_t)i] = q[0]; A->normal[3 * (size_t)i + 1] = q[1]; A->normal[3 * (size_t)i + 2] = q[2]; }
    if (A->min_dist) A->min_dist[i] = q[3];
    if (A->max_dist) A->max_dist[i] = q[4];
    if (A->status) { int s; memcpy(&s, q + 5, sizeof s); A->status[i] = (uint8_t)s; }
  }
  return ASD_OK;
}

static_assert(sizeof(asd_ba_graph_args) == 160 && offsetof(asd_ba_graph_args, local_kfs) == 24 && offsetof(asd_ba_graph_args, n_points) == 56 &&
              offsetof(asd_ba_graph_args, pose_fixed) == 88 && offsetof(asd_ba_graph_args, e_octave) == 136 && offsetof(asd_ba_graph_args, Xw) == 152,
              "asd_ba_graph_args: the layout the bindings restate");
static_assert(sizeof(asd_ba_apply_args) == 56 && offsetof(asd_ba_apply_args, bad_rows) == 32 && offsetof(asd_ba_apply_args, new_ref) == 48,
              "asd_ba_apply_args: the layout the bindings restate");

int asd_local_ba_graph(asd_ctx* ctx, asd_ba_graph_args* A) {
  if (!ctx) return ASD_ERR_INVALID;
  if (!A || A->kf < 0 || A->n_neigh < 0 || (A->n_neigh > 0 && !A->neigh) || A->kf_capacity < 0 || A->point_capacity < 0 || A->fixed_capacity < 0 ||
      A->pose_capacity < 0 || A->edge_capacity < 0 || (A->kf_capacity > 0 && !A->local_kfs) || (A->point_capacity > 0 && (!A->local_rows || !A->point_rank)) ||
      (A->fixed_capacity > 0 && !A->fixed_kfs) || (A->pose_capacity > 0 && (!A->pose_kfs || !A->pose_fixed)) ||
      (A->edge_capacity > 0 && (!A->e_point || !A->e_pose || !A->e_kf || !A->e_idx || !A->e_octave))) {
    ctx->set_error("asd_local_ba_graph: invalid argument");
    return ASD_ERR_INVALID;
  }
  if (A->Xw && ctx->prep_on) { ctx->set_error("asd_local_ba_graph: an asd_prep_async bracket is open"); return ASD_ERR_INVALID; }
  if (refuse(ctx, "asd_local_ba_graph")) return ASD_ERR_INVALID;
  A->n_local_kfs = 0; A->n_points = 0; A->n_fixed = 0; A->n_poses = 0; A->n_edges = 0;
  if (A->n_neigh > kMaxCand) { ctx->set_error("asd_local_ba_graph: %d neighbours exceed %d", A->n_neigh, kMaxCand); return ASD_ERR_CAPACITY; }
  LocalMapState* S = lstate(ctx);
  int kf_slot;
  if (!find_kf(ctx, S, "asd_local_ba_graph", A->kf, &kf_slot)) return ASD_ERR_INVALID;
  {
    std::vector<int> seen(A->neigh, A->neigh + A->n_neigh);
    seen.push_back(A->kf);
    std::sort(seen.begin(), seen.end());
    if (seen[0] < 0) { ctx->set_error("asd_local_ba_graph: keyframe id %d among the neighbours", seen[0]); return ASD_ERR_INVALID; }
    for (size_t i = 1; i < seen.size(); ++i)
      if (seen[i] == seen[i - 1]) { ctx->set_error("asd_local_ba_graph: keyframe %d occurs twice among the keyframe and its neighbours", seen[i]); return ASD_ERR_INVALID; }
  }
  if (S->live_without_oct > 0) {
    for (const auto& kv : S->by_kf)
      if (!S->slots[kv.second].has_oct) { ctx->set_error("asd_local_ba_graph: keyframe %d has no octaves (asd_map_put_octaves); %d live keyframes have none", kv.first, S->live_without_oct); break; }
    return ASD_ERR_INVALID;
  }
  // lLocalKeyFrames (:420-431): the slot table's host mirror knows isBad(); an id that is not in the table is not bad and has no row
  const int n_slots = (int)S->slots.size();
  std::vector<int> list_id, list_slot;
  std::vector<long long> base;
  std::vector<uint8_t> local(n_slots, 0);
  long long entries = 0;
  int maxn = 0;
  for (int i = -1; i < A->n_neigh; ++i) {
    const int id = i < 0 ? A->kf : A->neigh[i];
    const auto it = S->by_kf.find(id);
    const int sl = it == S->by_kf.end() ? -1 : it->second;
    if (sl >= 0 && S->slots[sl].bad && i >= 0) continue;
    list_id.push_back(id); list_slot.push_back(sl); base.push_back(entries);
    if (sl >= 0) { local[sl] = 1; entries += S->slots[sl].n; maxn = std::max(maxn, S->slots[sl].n); }
  }
  const int n_list = (int)list_id.size();
  if (entries >= kMaxEntriesPerQuery) {
    ctx->set_error("asd_local_ba_graph: the %d local keyframes hold %lld table entries, more than one call collects (%lld)", n_list, entries, kMaxEntriesPerQuery);
    return ASD_ERR_CAPACITY;
  }
  (void)hipSetDevice(ctx->cfg.device);
  hipStream_t st = ctx->stream;
  MatcherState* M = A->Xw ? matcher_state(ctx) : nullptr;
  const int row_cap = (int)S->row_cap;
  S->bg_valid = false;
  int rc;
  if ((rc = clean_tables(ctx, S)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_head, &S->head_cap, 16, 0, 0, 16)) != ASD_OK) return rc;
  if (!S->h_head) ASD_HIP_CHECK(ctx, hipHostMalloc(&S->h_head, 16 * sizeof(int)));
  int* const head = S->h_head;
  const size_t E = (size_t)entries + 4;
  if ((rc = lm_reserve(ctx, &S->d_bgp, &S->bgp_cap, 2 * E, 0, -1, 65536)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_bgk, &S->bgk_cap, 2 * (size_t)n_slots + 2, 0, -1, 2 * kInitSlots)) != ASD_OK) return rc;
  int* const d_pts = S->d_bgp; int* const d_second = d_pts + E;
  int* const d_kfclaim = S->d_bgk; int* const d_fixed = d_kfclaim + n_slots + 1;
  ASD_HIP_CHECK(ctx, S->up.begin(st, (size_t)n_list * 12 + (size_t)n_slots * 5 + 2048));
  const size_t o_slot = S->up.add(list_slot.data(), (size_t)n_list * sizeof(int)), o_base = S->up.add(base.data(), (size_t)n_list * sizeof(long long));
  const size_t o_loc = S->up.add(local.data(), (size_t)n_slots);
  ASD_HIP_CHECK(ctx, S->up.upload(st));
  const size_t o_pose = S->up.reserve((size_t)n_slots * sizeof(int));   // filled and sent further down
  ASD_HIP_CHECK(ctx, hipMemsetAsync(S->d_head, 0, 16 * sizeof(int), st));
  S->tables_dirty = true;
  if (entries > 0) {   // lLocalMapPoints (:435-449): the compaction of asd_update_local_map over these rows
    const int tiles_per_kf = (maxn + kTile - 1) / kTile;
    const size_t n_tiles = (size_t)tiles_per_kf * n_list;
    if ((rc = lm_reserve(ctx, &S->d_tile, &S->tile_cap, 4 * n_tiles, 0, -1, 4096)) != ASD_OK) return rc;
    LmPointArgs pa{};
    pa.table = S->d_table; pa.rows = S->d_rows; pa.list_slot = S->up.dev<int>(o_slot); pa.list_base = S->up.dev<long long>(o_base); pa.tiles_per_kf = tiles_per_kf;
    pa.pbad = S->d_pbad; pa.mark = S->d_mark; pa.claim = S->d_claim;
    pa.tile_cnt = S->d_tile; pa.tile_off = S->d_tile + 2 * n_tiles;
    pa.d_local = d_pts; pa.d_search = d_second;   // (not the resident search list: that one stays as it is)
    const dim3 grid((unsigned)n_list, (unsigned)tiles_per_kf);
    hipLaunchKernelGGL(k_lm_claim, grid, dim3(256), 0, st, pa);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lm_count, grid, dim3(256), 0, st, pa);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lm_tilescan, dim3(1), dim3(256), 0, st, S->d_tile, S->d_tile + 2 * n_tiles, (int)n_tiles, S->d_head);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lm_scatter, grid, dim3(256), 0, st, pa);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(head, S->d_head, 16 * sizeof(int), hipMemcpyDeviceToHost, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const int n = head[8];
  if (n > kMaxNdPoints) {   // (the claims are reset by the scatter; no mark has been set yet)
    S->tables_dirty = false;
    ctx->set_error("asd_local_ba_graph: %d local points exceed the %d one call takes", n, kMaxNdPoints);
    return ASD_ERR_CAPACITY;
  }
  // Observations() of every local point, its segment, point_rank
  const size_t N = ((size_t)n + 4) / 4 * 4;
  if ((rc = lm_reserve(ctx, &S->d_bgn, &S->bgn_cap, 7 * N, 0, -1, 65536)) != ASD_OK) return rc;
  int* const d_cnt = S->d_bgn; int* const d_cursor = d_cnt + N; int* const d_off = d_cursor + N; int* const d_rank = d_off + N;
  const dim3 per_point((n + 255) / 256), per_wave((n + 3) / 4), per_slot((n_slots + 3) / 4);
  auto unmark = [&]() -> int {
    if (n > 0) { hipLaunchKernelGGL(k_obs_unmark, per_point, dim3(256), 0, st, d_pts, n, row_cap, S->d_mark); ASD_HIP_CHECK(ctx, hipGetLastError()); }
    return ASD_OK;
  };
  long long total = 0;
  if (n > 0) {
    hipLaunchKernelGGL(k_bg_index, per_point, dim3(256), 0, st, d_pts, n, S->d_mark, d_cnt, d_cursor);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_cull_count, per_slot, dim3(256), 0, st, S->d_table, n_slots, S->d_rows, S->d_oct, S->d_mark, d_cnt, 1);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_nd_scan, dim3(1), dim3(256), 0, st, d_cnt, n, d_off, head);   // (head: pinned, the kernel stores the total there)
    ASD_HIP_CHECK(ctx, hipGetLastError());
    const size_t r_tiles = ((size_t)row_cap + kTile - 1) / kTile;
    if ((rc = lm_reserve(ctx, &S->d_tile, &S->tile_cap, 4 * r_tiles, 0, -1, 4096)) != ASD_OK) return rc;
    hipLaunchKernelGGL(k_bg_rank_count, dim3((unsigned)r_tiles), dim3(256), 0, st, S->d_mark, row_cap, S->d_tile);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lm_tilescan, dim3(1), dim3(256), 0, st, S->d_tile, S->d_tile + 2 * r_tiles, (int)r_tiles, S->d_head + 2);   // (its totals land in head[10..11], unused)
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_bg_rank_scatter, dim3((unsigned)r_tiles), dim3(256), 0, st, S->d_mark, row_cap, S->d_tile + 2 * r_tiles, d_rank);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
    total = ((long long)head[13] << 32) | (unsigned)head[12];
  }
  if (total > kMaxNdEntries) {
    if ((rc = unmark()) != ASD_OK) return rc;
    ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S->tables_dirty = false;
    ctx->set_error("asd_local_ba_graph: the %d local points have %lld observations, more than one call takes (%lld)", n, total, kMaxNdEntries);
    return ASD_ERR_CAPACITY;
  }
  const size_t T = (size_t)total + 4;
  const size_t n_tiles = ((size_t)total + kTile - 1) / kTile;
  if ((rc = lm_reserve(ctx, &S->d_bgs, &S->bgs_cap, 2 * T, 0, -1, 65536)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_bge, &S->bge_cap, T, 0, -1, 65536)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_tile, &S->tile_cap, 4 * n_tiles + 4, 0, -1, 4096)) != ASD_OK) return rc;
  LmBgArgs ga{};
  ga.table = S->d_table; ga.rows = S->d_rows; ga.oct = S->d_oct; ga.mark = S->d_mark; ga.n_slots = n_slots;
  ga.pts = d_pts; ga.n = n; ga.cnt = d_cnt; ga.cursor = d_cursor; ga.seg_off = d_off;
  ga.useg = S->d_bgs; ga.oseg = S->d_bgs + T; ga.local = S->up.dev<uint8_t>(o_loc); ga.kf_claim = d_kfclaim; ga.total = total;
  ga.tile_cnt = S->d_tile; ga.tile_off = S->d_tile + 2 * n_tiles; ga.fixed = d_fixed; ga.e_ent = S->d_bge;
  ASD_HIP_CHECK(ctx, hipMemsetAsync(S->d_head, 0, 16 * sizeof(int), st));
  if (total > 0) {
    ASD_HIP_CHECK(ctx, hipMemsetAsync(d_kfclaim, 0x7f, ((size_t)n_slots + 1) * sizeof(int), st));
    hipLaunchKernelGGL(k_bg_fill, per_slot, dim3(256), 0, st, ga);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_bg_order, per_wave, dim3(256), 0, st, ga);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_bg_count, dim3((unsigned)n_tiles), dim3(256), 0, st, ga);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lm_tilescan, dim3(1), dim3(256), 0, st, S->d_tile, S->d_tile + 2 * n_tiles, (int)n_tiles, S->d_head);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_bg_scatter, dim3((unsigned)n_tiles), dim3(256), 0, st, ga);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  if ((rc = unmark()) != ASD_OK) return rc;
  const size_t give_p = std::min((size_t)A->point_capacity, (size_t)n), give_e = std::min((size_t)A->edge_capacity, (size_t)total);
  ASD_HIP_CHECK(ctx, S->down.begin(st, ((size_t)n_slots + 2 * give_p + 4 * give_e) * sizeof(int) + give_e + (A->Xw ? (size_t)n * 24 : 0) + 4096));
  const size_t o_fix = S->down.reserve(((size_t)n_slots + 1) * sizeof(int)), o_pts = S->down.reserve(give_p * sizeof(int)), o_rank = S->down.reserve(give_p * sizeof(int));
  const size_t o_ep = S->down.reserve(give_e * sizeof(int)), o_eq = S->down.reserve(give_e * sizeof(int)), o_ek = S->down.reserve(give_e * sizeof(int));
  const size_t o_ei = S->down.reserve(give_e * sizeof(int)), o_eo = S->down.reserve(give_e), o_xw = A->Xw ? S->down.reserve((size_t)n * 24) : 0;
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(head, S->d_head, 16 * sizeof(int), hipMemcpyDeviceToHost, st));
  if (total > 0 && n_slots > 0) ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->down.h + o_fix, d_fixed, (size_t)n_slots * sizeof(int), hipMemcpyDeviceToHost, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  S->tables_dirty = false;
  const int n_fixed = head[8], n_edges = head[9];
  // the pose order of asd_ba_problem: local and fixed keyframes together in ascending id
  const int* fixed_ids = S->down.host<int>(o_fix);
  std::vector<std::pair<int, int>> poses;   // (id, fixed)
  for (int i = 0; i < n_list; ++i) poses.emplace_back(list_id[i], 0);
  for (int i = 0; i < n_fixed; ++i) poses.emplace_back(fixed_ids[i], 1);
  std::sort(poses.begin(), poses.end());
  const int n_poses = (int)poses.size();
  int* pose_idx = S->up.host<int>(o_pose);
  for (int s = 0; s < n_slots; ++s) pose_idx[s] = -1;
  for (int i = 0; i < n_poses; ++i) { const auto it = S->by_kf.find(poses[i].first); if (it != S->by_kf.end()) pose_idx[it->second] = i; }
  if (n_slots > 0) ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->up.d + o_pose, S->up.h + o_pose, (size_t)n_slots * sizeof(int), hipMemcpyHostToDevice, st));
  if (n_edges > 0 && give_e > 0) {
    LmBgEdgeArgs ea{};
    ea.oseg = ga.oseg; ea.e_ent = S->d_bge; ea.rank = d_rank; ea.pose_idx = S->up.dev<int>(o_pose); ea.n_edges = n_edges; ea.cap = (int)give_e;
    ea.e_point = S->down.host<int>(o_ep); ea.e_pose = S->down.host<int>(o_eq); ea.e_kf = S->down.host<int>(o_ek); ea.e_idx = S->down.host<int>(o_ei);
    ea.e_oct = S->down.host<uint8_t>(o_eo);
    hipLaunchKernelGGL(k_bg_edges, dim3((n_edges + 255) / 256), dim3(256), 0, st, ea);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  if (A->Xw && n > 0) {
    hipLaunchKernelGGL(k_bg_xw, per_point, dim3(256), 0, st, d_pts, d_rank, n, M->d_attr, (int)M->attr_cap, S->down.host<double>(o_xw), S->d_head);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(head, S->d_head, 16 * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  if (give_p) {
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->down.h + o_pts, d_pts, give_p * sizeof(int), hipMemcpyDeviceToHost, st));
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->down.h + o_rank, d_rank, give_p * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (A->Xw && n > 0 && head[15] > 0) {
    ctx->set_error("asd_local_ba_graph: bank row %d lies outside the attribute bank (%d rows): its position was never put", head[15] - 1, (int)M->attr_cap);
    return ASD_ERR_INVALID;
  }
  A->n_local_kfs = n_list; A->n_points = n; A->n_fixed = n_fixed; A->n_poses = n_poses; A->n_edges = n_edges;
  if (n_list > A->kf_capacity || n > A->point_capacity || n_fixed > A->fixed_capacity || n_poses > A->pose_capacity || n_edges > A->edge_capacity) {
    ctx->set_error("asd_local_ba_graph: %d local keyframes, %d points, %d fixed keyframes, %d poses, %d edges exceed the capacities %d, %d, %d, %d, %d", n_list, n,
                   n_fixed, n_poses, n_edges, A->kf_capacity, A->point_capacity, A->fixed_capacity, A->pose_capacity, A->edge_capacity);
    return ASD_ERR_CAPACITY;
  }
  memcpy(A->local_kfs, list_id.data(), (size_t)n_list * sizeof(int));
  if (n) { memcpy(A->local_rows, S->down.h + o_pts, (size_t)n * sizeof(int)); memcpy(A->point_rank, S->down.h + o_rank, (size_t)n * sizeof(int)); }
  if (n_fixed) memcpy(A->fixed_kfs, fixed_ids, (size_t)n_fixed * sizeof(int));
  for (int i = 0; i < n_poses; ++i) { A->pose_kfs[i] = poses[i].first; A->pose_fixed[i] = (uint8_t)poses[i].second; }
  if (n_edges) {
    memcpy(A->e_point, S->down.h + o_ep, (size_t)n_edges * sizeof(int)); memcpy(A->e_pose, S->down.h + o_eq, (size_t)n_edges * sizeof(int));
    memcpy(A->e_kf, S->down.h + o_ek, (size_t)n_edges * sizeof(int)); memcpy(A->e_idx, S->down.h + o_ei, (size_t)n_edges * sizeof(int));
    memcpy(A->e_octave, S->down.h + o_eo, (size_t)n_edges);
  }
  if (A->Xw && n) memcpy(A->Xw, S->down.h + o_xw, (size_t)n * 24);
  S->bg_valid = true; S->bg_version = S->version; S->bg_points = n; S->bg_edges = n_edges; S->bg_total = total; S->bg_N = N;
  return ASD_OK;
}

int asd_local_ba_apply(asd_ctx* ctx, asd_ba_apply_args* A) {
  if (!ctx) return ASD_ERR_INVALID;
  if (!A || A->n_edges < 0 || (A->n_edges > 0 && !A->erase) || A->bad_capacity < 0 || (A->bad_capacity > 0 && !A->bad_rows) || A->n_points < 0 ||
      (A->n_points > 0 && !A->new_ref)) {
    ctx->set_error("asd_local_ba_apply: invalid argument");
    return ASD_ERR_INVALID;
  }
  if (refuse(ctx, "asd_local_ba_apply")) return ASD_ERR_INVALID;
  A->n_erased = 0; A->n_bad = 0;
  LocalMapState* S = lstate(ctx);
  if (!S->bg_valid) { ctx->set_error("asd_local_ba_apply: no asd_local_ba_graph of this context has left a graph"); return ASD_ERR_INVALID; }
  if (S->bg_version != S->version) { ctx->set_error("asd_local_ba_apply: the observation table has changed since the last asd_local_ba_graph"); return ASD_ERR_INVALID; }
  if (A->n_edges != S->bg_edges || A->n_points != S->bg_points) {
    ctx->set_error("asd_local_ba_apply: %d edges and %d points, the resident graph has %d and %d", A->n_edges, A->n_points, S->bg_edges, S->bg_points);
    return ASD_ERR_INVALID;
  }
  const int n = S->bg_points, n_edges = S->bg_edges;
  const long long total = S->bg_total;
  bool any = false;
  for (int e = 0; e < n_edges; ++e) any = any || A->erase[e];
  if (n == 0 || !any) {   // nothing is flagged: nothing changes, the version stays
    for (int i = 0; i < n; ++i) A->new_ref[i] = -1;
    if (A->apply) S->bg_valid = false;
    return ASD_OK;
  }
  (void)hipSetDevice(ctx->cfg.device);
  hipStream_t st = ctx->stream;
  const size_t N = S->bg_N, T = (size_t)total + 4;
  int rc;
  if ((rc = lm_reserve(ctx, &S->d_bgf, &S->bgf_cap, T, 0, -1, 65536)) != ASD_OK) return rc;
  if (!S->h_head) ASD_HIP_CHECK(ctx, hipHostMalloc(&S->h_head, 16 * sizeof(int)));
  int* const head = S->h_head;
  int* const d_cnt = S->d_bgn; int* const d_off = d_cnt + 2 * N; int* const d_gone = d_cnt + 4 * N; int* const d_boff = d_cnt + 5 * N;   // (d_boff: n + 1 words of 2 N)
  ASD_HIP_CHECK(ctx, S->up.begin(st, (size_t)n_edges + 1024));
  const size_t o_er = S->up.add(A->erase, (size_t)n_edges);
  ASD_HIP_CHECK(ctx, S->up.upload(st));
  const size_t give_bad = std::min((size_t)A->bad_capacity, (size_t)n);
  ASD_HIP_CHECK(ctx, S->down.begin(st, ((size_t)n + give_bad + 16) * sizeof(int) + 1024));
  const size_t o_ref = S->down.reserve((size_t)n * sizeof(int)), o_bad = S->down.reserve(give_bad * sizeof(int)), o_hd = S->down.reserve(16 * sizeof(int));
  ASD_HIP_CHECK(ctx, hipMemsetAsync(S->d_head, 0, 16 * sizeof(int), st));
  ASD_HIP_CHECK(ctx, hipMemsetAsync(S->d_bgf, 0, T, st));
  LmBaArgs ba{};
  ba.table = S->d_table; ba.rows = S->d_rows; ba.pbad = S->d_pbad;
  ba.pts = S->d_bgp; ba.n = n; ba.cnt = d_cnt; ba.seg_off = d_off; ba.oseg = S->d_bgs + T; ba.flagged = S->d_bgf;
  ba.gone = d_gone; ba.boff = d_boff; ba.new_ref = S->down.host<int>(o_ref); ba.bad_rows = S->down.host<int>(o_bad); ba.bad_cap = (int)give_bad;
  ba.head = S->d_head; ba.apply = 0;
  const dim3 per_wave((n + 3) / 4);
  hipLaunchKernelGGL(k_ba_flag, dim3((n_edges + 255) / 256), dim3(256), 0, st, S->up.dev<uint8_t>(o_er), S->d_bge, n_edges, S->d_bgf);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_ba_point, per_wave, dim3(256), 0, st, ba);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_nd_scan, dim3(1), dim3(256), 0, st, d_gone, n, d_boff, head);   // (head[12]: the points that turned bad)
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->down.h + o_hd, S->d_head, 16 * sizeof(int), hipMemcpyDeviceToHost, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const int n_bad = head[12];
  A->n_erased = S->down.host<int>(o_hd)[14]; A->n_bad = n_bad;
  if (n_bad > A->bad_capacity) {   // nothing has been written but this call's scratch
    ctx->set_error("asd_local_ba_apply: %d points turn bad, bad_capacity is %d", n_bad, A->bad_capacity);
    return ASD_ERR_CAPACITY;
  }
  ba.apply = A->apply ? 1 : 0;
  if (n_bad > 0 || ba.apply) {
    hipLaunchKernelGGL(k_ba_write, per_wave, dim3(256), 0, st, ba);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  }
  memcpy(A->new_ref, S->down.h + o_ref, (size_t)n * sizeof(int));
  if (n_bad) memcpy(A->bad_rows, S->down.h + o_bad, (size_t)n_bad * sizeof(int));
  if (ba.apply) { ++S->version; S->bg_valid = false; }
  return ASD_OK;
}

static_assert(sizeof(asd_fuse_apply_args) == 96 && offsetof(asd_fuse_apply_args, cand) == 16 && offsetof(asd_fuse_apply_args, apply) == 32 &&
              offsetof(asd_fuse_apply_args, action) == 40 && offsetof(asd_fuse_apply_args, n_dropped) == 80 && offsetof(asd_fuse_apply_args, n_fused) == 88,
              "asd_fuse_apply_args: the layout the bindings restate");

int asd_fuse_apply(asd_ctx* ctx, asd_fuse_apply_args* A) {
  if (!ctx) return ASD_ERR_INVALID;
  if (!A || A->n < 0 || (A->n > 0 && (!A->cand || !A->best_idx || !A->action || !A->other || !A->obs_cand || !A->obs_other || !A->n_moved || !A->n_dropped))) {
    ctx->set_error("asd_fuse_apply: invalid argument");
    return ASD_ERR_INVALID;
  }
  if (refuse(ctx, "asd_fuse_apply")) return ASD_ERR_INVALID;
  if (A->mode < 0 || A->mode > 2) { ctx->set_error("asd_fuse_apply: mode %d (0 Fuse, 1 Fuse with Scw + SearchAndFuse's loop, 2 the loop fusion of CorrectLoop)", A->mode); return ASD_ERR_INVALID; }
  const int n = A->n;
  if (n > kMaxNdPoints) { ctx->set_error("asd_fuse_apply: %d candidates exceed the %d one call takes", n, kMaxNdPoints); return ASD_ERR_CAPACITY; }
  LocalMapState* S = lstate(ctx);
  int kf_slot;
  const LmSlot* K = find_kf(ctx, S, "asd_fuse_apply", A->kf, &kf_slot);
  if (!K) return ASD_ERR_INVALID;
  std::vector<int> h_cand, h_best, h_pos;   // the hits: candidates that take a step, in list order
  int max_row = -1;
  {
    std::unordered_set<int> seen;   // the candidate rows >= 0 met so far
    seen.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
      const int c = A->cand[i], b = A->best_idx[i];
      if (c < -1 || c >= kMaxRow) { ctx->set_error("asd_fuse_apply: bank row %d at candidate %d (rows are -1 or 0 .. %d)", c, i, kMaxRow - 1); return ASD_ERR_INVALID; }
      if (b < -1 || b >= K->n) { ctx->set_error("asd_fuse_apply: best_idx %d at candidate %d, the row of keyframe %d has %d entries", b, i, A->kf, K->n); return ASD_ERR_INVALID; }
      if (c < 0) continue;
      if (!seen.insert(c).second) { ctx->set_error("asd_fuse_apply: bank row %d occurs twice among the candidates", c); return ASD_ERR_INVALID; }
      if (b >= 0) { h_cand.push_back(c); h_best.push_back(b); h_pos.push_back(i); max_row = std::max(max_row, c); }
    }
  }
  A->n_fused = 0;   // (every check has passed: from here on the caller's arrays are written)
  for (int i = 0; i < n; ++i) { A->action[i] = 0; A->other[i] = -1; A->obs_cand[i] = 0; A->obs_other[i] = 0; A->n_moved[i] = 0; A->n_dropped[i] = 0; }
  const int nh = (int)h_cand.size();
  if (nh == 0) return ASD_OK;   // no candidate takes a step: nothing is launched
  (void)hipSetDevice(ctx->cfg.device);
  hipStream_t st = ctx->stream;
  const int n_slots = (int)S->slots.size();
  const int P = 2 * nh;
  int rc;
  if ((rc = ensure_rows(ctx, S, (size_t)max_row + 1)) != ASD_OK) return rc;   // a candidate created this keyframe may lie beyond the row tables
  if ((rc = clean_tables(ctx, S)) != ASD_OK) return rc;
  const size_t N = ((size_t)P + 8) / 4 * 4;
  if ((rc = lm_reserve(ctx, &S->d_fa, &S->fa_cap, 18 * N + (size_t)K->n + (size_t)n_slots + 16, 0, -1, 65536)) != ASD_OK) return rc;
  if (!S->h_head) ASD_HIP_CHECK(ctx, hipHostMalloc(&S->h_head, 16 * sizeof(int)));
  int* const head = S->h_head;
  LmFaArgs fa{};
  fa.table = S->d_table; fa.rows = S->d_rows; fa.pbad = S->d_pbad; fa.mark = S->d_mark; fa.n_slots = n_slots;
  fa.kf_slot = kf_slot; fa.kf_off = K->off; fa.mode = A->mode; fa.nh = nh; fa.P = P;
  fa.cnt = S->d_fa; fa.cursor = fa.cnt + N; fa.seg_off = fa.cursor + N; fa.pt_row = fa.seg_off + N; fa.gone = fa.pt_row + N; fa.head = fa.gone + N;
  fa.tail = fa.head + N; fa.inkf = fa.tail + N; fa.inkf0 = fa.inkf + N; fa.next = fa.inkf0 + N; fa.oidx = fa.next + 2 * N; fa.out = fa.oidx + N;
  fa.krow = fa.out + 6 * N; fa.stamp = fa.krow + K->n;
  ASD_HIP_CHECK(ctx, S->up.begin(st, (size_t)nh * 8 + 1024));
  const size_t o_cand = S->up.add(h_cand.data(), (size_t)nh * sizeof(int)), o_best = S->up.add(h_best.data(), (size_t)nh * sizeof(int));
  ASD_HIP_CHECK(ctx, S->up.upload(st));
  fa.cand = S->up.dev<int>(o_cand); fa.best = S->up.dev<int>(o_best);
  ASD_HIP_CHECK(ctx, hipMemsetAsync(fa.krow, 0xff, (size_t)K->n * sizeof(int), st));
  ASD_HIP_CHECK(ctx, hipMemsetAsync(fa.stamp, 0, ((size_t)n_slots + 1) * sizeof(int), st));
  const dim3 per_hit((nh + 255) / 256), per_point((P + 255) / 256), per_slot((n_slots + 3) / 4);
  S->tables_dirty = true;
  hipLaunchKernelGGL(k_fa_mark_cand, per_hit, dim3(256), 0, st, fa.cand, nh, S->d_mark);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_fa_mark_other, per_hit, dim3(256), 0, st, fa);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_fa_index, per_point, dim3(256), 0, st, fa);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_cull_count, per_slot, dim3(256), 0, st, S->d_table, n_slots, S->d_rows, S->d_oct, S->d_mark, fa.cnt, 1);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_nd_scan, dim3(1), dim3(256), 0, st, fa.cnt, P, fa.seg_off, head);   // (head: pinned, the kernel stores the total there)
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const long long total = ((long long)head[13] << 32) | (unsigned)head[12];
  auto finish = [&](int apply) -> int {
    fa.apply = apply;
    hipLaunchKernelGGL(k_fa_finish, per_point, dim3(256), 0, st, fa);
    ASD_HIP_CHECK(ctx, hipGetLastError());
    ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
    S->tables_dirty = false;
    return ASD_OK;
  };
  if (total > kMaxNdEntries) {   // nothing has been written but the marks
    if ((rc = finish(0)) != ASD_OK) return rc;
    ctx->set_error("asd_fuse_apply: the points involved have %lld observations, more than one call takes (%lld)", total, kMaxNdEntries);
    return ASD_ERR_CAPACITY;
  }
  if ((rc = lm_reserve(ctx, &S->d_fas, &S->fas_cap, (size_t)total + nh + 4, 0, -1, 65536)) != ASD_OK) return rc;
  fa.ent = S->d_fas; fa.total = (int)total;
  if (total > 0) {
    hipLaunchKernelGGL(k_fa_fill, per_slot, dim3(256), 0, st, fa);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(k_fa_walk, dim3(1), dim3(256), 0, st, fa);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, S->down.begin(st, 6 * (size_t)nh * sizeof(int) + 1024));
  const size_t o_out = S->down.reserve(6 * (size_t)nh * sizeof(int));
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->down.h + o_out, fa.out, 6 * (size_t)nh * sizeof(int), hipMemcpyDeviceToHost, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const int* out = S->down.host<int>(o_out);
  bool changed = false;
  int n_fused = 0;
  for (int j = 0; j < nh; ++j) {
    const int act = out[j];
    changed = changed || (act >= 1 && act <= 3);
    n_fused += act >= 1 && act <= 5;
  }
  const bool write = A->apply && changed;
  if (write) {
    hipLaunchKernelGGL(k_fa_write, dim3((unsigned)((total + nh + 255) / 256)), dim3(256), 0, st, fa);
    ASD_HIP_CHECK(ctx, hipGetLastError());
  }
  if ((rc = finish(write ? 1 : 0)) != ASD_OK) return rc;
  for (int j = 0; j < nh; ++j) {
    const int i = h_pos[j];
    A->action[i] = (uint8_t)out[j]; A->other[i] = out[nh + j]; A->obs_cand[i] = out[2 * nh + j]; A->obs_other[i] = out[3 * nh + j];
    A->n_moved[i] = out[4 * nh + j]; A->n_dropped[i] = out[5 * nh + j];
  }
  A->n_fused = n_fused;
  if (write) ++S->version;
  return ASD_OK;
}

int asd_map_get(asd_ctx* ctx, int32_t kf, int32_t capacity, int32_t* rows, int32_t* n) {
  if (!ctx) return ASD_ERR_INVALID;
  if (!n || capacity < 0 || (capacity > 0 && !rows)) { ctx->set_error("asd_map_get: invalid argument"); return ASD_ERR_INVALID; }
  if (refuse(ctx, "asd_map_get")) return ASD_ERR_INVALID;
  LocalMapState* S = lstate(ctx);
  int slot;
  const LmSlot* L = find_kf(ctx, S, "asd_map_get", kf, &slot);
  if (!L) return ASD_ERR_INVALID;
  *n = L->n;
  if (L->n > capacity) { ctx->set_error("asd_map_get: the row of keyframe %d has %d entries, the capacity is %d", kf, L->n, capacity); return ASD_ERR_CAPACITY; }
  if (L->n == 0) return ASD_OK;
  (void)hipSetDevice(ctx->cfg.device);
  hipStream_t st = ctx->stream;
  ASD_HIP_CHECK(ctx, S->down.begin(st, (size_t)L->n * sizeof(int)));
  const size_t o = S->down.reserve((size_t)L->n * sizeof(int));
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->down.h + o, S->d_rows + L->off, (size_t)L->n * sizeof(int), hipMemcpyDeviceToHost, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  memcpy(rows, S->down.h + o, (size_t)L->n * sizeof(int));
  return ASD_OK;
}

int asd_map_points(asd_ctx* ctx, int32_t n_kfs, const int32_t* kfs, int32_t capacity, int32_t* rows, int32_t* n) {
  if (!ctx) return ASD_ERR_INVALID;
  if (!n || n_kfs < 0 || (n_kfs > 0 && !kfs) || capacity < 0 || (capacity > 0 && !rows)) { ctx->set_error("asd_map_points: invalid argument"); return ASD_ERR_INVALID; }
  if (refuse(ctx, "asd_map_points")) return ASD_ERR_INVALID;
  *n = 0;
  if (n_kfs > kMaxSlots) { ctx->set_error("asd_map_points: %d keyframes exceed the %d the table holds", n_kfs, kMaxSlots); return ASD_ERR_CAPACITY; }
  LocalMapState* S = lstate(ctx);
  {
    std::vector<int> seen(kfs, kfs + n_kfs);
    std::sort(seen.begin(), seen.end());
    for (int i = 1; i < n_kfs; ++i) if (seen[i] == seen[i - 1]) { ctx->set_error("asd_map_points: keyframe %d occurs twice", seen[i]); return ASD_ERR_INVALID; }
  }
  std::vector<int> list_slot(n_kfs);
  std::vector<long long> base(n_kfs);
  long long entries = 0;
  int maxn = 0;
  for (int i = 0; i < n_kfs; ++i) {   // an id that is not in the table contributes nothing
    const auto it = S->by_kf.find(kfs[i]);
    list_slot[i] = it == S->by_kf.end() ? -1 : it->second;
    base[i] = entries;
    if (list_slot[i] >= 0) { entries += S->slots[list_slot[i]].n; maxn = std::max(maxn, S->slots[list_slot[i]].n); }
  }
  if (entries >= kMaxEntriesPerQuery) { ctx->set_error("asd_map_points: the %d keyframes hold %lld table entries, more than one call collects (%lld)", n_kfs, entries, kMaxEntriesPerQuery); return ASD_ERR_CAPACITY; }
  if (entries == 0) return ASD_OK;
  (void)hipSetDevice(ctx->cfg.device);
  hipStream_t st = ctx->stream;
  int rc;
  if ((rc = clean_tables(ctx, S)) != ASD_OK) return rc;
  if ((rc = lm_reserve(ctx, &S->d_head, &S->head_cap, 16, 0, 0, 16)) != ASD_OK) return rc;
  if (!S->h_head) ASD_HIP_CHECK(ctx, hipHostMalloc(&S->h_head, 16 * sizeof(int)));
  const size_t E = (size_t)entries + 4;
  if ((rc = lm_reserve(ctx, &S->d_cull, &S->cull_cap, 2 * E, 0, -1, 65536)) != ASD_OK) return rc;
  const int tiles_per_kf = (maxn + kTile - 1) / kTile;
  const size_t n_tiles = (size_t)tiles_per_kf * n_kfs;
  if ((rc = lm_reserve(ctx, &S->d_tile, &S->tile_cap, 4 * n_tiles, 0, -1, 4096)) != ASD_OK) return rc;
  ASD_HIP_CHECK(ctx, S->up.begin(st, (size_t)n_kfs * 12 + 1024));
  const size_t o_slot = S->up.add(list_slot.data(), (size_t)n_kfs * sizeof(int)), o_base = S->up.add(base.data(), (size_t)n_kfs * sizeof(long long));
  ASD_HIP_CHECK(ctx, S->up.upload(st));
  const size_t give = std::min((size_t)capacity, (size_t)entries);
  ASD_HIP_CHECK(ctx, S->down.begin(st, give * sizeof(int) + 1024));
  const size_t o_pts = S->down.reserve(give * sizeof(int));
  ASD_HIP_CHECK(ctx, hipMemsetAsync(S->d_head, 0, 16 * sizeof(int), st));
  LmPointArgs pa{};
  pa.table = S->d_table; pa.rows = S->d_rows; pa.list_slot = S->up.dev<int>(o_slot); pa.list_base = S->up.dev<long long>(o_base); pa.tiles_per_kf = tiles_per_kf;
  pa.pbad = S->d_pbad; pa.mark = S->d_mark; pa.claim = S->d_claim;
  pa.tile_cnt = S->d_tile; pa.tile_off = S->d_tile + 2 * n_tiles;
  pa.d_local = S->d_cull; pa.d_search = S->d_cull + E;   // (not the resident search list: that one stays as it is)
  pa.h_local = S->down.host<int>(o_pts); pa.cap_local = (int)give; pa.h_search = nullptr; pa.cap_search = 0;
  const dim3 grid((unsigned)n_kfs, (unsigned)tiles_per_kf);
  S->tables_dirty = true;
  hipLaunchKernelGGL(k_lm_claim, grid, dim3(256), 0, st, pa);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_lm_count, grid, dim3(256), 0, st, pa);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_lm_tilescan, dim3(1), dim3(256), 0, st, S->d_tile, S->d_tile + 2 * n_tiles, (int)n_tiles, S->d_head);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_lm_scatter, grid, dim3(256), 0, st, pa);
  ASD_HIP_CHECK(ctx, hipGetLastError());
  int* const head = S->h_head;
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(head, S->d_head, 16 * sizeof(int), hipMemcpyDeviceToHost, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  S->tables_dirty = false;   // (the scatter has reset every claim; no mark was set)
  *n = head[8];
  if (*n > capacity) { ctx->set_error("asd_map_points: %d points exceed the capacity %d", *n, capacity); return ASD_ERR_CAPACITY; }
  if (*n) memcpy(rows, S->down.h + o_pts, (size_t)*n * sizeof(int));
  return ASD_OK;
}

int32_t asd_debug_map(asd_ctx* ctx, int64_t out[8]) {
  if (!ctx || !out) return ASD_ERR_INVALID;
  const LocalMapState* S = lstate(ctx);
  out[0] = (int64_t)S->by_kf.size(); out[1] = S->live_entries; out[2] = (int64_t)S->table_cap; out[3] = S->entry_cap; out[4] = (int64_t)S->row_cap;
  out[5] = S->growths[0]; out[6] = S->growths[1]; out[7] = S->growths[2];
  return ASD_OK;
}

}  // extern "C"
