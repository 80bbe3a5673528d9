// kfdb.hip -- KeyFrameDatabase (reference src/vslam/src/KeyFrameDatabase.cc, whole file) and the BoW score
// (TemplatedVocabulary::score -> L1Scoring / L2Scoring / DotProductScoring::score, src/dbow2/DBoW2/ScoringObject.cpp:23-120, :271-311).
//
// Device layout: every keyframe's BowVector is resident in HBM in one CSR arena (int32 word ids and f64 values at the same offsets,
// ascending word id inside an entry) behind an entry table {offset, word count}; a free table slot has count -1.  A query is ONE
// brute-force pass over all table slots -- no inverted file on the device.  The query vector sits in LDS (12 B per word); a wave owns
// an entry, walks its words 64 at a time, and every lane looks its word up in the query by binary search.  Per entry the wave produces
// what the reference's walk over the inverted lists leaves behind: the number of common words (mnLoopWords / mnRelocWords), the smallest
// common word id (which places the entry in lKFsSharingWords, see below) and the sum of the score's chain.
//
// The chain.  The reference adds one f64 term per common word in ascending word order.  The lanes compute their terms in parallel; the
// additions are then made one after the other over the set bits of the chunk's hit mask, lowest lane first, chunk after chunk -- the
// same operands in the same order, so the sum has the reference's bit pattern (no contraction: the file builds with -ffp-contract=off).
// (Adding all 64 lanes of a chunk in lane order, +0.0 for a lane without a common word, would be legal too, up to the sign of a zero;
// it makes 64 dependent additions per chunk where this form makes one per common word, and was not built.)
// The closing expression of each scoring (-s / 2, 1 - sqrt(1 - s), s) is evaluated on the host by the function asd_bow_score uses.
//
// The order of lKFsSharingWords.  The reference appends a keyframe when the walk over the query's words (ascending) first meets it in
// a word's inverted list, and every list is in add() order (erase() keeps the order of the rest; a keyframe added again goes to the
// end).  So the list is ordered by (smallest common word id, add sequence number): the device returns the first, the host keeps the
// second and sorts.  tests/test_kfdb.py checks this against a restatement that keeps real inverted lists.
//
// Streams.  Every copy into the arena and every kernel that reads it is enqueued on ctx->stream, and every entry point returns with
// that stream drained.  Growth (grow_arena) therefore orders itself against the only stream that can hold a write to the old arena:
// the compaction kernel is enqueued behind them on ctx->stream, and the old arena is freed after that stream has been waited for.
#include <algorithm>
#include <climits>
#include <cmath>
#include <unordered_map>
#include <utility>

#include "ctx.h"

int bow_loaded_scoring(asd_ctx* ctx);   // bow.hip: the loaded vocabulary's scoring, -1 without one

namespace {

constexpr int kInitSlots = 256;         // entry table and arena start small (600 entries of 150 words grow both) and double
constexpr long long kInitWords = 32768;
constexpr int kMaxQueryWords = 160 * 1024 / 12;   // the query in LDS: 8 + 4 B per word of the CU's 160 KB
constexpr int kNeigh = 10;              // GetBestCovisibilityKeyFrames(10)

struct KfEntryDev { long long off; int n; int pad; };   // n < 0: free slot
struct KfOut { double sum; int cnt; int first; };
struct KfMove { long long from, to; int n; int pad; };

__device__ inline double lane_value(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// PRODUCT = false: L1's term |vi - wi| - |vi| - |wi|; true: vi * wi (L2 and DOT_PRODUCT).  vi = the query's value (v1 of score(v1, v2))
template <bool PRODUCT>
__global__ __launch_bounds__(256) void k_kfdb_score(const int* __restrict__ q_id, const double* __restrict__ q_val, int nq,
                                                    const KfEntryDev* __restrict__ table, const int* __restrict__ slots, int n_items,
                                                    const int* __restrict__ ids, const double* __restrict__ vals, KfOut* __restrict__ out) {
  extern __shared__ double s_mem[];
  double* s_val = s_mem;
  int* s_id = reinterpret_cast<int*>(s_mem + nq);
  for (int t = threadIdx.x; t < nq; t += 256) { s_val[t] = q_val[t]; s_id[t] = q_id[t]; }
  asd_syncthreads();
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= n_items) return;   // whole waves leave together
  const KfEntryDev e = table[slots ? slots[item] : item];
  int top = 1;
  while (top * 2 <= nq) top *= 2;
  double sum = 0.0;
  int cnt = 0, first = INT_MAX;
  for (int base = 0; base < e.n; base += 64) {
    const int i = base + lane;
    double term = 0.0;
    bool hit = false;
    int w = 0;
    if (i < e.n) {
      w = ids[e.off + i];
      int pos = 0;   // number of query words below w
      for (int s = top; s > 0; s >>= 1)
        if (pos + s <= nq && s_id[pos + s - 1] < w) pos += s;
      if (pos < nq && s_id[pos] == w) {
        hit = true;
        const double vi = s_val[pos], wi = vals[e.off + i];
        term = PRODUCT ? vi * wi : fabs(vi - wi) - fabs(vi) - fabs(wi);
      }
    }
    unsigned long long b = __ballot(hit);
    if (!b) continue;
    if (first == INT_MAX) first = __builtin_amdgcn_readlane(w, __builtin_ctzll(b));
    cnt += __popcll(b);
    for (; b; b &= b - 1) sum += lane_value(term, __builtin_ctzll(b));
  }
  if (lane == 0) out[item] = KfOut{sum, cnt, first};
}

// growth: one workgroup per live entry copies its words from the old arena into the new one
__global__ __launch_bounds__(256) void k_kfdb_move(const KfMove* __restrict__ mv, const int* __restrict__ ids0, const double* __restrict__ vals0,
                                                   int* __restrict__ ids1, double* __restrict__ vals1) {
  const KfMove m = mv[blockIdx.x];
  for (int t = threadIdx.x; t < m.n; t += 256) { ids1[m.to + t] = ids0[m.from + t]; vals1[m.to + t] = vals0[m.from + t]; }
}

struct KfEntry {   // the reference's per-keyframe fields (KeyFrame.h: mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore)
  int kf = -1;     // -1: free slot
  bool global_map = false;
  long long seq = 0;
  long long loop_stamp = 0, reloc_stamp = 0;   // 0 = never stamped; queries count from 1
  int loop_words = 0, reloc_words = 0;
  float loop_score = 0.0f, reloc_score = 0.0f;
};

struct LastQuery {
  bool valid = false;
  long long stamp = 0;
  int min_common = 0;
  float min_score = 0.0f;
  std::vector<std::pair<float, int>> scored;   // lScoreAndMatch: (si, slot)
};

struct KfdbState {
  int scoring = 0;
  std::vector<KfEntry> slots;
  std::vector<KfEntryDev> table;   // host copy of the device table
  std::vector<int> free_slots;
  std::unordered_map<int, int> by_kf;
  int live = 0;
  long long live_words = 0, next_seq = 1, next_stamp = 1;
  long long last_loop_stamp = 0, last_reloc_stamp = 0;
  LastQuery last[2];
  KfEntryDev* d_table = nullptr;
  int table_cap = 0;
  int* d_ids = nullptr;
  double* d_vals = nullptr;
  long long word_cap = 0, word_used = 0;
  int growths = 0;
  AsdXfer up, down;   // the calls' own staging: they may run beside an armed asd_track_* call, which owns ctx->up / ctx->down
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

KfdbState* kstate(asd_ctx* ctx) {
  if (!ctx->kfdb) ctx->kfdb = new KfdbState();
  return static_cast<KfdbState*>(ctx->kfdb);
}

void release_device(KfdbState* S) {
  if (S->d_table) (void)hipFree(S->d_table);
  if (S->d_ids) (void)hipFree(S->d_ids);
  if (S->d_vals) (void)hipFree(S->d_vals);
  S->d_table = nullptr; S->d_ids = nullptr; S->d_vals = nullptr;
  S->table_cap = 0; S->word_cap = S->word_used = 0;
}

int check_bow(asd_ctx* ctx, const char* who, int n, const int32_t* id, const double* val) {
  if (n < 0 || (n > 0 && (!id || !val))) { ctx->set_error("%s: invalid BowVector argument", who); return ASD_ERR_INVALID; }
  for (int i = 0; i < n; ++i)
    if (id[i] < 0 || (i > 0 && id[i] <= id[i - 1])) { ctx->set_error("%s: word ids are not non-negative and strictly ascending at %d", who, i); return ASD_ERR_INVALID; }
  return ASD_OK;
}

// the closing expression of L1Scoring / L2Scoring / DotProductScoring::score over the chain's sum
double finish_score(int scoring, double score) {
  if (scoring == 0) return -score / 2.0;
  if (scoring == 1) return score >= 1 ? 1.0 : 1.0 - sqrt(1.0 - score);
  return score;
}

// the whole host table to the device (after a reallocation or a compaction)
int upload_table(asd_ctx* ctx, KfdbState* S) {
  if (S->table.empty()) return ASD_OK;
  const size_t bytes = S->table.size() * sizeof(KfEntryDev);
  ASD_HIP_CHECK(ctx, S->up.begin(ctx->stream, bytes));
  const size_t off = S->up.add(S->table.data(), bytes);
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->d_table, S->up.h + off, bytes, hipMemcpyHostToDevice, ctx->stream));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return ASD_OK;
}

int grow_table(asd_ctx* ctx, KfdbState* S, int need) {
  if (need <= S->table_cap) return ASD_OK;
  const int cap = std::max(kInitSlots, std::max(need, 2 * S->table_cap));
  KfEntryDev* nt = nullptr;
  ASD_HIP_CHECK(ctx, hipMalloc(&nt, (size_t)cap * sizeof(KfEntryDev)));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));   // (nothing of these calls is left in flight; see the head of the file)
  if (S->d_table) (void)hipFree(S->d_table);
  S->d_table = nt;
  S->table_cap = cap;
  return upload_table(ctx, S);
}

// room for `need` more words behind word_used: a new arena of twice the live words, the live entries moved into it back to back in
// slot order (this is where the holes erase() left are closed)
int grow_arena(asd_ctx* ctx, KfdbState* S, long long need) {
  if (S->word_used + need <= S->word_cap) return ASD_OK;
  const long long cap = std::max(kInitWords, 2 * (S->live_words + need));
  const bool first = !S->d_ids;
  int* ni = nullptr;
  double* nv = nullptr;
  ASD_HIP_CHECK(ctx, hipMalloc(&ni, (size_t)cap * sizeof(int)));
  if (hipMalloc(&nv, (size_t)cap * sizeof(double)) != hipSuccess) { (void)hipFree(ni); ctx->set_error("kfdb: out of device memory for %lld words", cap); return ASD_ERR_HIP; }
  std::vector<KfMove> mv;
  long long used = 0;
  for (size_t s = 0; s < S->slots.size(); ++s) {
    if (S->slots[s].kf < 0 || S->table[s].n <= 0) continue;
    mv.push_back(KfMove{S->table[s].off, used, S->table[s].n, 0});
    S->table[s].off = used;
    used += S->table[s].n;
  }
  hipStream_t st = ctx->stream;
  int rc = ASD_OK;
  if (!mv.empty() && S->d_ids) {
    const size_t bytes = mv.size() * sizeof(KfMove);
    hipError_t e = S->up.begin(st, bytes);
    if (e == hipSuccess) { S->up.add(mv.data(), bytes); e = S->up.upload(st); }
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_kfdb_move, dim3((unsigned)mv.size()), dim3(256), 0, st, S->up.dev<KfMove>(0), S->d_ids, S->d_vals, ni, nv);
      e = hipGetLastError();
    }
    if (e != hipSuccess) { ctx->set_error("kfdb: arena growth failed: %s", hipGetErrorString(e)); rc = ASD_ERR_HIP; }
  }
  // the old arena goes only when the stream that read it (and wrote it: every add() copies on this stream) has drained
  const hipError_t es = hipStreamSynchronize(st);
  if (rc == ASD_OK && es != hipSuccess) { ctx->set_error("kfdb: arena growth failed: %s", hipGetErrorString(es)); rc = ASD_ERR_HIP; }
  if (S->d_ids) (void)hipFree(S->d_ids);
  if (S->d_vals) (void)hipFree(S->d_vals);
  S->d_ids = ni; S->d_vals = nv;
  S->word_cap = cap; S->word_used = used;
  if (!first) ++S->growths;
  if (rc != ASD_OK) return rc;
  return upload_table(ctx, S);
}

// one pass of k_kfdb_score over `n_items` table slots (d-side list `slot_list`, or null = slots 0 .. n_items-1): results in S->down
int run_score(asd_ctx* ctx, KfdbState* S, int nq, const int32_t* q_id, const double* q_val, const std::vector<int>* slot_list, int n_items,
              const KfOut** out) {
  if (nq > kMaxQueryWords) { ctx->set_error("kfdb: a query of %d words exceeds the %d that fit the LDS", nq, kMaxQueryWords); return ASD_ERR_CAPACITY; }
  hipStream_t st = ctx->stream;
  if (!S->ev0) { ASD_HIP_CHECK(ctx, hipEventCreate(&S->ev0)); ASD_HIP_CHECK(ctx, hipEventCreate(&S->ev1)); }
  ASD_HIP_CHECK(ctx, S->up.begin(st, (size_t)nq * 12 + (size_t)n_items * 4 + 1024));
  ASD_HIP_CHECK(ctx, S->down.begin(st, (size_t)n_items * sizeof(KfOut)));
  const size_t o_val = S->up.add(q_val, (size_t)nq * sizeof(double));
  const size_t o_id = S->up.add(q_id, (size_t)nq * sizeof(int));
  const size_t o_slots = slot_list ? S->up.add(slot_list->data(), (size_t)n_items * sizeof(int)) : 0;
  const size_t o_out = S->down.reserve((size_t)n_items * sizeof(KfOut));
  ASD_HIP_CHECK(ctx, hipEventRecord(S->ev0, st));
  ASD_HIP_CHECK(ctx, S->up.upload(st));
  const size_t lds = (size_t)nq * 12;
  if (lds > 64 * 1024) {   // more than 64 KB of dynamic LDS has to be asked for once per kernel and device
    static AsdPerDeviceOnce attr_set;
    if (attr_set.need(ctx->cfg.device)) {
      ASD_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_kfdb_score<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      ASD_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_kfdb_score<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      attr_set.done(ctx->cfg.device);
    }
  }
  hipLaunchKernelGGL(S->scoring == 0 ? k_kfdb_score<false> : k_kfdb_score<true>, dim3((n_items + 3) / 4), dim3(256), lds, st, S->up.dev<int>(o_id),
                     S->up.dev<double>(o_val), nq, S->d_table, slot_list ? S->up.dev<int>(o_slots) : nullptr, n_items, S->d_ids, S->d_vals,
                     S->down.dev<KfOut>(o_out));
  ASD_HIP_CHECK(ctx, hipGetLastError());
  ASD_HIP_CHECK(ctx, hipEventRecord(S->ev1, st));
  ASD_HIP_CHECK(ctx, S->down.download(st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  ASD_HIP_CHECK(ctx, hipEventElapsedTime(&ctx->ms_kfdb, S->ev0, S->ev1));
  *out = S->down.host<KfOut>(o_out);
  return ASD_OK;
}

// lKFsSharingWords of one query: the slots in `list` into the reference's order
void sort_sharing(const KfdbState* S, const KfOut* r, std::vector<int>& list) {
  std::sort(list.begin(), list.end(), [&](int a, int b) {
    return r[a].first != r[b].first ? r[a].first < r[b].first : S->slots[a].seq < S->slots[b].seq;
  });
}

int hand_out(asd_ctx* ctx, const char* who, const LastQuery& Q, const KfdbState* S, int capacity, int32_t* scored_kf, float* scored_score,
             int32_t* n_scored) {
  *n_scored = (int32_t)Q.scored.size();
  if ((int)Q.scored.size() > capacity) { ctx->set_error("%s: %zu scored keyframes exceed the capacity %d", who, Q.scored.size(), capacity); return ASD_ERR_CAPACITY; }
  for (size_t i = 0; i < Q.scored.size(); ++i) { scored_kf[i] = S->slots[Q.scored[i].second].kf; scored_score[i] = Q.scored[i].first; }
  return ASD_OK;
}

}  // namespace

void kfdb_free(asd_ctx* ctx) {
  if (!ctx->kfdb) return;
  KfdbState* S = static_cast<KfdbState*>(ctx->kfdb);
  release_device(S);
  S->up.release();
  S->down.release();
  if (S->ev0) (void)hipEventDestroy(S->ev0);
  if (S->ev1) (void)hipEventDestroy(S->ev1);
  delete S;
  ctx->kfdb = nullptr;
}

static thread_local std::string g_bow_score_error;
const char* kfdb_host_error() { return g_bow_score_error.c_str(); }

extern "C" {

int asd_bow_score(int32_t scoring, int32_t n1, const int32_t* id1, const double* val1, int32_t n2, const int32_t* id2, const double* val2,
                  double* score) {
  g_bow_score_error.clear();
  if (scoring >= 2 && scoring <= 4) {
    g_bow_score_error = "asd_bow_score: CHI_SQUARE, KL and BHATTACHARYYA scoring are not offered (L1 = 0, L2 = 1, DOT_PRODUCT = 5)";
    return ASD_ERR_INVALID;
  }
  if (scoring < 0 || scoring > 5 || !score || n1 < 0 || n2 < 0 || (n1 > 0 && (!id1 || !val1)) || (n2 > 0 && (!id2 || !val2))) {
    g_bow_score_error = "asd_bow_score: invalid argument";
    return ASD_ERR_INVALID;
  }
  for (int i = 1; i < n1; ++i) if (id1[i] <= id1[i - 1]) { g_bow_score_error = "asd_bow_score: word ids of the first vector are not strictly ascending"; return ASD_ERR_INVALID; }
  for (int i = 1; i < n2; ++i) if (id2[i] <= id2[i - 1]) { g_bow_score_error = "asd_bow_score: word ids of the second vector are not strictly ascending"; return ASD_ERR_INVALID; }
  double s = 0;
  for (int i = 0, j = 0; i < n1 && j < n2;) {   // the lower_bound jumps of the reference land where this merge does
    if (id1[i] == id2[j]) {
      const double vi = val1[i], wi = val2[j];
      s += scoring == 0 ? fabs(vi - wi) - fabs(vi) - fabs(wi) : vi * wi;
      ++i; ++j;
    } else if (id1[i] < id2[j]) ++i;
    else ++j;
  }
  *score = finish_score(scoring, s);
  return ASD_OK;
}

int asd_kfdb_clear(asd_ctx* ctx, int32_t scoring) {
  if (!ctx) return ASD_ERR_INVALID;
  if (scoring == -1) {
    scoring = bow_loaded_scoring(ctx);
    if (scoring < 0) { ctx->set_error("asd_kfdb_clear: scoring -1 asks for the loaded vocabulary's, and none is loaded"); return ASD_ERR_INVALID; }
  }
  if (scoring >= 2 && scoring <= 4) { ctx->set_error("asd_kfdb_clear: CHI_SQUARE, KL and BHATTACHARYYA scoring are not offered (L1 = 0, L2 = 1, DOT_PRODUCT = 5)"); return ASD_ERR_INVALID; }
  if (scoring < 0 || scoring > 5) { ctx->set_error("asd_kfdb_clear: scoring %d unknown", scoring); return ASD_ERR_INVALID; }
  (void)hipSetDevice(ctx->cfg.device);
  KfdbState* S = kstate(ctx);
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  release_device(S);
  S->scoring = scoring;
  S->slots.clear(); S->table.clear(); S->free_slots.clear(); S->by_kf.clear();
  S->live = 0; S->live_words = 0; S->growths = 0;
  S->last[0] = LastQuery(); S->last[1] = LastQuery();
  S->last_loop_stamp = S->last_reloc_stamp = 0;
  return ASD_OK;
}

int asd_kfdb_add(asd_ctx* ctx, int32_t kf, int32_t n_words, const int32_t* bow_id, const double* bow_val, int32_t global_map) {
  if (!ctx) return ASD_ERR_INVALID;
  if (kf < 0) { ctx->set_error("asd_kfdb_add: keyframe id %d", kf); return ASD_ERR_INVALID; }
  int rc = check_bow(ctx, "asd_kfdb_add", n_words, bow_id, bow_val);
  if (rc != ASD_OK) return rc;
  (void)hipSetDevice(ctx->cfg.device);
  KfdbState* S = kstate(ctx);
  if (S->by_kf.count(kf)) { ctx->set_error("asd_kfdb_add: keyframe %d is already in the database", kf); return ASD_ERR_INVALID; }
  int slot;
  if (!S->free_slots.empty()) { slot = S->free_slots.back(); S->free_slots.pop_back(); }
  else { slot = (int)S->slots.size(); S->slots.emplace_back(); S->table.push_back(KfEntryDev{0, -1, 0}); }
  auto undo = [&]() { S->free_slots.push_back(slot); };
  if ((rc = grow_table(ctx, S, (int)S->slots.size())) != ASD_OK) { undo(); return rc; }
  if ((rc = grow_arena(ctx, S, n_words)) != ASD_OK) { undo(); return rc; }
  hipStream_t st = ctx->stream;
  const KfEntryDev e{S->word_used, n_words, 0};
  hipError_t he = S->up.begin(st, (size_t)n_words * 12 + 1024);
  if (he == hipSuccess) {
    const size_t o_val = S->up.add(bow_val, (size_t)n_words * sizeof(double)), o_id = S->up.add(bow_id, (size_t)n_words * sizeof(int));
    const size_t o_e = S->up.add(&e, sizeof e);
    if (n_words > 0) {
      he = hipMemcpyAsync(S->d_vals + e.off, S->up.h + o_val, (size_t)n_words * sizeof(double), hipMemcpyHostToDevice, st);
      if (he == hipSuccess) he = hipMemcpyAsync(S->d_ids + e.off, S->up.h + o_id, (size_t)n_words * sizeof(int), hipMemcpyHostToDevice, st);
    }
    if (he == hipSuccess) he = hipMemcpyAsync(S->d_table + slot, S->up.h + o_e, sizeof e, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);   // the staging block is the next call's
  }
  if (he != hipSuccess) { undo(); ctx->set_error("asd_kfdb_add: %s", hipGetErrorString(he)); return ASD_ERR_HIP; }
  S->table[slot] = e;
  S->word_used += n_words;
  KfEntry& E = S->slots[slot];
  E = KfEntry();
  E.kf = kf; E.global_map = global_map != 0; E.seq = S->next_seq++;
  S->by_kf[kf] = slot;
  ++S->live; S->live_words += n_words;
  return ASD_OK;
}

int asd_kfdb_erase(asd_ctx* ctx, int32_t kf) {
  if (!ctx) return ASD_ERR_INVALID;
  KfdbState* S = kstate(ctx);
  const auto it = S->by_kf.find(kf);
  if (it == S->by_kf.end()) return ASD_OK;
  (void)hipSetDevice(ctx->cfg.device);
  const int slot = it->second;
  hipStream_t st = ctx->stream;
  const KfEntryDev e{0, -1, 0};
  ASD_HIP_CHECK(ctx, S->up.begin(st, 1024));
  const size_t o_e = S->up.add(&e, sizeof e);
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(S->d_table + slot, S->up.h + o_e, sizeof e, hipMemcpyHostToDevice, st));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(st));
  --S->live; S->live_words -= S->table[slot].n;
  S->table[slot] = e;   // its words stay in the arena until the next growth compacts it
  S->slots[slot] = KfEntry();
  S->free_slots.push_back(slot);
  S->by_kf.erase(it);
  S->last[0].valid = S->last[1].valid = false;   // a scored list may name the slot
  return ASD_OK;
}

int asd_kfdb_score(asd_ctx* ctx, int32_t n_q, const int32_t* q_id, const double* q_val, int32_t n, const int32_t* kfs, double* score) {
  if (!ctx) return ASD_ERR_INVALID;
  if (n < 0 || (n > 0 && (!kfs || !score))) { ctx->set_error("asd_kfdb_score: invalid argument"); return ASD_ERR_INVALID; }
  int rc = check_bow(ctx, "asd_kfdb_score", n_q, q_id, q_val);
  if (rc != ASD_OK) return rc;
  KfdbState* S = kstate(ctx);
  std::vector<int> list(n);
  for (int i = 0; i < n; ++i) {
    const auto it = S->by_kf.find(kfs[i]);
    if (it == S->by_kf.end()) { ctx->set_error("asd_kfdb_score: keyframe %d is not in the database", kfs[i]); return ASD_ERR_INVALID; }
    list[i] = it->second;
  }
  if (n == 0) return ASD_OK;
  if (n_q == 0) { for (int i = 0; i < n; ++i) score[i] = finish_score(S->scoring, 0.0); return ASD_OK; }
  (void)hipSetDevice(ctx->cfg.device);
  const KfOut* r = nullptr;
  if ((rc = run_score(ctx, S, n_q, q_id, q_val, &list, n, &r)) != ASD_OK) return rc;
  for (int i = 0; i < n; ++i) score[i] = finish_score(S->scoring, r[i].sum);
  return ASD_OK;
}

int asd_kfdb_query_loop(asd_ctx* ctx, int32_t n_q, const int32_t* q_id, const double* q_val, int32_t n_connected, const int32_t* connected,
                        float min_score, int32_t only_global_map, int32_t capacity, int32_t* scored_kf, float* scored_score, int32_t* n_scored) {
  if (!ctx) return ASD_ERR_INVALID;
  if (!n_scored || capacity < 0 || (capacity > 0 && (!scored_kf || !scored_score)) || n_connected < 0 || (n_connected > 0 && !connected)) {
    ctx->set_error("asd_kfdb_query_loop: invalid argument");
    return ASD_ERR_INVALID;
  }
  int rc = check_bow(ctx, "asd_kfdb_query_loop", n_q, q_id, q_val);
  if (rc != ASD_OK) return rc;
  KfdbState* S = kstate(ctx);
  LastQuery& Q = S->last[0];
  Q = LastQuery();
  Q.valid = true;
  Q.stamp = S->last_loop_stamp = S->next_stamp++;
  Q.min_score = min_score;
  *n_scored = 0;
  const int n_slots = (int)S->slots.size();
  if (n_q == 0 || S->live == 0) return ASD_OK;
  (void)hipSetDevice(ctx->cfg.device);
  const KfOut* r = nullptr;
  if ((rc = run_score(ctx, S, n_q, q_id, q_val, nullptr, n_slots, &r)) != ASD_OK) { Q.valid = false; return rc; }
  std::vector<char> is_connected(n_slots, 0);
  for (int i = 0; i < n_connected; ++i) {
    const auto it = S->by_kf.find(connected[i]);
    if (it != S->by_kf.end()) is_connected[it->second] = 1;
  }
  std::vector<int> list;   // lKFsSharingWords (:94-113)
  for (int s = 0; s < n_slots; ++s) {
    KfEntry& E = S->slots[s];
    if (E.kf < 0 || r[s].cnt == 0) continue;
    if (is_connected[s]) { E.loop_words = 1; continue; }   // never stamped: every visit resets the count to 0 in front of the ++ (:102-111)
    E.loop_stamp = Q.stamp;
    E.loop_words = r[s].cnt;
    list.push_back(s);
  }
  if (list.empty()) return ASD_OK;
  sort_sharing(S, r, list);
  int max_common = 0;
  for (int s : list) max_common = std::max(max_common, S->slots[s].loop_words);
  const int min_common = (int)(max_common * 0.6f);   // :129
  Q.min_common = min_common;
  for (int s : list) {
    KfEntry& E = S->slots[s];
    if (E.loop_words > min_common) {
      const float si = (float)finish_score(S->scoring, r[s].sum);
      E.loop_score = si;
      if (si >= min_score)
        if ((only_global_map && E.global_map) || !only_global_map) Q.scored.emplace_back(si, s);
    }
  }
  return hand_out(ctx, "asd_kfdb_query_loop", Q, S, capacity, scored_kf, scored_score, n_scored);
}

int asd_kfdb_query_reloc(asd_ctx* ctx, int32_t n_q, const int32_t* q_id, const double* q_val, int32_t only_global_map, int32_t capacity,
                         int32_t* scored_kf, float* scored_score, int32_t* n_scored) {
  if (!ctx) return ASD_ERR_INVALID;
  if (!n_scored || capacity < 0 || (capacity > 0 && (!scored_kf || !scored_score))) { ctx->set_error("asd_kfdb_query_reloc: invalid argument"); return ASD_ERR_INVALID; }
  int rc = check_bow(ctx, "asd_kfdb_query_reloc", n_q, q_id, q_val);
  if (rc != ASD_OK) return rc;
  KfdbState* S = kstate(ctx);
  LastQuery& Q = S->last[1];
  Q = LastQuery();
  Q.valid = true;
  Q.stamp = S->last_reloc_stamp = S->next_stamp++;
  *n_scored = 0;
  const int n_slots = (int)S->slots.size();
  if (n_q == 0 || S->live == 0) return ASD_OK;
  (void)hipSetDevice(ctx->cfg.device);
  const KfOut* r = nullptr;
  if ((rc = run_score(ctx, S, n_q, q_id, q_val, nullptr, n_slots, &r)) != ASD_OK) { Q.valid = false; return rc; }
  std::vector<int> list;   // :216-235
  for (int s = 0; s < n_slots; ++s) {
    KfEntry& E = S->slots[s];
    if (E.kf < 0 || r[s].cnt == 0) continue;
    E.reloc_stamp = Q.stamp;
    E.reloc_words = r[s].cnt;
    if ((only_global_map && E.global_map) || !only_global_map) list.push_back(s);
  }
  if (list.empty()) return ASD_OK;
  sort_sharing(S, r, list);
  int max_common = 0;
  for (int s : list) max_common = std::max(max_common, S->slots[s].reloc_words);
  const int min_common = (int)(max_common * 0.8f);   // :248
  Q.min_common = min_common;
  for (int s : list) {
    KfEntry& E = S->slots[s];
    if (E.reloc_words > min_common) {
      const float si = (float)finish_score(S->scoring, r[s].sum);
      E.reloc_score = si;
      Q.scored.emplace_back(si, s);
    }
  }
  return hand_out(ctx, "asd_kfdb_query_reloc", Q, S, capacity, scored_kf, scored_score, n_scored);
}

int asd_kfdb_select(asd_ctx* ctx, int32_t mode, int32_t n_scored, const int32_t* neigh, int32_t capacity, int32_t* cand, int32_t* n_cand) {
  if (!ctx) return ASD_ERR_INVALID;
  if ((mode != 0 && mode != 1) || !n_cand || n_scored < 0 || (n_scored > 0 && !neigh) || capacity < 0 || (capacity > 0 && !cand)) {
    ctx->set_error("asd_kfdb_select: invalid argument");
    return ASD_ERR_INVALID;
  }
  KfdbState* S = kstate(ctx);
  const LastQuery& Q = S->last[mode];
  if (!Q.valid || n_scored != (int)Q.scored.size()) {
    ctx->set_error("asd_kfdb_select: n_scored = %d is not what the last %s query left (%s)", n_scored, mode ? "reloc" : "loop",
                   Q.valid ? "another count" : "no query, or an erase since");
    return ASD_ERR_INVALID;
  }
  *n_cand = 0;
  if (n_scored == 0) return ASD_OK;
  std::vector<std::pair<float, int>> acc_and_match;   // lAccScoreAndMatch (:153-181, :271-300)
  acc_and_match.reserve(n_scored);
  float best_acc = mode == 0 ? Q.min_score : 0.0f;
  for (int i = 0; i < n_scored; ++i) {
    float best_score = Q.scored[i].first, acc = Q.scored[i].first;
    int best = Q.scored[i].second;
    for (int k = 0; k < kNeigh; ++k) {
      const int id = neigh[(size_t)i * kNeigh + k];
      if (id < 0) continue;
      const auto it = S->by_kf.find(id);
      if (it == S->by_kf.end()) continue;   // not in the database: never stamped by a query
      const KfEntry& N = S->slots[it->second];
      float sc;
      if (mode == 0) {
        if (!(N.loop_stamp == Q.stamp && N.loop_words > Q.min_common)) continue;
        sc = N.loop_score;
      } else {
        if (N.reloc_stamp != Q.stamp) continue;
        sc = N.reloc_score;
      }
      acc += sc;
      if (sc > best_score) { best = it->second; best_score = sc; }
    }
    acc_and_match.emplace_back(acc, best);
    if (acc > best_acc) best_acc = acc;
  }
  const float retain = (mode == 0 ? 0.55f : 0.75f) * best_acc;
  std::vector<int> out;
  for (const auto& am : acc_and_match)
    if (am.first > retain && std::find(out.begin(), out.end(), am.second) == out.end()) out.push_back(am.second);
  *n_cand = (int32_t)out.size();
  if ((int)out.size() > capacity) { ctx->set_error("asd_kfdb_select: %zu candidates exceed the capacity %d", out.size(), capacity); return ASD_ERR_CAPACITY; }
  for (size_t i = 0; i < out.size(); ++i) cand[i] = S->slots[out[i]].kf;
  return ASD_OK;
}

int32_t asd_debug_kfdb(asd_ctx* ctx, int64_t out[5]) {
  if (!ctx || !out) return ASD_ERR_INVALID;
  const KfdbState* S = kstate(ctx);
  out[0] = S->live; out[1] = S->live_words; out[2] = S->table_cap; out[3] = S->word_cap; out[4] = S->growths;
  return ASD_OK;
}

int32_t asd_debug_kfdb_entry(asd_ctx* ctx, int32_t kf, int32_t out[4], float score[2]) {
  if (!ctx || !out || !score) return ASD_ERR_INVALID;
  const KfdbState* S = kstate(ctx);
  const auto it = S->by_kf.find(kf);
  if (it == S->by_kf.end()) { ctx->set_error("asd_debug_kfdb_entry: keyframe %d is not in the database", kf); return ASD_ERR_INVALID; }
  const KfEntry& E = S->slots[it->second];
  out[0] = E.loop_stamp != 0 && E.loop_stamp == S->last_loop_stamp;
  out[1] = E.loop_words;
  out[2] = E.reloc_stamp != 0 && E.reloc_stamp == S->last_reloc_stamp;
  out[3] = E.reloc_words;
  score[0] = E.loop_score; score[1] = E.reloc_score;
  return ASD_OK;
}

}  // extern "C"
