// matcher_banks.cpp -- the device-resident banks the matchers read by row (MapPoint::mDescriptor; position, normal and distance range) and
// the bracket that moves frame construction to the context's second stream.  No kernels: device-to-device rows go through asd_copy_rows.
#include <algorithm>
#include <cstring>

#include "matcher.h"

namespace {
// rows [first_row, first_row + n) of a bank (first_row >= 0, n >= 0), summed in 64 bits: *end = first_row + n, or ASD_ERR_CAPACITY beyond
// ASD_BANK_MAX_ROWS.  Called before anything is allocated or enqueued.
int bank_range(asd_ctx* ctx, const char* who, int32_t first_row, int32_t n, int64_t* end) {
  *end = (int64_t)first_row + (int64_t)n;
  if (*end <= (int64_t)ASD_BANK_MAX_ROWS) return ASD_OK;
  ctx->set_error("%s: rows [%d, %lld) lie beyond ASD_BANK_MAX_ROWS (%d)", who, first_row, (long long)*end, (int)ASD_BANK_MAX_ROWS);
  return ASD_ERR_CAPACITY;
}
// capacity a bank grows to when `rows` (<= ASD_BANK_MAX_ROWS) are asked for
size_t bank_grown_cap(int64_t rows) {
  return std::min(std::max((size_t)rows + (size_t)rows / 2, (size_t)16384), (size_t)ASD_BANK_MAX_ROWS);
}

int ensure_bank(asd_ctx* ctx, MatcherState* m, int64_t rows) {   // rows <= ASD_BANK_MAX_ROWS (bank_range)
  if (rows <= (int64_t)m->bank_cap) return ASD_OK;
  const size_t cap = bank_grown_cap(rows);
  float* nb = nullptr;
  ASD_HIP_CHECK(ctx, hipMalloc(&nb, cap * 512));
  if (m->d_bank) {
    // growth is rare: everything that reads or writes the old bank has finished before it is snapshotted -- on EVERY stream of the
    // context (inside an asd_prep_async bracket the puts go to the second stream), as asd_mpbank_put's growth does it
    ASD_HIP_CHECK(ctx, hipDeviceSynchronize());
    ASD_HIP_CHECK(ctx, hipMemcpyAsync(nb, m->d_bank, (size_t)m->bank_cap * 512, hipMemcpyDeviceToDevice, ctx->stream));
    ASD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(m->d_bank);
  }
  m->d_bank = nb;
  m->bank_cap = (int)cap;
  return ASD_OK;
}
}  // namespace

int matcher_check_bank_rows(asd_ctx* ctx, const MatcherState* m, const int32_t* rows, const uint8_t* used, int n, bool attr_too) {
  for (int i = 0; i < n; ++i) {
    if (used && !used[i]) continue;
    if (rows[i] < 0 || rows[i] >= m->bank_cap) { ctx->set_error("bank row %d out of range (descriptor bank: %d rows)", rows[i], m->bank_cap); return ASD_ERR_INVALID; }
    if (attr_too && rows[i] >= m->attr_cap) { ctx->set_error("bank row %d out of range (attribute bank: %d rows)", rows[i], m->attr_cap); return ASD_ERR_INVALID; }
  }
  return ASD_OK;
}

extern "C" {

// MapPoint::mDescriptor rows kept on the device: written when a map point's descriptor changes
// (MapPoint::ComputeDistinctiveDescriptors, once per keyframe), read by the matchers every frame.
int asd_bank_put(asd_ctx* ctx, int32_t first_row, int32_t n, const float* desc) {
  if (!ctx || first_row < 0 || n < 0 || (n > 0 && !desc)) return ASD_ERR_INVALID;
  int64_t end;
  int rc = bank_range(ctx, "asd_bank_put", first_row, n, &end);
  if (rc != ASD_OK) return rc;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  rc = ensure_bank(ctx, m, end);
  if (rc != ASD_OK || n == 0) return rc;
  // the pinned staging block is matcher_upload_qdesc's too: an armed asd_track_* stage of the descriptor form may still have its copy out of it
  // pending, so the stream drains BEFORE the block is rewritten (or freed by matcher_ensure_qdesc) -- the wait this call makes anyway, moved up
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = matcher_ensure_qdesc(ctx, m, n)) != ASD_OK) return rc;
  memcpy(m->h_qdesc, desc, (size_t)n * 512);
  ASD_HIP_CHECK(ctx, hipMemcpyAsync(m->d_bank + (size_t)first_row * 128, m->h_qdesc, (size_t)n * 512, hipMemcpyHostToDevice, ctx->stream));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return ASD_OK;
}

// bank[first_row + i] = descriptor of keypoint i of frame `slot` (device to device), i in [0, n)
int asd_bank_put_from_frame(asd_ctx* ctx, int32_t slot, int32_t first_row, int32_t n) {
  AsdFrameSlot* F = matcher_slot(ctx, slot);
  if (!F || first_row < 0 || n < 0 || n > F->n) return ASD_ERR_INVALID;
  int64_t end;
  int rc = bank_range(ctx, "asd_bank_put_from_frame", first_row, n, &end);
  if (rc != ASD_OK) return rc;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  rc = ensure_bank(ctx, m, end);
  if (rc != ASD_OK || n == 0) return rc;
  ASD_HIP_CHECK(ctx, asd_copy_rows(asd_prep_stream(ctx), m->d_bank + (size_t)first_row * 128, F->d_desc, (size_t)n * 512));
  return ASD_OK;
}

// MapPoint::{mWorldPos, mNormalVector, mfMinDistance, mfMaxDistance} of rows [first_row, first_row + n) of the bank
int asd_mpbank_put(asd_ctx* ctx, int32_t first_row, int32_t n, const float* Xw, const float* normal, const float* min_dist, const float* max_dist) {
  if (!ctx || first_row < 0 || n < 0 || (n > 0 && (!Xw || !normal || !min_dist || !max_dist))) return ASD_ERR_INVALID;
  int64_t end;
  const int rc = bank_range(ctx, "asd_mpbank_put", first_row, n, &end);
  if (rc != ASD_OK) return rc;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  if (end > (int64_t)m->attr_cap) {
    const size_t cap = bank_grown_cap(end);
    float* nb = nullptr;
    ASD_HIP_CHECK(ctx, hipMalloc(&nb, cap * 32));
    ASD_HIP_CHECK(ctx, hipDeviceSynchronize());   // (growth is rare: everything that reads or writes the old table has finished)
    if (m->d_attr) { ASD_HIP_CHECK(ctx, hipMemcpy(nb, m->d_attr, (size_t)m->attr_cap * 32, hipMemcpyDeviceToDevice)); (void)hipFree(m->d_attr); }
    m->d_attr = nb;
    m->attr_cap = (int)cap;
  }
  if (n == 0) return ASD_OK;
  const int k = m->attr_turn ^= 1;
  if (!m->ev_attr[k]) ASD_HIP_CHECK(ctx, hipEventCreateWithFlags(&m->ev_attr[k], hipEventDisableTiming));
  else ASD_HIP_CHECK(ctx, hipEventSynchronize(m->ev_attr[k]));   // this staging buffer's previous upload has left it
  if (m->h_attr_cap[k] < (size_t)n * 32) {
    if (m->h_attr[k]) (void)hipHostFree(m->h_attr[k]);
    m->h_attr[k] = nullptr; m->h_attr_cap[k] = 0;
    ASD_HIP_CHECK(ctx, hipHostMalloc(&m->h_attr[k], (size_t)n * 48));
    m->h_attr_cap[k] = (size_t)n * 48;
  }
  float* h = m->h_attr[k];
  for (int i = 0; i < n; ++i) {
    float* r = h + 8 * (size_t)i;
    r[0] = Xw[3 * i]; r[1] = Xw[3 * i + 1]; r[2] = Xw[3 * i + 2];
    r[3] = normal[3 * i]; r[4] = normal[3 * i + 1]; r[5] = normal[3 * i + 2];
    r[6] = min_dist[i]; r[7] = max_dist[i];
  }
  hipStream_t st = asd_prep_stream(ctx);
  ASD_HIP_CHECK(ctx, asd_copy_rows(st, m->d_attr + 8 * (size_t)first_row, h, (size_t)n * 32));
  ASD_HIP_CHECK(ctx, hipEventRecord(m->ev_attr[k], st));
  return ASD_OK;
}

// Test aid: rows [first_row, first_row + n) of the two banks as a consumer would read them -- copies enqueued on the context's stream, that
// stream alone waited for.  It does NOT wait for the second stream: a bracket that failed to order its writes must show here.
int32_t asd_debug_bank_get(asd_ctx* ctx, int32_t first_row, int32_t n, float* desc, float* attr) {
  if (!ctx) return ASD_ERR_INVALID;
  if (first_row < 0 || n < 0) { ctx->set_error("asd_debug_bank_get: first_row %d, n %d", first_row, n); return ASD_ERR_INVALID; }
  if (ctx->prep_on) { ctx->set_error("asd_debug_bank_get: an asd_prep_async bracket is open"); return ASD_ERR_INVALID; }
  if (asd_track_busy(ctx, "asd_debug_bank_get")) return ASD_ERR_INVALID;
  MatcherState* m = matcher_state(ctx);
  const int64_t end = (int64_t)first_row + (int64_t)n;
  if (desc && end > (int64_t)m->bank_cap) { ctx->set_error("asd_debug_bank_get: rows [%d, %lld) outside the descriptor bank (%d rows)", first_row, (long long)end, m->bank_cap); return ASD_ERR_INVALID; }
  if (attr && end > (int64_t)m->attr_cap) { ctx->set_error("asd_debug_bank_get: rows [%d, %lld) outside the attribute bank (%d rows)", first_row, (long long)end, m->attr_cap); return ASD_ERR_INVALID; }
  if (n == 0 || (!desc && !attr)) return ASD_OK;
  (void)hipSetDevice(ctx->cfg.device);
  if (desc) ASD_HIP_CHECK(ctx, hipMemcpyAsync(desc, m->d_bank + (size_t)first_row * 128, (size_t)n * 512, hipMemcpyDeviceToHost, ctx->stream));
  if (attr) ASD_HIP_CHECK(ctx, hipMemcpyAsync(attr, m->d_attr + (size_t)first_row * 8, (size_t)n * 32, hipMemcpyDeviceToHost, ctx->stream));
  ASD_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return ASD_OK;
}

// Frame construction beside the stages in flight: between asd_prep_async(ctx, 1) and asd_prep_async(ctx, 0) the device work of
// asd_frame_set, asd_bank_put_from_frame and asd_mpbank_put goes to a second stream of the context instead of queueing behind the
// outstanding asd_track_* stage; closing the bracket makes everything enqueued on the context's stream AFTERWARDS wait for it.
int asd_prep_async(asd_ctx* ctx, int32_t on) {
  if (!ctx) return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  if (on) {
    if (!ctx->stream_prep) {
      int lo = 0, hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
      // highest priority, like the main stream
      ASD_HIP_CHECK(ctx, hipStreamCreateWithPriority(&ctx->stream_prep, hipStreamNonBlocking, hi));
      ASD_HIP_CHECK(ctx, hipEventCreateWithFlags(&ctx->ev_prep, hipEventDisableTiming));
    }
    ctx->prep_on = true;
    return ASD_OK;
  }
  if (!ctx->prep_on) return ASD_OK;
  ctx->prep_on = false;
  ASD_HIP_CHECK(ctx, hipEventRecord(ctx->ev_prep, ctx->stream_prep));
  ASD_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_prep, 0));
  return ASD_OK;
}

}  // extern "C"
