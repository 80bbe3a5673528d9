// matcher.h -- what the matcher's three units share: matcher.hip (the kernels, the frame slots, the tracking stages), matcher_replay.cpp
// (the searches that replay the reference's best / claim / histogram logic on the host) and matcher_banks.cpp (the descriptor and
// attribute banks, the prep-stream bracket).  Kernels are launched from matcher.hip only.
#pragma once
#include <chrono>
#include <vector>

#include "ctx.h"

// A window query = one GetFeaturesInArea call + the descriptor it is matched against.
using WinQuery = AsdWinQuery;   // (ctx.h: the solver's tail makes queries too)

struct MatcherState {
  int q_cap = 0, cand_cap = 0, h_cand_cap = 0, qdesc_cap = 0;   // cand_cap: device candidate buffers; h_cand_cap: their pinned host twins (host replay only)
  int last_total[4] = {1 << 15, 1 << 15, 1 << 15, 1 << 15};  // candidates the previous search of each kind produced
  WinQuery *d_queries = nullptr, *h_queries = nullptr;   // h_* pinned
  int *d_q_off = nullptr, *d_q_cnt = nullptr, *d_total = nullptr, *d_idx = nullptr;
  float* d_dist = nullptr;
  int *h_q = nullptr;      // [2*q_cap + 1]: off, cnt, total
  int* h_idx = nullptr;
  float* h_dist = nullptr;
  float *d_qdesc = nullptr, *h_qdesc = nullptr;
  float* d_bank = nullptr;  // device-resident descriptor bank (MapPoint::mDescriptor rows)
  int bank_cap = 0;
  // map-point attribute bank, same row ids: [row][8] = mWorldPos, mNormalVector, mfMinDistance, mfMaxDistance (asd_mpbank_put)
  float* d_attr = nullptr;
  int attr_cap = 0;
  float* d_cxw = nullptr;     // asd_track_local_points_rows: the candidates' positions as k_frustum_queries read them from the bank (the solver's table)
  size_t cxw_cap = 0;
  float* h_attr[2] = {nullptr, nullptr};   // pinned staging, used alternately
  size_t h_attr_cap[2] = {0, 0};
  hipEvent_t ev_attr[2] = {nullptr, nullptr};
  int attr_turn = 0;
  bool replay_host = false;  // ASD_MATCH_REPLAY=host at asd_ctx_create
};

// result of one batched window search: per query q the candidates idx[off[q] .. off[q]+cnt[q]) in
// Frame::GetFeaturesInArea order with their DescriptorDistance to the query's descriptor
struct SearchResult { const int* off; const int* cnt; const int* idx; const float* dist; };

// Node-restricted search (BoW-guided matchers): query q is matched against the explicit candidate list
// cand[cbeg[q] .. cend[q]) (the frame-2 members of the query's vocabulary node); distances land at
// out[ooff[q] + t] in list order.
struct ListQuery { int qrow, cbeg, cend, ooff; };

// ---- matcher.hip
MatcherState* matcher_state(asd_ctx* ctx);
AsdFrameSlot* matcher_slot(asd_ctx* ctx, int s);
int matcher_ensure_queries(asd_ctx* ctx, MatcherState* m, int nq);
int matcher_ensure_qdesc(asd_ctx* ctx, MatcherState* m, int n);
// query descriptors: host table -> pinned staging -> device (one async copy)
int matcher_upload_qdesc(asd_ctx* ctx, MatcherState* m, const float* desc, int n);
// queries are already in m->h_queries[0..nq); d_q = query descriptor table on the device
// kind: 0 frame-to-frame, 1 local map, 2 fuse, 3 other -- only sizes the speculative read-back
int matcher_window_search(asd_ctx* ctx, MatcherState* m, const AsdFrameSlot& F, int nq, const float* d_q, SearchResult* res, int kind = 3);
// distances of every (query keypoint of A, same-node keypoint of B) pair; queries in reference visiting order.
// On return lq[k] describes query k (qrow = keypoint in A, candidates fvB->idx[cbeg..cend), distances at dist[ooff..]).
int matcher_list_search(asd_ctx* ctx, MatcherState* m, const AsdFrameSlot& A, const AsdFrameSlot& B, const asd_feature_vector* fvA,
                        const asd_feature_vector* fvB, const uint8_t* skipA, bool skip_if_set, std::vector<ListQuery>& lq, const float** dist_out);

// ---- matcher_banks.cpp
// bank rows named by a caller: rows[i] for every i (or every i with used[i]) inside the descriptor bank and, with `attr_too`, inside the
// attribute bank as well
int matcher_check_bank_rows(asd_ctx* ctx, const MatcherState* m, const int32_t* rows, const uint8_t* used, int n, bool attr_too);

// ---- matcher_replay.cpp: the host replays of match_project_frame_impl / match_project_points_impl (ASD_MATCH_REPLAY=host, or tables beyond
// the replay workgroup), over the table the impl left in m->h_queries.  tm0: when the impl started projecting (ASD_TIMING).
int matcher_replay_frame(asd_ctx* ctx, MatcherState* m, const AsdFrameSlot& C, const AsdFrameSlot& L, const float* d_q, const uint8_t* obs_pos,
                         int check_orientation, int32_t* match_cur, int32_t* n_matches, std::chrono::steady_clock::time_point tm0);
int matcher_replay_points(asd_ctx* ctx, MatcherState* m, const AsdFrameSlot& F, int n_mp, const float* d_q, const uint8_t* occupied,
                          const uint8_t* obs_pos, float nn_ratio, int32_t* match_cur, int32_t* n_matches);

// ---- host helpers of more than one unit (f32 expressions of the reference: every unit that uses them is built with -ffp-contract=off)
// The table-filling half of a search: n queries in m->h_queries, each blank unless make(i, Q) writes it.
template <class Make>
int matcher_fill_queries(asd_ctx* ctx, MatcherState* m, int n, Make make) {
  const int rc = matcher_ensure_queries(ctx, m, n);
  if (rc != ASD_OK) return rc;
  for (int i = 0; i < n; ++i) {
    WinQuery& Q = m->h_queries[i];
    Q = WinQuery{0.f, 0.f, 0.f, 0, 0, -1};
    make(i, Q);
  }
  return ASD_OK;
}
// cv::Mat Rcw*x + tcw (gemm 3x3*3x1 small-matrix path, A*B+C folded): left-to-right f32 dot, then + t
inline void matcher_transform(const float* T, const float* X, float* out) {
  for (int r = 0; r < 3; ++r) {
    const float t0 = T[r * 4 + 0] * X[0] + T[r * 4 + 1] * X[1] + T[r * 4 + 2] * X[2];
    out[r] = (float)((double)t0 + (double)T[r * 4 + 3]);
  }
}
// mOw = -mRcw.t()*mtcw (Frame.cc:157): gemm with the transpose flag = general path, double accumulation.  R with rows of ld floats, t with
// elements inc apart: (Tcw, 4, Tcw + 3, 4) for a pose matrix, (R, 3, t, 1) for the pair
inline void matcher_camera_centre(const float* R, int ld, const float* t, int inc, float* Ow) {
  for (int i = 0; i < 3; ++i) {
    double sum = 0;
    for (int k = 0; k < 3; ++k) sum += (double)R[k * ld + i] * (double)t[k * inc];
    Ow[i] = (float)(-1.0 * sum);
  }
}
// KeyFrame::SetPose: Ow = -Rwc*tcw with Rwc materialised (gemm small-matrix path, f32 sums) -- ORBmatcher::Fuse's centre, NOT the double form
inline void matcher_keyframe_centre(const float* Tcw, float* Ow) {
  for (int i = 0; i < 3; ++i) {
    const float t0 = Tcw[0 * 4 + i] * Tcw[3] + Tcw[1 * 4 + i] * Tcw[7] + Tcw[2 * 4 + i] * Tcw[11];
    Ow[i] = (float)((double)t0 * -1.0);
  }
}
