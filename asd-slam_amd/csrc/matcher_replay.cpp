// matcher_replay.cpp -- the ORBmatcher searches that launch no kernel of their own: the host evaluates the per-point gates in the
// reference's f32 arithmetic (-ffp-contract=off) and fills the query table, matcher.hip's k_window_search / k_list_dist walk the grid or the
// vocabulary node and evaluate the candidates' distances, the host replays the reference's best / claim / histogram logic over the lists.
// One skeleton (query_search, best_of, RotHist); each site keeps its own projection and acceptance, which mirror different lines of the
// reference: how 1/z is rounded, the product order, inclusive or exclusive image bounds, the depth gate, thresholds and level windows.
//
// Reference (src/vslam/src): ORBmatcher.cc:44-122, :1318-1452 (the tracking searches' host replays), :416-531 (initialisation), :183-278,
// :533-666, :669-822 (BoW-guided), :825-936, :963-1086 (Fuse), :300-413, :1090-1314, :1455-1582 (loop closing, relocalisation),
// :1584-1625 (ComputeThreeMaxima), Frame.cc:160-217 (isInFrustum), :219-274 (GetFeaturesInArea).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "matcher.h"
#include "resolve2.h"   // TH_HIGH, TH_LOW, HISTO

namespace {
inline void three_maxima(const int* cnt, int& ind1, int& ind2, int& ind3) {  // ORBmatcher.cc:1584-1625
  int max1 = 0, max2 = 0, max3 = 0;
  ind1 = ind2 = ind3 = -1;
  for (int i = 0; i < HISTO; i++) {
    const int s = cnt[i];
    if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
    else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
    else if (s > max3) { max3 = s; ind3 = i; }
  }
  if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
  else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
}

inline int rot_bin(float a1, float a2) {  // :1419-1425
  float rot = a1 - a2;
  if (rot < 0.0) rot += 360.0f;
  int bin = (int)std::round(rot * (1.0f / HISTO));
  if (bin == HISTO) bin = 0;
  return bin;
}

// The rotation histogram of a search (rotHist[], ComputeThreeMaxima and the erase loop): items are whatever the site's matches are keyed
// by, drop(item) is the site's own erase action for an item outside the three largest bins
struct RotHist {
  std::vector<int> hist[HISTO];
  void add(int bin, int item) { hist[bin].push_back(item); }
  template <class Drop>
  void prune(Drop drop) const {
    int cnt[HISTO], i1, i2, i3;
    for (int b = 0; b < HISTO; ++b) cnt[b] = (int)hist[b].size();
    three_maxima(cnt, i1, i2, i3);
    for (int b = 0; b < HISTO; ++b)
      if (b != i1 && b != i2 && b != i3)
        for (int item : hist[b]) drop(item);
  }
};

// The smallest and second smallest distance below `start` among the candidates (idx[t], dist[t]), t < n, that accept(keypoint) lets
// through, and the keypoint of the smallest: the first one in list order among equals (strict `<`), -1 if none.  Of a window search's query i
// in the second form.
struct Best { float dist, dist2; int idx; };
template <class Accept>
inline Best best_of(const int* idx, const float* dist, int n, float start, Accept accept) {
  Best b{start, start, -1};
  for (int t = 0; t < n; ++t) {
    if (!accept(idx[t])) continue;
    if (dist[t] < b.dist) { b.dist2 = b.dist; b.dist = dist[t]; b.idx = idx[t]; }
    else if (dist[t] < b.dist2) b.dist2 = dist[t];
  }
  return b;
}
template <class Accept>
inline Best best_of(const SearchResult& R, int i, float start, Accept accept) {
  return best_of(R.idx + R.off[i], R.dist + R.off[i], R.cnt[i], start, accept);
}

// One batched window search over frame F: n queries, each blank unless make(i, Q) writes it, matched by the rows of `desc` (host table,
// uploaded) or, without one, of the resident table d_q
template <class Make>
int query_search(asd_ctx* ctx, MatcherState* m, const AsdFrameSlot& F, int n, const float* desc, const float* d_q, int kind, SearchResult* R, Make make) {
  int rc = matcher_fill_queries(ctx, m, n, make);
  if (rc == ASD_OK && desc) rc = matcher_upload_qdesc(ctx, m, desc, n);
  return rc != ASD_OK ? rc : matcher_window_search(ctx, m, F, n, desc ? m->d_qdesc : d_q, R, kind);
}

inline void split_pose(const float* Tcw, float* R, float* t) {
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) R[r * 3 + c] = Tcw[r * 4 + c]; t[r] = Tcw[r * 4 + 3]; }
}
// Scw -> Rcw = sRcw / scw, tcw = Scw.col(3) / scw (ORBmatcher.cc:310-313; Mat / scalar = convertTo with a float scale)
void decompose_sim3(const float* Scw, float* Rcw, float* tcw) {
  double d = 0;
  for (int k = 0; k < 3; ++k) d += (double)Scw[k] * (double)Scw[k];
  const float scw = (float)std::sqrt(d);
  const float inv = (float)(1.0 / (double)scw);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rcw[r * 3 + c] = Scw[r * 4 + c] * inv + 0.0f;
    tcw[r] = Scw[r * 4 + 3] * inv + 0.0f;
  }
}
inline void rot_add(const float* R, const float* t, const float* X, float* out) {
  for (int r = 0; r < 3; ++r) {
    const float t0 = R[r * 3 + 0] * X[0] + R[r * 3 + 1] * X[1] + R[r * 3 + 2] * X[2];
    out[r] = (float)((double)t0 + (double)t[r]);
  }
}
inline float norm3f(const float* p) {
  return (float)std::sqrt((double)p[0] * p[0] + (double)p[1] * p[1] + (double)p[2] * p[2]);
}
inline int predict_scale(const asd_ctx* ctx, float maxd_raw, float dist) {  // MapPoint::PredictScale (MapPoint.cc:438-453)
  int s = (int)std::ceil(std::log(maxd_raw / dist) / std::log(ctx->cfg.scale_factor));
  if (s < 0) s = 0;
  else if (s >= ctx->cfg.n_levels) s = ctx->cfg.n_levels - 1;
  return s;
}
// front half shared by the two Scw searches (:300-366, :963-1010)
bool sim3_project(const asd_ctx* ctx, const AsdFrameSlot& KF, const float* Rcw, const float* tcw, const float* Ow, const float* K,
                  const float* P, const float* Pn, float mind_raw, float maxd_raw, bool double_invz, float* u, float* v, int* level) {
  float Pc[3];
  rot_add(Rcw, tcw, P, Pc);
  if (Pc[2] < 0.0f) return false;
  const float invz = double_invz ? (float)(1.0 / Pc[2]) : 1 / Pc[2];
  *u = K[0] * (Pc[0] * invz) + K[2];
  *v = K[1] * (Pc[1] * invz) + K[3];
  if (!(*u >= KF.min_x && *u < KF.max_x && *v >= KF.min_y && *v < KF.max_y)) return false;
  const float PO[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
  const float dist = norm3f(PO);
  if (dist < 0.8f * mind_raw || dist > 1.2f * maxd_raw) return false;
  const double dot = (double)PO[0] * Pn[0] + (double)PO[1] * Pn[1] + (double)PO[2] * Pn[2];
  if (dot < 0.5 * dist) return false;
  *level = predict_scale(ctx, maxd_raw, dist);
  return true;
}

// Frame::GetFeaturesInArea (Frame.cc:219-274) on the host CSR mirror (asd_frame_features_in_area only)
void features_in_area(const AsdFrameSlot& F, float x, float y, float r, int minLevel, int maxLevel, std::vector<int>& out) {
  constexpr int GC = ASD_GRID_COLS, GR = ASD_GRID_ROWS;
  const int nMinCellX = std::max(0, (int)std::floor((x - F.min_x - r) * F.inv_w));
  if (nMinCellX >= GC) return;
  const int nMaxCellX = std::min(GC - 1, (int)std::ceil((x - F.min_x + r) * F.inv_w));
  if (nMaxCellX < 0) return;
  const int nMinCellY = std::max(0, (int)std::floor((y - F.min_y - r) * F.inv_h));
  if (nMinCellY >= GR) return;
  const int nMaxCellY = std::min(GR - 1, (int)std::ceil((y - F.min_y + r) * F.inv_h));
  if (nMaxCellY < 0) return;
  const bool check = (minLevel > 0) || (maxLevel >= 0);
  for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
    const int b = F.cell_start[ix * GR + nMinCellY], e = F.cell_start[ix * GR + nMaxCellY + 1];
    for (int t = b; t < e; ++t) {
      const int idx = F.cell_items[t];
      const asd_keypoint& kp = F.kps[idx];
      if (check) {
        if (kp.octave < minLevel) continue;
        if (maxLevel >= 0 && kp.octave > maxLevel) continue;
      }
      const float dx = kp.x - x, dy = kp.y - y;
      if (std::fabs(dx) < r && std::fabs(dy) < r) out.push_back(idx);
    }
  }
}

bool fv_valid(const asd_feature_vector* fv, int n) {
  if (!fv || fv->n_nodes < 0 || (fv->n_nodes > 0 && (!fv->node_id || !fv->start || !fv->idx))) return false;
  for (int i = 0; i < fv->n_nodes; ++i) {
    if (i > 0 && fv->node_id[i] <= fv->node_id[i - 1]) return false;
    if (fv->start[i + 1] < fv->start[i]) return false;
  }
  for (int t = fv->n_nodes ? fv->start[0] : 0; t < (fv->n_nodes ? fv->start[fv->n_nodes] : 0); ++t)
    if (fv->idx[t] < 0 || fv->idx[t] >= n) return false;
  return true;
}
}  // namespace

// ---- the host replays of the two tracking searches ----------------------------------------------------------------------------------
// SearchByProjection(CurrentFrame, LastFrame, th) (ORBmatcher.cc:1370-1450) behind the projection loop of match_project_frame_impl
int matcher_replay_frame(asd_ctx* ctx, MatcherState* m, const AsdFrameSlot& C, const AsdFrameSlot& L, const float* d_q, const uint8_t* obs_pos,
                         int check_orientation, int32_t* match_cur, int32_t* n_matches, std::chrono::steady_clock::time_point tm0) {
  static const bool timing = getenv("ASD_TIMING") != nullptr;
  static double tacc[3]; static long tcalls;
  int rc;
  SearchResult R;
  const auto tm1 = std::chrono::steady_clock::now();
  if ((rc = matcher_window_search(ctx, m, C, L.n, d_q, &R, 0)) != ASD_OK) return rc;
  const auto tm2 = std::chrono::steady_clock::now();
  int nmatches = 0;
  // rotation histogram (ORBmatcher.cc:1419-1425, 1437-1450) without per-bin vectors: a current keypoint is matched at most
  // once, so its bin is kept per keypoint and the bins only need their counts
  static thread_local std::vector<int8_t> bin_of;
  // with map points that have no observations a keypoint can be written -- and enter the histogram -- more than once
  // (ORBmatcher.cc:1392-1395): those calls keep the reference's per-write entries (keypoint, bin)
  static thread_local std::vector<std::pair<int, int8_t>> writes;
  if (obs_pos) writes.clear();
  int cnt[HISTO];
  for (int b = 0; b < HISTO; ++b) cnt[b] = 0;
  if (check_orientation) bin_of.assign(C.n, -1);
  constexpr int kAhead = 12;  // the lists were just written by DMA: every line is a DRAM miss, and segments sit in launch order, not query order
  for (int i = 0; i < L.n; ++i) {
    if (i + kAhead < L.n && R.cnt[i + kAhead] > 0) {
      __builtin_prefetch(R.idx + R.off[i + kAhead]);
      __builtin_prefetch(R.dist + R.off[i + kAhead]);
    }
    if (R.cnt[i] == 0) continue;
    float best = 100;
    int best_idx = -1;
    const int* idx = R.idx + R.off[i];
    const float* dist = R.dist + R.off[i];
    for (int t = 0, e = R.cnt[i]; t < e; ++t) {
      const int j = idx[t];
      if (match_cur[j] >= 0 && (!obs_pos || obs_pos[match_cur[j]])) continue;  // holds a map point with Observations() > 0
      if (dist[t] < best) { best = dist[t]; best_idx = j; }
    }
    if (best <= TH_HIGH) {
      match_cur[best_idx] = i;
      nmatches++;
      if (check_orientation) {
        const int b = rot_bin(L.kps[i].angle, C.kps[best_idx].angle);
        if (obs_pos) writes.emplace_back(best_idx, (int8_t)b);
        else bin_of[best_idx] = (int8_t)b;
        ++cnt[b];
      }
    }
  }
  if (check_orientation) {
    int i1, i2, i3;
    three_maxima(cnt, i1, i2, i3);
    if (obs_pos) {
      for (const auto& w : writes)
        if (w.second != i1 && w.second != i2 && w.second != i3) { match_cur[w.first] = -1; nmatches--; }
    } else {
      for (int j = 0; j < C.n; ++j) {
        const int b = bin_of[j];
        if (b >= 0 && b != i1 && b != i2 && b != i3) { match_cur[j] = -1; nmatches--; }
      }
    }
  }
  *n_matches = nmatches;
  if (timing) {
    const auto tm3 = std::chrono::steady_clock::now();
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    tacc[0] += ms(tm0, tm1); tacc[1] += ms(tm1, tm2); tacc[2] += ms(tm2, tm3);
    if (++tcalls % 200 == 0)
      fprintf(stderr, "[match_project_frame] project %.3f search %.3f select %.3f ms\n", tacc[0] / tcalls, tacc[1] / tcalls, tacc[2] / tcalls);
  }
  return ASD_OK;
}

// SearchByProjection(F, vpMapPoints, th) (ORBmatcher.cc:72-119) behind the window table of match_project_points_impl
int matcher_replay_points(asd_ctx* ctx, MatcherState* m, const AsdFrameSlot& F, int n_mp, const float* d_q, const uint8_t* occupied,
                          const uint8_t* obs_pos, float nn_ratio, int32_t* match_cur, int32_t* n_matches) {
  SearchResult R;
  const int rc = matcher_window_search(ctx, m, F, n_mp, d_q, &R, 1);
  if (rc != ASD_OK) return rc;
  int nmatches = 0;
  for (int q = 0; q < n_mp; ++q) {
    if (R.cnt[q] == 0) continue;
    float best = 256, best2 = 256;
    int best_lvl = -1, best_lvl2 = -1, best_idx = -1;
    for (int t = R.off[q]; t < R.off[q] + R.cnt[q]; ++t) {
      const int j = R.idx[t];
      if (occupied[j] || (match_cur[j] >= 0 && (!obs_pos || obs_pos[match_cur[j]]))) continue;
      const float d = R.dist[t];
      if (d < best) {
        best2 = best; best = d;
        best_lvl2 = best_lvl; best_lvl = F.kps[j].octave;
        best_idx = j;
      } else if (d < best2) {
        best_lvl2 = F.kps[j].octave;
        best2 = d;
      }
    }
    if (best <= TH_HIGH) {
      if (best_lvl == best_lvl2 && best > nn_ratio * best2) continue;
      match_cur[best_idx] = q;
      nmatches += 2;  // the reference increments twice per match (ORBmatcher.cc:116-117)
    }
  }
  *n_matches = nmatches;
  return ASD_OK;
}

extern "C" {

int asd_frame_features_in_area(asd_ctx* ctx, int32_t slot, float x, float y, float r, int32_t min_level,
                               int32_t max_level, int32_t capacity, int32_t* idx_out, int32_t* n_out) {
  AsdFrameSlot* F = matcher_slot(ctx, slot);
  if (!F || !idx_out || !n_out) return ASD_ERR_INVALID;
  // single query through the same kernel the matchers use (so the test of this entry point is a
  // test of the device grid walk); the host mirror cross-checks it
  MatcherState* m = matcher_state(ctx);
  int rc = matcher_ensure_queries(ctx, m, 1);
  if (rc != ASD_OK) return rc;
  if (F->n == 0) { *n_out = 0; return ASD_OK; }
  m->h_queries[0] = WinQuery{x, y, r, min_level, max_level, 0};
  SearchResult res;
  if ((rc = matcher_window_search(ctx, m, *F, 1, F->d_desc, &res)) != ASD_OK) return rc;
  std::vector<int> host;
  features_in_area(*F, x, y, r, min_level, max_level, host);
  if ((int)host.size() != res.cnt[0] || !std::equal(host.begin(), host.end(), res.idx + res.off[0])) {
    ctx->set_error("device grid walk disagrees with the host mirror");
    return ASD_ERR_HIP;
  }
  const int n = std::min(res.cnt[0], capacity);
  for (int i = 0; i < n; ++i) idx_out[i] = res.idx[res.off[0] + i];
  *n_out = n;
  return ASD_OK;
}

// ORBmatcher::Fuse, search half (ORBmatcher.cc:825-936): the Replace / AddObservation side effects
// (:938-956) do not feed back into the search, so every map point is an independent window query.
int asd_fuse_search(asd_ctx* ctx, int32_t slot_kf, int32_t n_mp, const uint8_t* valid, const float* Xw, const float* normal,
                    const float* min_dist, const float* max_dist, const float* desc, const float* Tcw, const float* K,
                    float th, int32_t* best_idx, float* best_dist) {
  AsdFrameSlot* KF = matcher_slot(ctx, slot_kf);
  if (!KF || n_mp < 0 || !Tcw || !K || (n_mp > 0 && (!valid || !Xw || !normal || !min_dist || !max_dist || !desc || !best_idx || !best_dist)))
    return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  for (int i = 0; i < n_mp; ++i) { best_idx[i] = -1; best_dist[i] = 256.f; }
  if (n_mp == 0 || KF->n == 0) return ASD_OK;
  const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  float Ow[3];
  matcher_keyframe_centre(Tcw, Ow);
  std::vector<int> pred(n_mp, 0);
  std::vector<float> pu(n_mp), pv(n_mp);
  SearchResult R;
  const int rc = query_search(ctx, m, *KF, n_mp, desc, nullptr, 2, &R, [&](int i, WinQuery& Q) {
    if (!valid[i]) return;
    const float* P = Xw + 3 * i;
    float Pc[3];
    matcher_transform(Tcw, P, Pc);
    if (Pc[2] < 0.0f) return;
    const float invz = 1 / Pc[2];
    const float u = fx * (Pc[0] * invz) + cx, v = fy * (Pc[1] * invz) + cy;
    if (!(u >= KF->min_x && u < KF->max_x && v >= KF->min_y && v < KF->max_y)) return;  // KeyFrame::IsInImage
    const float maxD = 1.2f * max_dist[i], minD = 0.8f * min_dist[i];
    const float PO[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
    const double nn = (double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2];
    const float dist3D = (float)std::sqrt(nn);
    if (dist3D < minD || dist3D > maxD) return;
    const float* Pn = normal + 3 * i;
    const double dot = (double)PO[0] * Pn[0] + (double)PO[1] * Pn[1] + (double)PO[2] * Pn[2];
    if (dot < 0.5 * dist3D) return;
    pred[i] = predict_scale(ctx, max_dist[i], dist3D); pu[i] = u; pv[i] = v;
    Q = WinQuery{u, v, th * ctx->scale[pred[i]], -1, -1, i};  // KeyFrame::GetFeaturesInArea: no level filter
  });
  if (rc != ASD_OK) return rc;
  for (int i = 0; i < n_mp; ++i) {
    if (R.cnt[i] == 0) continue;
    const Best b = best_of(R, i, 256, [&](int j) {
      const asd_keypoint& kp = KF->kps[j];
      if (kp.octave < pred[i] - 1 || kp.octave > pred[i]) return false;
      const float ex = pu[i] - kp.x, ey = pv[i] - kp.y;
      const float e2 = ex * ex + ey * ey;
      return !(e2 * ctx->inv_sigma2[kp.octave] > 5.99);
    });
    if (b.dist <= TH_LOW) { best_idx[i] = b.idx; best_dist[i] = b.dist; }
  }
  return ASD_OK;
}

// ---- relocalisation / loop-closing variants of the projection searches -----------------------

// ORBmatcher::SearchByProjection(Frame&, KeyFrame*, const set<MapPoint*>&, float th, float ORBdist) (:1455-1582)
int asd_match_project_keyframe(asd_ctx* ctx, int32_t slot_cur, int32_t n_kf, const uint8_t* valid, const float* Xw, const float* min_dist,
                               const float* max_dist, const float* desc, const float* kf_angle, const uint8_t* occupied, const float* Tcw,
                               const float* K, float th, float orb_dist, int32_t check_orientation, int32_t* match_cur,
                               int32_t* n_matches) {
  AsdFrameSlot* C = matcher_slot(ctx, slot_cur);
  if (!C || n_kf < 0 || !Tcw || !K || !match_cur || !n_matches || (C->n > 0 && !occupied) ||
      (n_kf > 0 && (!valid || !Xw || !min_dist || !max_dist || !desc || !kf_angle)))
    return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  std::fill(match_cur, match_cur + C->n, -1);
  *n_matches = 0;
  if (n_kf == 0 || C->n == 0) return ASD_OK;
  float Ow[3];
  matcher_camera_centre(Tcw, 4, Tcw + 3, 4, Ow);
  SearchResult R;
  const int rc = query_search(ctx, m, *C, n_kf, desc, nullptr, 3, &R, [&](int i, WinQuery& Q) {
    if (!valid[i]) return;
    const float* P = Xw + 3 * i;
    float Pc[3];
    matcher_transform(Tcw, P, Pc);
    const float invzc = 1.0 / Pc[2];
    const float u = K[0] * Pc[0] * invzc + K[2];
    const float v = K[1] * Pc[1] * invzc + K[3];
    if (!(u >= C->min_x && u <= C->max_x && v >= C->min_y && v <= C->max_y)) return;  // also drops NaN (z == 0)
    const float PO[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
    const float dist3D = norm3f(PO);
    if (dist3D < 0.8f * min_dist[i] || dist3D > 1.2f * max_dist[i]) return;
    const int lvl = predict_scale(ctx, max_dist[i], dist3D);
    Q = WinQuery{u, v, th * ctx->scale[lvl], lvl - 1, lvl + 1, i};
  });
  if (rc != ASD_OK) return rc;
  std::vector<uint8_t> occ(occupied, occupied + C->n);
  RotHist hist;
  int nmatches = 0;
  for (int i = 0; i < n_kf; ++i) {
    if (R.cnt[i] == 0) continue;
    const Best b = best_of(R, i, 256, [&](int j) { return !occ[j]; });
    if (b.dist <= orb_dist) {
      occ[b.idx] = 1;
      match_cur[b.idx] = i;
      nmatches++;
      if (check_orientation) hist.add(rot_bin(kf_angle[i], C->kps[b.idx].angle), b.idx);
    }
  }
  if (check_orientation) hist.prune([&](int j) { match_cur[j] = -1; nmatches--; });
  *n_matches = nmatches;
  return ASD_OK;
}

// ORBmatcher::SearchByProjection(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, vector<MapPoint*>& vpMatched, int th) (:300-413)
int asd_match_project_sim3(asd_ctx* ctx, int32_t slot_kf, const float* Scw, int32_t n_mp, const uint8_t* valid, const float* Xw,
                           const float* normal, const float* min_dist, const float* max_dist, const float* desc, const float* K,
                           int32_t th, int32_t* matched_kp, int32_t* n_matches) {
  AsdFrameSlot* KF = matcher_slot(ctx, slot_kf);
  if (!KF || !Scw || n_mp < 0 || !K || !n_matches || (KF->n > 0 && !matched_kp) ||
      (n_mp > 0 && (!valid || !Xw || !normal || !min_dist || !max_dist || !desc)))
    return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  *n_matches = 0;
  if (n_mp == 0 || KF->n == 0) return ASD_OK;
  float Rcw[9], tcw[3], Ow[3];
  decompose_sim3(Scw, Rcw, tcw);
  matcher_camera_centre(Rcw, 3, tcw, 1, Ow);
  std::vector<int> pred(n_mp, 0);
  SearchResult R;
  const int rc = query_search(ctx, m, *KF, n_mp, desc, nullptr, 3, &R, [&](int i, WinQuery& Q) {
    float u, v;
    if (!valid[i] || !sim3_project(ctx, *KF, Rcw, tcw, Ow, K, Xw + 3 * i, normal + 3 * i, min_dist[i], max_dist[i], false, &u, &v, &pred[i])) return;
    Q = WinQuery{u, v, (float)th * ctx->scale[pred[i]], -1, -1, i};
  });
  if (rc != ASD_OK) return rc;
  int nmatches = 0;
  for (int i = 0; i < n_mp; ++i) {
    if (R.cnt[i] == 0) continue;
    const Best b = best_of(R, i, 256, [&](int j) {
      if (matched_kp[j] != -1) return false;  // vpMatched[idx] already holds a map point
      const int lv = KF->kps[j].octave;
      return !(lv < pred[i] - 1 || lv > pred[i]);
    });
    if (b.dist <= TH_LOW) { matched_kp[b.idx] = i; nmatches++; }
  }
  *n_matches = nmatches;
  return ASD_OK;
}

// ORBmatcher::Fuse(KeyFrame*, cv::Mat Scw, const vector<MapPoint*>&, float th, vector<MapPoint*>& vpReplacePoint) (:963-1086)
int asd_fuse_search_sim3(asd_ctx* ctx, int32_t slot_kf, const float* Scw, int32_t n_mp, const uint8_t* valid, const float* Xw,
                         const float* normal, const float* min_dist, const float* max_dist, const float* desc, const float* K, float th,
                         int32_t* best_idx, float* best_dist) {
  AsdFrameSlot* KF = matcher_slot(ctx, slot_kf);
  if (!KF || !Scw || n_mp < 0 || !K || (n_mp > 0 && (!valid || !Xw || !normal || !min_dist || !max_dist || !desc || !best_idx || !best_dist)))
    return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  for (int i = 0; i < n_mp; ++i) { best_idx[i] = -1; best_dist[i] = 100.f; }
  if (n_mp == 0 || KF->n == 0) return ASD_OK;
  float Rcw[9], tcw[3], Ow[3];
  decompose_sim3(Scw, Rcw, tcw);
  matcher_camera_centre(Rcw, 3, tcw, 1, Ow);
  std::vector<int> pred(n_mp, 0);
  SearchResult R;
  const int rc = query_search(ctx, m, *KF, n_mp, desc, nullptr, 2, &R, [&](int i, WinQuery& Q) {
    float u, v;
    if (!valid[i] || !sim3_project(ctx, *KF, Rcw, tcw, Ow, K, Xw + 3 * i, normal + 3 * i, min_dist[i], max_dist[i], true, &u, &v, &pred[i])) return;
    Q = WinQuery{u, v, th * ctx->scale[pred[i]], -1, -1, i};
  });
  if (rc != ASD_OK) return rc;
  for (int i = 0; i < n_mp; ++i) {
    if (R.cnt[i] == 0) continue;
    const Best b = best_of(R, i, 100, [&](int j) { return !(KF->kps[j].octave < pred[i] - 1 || KF->kps[j].octave > pred[i]); });
    if (b.dist <= TH_LOW) { best_idx[i] = b.idx; best_dist[i] = b.dist; }
  }
  return ASD_OK;
}

// ORBmatcher::SearchBySim3 (:1090-1314)
int asd_match_sim3(asd_ctx* ctx, int32_t slot1, int32_t slot2, const uint8_t* has1, const uint8_t* has2, const float* Xw1, const float* Xw2,
                   const float* min_dist1, const float* max_dist1, const float* min_dist2, const float* max_dist2, const float* desc1,
                   const float* desc2, const float* T1w, const float* T2w, float s12, const float* R12, const float* t12, const float* K,
                   float th, int32_t* match12, int32_t* n_matches) {
  AsdFrameSlot *KF1 = matcher_slot(ctx, slot1), *KF2 = matcher_slot(ctx, slot2);
  if (!KF1 || !KF2 || !T1w || !T2w || !R12 || !t12 || !K || !n_matches || (KF1->n > 0 && (!has1 || !Xw1 || !min_dist1 || !max_dist1 || !desc1 || !match12)) ||
      (KF2->n > 0 && (!has2 || !Xw2 || !min_dist2 || !max_dist2 || !desc2)))
    return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  *n_matches = 0;
  std::fill(match12, match12 + KF1->n, -1);
  if (KF1->n == 0 || KF2->n == 0) return ASD_OK;
  float R1w[9], t1w[3], R2w[9], t2w[3], sR12[9], sR21[9], t21[3];
  split_pose(T1w, R1w, t1w);
  split_pose(T2w, R2w, t2w);
  const float a12 = (float)(double)s12, a21 = (float)(1.0 / (double)s12);  // scaled Mat = convertTo with a float scale
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) { sR12[r * 3 + c] = R12[r * 3 + c] * a12 + 0.0f; sR21[r * 3 + c] = R12[c * 3 + r] * a21 + 0.0f; }
  for (int r = 0; r < 3; ++r) {
    const float t0 = sR21[r * 3 + 0] * t12[0] + sR21[r * 3 + 1] * t12[1] + sR21[r * 3 + 2] * t12[2];
    t21[r] = (float)((double)t0 * -1.0);
  }
  auto one_way = [&](AsdFrameSlot& A, AsdFrameSlot& B, const uint8_t* has, const float* Xw, const float* mind, const float* maxd,
                     const float* desc, const float* Raw, const float* taw, const float* sRba, const float* tba, std::vector<int>& out) -> int {
    std::vector<int> pred(A.n, 0);
    SearchResult R;
    const int rc = query_search(ctx, m, B, A.n, desc, nullptr, 3, &R, [&](int i, WinQuery& Q) {
      if (!has[i]) return;
      float pA[3], pB[3];
      rot_add(Raw, taw, Xw + 3 * i, pA);
      rot_add(sRba, tba, pA, pB);
      if (pB[2] < 0.0) return;
      const float invz = 1.0 / pB[2];
      const float u = K[0] * (pB[0] * invz) + K[2], v = K[1] * (pB[1] * invz) + K[3];
      if (!(u >= B.min_x && u < B.max_x && v >= B.min_y && v < B.max_y)) return;
      const float dist3D = norm3f(pB);
      if (dist3D < 0.8f * mind[i] || dist3D > 1.2f * maxd[i]) return;
      pred[i] = predict_scale(ctx, maxd[i], dist3D);
      Q = WinQuery{u, v, th * ctx->scale[pred[i]], -1, -1, i};
    });
    if (rc != ASD_OK) return rc;
    out.assign(A.n, -1);
    for (int i = 0; i < A.n; ++i) {
      if (R.cnt[i] == 0) continue;
      const Best b = best_of(R, i, 100, [&](int j) { return !(B.kps[j].octave < pred[i] - 1 || B.kps[j].octave > pred[i]); });
      if (b.dist <= TH_HIGH) out[i] = b.idx;
    }
    return ASD_OK;
  };
  std::vector<int> m1, m2;
  int rc = one_way(*KF1, *KF2, has1, Xw1, min_dist1, max_dist1, desc1, R1w, t1w, sR21, t21, m1);
  if (rc != ASD_OK) return rc;
  if ((rc = one_way(*KF2, *KF1, has2, Xw2, min_dist2, max_dist2, desc2, R2w, t2w, sR12, t12, m2)) != ASD_OK) return rc;
  int found = 0;
  for (int i1 = 0; i1 < KF1->n; ++i1) {
    const int i2 = m1[i1];
    if (i2 >= 0 && m2[i2] == i1) { match12[i1] = i2; ++found; }
  }
  *n_matches = found;
  return ASD_OK;
}

// ---- BoW-guided searches: matcher_list_search's lists, three replays ------------------------------------------------

int asd_match_bow(asd_ctx* ctx, int32_t slot_kf, int32_t slot_f, const asd_feature_vector* fv_kf,
                  const asd_feature_vector* fv_f, const uint8_t* has_mp_kf, float nn_ratio, int32_t check_orientation,
                  int32_t* match_f, int32_t* n_matches) {
  AsdFrameSlot *KF = matcher_slot(ctx, slot_kf), *F = matcher_slot(ctx, slot_f);
  if (!KF || !F || !has_mp_kf || !match_f || !n_matches || !fv_valid(fv_kf, KF->n) || !fv_valid(fv_f, F->n)) return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  std::fill(match_f, match_f + F->n, -1);
  *n_matches = 0;
  std::vector<ListQuery> lq;
  const float* dist = nullptr;
  int rc = matcher_list_search(ctx, m, *KF, *F, fv_kf, fv_f, has_mp_kf, /*skip_if_set=*/false, lq, &dist);
  if (rc != ASD_OK) return rc;
  int nmatches = 0;
  RotHist hist;
  for (const ListQuery& Q : lq) {  // reference order: node by node, KF keypoints of the node in order (:194-262)
    const Best b = best_of(fv_f->idx + Q.cbeg, dist + Q.ooff, Q.cend - Q.cbeg, 256, [&](int j) { return match_f[j] < 0; });
    if (b.dist <= TH_LOW && b.dist < nn_ratio * b.dist2) {
      match_f[b.idx] = Q.qrow;
      if (check_orientation) hist.add(rot_bin(KF->kps[Q.qrow].angle, F->kps[b.idx].angle), b.idx);
      nmatches++;
    }
  }
  if (check_orientation) hist.prune([&](int j) { match_f[j] = -1; nmatches--; });
  *n_matches = nmatches;
  return ASD_OK;
}

// SearchByBoW(KeyFrame*, KeyFrame*, ...) (ORBmatcher.cc:533-666): the same list search, another replay.  A candidate of keyframe 2
// needs a map point and must not have been taken (vbMatched2, :587), the claim is on keyframe 2's index, the threshold is strict
// (:609) and the histogram holds idx1 (:625).
int asd_match_bow_kf(asd_ctx* ctx, int32_t slot1, int32_t slot2, const asd_feature_vector* fv1, const asd_feature_vector* fv2,
                     const uint8_t* has_mp1, const uint8_t* has_mp2, float nn_ratio, int32_t check_orientation,
                     int32_t* match12, int32_t* n_matches) {
  AsdFrameSlot *K1 = matcher_slot(ctx, slot1), *K2 = matcher_slot(ctx, slot2);
  if (!K1 || !K2 || !has_mp1 || !has_mp2 || !match12 || !n_matches || !fv_valid(fv1, K1->n) || !fv_valid(fv2, K2->n)) return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  std::fill(match12, match12 + K1->n, -1);
  *n_matches = 0;
  std::vector<ListQuery> lq;
  const float* dist = nullptr;
  int rc = matcher_list_search(ctx, m, *K1, *K2, fv1, fv2, has_mp1, /*skip_if_set=*/false, lq, &dist);
  if (rc != ASD_OK) return rc;
  int nmatches = 0;
  std::vector<uint8_t> matched2((size_t)K2->n, 0);
  RotHist hist;
  for (const ListQuery& Q : lq) {  // reference order: node by node, keyframe 1's keypoints of the node in order (:561-634)
    const Best b = best_of(fv2->idx + Q.cbeg, dist + Q.ooff, Q.cend - Q.cbeg, 256, [&](int j) { return !matched2[j] && has_mp2[j]; });
    if (b.dist < TH_LOW && b.dist < nn_ratio * b.dist2) {
      match12[Q.qrow] = b.idx;
      matched2[b.idx] = 1;
      if (check_orientation) hist.add(rot_bin(K1->kps[Q.qrow].angle, K2->kps[b.idx].angle), Q.qrow);
      nmatches++;
    }
  }
  if (check_orientation) hist.prune([&](int i1) { match12[i1] = -1; nmatches--; });
  *n_matches = nmatches;
  return ASD_OK;
}

int asd_match_triangulate(asd_ctx* ctx, int32_t slot1, int32_t slot2, const asd_feature_vector* fv1,
                          const asd_feature_vector* fv2, const uint8_t* has_mp1, const uint8_t* has_mp2, const float* F12,
                          float ex, float ey, int32_t check_orientation, int32_t* matches12, int32_t* n_matches) {
  AsdFrameSlot *K1 = matcher_slot(ctx, slot1), *K2 = matcher_slot(ctx, slot2);
  if (!K1 || !K2 || !has_mp1 || !has_mp2 || !F12 || !matches12 || !n_matches || !fv_valid(fv1, K1->n) || !fv_valid(fv2, K2->n))
    return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  std::fill(matches12, matches12 + K1->n, -1);
  *n_matches = 0;
  std::vector<ListQuery> lq;
  const float* dist = nullptr;
  int rc = matcher_list_search(ctx, m, *K1, *K2, fv1, fv2, has_mp1, /*skip_if_set=*/true, lq, &dist);
  if (rc != ASD_OK) return rc;
  int nmatches = 0;
  RotHist hist;
  for (const ListQuery& Q : lq) {
    const asd_keypoint& kp1 = K1->kps[Q.qrow];
    // epipolar line of kp1 in image 2 (CheckDistEpipolarLine, ORBmatcher.cc:136-153)
    const float la = kp1.x * F12[0] + kp1.y * F12[3] + F12[6];
    const float lb = kp1.x * F12[1] + kp1.y * F12[4] + F12[7];
    const float lc = kp1.x * F12[2] + kp1.y * F12[5] + F12[8];
    const float den = la * la + lb * lb;
    float best = TH_LOW;
    int best_idx = -1;
    for (int t = Q.cbeg; t < Q.cend; ++t) {
      const int idx2 = fv2->idx[t];
      if (has_mp2[idx2]) continue;  // vbMatched2 is never set by the reference (:688, :729)
      const float d = dist[Q.ooff + (t - Q.cbeg)];
      if (d > TH_LOW || d > best) continue;
      const asd_keypoint& kp2 = K2->kps[idx2];
      const float dex = ex - kp2.x, dey = ey - kp2.y;
      if (dex * dex + dey * dey < 100 * ctx->scale[kp2.octave]) continue;
      const float num = la * kp2.x + lb * kp2.y + lc;
      if (den == 0) continue;
      const float dsqr = num * num / den;
      if (dsqr < 3.84 * ctx->sigma2[kp2.octave]) { best_idx = idx2; best = d; }
    }
    if (best_idx >= 0) {
      matches12[Q.qrow] = best_idx;
      nmatches++;
      if (check_orientation) hist.add(rot_bin(kp1.angle, K2->kps[best_idx].angle), Q.qrow);
    }
  }
  if (check_orientation) hist.prune([&](int i1) { matches12[i1] = -1; nmatches--; });
  *n_matches = nmatches;
  return ASD_OK;
}

int asd_frustum(asd_ctx* ctx, int32_t slot_cur, int32_t n, const float* Xw, const float* normal, const float* min_dist,
                const float* max_dist, const float* Tcw, const float* K, float cos_limit, uint8_t* in_view,
                float* proj, int32_t* level, float* view_cos) {
  AsdFrameSlot* F = matcher_slot(ctx, slot_cur);
  if (!F || n < 0 || !Tcw || !K || (n > 0 && (!Xw || !normal || !min_dist || !max_dist || !in_view || !proj || !level || !view_cos)))
    return ASD_ERR_INVALID;
  const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  float Ow[3];
  matcher_camera_centre(Tcw, 4, Tcw + 3, 4, Ow);
  for (int q = 0; q < n; ++q) {
    in_view[q] = 0; proj[2 * q] = proj[2 * q + 1] = 0.f; level[q] = 0; view_cos[q] = 0.f;
    const float* P = Xw + 3 * q;
    float Pc[3];
    matcher_transform(Tcw, P, Pc);
    if (Pc[2] < 0.0f) continue;
    const float invz = 1.0f / Pc[2];
    const float u = fx * Pc[0] * invz + cx, v = fy * Pc[1] * invz + cy;
    if (u < F->min_x || u > F->max_x || v < F->min_y || v > F->max_y) continue;
    const float maxD = 1.2f * max_dist[q], minD = 0.8f * min_dist[q];  // MapPoint.cc:409-419
    const float PO[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
    const double nn = (double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2];
    const float dist = (float)std::sqrt(nn);
    if (dist < minD || dist > maxD) continue;
    const float* Pn = normal + 3 * q;
    const double dot = (double)PO[0] * Pn[0] + (double)PO[1] * Pn[1] + (double)PO[2] * Pn[2];
    const float vc = (float)(dot / dist);
    if (vc < cos_limit) continue;
    in_view[q] = 1;
    proj[2 * q] = u; proj[2 * q + 1] = v;
    level[q] = predict_scale(ctx, max_dist[q], dist);
    view_cos[q] = vc;
  }
  return ASD_OK;
}

int asd_match_init(asd_ctx* ctx, int32_t slot1, int32_t slot2, float* prev_matched, int32_t window, float nn_ratio,
                   int32_t check_orientation, int32_t* matches12, int32_t* n_matches) {
  AsdFrameSlot *F1 = matcher_slot(ctx, slot1), *F2 = matcher_slot(ctx, slot2);
  if (!F1 || !F2 || !prev_matched || !matches12 || !n_matches) return ASD_ERR_INVALID;
  (void)hipSetDevice(ctx->cfg.device);
  MatcherState* m = matcher_state(ctx);
  std::fill(matches12, matches12 + F1->n, -1);
  *n_matches = 0;
  if (F1->n == 0 || F2->n == 0) return ASD_OK;
  SearchResult R;
  const int rc = query_search(ctx, m, *F2, F1->n, nullptr, F1->d_desc, 3, &R, [&](int i1, WinQuery& Q) {  // query descriptors: frame 1's, resident
    if (F1->kps[i1].octave > 0) return;  // :434-436
    Q = WinQuery{prev_matched[2 * i1], prev_matched[2 * i1 + 1], (float)window, 0, 0, i1};
  });
  if (rc != ASD_OK) return rc;
  std::vector<float> matched_dist(F2->n, 100.f);
  std::vector<int> matches21(F2->n, -1);
  RotHist hist;
  int nmatches = 0;
  for (int i1 = 0; i1 < F1->n; ++i1) {
    if (R.cnt[i1] == 0) continue;
    float best = 100.f, best2 = 100.f;
    int best_idx = -1;
    for (int t = R.off[i1]; t < R.off[i1] + R.cnt[i1]; ++t) {
      const int i2 = R.idx[t];
      const float d = R.dist[t];
      if (matched_dist[i2] <= d) continue;
      if (d < best) { best2 = best; best = d; best_idx = i2; }
      else if (d < best2) best2 = d;
    }
    if (best <= TH_LOW && best < best2 * nn_ratio) {
      if (matches21[best_idx] >= 0) { matches12[matches21[best_idx]] = -1; nmatches--; }
      matches12[i1] = best_idx;
      matches21[best_idx] = i1;
      matched_dist[best_idx] = best;
      nmatches++;
      if (check_orientation) hist.add(rot_bin(F1->kps[i1].angle, F2->kps[best_idx].angle), i1);
    }
  }
  if (check_orientation)
    hist.prune([&](int idx1) { if (matches12[idx1] >= 0) { matches12[idx1] = -1; nmatches--; } });
  for (int i1 = 0; i1 < F1->n; ++i1)
    if (matches12[i1] >= 0) {
      prev_matched[2 * i1] = F2->kps[matches12[i1]].x;
      prev_matched[2 * i1 + 1] = F2->kps[matches12[i1]].y;
    }
  *n_matches = nmatches;
  return ASD_OK;
}

}  // extern "C"
