// test_fuse_apply.cpp -- probe for asd::LocalMapping::SearchInNeighbors, asd::ORBmatcher::Fuse (search + apply), asd::LoopClosing::SearchAndFuse
// and asd::LoopClosing::FuseMatchedPoints (asd_adapters.hpp) over frames in the context's slots and the context's observation table;
// tests/test_fuse_apply_host.py writes the problem and reads the output.
//
//   test_fuse_apply PROBLEM_FILE
//     The file (binary, little-endian, i = int32, f = float32): i nKF, i nPoints, f K[4]; per keyframe i mnId, i nKeys, f Tcw[16],
//     asd_keypoint[nKeys], f desc[nKeys][128], i row[nKeys]; per point (bank rows 0 .. nPoints-1) f Xw[3], normal[3], min, max; f
//     desc[nPoints][128]; f desc2[nPoints][128] (the descriptor a point takes when onReplaced names it); i nBad, i bad[nBad];
//     i currentKF, i nTargets, i targets[]; i loopKF, i nLoopKFs, i loopKFs[]; i matchedKF, i n, i matched[n].
//     The three steps run in that order on one table: SearchInNeighbors; SearchAndFuse of loopKF with Scw = its Tcw and
//     mvpLoopMapPoints = asd_map_points(loopKFs); FuseMatchedPoints.
//     Prints JSON: neighbors {rc, matches, candidates, targets [outcome], current outcome}, on_replaced [{rows}], loop_points,
//     search_and_fuse outcome, fuse_matched outcome, rows [[mnId, {row}]]; outcome = {rc, best_idx, action, other, obs_cand, obs_other,
//     n_moved, n_dropped, n_fused, winners}.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "asd_adapters.hpp"

namespace {

template <typename T>
bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
bool read_int(FILE* f, int32_t* v) { return fread(v, 4, 1, f) == 1; }

void print_ints(const char* name, const std::vector<int32_t>& v, bool last = false) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? ", " : "", v[i]);
  printf("]%s", last ? "" : ", ");
}

void print_outcome(const asd::FuseOutcome& R) {
  printf("{\"rc\": %d, ", R.rc);
  print_ints("best_idx", R.bestIdx);
  print_ints("action", std::vector<int32_t>(R.action.begin(), R.action.end()));
  print_ints("other", R.other);
  print_ints("obs_cand", R.obsCand);
  print_ints("obs_other", R.obsOther);
  print_ints("n_moved", R.nMoved);
  print_ints("n_dropped", R.nDropped);
  printf("\"n_fused\": %d, ", R.nFused);
  print_ints("winners", R.winners, true);
  printf("}");
}

// the caller's map as SearchInNeighbors reads it
struct View {
  std::map<int32_t, asd::FrameView> kfs;
  std::vector<float> attr, desc, desc2;   // [nPoints][8], [nPoints][128] twice
  std::vector<uint8_t> refreshed;         // onReplaced named the point: it reads desc2 from then on
  const asd::FrameView& KF(int32_t id) const { return kfs.at(id); }
  asd::MapPointView MP(int32_t row) const {
    asd::MapPointView p{};
    const float* a = attr.data() + 8 * (size_t)row;
    for (int k = 0; k < 3; ++k) { p.Xw[k] = a[k]; p.normal[k] = a[3 + k]; }
    p.mfMinDistance = a[6]; p.mfMaxDistance = a[7];
    p.descriptor = (refreshed[row] ? desc2.data() : desc.data()) + (size_t)ASD_DESC_DIM * row;
    return p;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s PROBLEM_FILE\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  try {
    asd::Context ctx(2000, 1.2f, 8, 20, 7, 1241, 376);
    int32_t nKF = 0, nPoints = 0;
    float Kv[4];
    if (!read_int(f, &nKF) || !read_int(f, &nPoints) || fread(Kv, 4, 4, f) != 4) return 2;
    const asd::Camera K{Kv[0], Kv[1], Kv[2], Kv[3]};
    View view;
    std::vector<int32_t> ids(nKF);
    for (int k = 0; k < nKF; ++k) {
      int32_t nKeys = 0;
      if (!read_int(f, &ids[k]) || !read_int(f, &nKeys)) return 2;
      asd::FrameView& F = view.kfs[ids[k]];
      F.slot = k;
      F.mnMinX = 0; F.mnMaxX = 1241; F.mnMinY = 0; F.mnMaxY = 376;
      std::vector<int32_t> row;
      if (fread(F.mTcw, 4, 16, f) != 16 || !read_vec(f, F.mvKeysUn, nKeys) || !read_vec(f, F.mDescriptors, (size_t)nKeys * ASD_DESC_DIM) || !read_vec(f, row, nKeys)) return 2;
      if (asd_frame_set(ctx.get(), F.slot, F.mvKeysUn.data(), F.mDescriptors.data(), nKeys, F.mnMinX, F.mnMaxX, F.mnMinY, F.mnMaxY) != ASD_OK ||
          asd_map_put(ctx.get(), ids[k], nKeys, row.data()) != ASD_OK) {
        fprintf(stderr, "asd_frame_set / asd_map_put: %s\n", ctx.error());
        return 3;
      }
    }
    if (!read_vec(f, view.attr, (size_t)nPoints * 8) || !read_vec(f, view.desc, (size_t)nPoints * ASD_DESC_DIM) ||
        !read_vec(f, view.desc2, (size_t)nPoints * ASD_DESC_DIM))
      return 2;
    view.refreshed.assign(nPoints, 0);
    int32_t nBad = 0;
    std::vector<int32_t> bad;
    if (!read_int(f, &nBad) || !read_vec(f, bad, nBad)) return 2;
    if (asd_map_point_bad(ctx.get(), nBad, bad.data(), 1) != ASD_OK) { fprintf(stderr, "asd_map_point_bad: %s\n", ctx.error()); return 3; }

    std::vector<std::vector<int32_t>> replaced;
    auto onReplaced = [&](const std::vector<int32_t>& winners) {
      replaced.push_back(winners);
      for (const int32_t r : winners) view.refreshed[r] = 1;
    };

    int32_t cur = 0, nTargets = 0;
    std::vector<int32_t> targets;
    if (!read_int(f, &cur) || !read_int(f, &nTargets) || !read_vec(f, targets, nTargets)) return 2;
    const asd::LocalMapping::Neighbors N = asd::LocalMapping::SearchInNeighbors(ctx, cur, targets, view, onReplaced, K);
    if (N.rc != ASD_OK) fprintf(stderr, "SearchInNeighbors: %s\n", ctx.error());
    printf("{\"neighbors\": {\"rc\": %d, ", N.rc);
    print_ints("matches", N.vpMapPointMatches);
    print_ints("candidates", N.vpFuseCandidates);
    printf("\"targets\": [");
    for (size_t i = 0; i < N.perTarget.size(); ++i) { if (i) printf(", "); print_outcome(N.perTarget[i]); }
    printf("], \"current\": ");
    print_outcome(N.intoCurrent);
    printf("}, \"on_replaced\": [");
    for (size_t i = 0; i < replaced.size(); ++i) { printf("%s{", i ? ", " : ""); print_ints("rows", replaced[i], true); printf("}"); }

    int32_t loopKF = 0, nLoopKFs = 0;
    std::vector<int32_t> loopKFs, loopPoints;
    if (!read_int(f, &loopKF) || !read_int(f, &nLoopKFs) || !read_vec(f, loopKFs, nLoopKFs)) return 2;
    if (asd::GetMapPointsOf(ctx, loopKFs, loopPoints) != ASD_OK) { fprintf(stderr, "asd_map_points: %s\n", ctx.error()); return 3; }
    std::vector<asd::MapPointView> loopViews;
    for (const int32_t r : loopPoints) loopViews.push_back(view.MP(r));
    const asd::FrameView& L = view.KF(loopKF);
    const asd::FuseOutcome S = asd::LoopClosing::SearchAndFuse(ctx, loopKF, L, L.mTcw, loopViews, loopPoints, K);
    if (S.rc != ASD_OK) fprintf(stderr, "SearchAndFuse: %s\n", ctx.error());
    printf("], ");
    print_ints("loop_points", loopPoints);
    printf("\"search_and_fuse\": ");
    print_outcome(S);

    int32_t matchedKF = 0, nMatched = 0;
    std::vector<int32_t> matched;
    if (!read_int(f, &matchedKF) || !read_int(f, &nMatched) || !read_vec(f, matched, nMatched)) return 2;
    const asd::FuseOutcome M = asd::LoopClosing::FuseMatchedPoints(ctx, matchedKF, matched);
    if (M.rc != ASD_OK) fprintf(stderr, "FuseMatchedPoints: %s\n", ctx.error());
    printf(", \"fuse_matched\": ");
    print_outcome(M);

    printf(", \"rows\": [");
    for (int k = 0; k < nKF; ++k) {
      std::vector<int32_t> row;
      if (asd::GetMapPointMatches(ctx, ids[k], row) != ASD_OK) { fprintf(stderr, "asd_map_get: %s\n", ctx.error()); return 3; }
      printf("%s[%d, {", k ? ", " : "", ids[k]);
      print_ints("row", row, true);
      printf("}]");
    }
    printf("]}\n");
    fclose(f);
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
