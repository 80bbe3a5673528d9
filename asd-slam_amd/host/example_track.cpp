// example_track.cpp -- two-frame tracking with the host-side mirror classes (asd_adapters.hpp):
// what Tracking::GrabImageMonocular + TrackWithMotionModel do with the hot path (Tracking.cc:102-110,
// 664-723), minus the map.  Usage: example_track weights.bin frame0.raw frame1.raw W H
// weights.bin = 7 x (conv_w, bn_mean, bn_var) f32 blobs in ASDNet.py:334-356 order.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <utility>
#include <vector>

#include "asd_adapters.hpp"

static std::vector<uint8_t> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc < 6) { fprintf(stderr, "usage: %s weights.bin frame0.raw frame1.raw W H\n", argv[0]); return 2; }
  const int W = atoi(argv[4]), H = atoi(argv[5]);
  const int cout_[7] = {32, 32, 64, 64, 128, 128, 128}, cin_[7] = {1, 32, 32, 64, 64, 128, 128}, k_[7] = {3, 3, 3, 3, 3, 3, 8};
  std::vector<uint8_t> wb = slurp(argv[1]);
  const float* p = reinterpret_cast<const float*>(wb.data());
  const float *cw[7], *bm[7], *bv[7];
  for (int l = 0; l < 7; ++l) {
    cw[l] = p; p += (size_t)cout_[l] * cin_[l] * k_[l] * k_[l];
    bm[l] = p; p += cout_[l];
    bv[l] = p; p += cout_[l];
  }
  if ((const uint8_t*)p != wb.data() + wb.size()) { fprintf(stderr, "weights.bin has the wrong size\n"); return 2; }
  try {
    asd::Context ctx(2000, 1.2f, 8, 20, 7, W, H);
    asd::ORBextractor extractor(ctx, cw, bm, bv);
    const asd::Camera K{718.856f, 718.856f, 607.1928f, 185.2157f};
    asd::FrameView F[2];
    for (int t = 0; t < 2; ++t) {
      std::vector<uint8_t> img = slurp(argv[2 + t]);
      if ((int)img.size() != W * H) { fprintf(stderr, "frame %d has the wrong size\n", t); return 2; }
      F[t].slot = t;
      F[t].mnMinX = 0; F[t].mnMaxX = (float)W; F[t].mnMinY = 0; F[t].mnMaxY = (float)H;
      if (extractor.ExtractDesc(img.data(), W, H, W, F[t].mvKeysUn, F[t].mDescriptors) < 0) { fprintf(stderr, "%s\n", ctx.error()); return 1; }
      if (asd::FrameAssignFeaturesToGrid(ctx, F[t]) != ASD_OK) { fprintf(stderr, "%s\n", ctx.error()); return 1; }
    }
    // every keypoint of frame 0 carries a map point 20 m in front of the camera (planar stand-in for the map)
    std::vector<asd::MapPointView> mps(F[0].N());
    std::vector<const asd::MapPointView*> pmp(F[0].N());
    F[0].mvpMapPoints.resize(F[0].N());
    for (int i = 0; i < F[0].N(); ++i) {
      const float z = 20.f, u = (F[0].mvKeysUn[i].x - 620.5f) * 1.003f + 620.5f - 3.009f, v = (F[0].mvKeysUn[i].y - 188.f) * 1.003f + 188.f - 0.2006f;
      mps[i].Xw[0] = (u - K.cx) / K.fx * z; mps[i].Xw[1] = (v - K.cy) / K.fy * z; mps[i].Xw[2] = z;
      mps[i].normal[0] = 0; mps[i].normal[1] = 0; mps[i].normal[2] = 1;
      mps[i].mfMinDistance = 1; mps[i].mfMaxDistance = 200;
      mps[i].descriptor = &F[0].mDescriptors[(size_t)i * ASD_DESC_DIM];
      pmp[i] = &mps[i];
      F[0].mvpMapPoints[i] = i;
    }
    asd::ORBmatcher matcher(ctx, 0.8f, true);                                   // Tracking.cc:666
    const int nmatches = matcher.SearchByProjection(F[1], F[0], pmp, K, 15.f);  // Tracking.cc:679
    std::vector<const asd::MapPointView*> cur_pts(F[1].N(), nullptr);
    for (int j = 0; j < F[1].N(); ++j) if (F[1].mvpMapPoints[j] >= 0) cur_pts[j] = &mps[F[1].mvpMapPoints[j]];
    const int ninl = asd::Optimizer::PoseOptimization(ctx, &F[1], cur_pts, K, extractor.GetInverseScaleSigmaSquares());  // :693
    // the same stage as ONE submission (asd::Tracking::TrackWithMotionModel = asd_track_motion_model): same matches, same pose bits
    int chain_ok = 0;
    {
      asd::FrameView G = F[1];
      G.mvpMapPoints.clear(); G.mvbOutlier.clear();
      for (int k = 0; k < 16; ++k) G.mTcw[k] = (k % 5 == 0) ? 1.f : 0.f;      // the pose the separate calls started from
      int nm2 = 0, ninl2 = 0;
      const bool ok = asd::Tracking::TrackWithMotionModel(ctx, G, F[0], pmp, K, true, &nm2, &ninl2);
      bool same = ok && nm2 == nmatches && ninl2 == ninl;
      for (int k = 0; k < 16 && same; ++k) same = G.mTcw[k] == F[1].mTcw[k];
      for (int j = 0; j < G.N() && same; ++j)   // the frame keeps its inlier matches (Tracking.cc:704-719)
        same = G.mvpMapPoints[j] == (F[1].mvbOutlier[j] ? -1 : F[1].mvpMapPoints[j]);
      chain_ok = same;
      // ... and TrackLocalMap's body on the points the frame did not take, with LocalBundleAdjustment running on its lane meanwhile
      std::vector<asd::MapPointView> local;
      std::vector<int32_t> ids;
      std::vector<uint8_t> taken(mps.size(), 0);
      std::vector<const asd::MapPointView*> curp(G.N(), nullptr);
      for (int j = 0; j < G.N(); ++j) if (G.mvpMapPoints[j] >= 0) { taken[G.mvpMapPoints[j]] = 1; curp[j] = &mps[G.mvpMapPoints[j]]; }
      for (size_t i = 0; i < mps.size(); ++i) if (!taken[i]) { local.push_back(mps[i]); ids.push_back((int32_t)i); }
      // a small bundle: two keyframes (the first fixed) observing the frame's inlier points
      std::vector<double> poses = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0}, pts, eobs, einfo;
      std::vector<uint8_t> fixed = {1, 0};
      std::vector<int32_t> ept, eps;
      asd_tcw_to_pose7(G.mTcw, &poses[7]);
      for (int j = 0; j < G.N() && pts.size() < 3 * 400; ++j)
        if (curp[j]) {
          const int m = G.mvpMapPoints[j], pid = (int)pts.size() / 3;
          int j0 = -1;
          for (int q = 0; q < F[0].N(); ++q) if (F[0].mvpMapPoints[q] == m) { j0 = q; break; }
          if (j0 < 0) continue;
          for (int k = 0; k < 3; ++k) pts.push_back(mps[m].Xw[k]);
          ept.push_back(pid); eps.push_back(0); eobs.push_back(F[0].mvKeysUn[j0].x); eobs.push_back(F[0].mvKeysUn[j0].y); einfo.push_back(1.0);
          ept.push_back(pid); eps.push_back(1); eobs.push_back(G.mvKeysUn[j].x); eobs.push_back(G.mvKeysUn[j].y); einfo.push_back(1.0);
        }
      asd_ba_problem pr{};
      pr.n_poses = 2; pr.n_points = (int32_t)pts.size() / 3; pr.n_edges = (int32_t)ept.size();
      pr.poses = poses.data(); pr.fixed = fixed.data(); pr.points = pts.data(); pr.e_point = ept.data(); pr.e_pose = eps.data();
      pr.e_obs = eobs.data(); pr.e_info = einfo.data(); pr.K[0] = K.fx; pr.K[1] = K.fy; pr.K[2] = K.cx; pr.K[3] = K.cy; pr.its_first = 5; pr.its_second = 10;
      std::vector<double> chi2(ept.size()); std::vector<uint8_t> dpos(ept.size()), out1(ept.size());
      asd_ba_result rs{};
      rs.edge_chi2 = chi2.data(); rs.edge_depth_pos = dpos.data(); rs.edge_outlier1 = out1.data();
      const bool ba_sub = pr.n_points >= 10 && asd::LocalMapping::LocalBundleAdjustmentSubmit(ctx, &pr, &rs) == ASD_OK;
      const int ninl3 = asd::Tracking::TrackLocalMap(ctx, G, local, ids, curp, K);
      const bool ba_ok = ba_sub && asd::LocalMapping::LocalBundleAdjustmentWait(ctx) == ASD_OK && rs.iters_second > 0;
      printf("chain: same=%d local-map inliers=%d lane BA ok=%d (%d points, chi2 %.3f)\n", (int)same, ninl3, (int)ba_ok, pr.n_points, rs.chi2_second);
      chain_ok = chain_ok && ninl3 > 50 && ba_ok;
    }
    // what LocalMapping::SearchInNeighbors does with the same points once frame 1 became a keyframe (LocalMapping.cc:557-636)
    asd::ORBmatcher fuser(ctx);
    std::vector<int32_t> bestIdx;
    const int nfused = fuser.Fuse(F[1], mps, std::vector<uint8_t>(mps.size(), 1), K, bestIdx);
    // Frame::ComputeBoW + SearchByBoW(KeyFrame*, Frame&, ...) (Tracking::TrackReferenceKeyFrame, Tracking.cc:607-620) with a
    // small random vocabulary standing in for the missing vocabulary file: k = 8, L = 2, node ids breadth-first
    int nbow = 0;
    bool loop_ok = false;
    {
      const int k = 8, L = 2, n_nodes = 1 + k + k * k;
      std::vector<int32_t> start(n_nodes + 1, 0), kids, word(n_nodes, -1);
      std::vector<double> weight(n_nodes, 0.0);
      std::vector<float> d((size_t)n_nodes * 128, 0.f);
      for (int i = 0; i < n_nodes; ++i) {
        if (i < 1 + k) for (int c = 0; c < k; ++c) kids.push_back(1 + i * k + c);
        start[i + 1] = (int32_t)kids.size();
      }
      uint32_t seed = 12345u;
      for (int i = 1; i < n_nodes; ++i) {
        if (i > k) { word[i] = i - 1 - k; weight[i] = 1.0 + (i % 7); }
        // children scatter around a real descriptor of frame 0 so that the words are populated
        const float* base = &F[0].mDescriptors[(size_t)((i * 37) % F[0].N()) * ASD_DESC_DIM];
        for (int q = 0; q < 128; ++q) { seed = seed * 1664525u + 1013904223u; d[(size_t)i * 128 + q] = base[q] + ((seed >> 8) & 0xffff) * (0.2f / 65536.f) - 0.1f; }
      }
      if (asd_voc_load(ctx.get(), n_nodes, k, L, 0, 0, start.data(), kids.data(), weight.data(), word.data(), d.data()) != ASD_OK) { fprintf(stderr, "%s\n", ctx.error()); return 1; }
      std::vector<std::pair<int32_t, double>> bow0, bow1;
      asd::ORBmatcher::FeatVec fv0, fv1;
      if (asd::ComputeBoW(ctx, F[0], bow0, fv0, 1) != ASD_OK || asd::ComputeBoW(ctx, F[1], bow1, fv1, 1) != ASD_OK) { fprintf(stderr, "%s\n", ctx.error()); return 1; }
      asd::ORBmatcher bowmatcher(ctx, 0.7f, true);                               // Tracking.cc:616
      std::vector<int32_t> vpMapPointMatches;
      nbow = bowmatcher.SearchByBoW(F[0], fv0, F[1], fv1, vpMapPointMatches);
      // LoopClosing::ComputeSim3 for one candidate (LoopClosing.cc:304-375, :415) with frame 1 as the current keyframe and frame 0 as
      // the loop candidate: SearchByBoW(KF, KF), the caller's Sim3 (here the known relative pose instead of Sim3Solver's RANSAC),
      // SearchBySim3, OptimizeSim3 and SearchByProjection(KF, Scw) -- every step but the solver behind the C ABI
      std::vector<int32_t> loop_ids(mps.size()), vpCurrentMatchedPoints;
      for (size_t i = 0; i < mps.size(); ++i) loop_ids[i] = (int32_t)i;
      const float* T1 = F[1].mTcw;   // frame 0 sits at the origin: S12 = (R1w, t1w, 1)
      auto solver = [&](const std::vector<int32_t>&, const std::vector<int32_t>&, float* s12, float* R12, float* t12) {
        *s12 = 1.f;
        for (int r = 0; r < 3; ++r) { for (int q = 0; q < 3; ++q) R12[r * 3 + q] = T1[r * 4 + q]; t12[r] = T1[r * 4 + 3]; }
        return true;
      };
      const asd::LoopClosing::Result lc = asd::LoopClosing::ComputeSim3Candidate(ctx, F[1], fv1, F[0], fv0, mps, loop_ids, K, extractor.GetInverseScaleSigmaSquares(),
                                                                                  false, solver, vpCurrentMatchedPoints);
      printf("loop: bow=%d sim3=%d inliers=%d total=%d match=%d scale=%.6f\n", lc.nBoW, lc.nSim3, lc.nInliers, lc.nTotalMatches, (int)lc.bMatch, lc.g2oScm[7]);
      loop_ok = lc.bMatch && lc.nInliers >= 20;   // LoopClosing.cc:364
      // the same over the candidate list with asd::Sim3Solver's RANSAC on the device (LoopClosing.cc:291-377): informative only,
      // the exit status does not depend on it
      {
        std::srand(1);
        asd::DrawStream draws;   // ::rand
        std::vector<int32_t> matched;
        const std::vector<const asd::FrameView*> cands = {&F[0]};
        const std::vector<const asd::ORBmatcher::FeatVec*> cand_fv = {&fv0};
        const asd::LoopClosing::Result ls = asd::LoopClosing::ComputeSim3(ctx, F[1], fv1, cands, cand_fv, mps, [&](int) { return loop_ids; }, K,
                                                                          extractor.GetScaleSigmaSquares(), extractor.GetInverseScaleSigmaSquares(),
                                                                          false, draws, matched);
        printf("loop-solver: candidate=%d bow=%d sim3=%d inliers=%d total=%d match=%d scale=%.6f\n", ls.iMatched, ls.nBoW, ls.nSim3, ls.nInliers,
               ls.nTotalMatches, (int)ls.bMatch, ls.g2oScm[7]);
      }
      // Tracking::Relocalization's solver step (Tracking.cc:1128-1174) with frame 0 as the one candidate keyframe: the BoW matches above,
      // asd::PnPsolver's EPnP RANSAC on the device, passes of 5 iterations until a pose comes back; the tail (:1176-1247) is left to a
      // callback that accepts the first pose.  Informative only, the exit status does not depend on it
      {
        std::srand(1);
        asd::DrawStream draws;   // ::rand
        asd::PnPsolver pnp(ctx, F[1], vpMapPointMatches, mps, K, extractor.GetScaleSigmaSquares(), draws);
        pnp.SetRansacParameters(0.99, 10, 300, 4, 0.5f, 5.991f);                  // :1141
        std::vector<asd::PnPsolver*> solvers = {&pnp};
        std::vector<bool> discarded = {false};
        int matched = -1, n_pnp = 0, passes = 0;
        float Tpnp[16] = {};
        while (!discarded[0] && matched < 0) {
          ++passes;
          matched = asd::Tracking::RelocalizationRound(ctx, solvers, discarded, 5, [&](int, const float* Tcw, const std::vector<bool>&, int nInl) {
            n_pnp = nInl;
            for (int i = 0; i < 16; ++i) Tpnp[i] = Tcw[i];
            return true;
          });
        }
        printf("reloc-solver: candidate=%d n=%d min=%d passes=%d iterations=%d inliers=%d t=(%.4f %.4f %.4f)\n", matched, pnp.GetN(), pnp.GetMinInliers(),
               passes, pnp.GetIterations(), n_pnp, Tpnp[3], Tpnp[7], Tpnp[11]);
      }
    }
    // Tracking::MonocularInitialization (Tracking.cc:385-438) on the same pair: SearchForInitialization, then Initializer(frame, 1.0, 200)
    // and Initialize -- both RANSACs and the reconstruction in one asd_initialize call.  Informative only, the exit status does not depend on it
    {
      asd::ORBmatcher ini_matcher(ctx, 0.9f, true);                                                          // :425
      std::vector<float> vbPrevMatched;                                                                      // :399-402
      for (const asd_keypoint& k : F[0].mvKeysUn) { vbPrevMatched.push_back(k.x); vbPrevMatched.push_back(k.y); }
      std::vector<int> vIniMatches;
      const int nini = ini_matcher.SearchForInitialization(F[0], F[1], vbPrevMatched, vIniMatches, 100);     // :426
      asd::Initializer initializer(ctx.get(), F[0], K, 1.0f, 200);                                           // :407
      float R21[9] = {}, t21[3] = {};
      std::vector<asd::Point3f> vIniP3D;
      std::vector<bool> vbTriangulated;
      const bool ini_ok = initializer.Initialize(F[1], vIniMatches, R21, t21, vIniP3D, vbTriangulated);      // :438
      int ntri = 0;
      for (bool b : vbTriangulated) ntri += b;
      printf("initializer: matches=%d ok=%d model=%s SH=%.1f SF=%.1f triangulated=%d t21=(%.4f %.4f %.4f)\n", nini, (int)ini_ok,
             initializer.Last().model == 0 ? "H" : "F", initializer.Last().SH, initializer.Last().SF, ntri, t21[0], t21[1], t21[2]);
      // Tracking::CreateInitialMapMonocular (Tracking.cc:472-570) on that result: the two keyframes, a map point per triangulated match,
      // Optimizer::GlobalBundleAdjustemnt(mpMap, 20) (:535) and the median-depth rescaling (:539-565)
      if (ini_ok) {
        const std::vector<float> invSigma2 = extractor.GetInverseScaleSigmaSquares();
        std::vector<asd::Optimizer::BAKeyFrame> kfs(2);
        for (int q = 0; q < 2; ++q) { kfs[q].mnId = q; kfs[q].mvKeysUn = &F[q].mvKeysUn; kfs[q].mvInvLevelSigma2 = &invSigma2; }
        for (int r = 0; r < 3; ++r) { for (int q = 0; q < 3; ++q) kfs[1].Tcw[r * 4 + q] = R21[r * 3 + q]; kfs[1].Tcw[r * 4 + 3] = t21[r]; }   // :449-453
        std::vector<asd::Optimizer::BAMapPoint> map;
        std::vector<int32_t> iniPoints(F[0].N(), -1);
        for (size_t i = 0; i < vIniMatches.size(); ++i) {
          if (vIniMatches[i] < 0 || !vbTriangulated[i]) continue;                                          // :489-491
          asd::Optimizer::BAMapPoint mp;
          mp.mnId = map.size();
          mp.Xw[0] = vIniP3D[i].x; mp.Xw[1] = vIniP3D[i].y; mp.Xw[2] = vIniP3D[i].z;
          mp.observations = {{0, i}, {1, (size_t)vIniMatches[i]}};                                         // :501-502
          iniPoints[i] = (int32_t)map.size();
          map.push_back(mp);
        }
        const asd::Optimizer::BAResult ba = asd::Optimizer::GlobalBundleAdjustemnt(ctx, kfs, map, K, 20);  // :535
        float median = 0;
        bool scaled = false;
        if (ba.rc == ASD_OK) {
          float Tcur[16];
          for (int q = 0; q < 16; ++q) Tcur[q] = ba.Tcw[16 + q];
          std::vector<float> Xw = ba.Xw;
          scaled = asd::Tracking::InitialMapScale(ba.Tcw.data(), Tcur, iniPoints, Xw, (int)map.size(), &median);
          printf("initial-map: points=%d edges=%d gba_iterations=%d trials=%d chi2=%.3f median_depth=%.4f scaled=%d t=(%.4f %.4f %.4f)\n", (int)map.size(),
                 ba.n_edges, ba.iterations, ba.trials, ba.chi2, median, (int)scaled, Tcur[3], Tcur[7], Tcur[11]);
        } else {
          printf("initial-map: points=%d asd_bundle_adjustment failed (%d): %s\n", (int)map.size(), ba.rc, ctx.error());
        }
      }
    }
    printf("kp0=%d kp1=%d matches=%d inliers=%d fused=%d bow=%d t=(%.4f %.4f %.4f)\n", F[0].N(), F[1].N(), nmatches, ninl, nfused, nbow,
           F[1].mTcw[3], F[1].mTcw[7], F[1].mTcw[11]);
    return (nmatches > 100 && ninl > 50 && nfused > 0 && nbow > 0 && chain_ok && loop_ok) ? 0 : 1;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
