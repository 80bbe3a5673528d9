// asd_adapters.hpp -- C++ host-side mirror of the reference's call surface for the hot path.
//
// The reference reaches the hot path through three classes of libvslam:
//   ORB_SLAM2::ORBextractor  src/vslam/include/ORBextractor.h:54-87
//   ORB_SLAM2::ORBmatcher    src/vslam/include/ORBmatcher.h:48-90
//   ORB_SLAM2::Optimizer     src/vslam/include/Optimizer.h:45-46
// Their signatures carry cv::Mat / Frame / MapPoint*; OpenCV and the vslam headers are not
// available here, so these mirrors keep the METHOD NAMES, ARGUMENT MEANING and RETURN VALUES but
// take the flat views the methods actually read (asd::FrameView, asd::MapPointView).  Each
// method documents the reference line it stands for.  Header only, depends on include/asd_slam.h
// and the C++ standard library; link with -lasdhip.  INTEGRATION.md shows the few lines that wrap
// these into the reference's own classes inside the catkin workspace.
//
// Error behaviour follows the reference (no exceptions on the data path, "return 0 / -1" on
// failure) except construction, which throws std::runtime_error if no HIP device is usable.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <deque>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <algorithm>
#include <vector>

#include "../../include/asd_slam.h"
#include "map_point_culling.hpp"

namespace asd {

struct Camera { float fx, fy, cx, cy; };

// What the matchers and the optimizer read from a Frame (Frame.h): undistorted keypoints,
// descriptors (row-major N x 128 f32), image bounds, pose Tcw (row-major 4x4 f32).
struct FrameView {
  int slot = 0;                         // asd_frame_set slot holding mvKeysUn / mDescriptors / mGrid
  std::vector<asd_keypoint> mvKeysUn;
  std::vector<float> mDescriptors;
  float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
  float mTcw[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::vector<int32_t> mvpMapPoints;    // index into the caller's map point table, -1 = NULL
  std::vector<uint8_t> mvbOutlier;
  int N() const { return (int)mvKeysUn.size(); }
};

// What SearchByProjection / isInFrustum / PoseOptimization read from MapPoint (MapPoint.h).
struct MapPointView {
  float Xw[3];          // GetWorldPos
  float normal[3];      // GetNormal
  float mfMinDistance, mfMaxDistance;
  const float* descriptor;  // GetDescriptor, 128 f32
  int nObs = 1;             // Observations(): a keypoint holding a map point with nObs == 0 is not skipped (ORBmatcher.cc:86-88)
};

class Context {
 public:
  Context(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int maxWidth, int maxHeight,
          int device = 0) {
    asd_config cfg{nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, maxWidth, maxHeight, 2 * nfeatures, device};
    const int rc = asd_ctx_create(&cfg, &ctx_);
    if (rc != ASD_OK) throw std::runtime_error("asd_ctx_create failed (" + std::to_string(rc) + "): no usable HIP device");
  }
  ~Context() { if (ctx_) asd_ctx_destroy(ctx_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  asd_ctx* get() const { return ctx_; }
  const char* error() const { return asd_last_error(ctx_); }
  // Tracking's constructor (Tracking.cc:59-72): mK = (fx, fy, cx, cy), mDistCoef = (k1, k2, p1, p2).  Replaces the per-frame
  // cv::undistort(im, mImGray, mK, mDistCoef) of Tracking.cc:104,125: the raw image goes to ExtractDesc / asd_extract_submit and
  // the Frame still gets distCoefZero.  Zero coefficients set no map.
  void SetUndistortion(const float K[4], const float distCoef[4], int width, int height) {
    if (asd_set_undistortion(ctx_, K, distCoef, width, height) != ASD_OK) throw std::runtime_error(error());
  }
 private:
  asd_ctx* ctx_ = nullptr;
};

// ---- ORBextractor (ORBextractor.h:54-87; ctor ORBextractor.cc:452-516) -------------------------
class ORBextractor {
 public:
  // weights replace torch::jit::load("...bestmodel_c.pt") (ORBextractor.cc:457)
  ORBextractor(Context& c, const float* const conv_w[7], const float* const bn_mean[7], const float* const bn_var[7],
               float bn_eps = 1e-5f)
      : c_(c) {
    if (asd_load_weights(c_.get(), conv_w, bn_mean, bn_var, bn_eps) != ASD_OK) throw std::runtime_error(c_.error());
    asd_config dummy{};
    (void)dummy;
  }
  // void ExtractDesc(InputArray image, InputArray mask, vector<KeyPoint>&, OutputArray desc, bool use_orb)
  // (ORBextractor.cc:1137).  mask is ignored by the reference; use_orb=false is the ASD path.
  // Returns the number of keypoints, -1 on error (the reference returns void and asserts).
  int ExtractDesc(const uint8_t* image, int width, int height, int stride, std::vector<asd_keypoint>& keypoints,
                  std::vector<float>& descriptors, int nfeatures_override = 0) {
    const int cap = capacity();
    keypoints.resize(cap);
    descriptors.resize((size_t)cap * ASD_DESC_DIM);
    int32_t n = 0;
    if (asd_extract(c_.get(), image, width, height, stride, nfeatures_override, keypoints.data(), descriptors.data(), &n) != ASD_OK)
      return -1;
    keypoints.resize(n);
    descriptors.resize((size_t)n * ASD_DESC_DIM);
    return n;
  }
  int GetLevels() const { return levels(); }
  std::vector<float> GetScaleFactors() const { return table(0); }
  std::vector<float> GetInverseScaleFactors() const { return table(1); }
  std::vector<float> GetScaleSigmaSquares() const { return table(2); }
  std::vector<float> GetInverseScaleSigmaSquares() const { return table(3); }
  // mvImagePyramid[level] without the 19 px border (ORBextractor.h:87)
  std::vector<uint8_t> ImagePyramidLevel(int level, int* w, int* h) const {
    int32_t ww = 0, hh = 0;
    if (asd_get_level_size(c_.get(), level, &ww, &hh) != ASD_OK) return {};
    std::vector<uint8_t> img((size_t)ww * hh);
    asd_get_level_image(c_.get(), level, 0, img.data());
    *w = ww; *h = hh;
    return img;
  }
 private:
  int levels() const { int n = 0; float s[ASD_MAX_LEVELS]; int32_t f[ASD_MAX_LEVELS]; asd_get_scale_tables(c_.get(), s, nullptr, nullptr, nullptr, f); for (; n < ASD_MAX_LEVELS && f[n] > 0; ++n) {} return n; }
  int capacity() const { return 1 << 13; }
  std::vector<float> table(int which) const {
    float t[4][ASD_MAX_LEVELS] = {};
    asd_get_scale_tables(c_.get(), t[0], t[1], t[2], t[3], nullptr);
    return std::vector<float>(t[which], t[which] + levels());
  }
  Context& c_;
};

// ---- Frame bookkeeping (Frame.cc:64-138): call after ExtractDesc ------------------------------
inline int FrameAssignFeaturesToGrid(Context& c, FrameView& F, bool adopt_last_extract = true) {
  return asd_frame_set(c.get(), F.slot, F.mvKeysUn.data(), adopt_last_extract ? nullptr : F.mDescriptors.data(), F.N(),
                       F.mnMinX, F.mnMaxX, F.mnMinY, F.mnMaxY);
}

// ---- ORBmatcher (ORBmatcher.h:48-90) -----------------------------------------------------------
class ORBmatcher {
 public:
  ORBmatcher(Context& c, float nnratio = 0.6f, bool checkOri = true) : c_(c), mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

  // static float DescriptorDistance(const cv::Mat&, const cv::Mat&)  (ORBmatcher.cc:1629)
  float DescriptorDistance(const float* a, const float* b) {
    float d = -1.f;
    asd_dist_matrix(c_.get(), a, 1, b, 1, &d);
    return d;
  }

  // int SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, float th, bool bMono)  (:1318)
  // `points` are LastFrame's map points indexed like LastFrame.mvKeysUn (null where mvpMapPoints[i]==NULL
  // or mvbOutlier[i]).  Writes CurrentFrame.mvpMapPoints like the reference.
  int SearchByProjection(FrameView& Cur, const FrameView& Last, const std::vector<const MapPointView*>& points,
                         const Camera& K, float th, bool /*bMono: the reference is monocular only*/ = true) {
    const int nl = Last.N();
    std::vector<uint8_t> has(nl, 0), obs(nl, 1);
    std::vector<float> Xw((size_t)nl * 3, 0.f), desc((size_t)nl * ASD_DESC_DIM, 0.f);
    for (int i = 0; i < nl; ++i)
      if (points[i]) {
        has[i] = 1;
        obs[i] = points[i]->nObs > 0;
        for (int k = 0; k < 3; ++k) Xw[3 * i + k] = points[i]->Xw[k];
        for (int k = 0; k < ASD_DESC_DIM; ++k) desc[(size_t)i * ASD_DESC_DIM + k] = points[i]->descriptor[k];
      }
    std::vector<int32_t> match(Cur.N(), -1);
    int32_t n = 0;
    const float Kv[4] = {K.fx, K.fy, K.cx, K.cy};
    if (asd_match_project_frame(c_.get(), Cur.slot, Last.slot, has.data(), Xw.data(), desc.data(), Cur.mTcw, Kv, th,
                                mbCheckOrientation, match.data(), &n, obs.data()) != ASD_OK)
      return 0;
    Cur.mvpMapPoints.assign(Cur.N(), -1);
    for (int j = 0; j < Cur.N(); ++j)
      if (match[j] >= 0) Cur.mvpMapPoints[j] = Last.mvpMapPoints[match[j]];
    return n;
  }

  // int SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, float th)  (:44), preceded by
  // Frame::isInFrustum for every point as Tracking::SearchLocalPoints does (Tracking.cc:803-851).
  int SearchByProjection(FrameView& F, const std::vector<MapPointView>& vpMapPoints, const std::vector<int32_t>& ids,
                         const Camera& K, float th = 3.f) {
    const int n = (int)vpMapPoints.size();
    std::vector<float> Xw((size_t)n * 3), nrm((size_t)n * 3), mind(n), maxd(n), desc((size_t)n * ASD_DESC_DIM);
    for (int m = 0; m < n; ++m) {
      for (int k = 0; k < 3; ++k) { Xw[3 * m + k] = vpMapPoints[m].Xw[k]; nrm[3 * m + k] = vpMapPoints[m].normal[k]; }
      mind[m] = vpMapPoints[m].mfMinDistance; maxd[m] = vpMapPoints[m].mfMaxDistance;
      for (int k = 0; k < ASD_DESC_DIM; ++k) desc[(size_t)m * ASD_DESC_DIM + k] = vpMapPoints[m].descriptor[k];
    }
    std::vector<uint8_t> in_view(n), occupied(F.N(), 0), obs(n, 1);
    for (int m = 0; m < n; ++m) obs[m] = vpMapPoints[m].nObs > 0;
    std::vector<float> proj((size_t)n * 2), vc(n);
    std::vector<int32_t> level(n), match(F.N(), -1);
    const float Kv[4] = {K.fx, K.fy, K.cx, K.cy};
    if (asd_frustum(c_.get(), F.slot, n, Xw.data(), nrm.data(), mind.data(), maxd.data(), F.mTcw, Kv, 0.5f,
                    in_view.data(), proj.data(), level.data(), vc.data()) != ASD_OK)
      return 0;
    for (int j = 0; j < F.N(); ++j) occupied[j] = F.mvpMapPoints.size() == (size_t)F.N() && F.mvpMapPoints[j] >= 0;
    int32_t nm = 0;
    if (asd_match_project_points(c_.get(), F.slot, n, in_view.data(), proj.data(), level.data(), vc.data(), desc.data(),
                                 occupied.data(), th, mfNNratio, match.data(), &nm, obs.data()) != ASD_OK)
      return 0;
    F.mvpMapPoints.resize(F.N(), -1);
    for (int j = 0; j < F.N(); ++j)
      if (match[j] >= 0) F.mvpMapPoints[j] = ids[match[j]];
    return nm;
  }

  // int SearchForInitialization(Frame& F1, Frame& F2, vector<Point2f>& vbPrevMatched, vector<int>& vnMatches12,
  //                             int windowSize)  (:416)
  int SearchForInitialization(const FrameView& F1, const FrameView& F2, std::vector<float>& vbPrevMatched,
                              std::vector<int>& vnMatches12, int windowSize = 10) {
    vnMatches12.assign(F1.N(), -1);
    int32_t n = 0;
    if (asd_match_init(c_.get(), F1.slot, F2.slot, vbPrevMatched.data(), windowSize, mfNNratio, mbCheckOrientation,
                       vnMatches12.data(), &n) != ASD_OK)
      return 0;
    return n;
  }

  // DBoW2::FeatureVector as the matchers read it (node id -> keypoint indices), CSR over ascending node ids
  struct FeatVec {
    std::vector<int32_t> node, start{0}, idx;
    asd_feature_vector view() const { return asd_feature_vector{(int32_t)node.size(), node.data(), start.data(), idx.data()}; }
  };

  // int SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)  (:156)
  // vpMapPointMatches[j] = pKF's map point id matched to F's keypoint j, -1 = NULL
  int SearchByBoW(const FrameView& KF, const FeatVec& fvKF, const FrameView& F, const FeatVec& fvF,
                  std::vector<int32_t>& vpMapPointMatches) {
    std::vector<uint8_t> has(KF.N(), 0);
    for (int i = 0; i < KF.N(); ++i) has[i] = KF.mvpMapPoints.size() == (size_t)KF.N() && KF.mvpMapPoints[i] >= 0;
    std::vector<int32_t> m(F.N(), -1);
    int32_t n = 0;
    const asd_feature_vector a = fvKF.view(), b = fvF.view();
    if (asd_match_bow(c_.get(), KF.slot, F.slot, &a, &b, has.data(), mfNNratio, mbCheckOrientation, m.data(), &n) != ASD_OK) return 0;
    vpMapPointMatches.assign(F.N(), -1);
    for (int j = 0; j < F.N(); ++j)
      if (m[j] >= 0) vpMapPointMatches[j] = KF.mvpMapPoints[m[j]];
    return n;
  }

  // int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)  (:533), the loop-closing overload
  // (LoopClosing.cc:304).  vpMatches12[i1] = pKF2's map point id matched to pKF1's keypoint i1, -1 = NULL; vnIdx2[i1] = that
  // point's keypoint in pKF2 (what pMP2->GetIndexInKeyFrame(pKF2) gives OptimizeSim3, Optimizer.cc:1063).  mvpMapPoints[i] >= 0
  // stands for "the keyframe has a map point there and it is not bad".
  int SearchByBoW(const FrameView& KF1, const FeatVec& fv1, const FrameView& KF2, const FeatVec& fv2, std::vector<int32_t>& vpMatches12,
                  std::vector<int32_t>& vnIdx2) {
    std::vector<uint8_t> h1(KF1.N(), 0), h2(KF2.N(), 0);
    for (int i = 0; i < KF1.N(); ++i) h1[i] = KF1.mvpMapPoints.size() == (size_t)KF1.N() && KF1.mvpMapPoints[i] >= 0;
    for (int i = 0; i < KF2.N(); ++i) h2[i] = KF2.mvpMapPoints.size() == (size_t)KF2.N() && KF2.mvpMapPoints[i] >= 0;
    vnIdx2.assign(KF1.N(), -1);
    vpMatches12.assign(KF1.N(), -1);
    int32_t n = 0;
    const asd_feature_vector a = fv1.view(), b = fv2.view();
    if (asd_match_bow_kf(c_.get(), KF1.slot, KF2.slot, &a, &b, h1.data(), h2.data(), mfNNratio, mbCheckOrientation, vnIdx2.data(), &n) != ASD_OK) {
      vnIdx2.assign(KF1.N(), -1);
      return 0;
    }
    for (int i = 0; i < KF1.N(); ++i)
      if (vnIdx2[i] >= 0) vpMatches12[i] = KF2.mvpMapPoints[vnIdx2[i]];
    return n;
  }

  // int SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, cv::Mat F12, vector<pair<size_t,size_t>>& vMatchedPairs,
  //                            bool bOnlyStereo)  (:669).  (ex, ey) = epipole of camera 1 in image 2 (:675-683).
  int SearchForTriangulation(const FrameView& KF1, const FeatVec& fv1, const FrameView& KF2, const FeatVec& fv2, const float F12[9],
                             float ex, float ey, std::vector<std::pair<size_t, size_t>>& vMatchedPairs) {
    std::vector<uint8_t> h1(KF1.N(), 0), h2(KF2.N(), 0);
    for (int i = 0; i < KF1.N(); ++i) h1[i] = KF1.mvpMapPoints.size() == (size_t)KF1.N() && KF1.mvpMapPoints[i] >= 0;
    for (int i = 0; i < KF2.N(); ++i) h2[i] = KF2.mvpMapPoints.size() == (size_t)KF2.N() && KF2.mvpMapPoints[i] >= 0;
    std::vector<int32_t> m(KF1.N(), -1);
    int32_t n = 0;
    const asd_feature_vector a = fv1.view(), b = fv2.view();
    vMatchedPairs.clear();
    if (asd_match_triangulate(c_.get(), KF1.slot, KF2.slot, &a, &b, h1.data(), h2.data(), F12, ex, ey, mbCheckOrientation, m.data(), &n) != ASD_OK)
      return 0;
    for (int i = 0; i < KF1.N(); ++i)
      if (m[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m[i]);   // :809-816: ascending idx1
    return n;
  }

  // int Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, float th)  (:825): search half.  bestIdx[i] = keypoint
  // of pKF that map point i should be fused into (-1 = none); the Replace / AddObservation loop (:938-956) is asd::FuseApply(c,
  // kfId, 0, rows, bestIdx) over the observation table, and the static Fuse(c, kfId, ...) below is both halves as one call
  // (host/fuse_apply.hpp for a caller that keeps its own lists).  valid[i] = pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF).
  int Fuse(const FrameView& KF, const std::vector<MapPointView>& vpMapPoints, const std::vector<uint8_t>& valid, const Camera& K,
           std::vector<int32_t>& bestIdx, float th = 3.f) {
    const int n = (int)vpMapPoints.size();
    std::vector<float> Xw((size_t)n * 3), nrm((size_t)n * 3), mind(n), maxd(n), desc((size_t)n * ASD_DESC_DIM), bd(n);
    for (int m = 0; m < n; ++m) {
      for (int k = 0; k < 3; ++k) { Xw[3 * m + k] = vpMapPoints[m].Xw[k]; nrm[3 * m + k] = vpMapPoints[m].normal[k]; }
      mind[m] = vpMapPoints[m].mfMinDistance; maxd[m] = vpMapPoints[m].mfMaxDistance;
      for (int k = 0; k < ASD_DESC_DIM; ++k) desc[(size_t)m * ASD_DESC_DIM + k] = vpMapPoints[m].descriptor[k];
    }
    bestIdx.assign(n, -1);
    const float Kv[4] = {K.fx, K.fy, K.cx, K.cy};
    if (asd_fuse_search(c_.get(), KF.slot, n, valid.data(), Xw.data(), nrm.data(), mind.data(), maxd.data(), desc.data(), KF.mTcw, Kv, th,
                        bestIdx.data(), bd.data()) != ASD_OK)
      return 0;
    int nFused = 0;
    for (int m = 0; m < n; ++m) nFused += bestIdx[m] >= 0;
    return nFused;
  }

  // what both Fuse searches read, from the caller's views and the table: valid[i] = rows[i] names a point that kfId's row does not hold
  // (pMP && !IsInKeyFrame(pKF) / !spAlreadyFound.count(pMP), from asd_map_get); isBad() is left to asd_fuse_apply's gate, which tests it
  // at the candidate's turn -- a bad point costs a search and takes no step
  static int FuseSearchInput(Context& c, int32_t kfId, const std::vector<MapPointView>& points, const std::vector<int32_t>& rows,
                             std::vector<uint8_t>& valid, std::vector<float>& Xw, std::vector<float>& nrm, std::vector<float>& mind,
                             std::vector<float>& maxd, std::vector<float>& desc);
  // int Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, float th)  (:825-960) as the reference's ONE call over the observation
  // table: the search (asd_fuse_search) and the side effects (asd_fuse_apply mode 0).  kfId = pKF->mnId, KF its view (slot, pose);
  // points[i] = the view of bank row rows[i], ignored where rows[i] < 0.  nFused is the reference's return value.
  static struct FuseOutcome Fuse(Context& c, int32_t kfId, const FrameView& KF, const std::vector<MapPointView>& points,
                                 const std::vector<int32_t>& rows, const Camera& K, float th = 3.f);

 private:
  Context& c_;
  float mfNNratio;
  bool mbCheckOrientation;
};

// ---- Optimizer (Optimizer.h:45-46) -------------------------------------------------------------
struct Optimizer {
  // int static PoseOptimization(Frame* pFrame)  (Optimizer.cc:239): returns the number of inliers, writes
  // pFrame->mTcw and mvbOutlier.  inv_level_sigma2 = pFrame->mvInvLevelSigma2.
  static int PoseOptimization(Context& c, FrameView* pFrame, const std::vector<const MapPointView*>& points,
                              const Camera& K, const std::vector<float>& inv_level_sigma2) {
    std::vector<int> idx;
    std::vector<double> Xw, obs, info;
    for (int i = 0; i < pFrame->N(); ++i)
      if (points[i]) {
        idx.push_back(i);
        for (int k = 0; k < 3; ++k) Xw.push_back(points[i]->Xw[k]);
        obs.push_back(pFrame->mvKeysUn[i].x); obs.push_back(pFrame->mvKeysUn[i].y);
        info.push_back(inv_level_sigma2[pFrame->mvKeysUn[i].octave]);
      }
    pFrame->mvbOutlier.assign(pFrame->N(), 0);
    double pose[7];
    asd_tcw_to_pose7(pFrame->mTcw, pose);
    std::vector<uint8_t> out(idx.size());
    const double Kd[4] = {K.fx, K.fy, K.cx, K.cy};
    int32_t ninl = 0;
    if (asd_pose_optimize(c.get(), pose, (int)idx.size(), Xw.data(), obs.data(), info.data(), Kd, out.data(), &ninl) != ASD_OK)
      return 0;
    for (size_t k = 0; k < idx.size(); ++k) pFrame->mvbOutlier[idx[k]] = out[k];
    asd_pose7_to_tcw(pose, pFrame->mTcw);
    return ninl;
  }

  // int static OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
  //                         const bool bFixScale)  (Optimizer.cc:1002).  vpMatches1[i] = pKF2's map point id matched to pKF1's keypoint i
  // (-1 = NULL) and vnIdx2[i] its keypoint in pKF2, as SearchByBoW / SearchBySim3 leave them; `points` = the caller's map point
  // table those ids index.  g2oS12 = qx qy qz qw tx ty tz s.  Returns nIn; matches the optimiser dropped are set to -1 in both
  // vectors; on the early return (:1165) it returns 0 and leaves g2oS12 alone.  invLevelSigma2_1 / _2 = mvInvLevelSigma2.
  static int OptimizeSim3(Context& c, const FrameView& KF1, const FrameView& KF2, const std::vector<MapPointView>& points,
                          std::vector<int32_t>& vpMatches1, std::vector<int32_t>& vnIdx2, double g2oS12[8], float th2, bool bFixScale,
                          const Camera& K1, const Camera& K2, const std::vector<float>& invLevelSigma2_1,
                          const std::vector<float>& invLevelSigma2_2) {
    std::vector<int> idx;
    std::vector<double> P1c, P2c, o1, o2, s1, s2;
    auto to_camera = [](const float* T, const float* X, std::vector<double>& out) {   // R * P3Dw + t in f32 (cv::Mat CV_32F), :1071
      for (int r = 0; r < 3; ++r) out.push_back((double)((T[r * 4] * X[0] + T[r * 4 + 1] * X[1] + T[r * 4 + 2] * X[2]) + T[r * 4 + 3]));
    };
    for (int i = 0; i < KF1.N(); ++i) {
      if (vpMatches1[i] < 0) continue;
      const int i2 = vnIdx2[i];
      if (KF1.mvpMapPoints[i] < 0 || i2 < 0) continue;                               // :1065-1089
      idx.push_back(i);
      to_camera(KF1.mTcw, points[KF1.mvpMapPoints[i]].Xw, P1c);
      to_camera(KF2.mTcw, points[vpMatches1[i]].Xw, P2c);
      o1.push_back(KF1.mvKeysUn[i].x); o1.push_back(KF1.mvKeysUn[i].y);
      o2.push_back(KF2.mvKeysUn[i2].x); o2.push_back(KF2.mvKeysUn[i2].y);
      s1.push_back(invLevelSigma2_1[KF1.mvKeysUn[i].octave]);
      s2.push_back(invLevelSigma2_2[KF2.mvKeysUn[i2].octave]);
    }
    const double k1[4] = {K1.fx, K1.fy, K1.cx, K1.cy}, k2[4] = {K2.fx, K2.fy, K2.cx, K2.cy};
    std::vector<uint8_t> keep(idx.size() + 1, 0);
    int32_t nIn = 0;
    if (asd_optimize_sim3(c.get(), g2oS12, (int32_t)idx.size(), P1c.data(), P2c.data(), o1.data(), o2.data(), s1.data(), s2.data(), k1, k2, th2,
                          bFixScale, keep.data(), &nIn) != ASD_OK)
      return 0;
    for (size_t k = 0; k < idx.size(); ++k)
      if (!keep[k]) { vpMatches1[idx[k]] = -1; vnIdx2[idx[k]] = -1; }
    return nIn;
  }

  // What Optimizer::BundleAdjustment reads from a KeyFrame and a MapPoint, flat.  A keyframe that a map point observes but that is not
  // among vpKFs is still listed, with in_set = false: only its mnId and bad are read (the `pKF->mnId > maxKFid` test of :116).
  struct BAKeyFrame {
    unsigned long mnId = 0;
    bool bad = false;                                   // isBad()
    bool in_set = true;                                 // one of vpKFs
    float Tcw[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // GetPose()
    const std::vector<asd_keypoint>* mvKeysUn = nullptr;
    const std::vector<float>* mvInvLevelSigma2 = nullptr;
  };
  struct BAMapPoint {
    unsigned long mnId = 0;
    bool bad = false;                                   // isBad()
    float Xw[3] = {0, 0, 0};                            // GetWorldPos()
    std::vector<std::pair<int, size_t>> observations;   // GetObservations() in the map's order: (index into the keyframe vector, keypoint)
  };
  // What :193-235 write back.  kf_written[i]: keyframe i is not bad (SetPose, or mTcwGBA / mnBAGlobalForKF when nLoopKF != 0: that
  // choice stays the caller's); mp_written[i]: map point i is not bad and was included (vbNotIncludedMP, :153-161).
  struct BAResult {
    int rc = ASD_OK, iterations = 0, trials = 0, n_edges = 0;
    double chi2 = 0;
    std::vector<uint8_t> kf_written, mp_written, vbNotIncludedMP;
    std::vector<float> Tcw;   // [keyframes][16]
    std::vector<float> Xw;    // [points][3]
  };
  // void static BundleAdjustment(const vector<KeyFrame*>& vpKFs, const vector<MapPoint*>& vpMP, int nIterations, bool* pbStopFlag,
  //                              const unsigned long nLoopKF, const bool bRobust)  (Optimizer.cc:51-237) over asd_bundle_adjustment.
  // The gather is :69-162: bad keyframes and bad map points get no vertex; an observation of a bad keyframe, or of one with
  // mnId > maxKFid (the largest id among the keyframes that are not bad), gets no edge; a point left without an edge is not included;
  // keyframe mnId == 0 is fixed.  Vertices go to the device by ascending id, the edges point by point in the observations' order.
  static BAResult BundleAdjustment(Context& c, const std::vector<BAKeyFrame>& keyframes, const std::vector<BAMapPoint>& points, const Camera& K,
                                   int nIterations = 5, const volatile int32_t* pbStopFlag = nullptr, bool bRobust = true) {
    BAResult out;
    const int nKF = (int)keyframes.size(), nMP = (int)points.size();
    out.kf_written.assign(nKF, 0); out.mp_written.assign(nMP, 0); out.vbNotIncludedMP.assign(nMP, 0);
    out.Tcw.assign((size_t)nKF * 16, 0.f); out.Xw.assign((size_t)nMP * 3, 0.f);
    unsigned long maxKFid = 0;
    std::vector<int> kf_order, mp_order, kf_row(nKF, -1), mp_row(nMP, -1);
    for (int i = 0; i < nKF; ++i) {
      if (!keyframes[i].in_set || keyframes[i].bad) continue;                      // :79-80
      kf_order.push_back(i);
      if (keyframes[i].mnId > maxKFid) maxKFid = keyframes[i].mnId;                // :86-87
    }
    for (int i = 0; i < nMP; ++i) if (!points[i].bad) mp_order.push_back(i);      // :99-100
    std::stable_sort(kf_order.begin(), kf_order.end(), [&](int a, int b) { return keyframes[a].mnId < keyframes[b].mnId; });
    std::stable_sort(mp_order.begin(), mp_order.end(), [&](int a, int b) { return points[a].mnId < points[b].mnId; });
    std::vector<double> poses(kf_order.size() * 7), X(mp_order.size() * 3), obs, info;
    std::vector<uint8_t> fixed(kf_order.size(), 0);
    std::vector<int32_t> e_point, e_pose;
    for (size_t r = 0; r < kf_order.size(); ++r) {
      kf_row[kf_order[r]] = (int)r;
      asd_tcw_to_pose7(keyframes[kf_order[r]].Tcw, poses.data() + 7 * r);         // Converter::toSE3Quat(pKF->GetPose()), :82
      fixed[r] = keyframes[kf_order[r]].mnId == 0;                                 // :84
    }
    for (size_t r = 0; r < mp_order.size(); ++r) {
      const BAMapPoint& mp = points[mp_order[r]];
      mp_row[mp_order[r]] = (int)r;
      for (int k = 0; k < 3; ++k) X[3 * r + k] = mp.Xw[k];
      int nEdges = 0;
      for (const std::pair<int, size_t>& ob : mp.observations) {
        const BAKeyFrame& kf = keyframes[ob.first];
        if (kf.bad || kf.mnId > maxKFid) continue;                                 // :116-117
        if (kf_row[ob.first] < 0) throw std::runtime_error("asd::Optimizer::BundleAdjustment: an observation of a keyframe that is not among vpKFs and has no larger id (the reference would set a null vertex)");
        ++nEdges;
        const asd_keypoint& kp = (*kf.mvKeysUn)[ob.second];
        e_point.push_back((int32_t)r); e_pose.push_back(kf_row[ob.first]);
        obs.push_back(kp.x); obs.push_back(kp.y);
        info.push_back((*kf.mvInvLevelSigma2)[kp.octave]);
      }
      out.vbNotIncludedMP[mp_order[r]] = nEdges == 0;                              // :153-161
    }
    asd_gba_problem pr{};
    pr.n_poses = (int32_t)kf_order.size(); pr.n_points = (int32_t)mp_order.size(); pr.n_edges = (int32_t)e_point.size();
    pr.poses = poses.data(); pr.fixed = fixed.data(); pr.points = X.data();
    pr.e_point = e_point.data(); pr.e_pose = e_pose.data(); pr.e_obs = obs.data(); pr.e_info = info.data();
    pr.K[0] = K.fx; pr.K[1] = K.fy; pr.K[2] = K.cx; pr.K[3] = K.cy;
    pr.n_iterations = nIterations; pr.robust = bRobust; pr.stop = pbStopFlag;
    std::vector<double> edge_chi2(e_point.size() + 1);
    asd_gba_result res{};
    res.edge_chi2 = edge_chi2.data();
    out.n_edges = pr.n_edges;
    out.rc = asd_bundle_adjustment(c.get(), &pr, &res);
    if (out.rc != ASD_OK) return out;
    out.iterations = res.iterations; out.trials = res.trials; out.chi2 = res.chi2;
    for (size_t r = 0; r < kf_order.size(); ++r) {                                 // :193-210
      out.kf_written[kf_order[r]] = 1;
      asd_pose7_to_tcw(poses.data() + 7 * r, out.Tcw.data() + (size_t)kf_order[r] * 16);
    }
    for (size_t r = 0; r < mp_order.size(); ++r) {                                 // :213-235
      if (out.vbNotIncludedMP[mp_order[r]]) continue;
      out.mp_written[mp_order[r]] = 1;
      for (int k = 0; k < 3; ++k) out.Xw[(size_t)mp_order[r] * 3 + k] = (float)X[3 * r + k];   // Converter::toCvMat(Vector3d): CV_32F
    }
    return out;
  }
  // void static GlobalBundleAdjustemnt(Map* pMap, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust)
  // (Optimizer.cc:43-48): pMap->GetAllKeyFrames() / GetAllMapPoints() are the caller's two vectors.
  static BAResult GlobalBundleAdjustemnt(Context& c, const std::vector<BAKeyFrame>& allKeyFrames, const std::vector<BAMapPoint>& allMapPoints,
                                         const Camera& K, int nIterations = 5, const volatile int32_t* pbStopFlag = nullptr, bool bRobust = true) {
    return BundleAdjustment(c, allKeyFrames, allMapPoints, K, nIterations, pbStopFlag, bRobust);
  }

  // g2o::Sim3 as the 8 doubles of the C ABI (qx qy qz qw tx ty tz s), with the three operations the gather of OptimizeEssentialGraph
  // needs, in f64 on the host: Sim3(R, t, s) (Eigen's Quaterniond(Matrix3d), not renormalised), inverse() and operator* (sim3.h:64-67,
  // :237-240, :270-276)
  struct Sim3 {
    double v[8] = {0, 0, 0, 1, 0, 0, 0, 1};
    static void rotate(const double* q, const double* p, double* out) {   // Eigen: v + w uv + q x uv, uv = 2 q x v
      double ux = q[1] * p[2] - q[2] * p[1], uy = q[2] * p[0] - q[0] * p[2], uz = q[0] * p[1] - q[1] * p[0];
      ux += ux; uy += uy; uz += uz;
      out[0] = p[0] + q[3] * ux + (q[1] * uz - q[2] * uy);
      out[1] = p[1] + q[3] * uy + (q[2] * ux - q[0] * uz);
      out[2] = p[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
    }
    static Sim3 fromTcw(const float* T) {   // Converter::toMatrix3d / toVector3d of a float pose, then Sim3(Rcw, tcw, 1.0) (:783-785)
      double R[9];
      for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[3 * r + c] = T[4 * r + c];
      Sim3 o;
      double* q = o.v;
      double t = R[0] + R[4] + R[8];
      if (t > 0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
      } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R[3 * k + j] - R[3 * j + k]) * t;
        q[j] = (R[3 * j + i] + R[3 * i + j]) * t;
        q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
      }
      for (int r = 0; r < 3; ++r) o.v[4 + r] = T[4 * r + 3];
      o.v[7] = 1.0;
      return o;
    }
    Sim3 inverse() const {
      Sim3 o;
      o.v[0] = -v[0]; o.v[1] = -v[1]; o.v[2] = -v[2]; o.v[3] = v[3];
      const double k = -1. / v[7];
      const double p[3] = {k * v[4], k * v[5], k * v[6]};
      rotate(o.v, p, o.v + 4);
      o.v[7] = 1. / v[7];
      return o;
    }
    Sim3 operator*(const Sim3& b) const {
      Sim3 o;
      const double *a = v, *c = b.v;
      o.v[3] = a[3] * c[3] - a[0] * c[0] - a[1] * c[1] - a[2] * c[2];
      o.v[0] = a[3] * c[0] + a[0] * c[3] + a[1] * c[2] - a[2] * c[1];
      o.v[1] = a[3] * c[1] + a[1] * c[3] + a[2] * c[0] - a[0] * c[2];
      o.v[2] = a[3] * c[2] + a[2] * c[3] + a[0] * c[1] - a[1] * c[0];
      double r[3];
      rotate(a, c + 4, r);
      for (int k = 0; k < 3; ++k) o.v[4 + k] = a[7] * r[k] + a[4 + k];
      o.v[7] = a[7] * c[7];
      return o;
    }
  };
  // What Optimizer::OptimizeEssentialGraph reads from a KeyFrame and a MapPoint, flat.  Other keyframes are named by their index in
  // the caller's vector (GetAllKeyFrames(): no bad keyframe -- the reference dereferences a null vertex at :954 for one); the
  // reference's sets of KeyFrame* are walked in the order the vectors list them.
  struct EGKeyFrame {
    unsigned long mnId = 0;
    float Tcw[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // GetPose()
    int parent = -1;                                    // GetParent()
    std::vector<int> children;                          // hasChild()
    std::vector<int> loopEdges;                         // GetLoopEdges()
    std::vector<std::pair<int, int>> covisibles;        // (keyframe, weight) ordered by weight: mvpOrderedConnectedKeyFrames / mvOrderedWeights
    bool hasCorrected = false, hasNonCorrected = false; // CorrectedSim3.find(pKF) / NonCorrectedSim3.find(pKF)
    Sim3 corrected, nonCorrected;
    int GetWeight(int other) const {                    // KeyFrame::GetWeight: 0 for a keyframe that is not connected
      for (const std::pair<int, int>& c : covisibles) if (c.first == other) return c.second;
      return 0;
    }
  };
  struct EGMapPoint {
    bool bad = false;                                   // isBad()
    float Xw[3] = {0, 0, 0};                            // GetWorldPos()
    int refKF = -1;                                     // GetReferenceKeyFrame()
    unsigned long mnCorrectedByKF = 0, mnCorrectedReference = 0;
  };
  typedef std::vector<std::pair<int, std::vector<int>>> EGLoopConnections;   // map<KeyFrame*, set<KeyFrame*>> in the caller's order
  // The flat problem of asd_optimize_essential_graph; rows by ascending mnId, row_of[i] = the row of keyframes[i]
  struct EGProblem {
    std::vector<int> row_of;
    std::vector<double> sim3, e_meas;
    std::vector<uint8_t> fixed;
    std::vector<int32_t> e_i, e_j;
  };
  struct EGResult {   // rc: asd_optimize_essential_graph's, or ASD_ERR_INVALID for a map point whose reference keyframe is not listed
    int rc = ASD_OK, iterations = 0, trials = 0, n_edges = 0;
    double chi2 = 0;
    std::vector<double> sim3;        // [keyframes][8], in the caller's order: the optimised CorrectedSiw
    std::vector<float> Tcw;          // [keyframes][16]: what pKFi->SetPose gets (:963-965)
    std::vector<uint8_t> mp_written; // map point i is not bad
    std::vector<float> Xw;           // [points][3]: what pMP->SetWorldPos gets (:995-996); Optimizer::WriteBack hands it to the bank with UpdateNormalAndDepth (:998)
  };
  // The vertices and edges of :765-939, without a device: vScw (CorrectedSim3 where present, else (Rcw, tcw, 1)), pLoopKF fixed, then
  // the LoopConnections edges (minFeat = 100 with the pCurKF <-> pLoopKF exemption of :819) and per keyframe -- in the vector's order --
  // its spanning-tree edge, its loop edges towards smaller ids and its covisibility edges (weight >= minFeat, not the parent, not a
  // child, not a loop edge, smaller id, not in sInsertedEdges).  Each end's pose is the NonCorrectedSim3 where present; Sji = Sjw * Swi.
  static EGProblem EssentialGraphProblem(const std::vector<EGKeyFrame>& keyframes, int pLoopKF, int pCurKF, const EGLoopConnections& LoopConnections) {
    const int nKF = (int)keyframes.size();
    EGProblem p;
    std::vector<int> order(nKF);
    for (int i = 0; i < nKF; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return keyframes[a].mnId < keyframes[b].mnId; });
    p.row_of.assign(nKF, -1);
    for (int r = 0; r < nKF; ++r) p.row_of[order[r]] = r;
    std::vector<Sim3> vScw(nKF);
    p.sim3.assign((size_t)nKF * 8, 0.0); p.fixed.assign(nKF, 0);
    for (int i = 0; i < nKF; ++i) {
      vScw[i] = keyframes[i].hasCorrected ? keyframes[i].corrected : Sim3::fromTcw(keyframes[i].Tcw);   // :774-788
      for (int k = 0; k < 8; ++k) p.sim3[(size_t)p.row_of[i] * 8 + k] = vScw[i].v[k];
      if (i == pLoopKF) p.fixed[p.row_of[i]] = 1;                                                        // :790-791
    }
    auto add = [&](int i, int j, const Sim3& Sji) {
      p.e_i.push_back(p.row_of[i]); p.e_j.push_back(p.row_of[j]);
      p.e_meas.insert(p.e_meas.end(), Sji.v, Sji.v + 8);
    };
    const int minFeat = 100;
    std::vector<std::pair<unsigned long, unsigned long>> sInsertedEdges;
    auto id_pair = [&](int a, int b) { return std::make_pair(std::min(keyframes[a].mnId, keyframes[b].mnId), std::max(keyframes[a].mnId, keyframes[b].mnId)); };
    for (const std::pair<int, std::vector<int>>& mit : LoopConnections) {                                // :808-836
      const int i = mit.first;
      const Sim3 Swi = vScw[i].inverse();
      for (int j : mit.second) {
        if ((keyframes[i].mnId != keyframes[pCurKF].mnId || keyframes[j].mnId != keyframes[pLoopKF].mnId) && keyframes[i].GetWeight(j) < minFeat) continue;
        add(i, j, vScw[j] * Swi);
        sInsertedEdges.push_back(id_pair(i, j));
      }
    }
    for (int i = 0; i < nKF; ++i) {                                                                      // :839-939
      const EGKeyFrame& kf = keyframes[i];
      const Sim3 Swi = (kf.hasNonCorrected ? kf.nonCorrected : vScw[i]).inverse();
      auto Sw = [&](int j) { return keyframes[j].hasNonCorrected ? keyframes[j].nonCorrected : vScw[j]; };
      if (kf.parent >= 0) add(i, kf.parent, Sw(kf.parent) * Swi);
      for (int l : kf.loopEdges)
        if (keyframes[l].mnId < kf.mnId) add(i, l, Sw(l) * Swi);
      for (const std::pair<int, int>& c : kf.covisibles) {
        if (c.second < minFeat) break;                                                                   // GetCovisiblesByWeight(minFeat)
        const int n = c.first;
        if (n == kf.parent || std::find(kf.children.begin(), kf.children.end(), n) != kf.children.end() ||
            std::find(kf.loopEdges.begin(), kf.loopEdges.end(), n) != kf.loopEdges.end())
          continue;
        if (!(keyframes[n].mnId < kf.mnId)) continue;
        if (std::find(sInsertedEdges.begin(), sInsertedEdges.end(), id_pair(i, n)) != sInsertedEdges.end()) continue;
        add(i, n, Sw(n) * Swi);
      }
    }
    return p;
  }
  // void static OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const KeyFrameAndPose& NonCorrectedSim3,
  //                                    const KeyFrameAndPose& CorrectedSim3, const map<KeyFrame*, set<KeyFrame*>>& LoopConnections,
  //                                    const bool& bFixScale)  (Optimizer.cc:737-1000) over asd_optimize_essential_graph: the gather
  // above, the one call, and what :947-999 write back.  The two Sim3 maps are the hasCorrected / hasNonCorrected fields of the views.
  static EGResult OptimizeEssentialGraph(Context& c, const std::vector<EGKeyFrame>& keyframes, const std::vector<EGMapPoint>& points, int pLoopKF,
                                         int pCurKF, const EGLoopConnections& LoopConnections, bool bFixScale, int nIterations = 20) {
    EGResult out;
    const int nKF = (int)keyframes.size(), nMP = (int)points.size();
    EGProblem p = EssentialGraphProblem(keyframes, pLoopKF, pCurKF, LoopConnections);
    std::vector<int32_t> mp_ref;
    std::vector<float> X;
    std::vector<int> mp_of;
    std::vector<std::pair<unsigned long, int>> kf_of_id(nKF);   // mnCorrectedReference is an mnId: sorted once, looked up per point
    for (int k = 0; k < nKF; ++k) kf_of_id[k] = std::make_pair(keyframes[k].mnId, k);
    std::sort(kf_of_id.begin(), kf_of_id.end());
    for (int i = 0; i < nMP; ++i) {                                                                      // :969-985
      if (points[i].bad) continue;
      int r = points[i].refKF;
      if (points[i].mnCorrectedByKF == keyframes[pCurKF].mnId) {
        const auto it = std::lower_bound(kf_of_id.begin(), kf_of_id.end(), std::make_pair(points[i].mnCorrectedReference, 0));
        r = it != kf_of_id.end() && it->first == points[i].mnCorrectedReference ? it->second : -1;
      }
      if (r < 0 || r >= nKF) { out.rc = ASD_ERR_INVALID; return out; }   // the reference keyframe is not among the keyframes
      mp_of.push_back(i); mp_ref.push_back(p.row_of[r]);
      X.insert(X.end(), points[i].Xw, points[i].Xw + 3);
    }
    std::vector<float> T((size_t)nKF * 16 + 1);
    std::vector<double> edge_chi2(p.e_i.size() + 1);
    asd_essgraph_problem pr{};
    pr.n_kf = nKF; pr.n_edges = (int32_t)p.e_i.size();
    pr.sim3 = p.sim3.data(); pr.fixed = p.fixed.data(); pr.e_i = p.e_i.data(); pr.e_j = p.e_j.data(); pr.e_meas = p.e_meas.data();
    pr.fix_scale = bFixScale; pr.n_iterations = nIterations;
    pr.Tcw_out = T.data(); pr.n_mp = (int32_t)mp_of.size(); pr.mp_ref = mp_ref.data(); pr.mp_Xw = X.data();
    asd_essgraph_result res{};
    res.edge_chi2 = edge_chi2.data();
    out.n_edges = pr.n_edges;
    out.rc = asd_optimize_essential_graph(c.get(), &pr, &res);
    if (out.rc != ASD_OK) return out;
    out.iterations = res.iterations; out.trials = res.trials; out.chi2 = res.chi2;
    out.sim3.assign((size_t)nKF * 8, 0.0); out.Tcw.assign((size_t)nKF * 16, 0.f);
    out.mp_written.assign(nMP, 0); out.Xw.assign((size_t)nMP * 3, 0.f);
    for (int i = 0; i < nKF; ++i) {
      for (int k = 0; k < 8; ++k) out.sim3[(size_t)i * 8 + k] = p.sim3[(size_t)p.row_of[i] * 8 + k];
      for (int k = 0; k < 16; ++k) out.Tcw[(size_t)i * 16 + k] = T[(size_t)p.row_of[i] * 16 + k];
    }
    for (size_t q = 0; q < mp_of.size(); ++q) {
      out.mp_written[mp_of[q]] = 1;
      for (int k = 0; k < 3; ++k) out.Xw[(size_t)mp_of[q] * 3 + k] = X[3 * q + k];
    }
    return out;
  }

  // void static LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap)  (Optimizer.cc:415): the
  // caller gathers local / fixed keyframes and map points exactly as :423-467 and hands them over flat;
  // on return it applies the erase policy of :652-700 from edge_chi2 / edge_depth_pos.
  static int LocalBundleAdjustment(Context& c, asd_ba_problem* problem, asd_ba_result* result, const bool* pbStopFlag = nullptr) {
    if (pbStopFlag && *pbStopFlag) return 0;  // :595-597
    return asd_local_ba(c.get(), problem, result);
  }

  // The write-back of LocalBundleAdjustment (Optimizer.cc:718-732), BundleAdjustment (:196-228) and OptimizeEssentialGraph (:960-999) over the
  // resident tables: pKF->SetPose for the keyframes (their new camera centres, asd_map_kf_centers), then pMP->SetWorldPos and
  // pMP->UpdateNormalAndDepth for the points (asd_update_normal_and_depth with Xw) -- two calls, and the attribute bank is current.  Ow
  // [kfIds][3] = KeyFrame::GetCameraCenter() after SetPose, Xw [rows][3], refKFs = mpRefKF->mnId per point.  status (may be null): per
  // point 0 updated, 1 bad, 2 no observations, 3 mpRefKF does not observe it (include/asd_slam.h).
  static int WriteBack(Context& c, const std::vector<int32_t>& kfIds, const std::vector<float>& Ow, const std::vector<int32_t>& rows,
                       const std::vector<int32_t>& refKFs, const std::vector<float>& Xw, std::vector<uint8_t>* status = nullptr) {
    if (Ow.size() != 3 * kfIds.size() || refKFs.size() != rows.size() || Xw.size() != 3 * rows.size()) return ASD_ERR_INVALID;
    const int rc = asd_map_kf_centers(c.get(), (int32_t)kfIds.size(), kfIds.data(), Ow.data());
    if (rc != ASD_OK) return rc;
    if (status) status->assign(rows.size(), 0);
    asd_normal_depth_args a{};
    a.n = (int32_t)rows.size(); a.rows = rows.data(); a.ref_kf = refKFs.data(); a.Xw = Xw.data();
    a.status = status ? status->data() : nullptr;
    return asd_update_normal_and_depth(c.get(), &a);
  }

  // The lists and edges of LocalBundleAdjustment (Optimizer.cc:418-467, :484-593) over the resident observation table -- the caller keeps
  // no mObservations for it.  kf = pKF->mnId, neigh = pKF->GetVectorCovisibleKeyFrames() as ids in its order.
  struct LocalBAGraph {
    int rc = ASD_OK;
    std::vector<int32_t> lLocalKeyFrames, lLocalMapPoints, lFixedCameras;   // ids, bank rows, ids
    std::vector<int32_t> pose_kfs, point_rank;                              // asd_ba_problem's pose order; per local point its index in the point order
    std::vector<uint8_t> pose_fixed;                                        // 1 = member of lFixedCameras
    std::vector<int32_t> e_point, e_pose, e_kf, e_idx;                      // the edges in insertion order (:534-593)
    std::vector<uint8_t> e_octave;
    std::vector<double> Xw;                                                 // [points][3] in point order (with wantXw)
  };
  static LocalBAGraph LocalBundleAdjustmentGraph(Context& c, int32_t kf, const std::vector<int32_t>& neigh, bool wantXw = false) {
    LocalBAGraph G;
    int32_t cap[5] = {(int32_t)neigh.size() + 1, 4096, 64, (int32_t)neigh.size() + 65, 16384};
    for (int attempt = 0; attempt < 2; ++attempt) {   // repeated once with the counts the library asked for
      G.lLocalKeyFrames.assign(cap[0], 0); G.lLocalMapPoints.assign(cap[1], 0); G.point_rank.assign(cap[1], 0); G.lFixedCameras.assign(cap[2], 0);
      G.pose_kfs.assign(cap[3], 0); G.pose_fixed.assign(cap[3], 0);
      G.e_point.assign(cap[4], 0); G.e_pose.assign(cap[4], 0); G.e_kf.assign(cap[4], 0); G.e_idx.assign(cap[4], 0); G.e_octave.assign(cap[4], 0);
      G.Xw.assign(wantXw ? 3 * (size_t)cap[1] + 1 : 0, 0.0);
      asd_ba_graph_args a{};
      a.kf = kf; a.n_neigh = (int32_t)neigh.size(); a.neigh = neigh.data();
      a.kf_capacity = cap[0]; a.local_kfs = G.lLocalKeyFrames.data();
      a.point_capacity = cap[1]; a.local_rows = G.lLocalMapPoints.data(); a.point_rank = G.point_rank.data();
      a.fixed_capacity = cap[2]; a.fixed_kfs = G.lFixedCameras.data();
      a.pose_capacity = cap[3]; a.pose_kfs = G.pose_kfs.data(); a.pose_fixed = G.pose_fixed.data();
      a.edge_capacity = cap[4]; a.e_point = G.e_point.data(); a.e_pose = G.e_pose.data(); a.e_kf = G.e_kf.data(); a.e_idx = G.e_idx.data();
      a.e_octave = G.e_octave.data();
      a.Xw = wantXw ? G.Xw.data() : nullptr;
      G.rc = asd_local_ba_graph(c.get(), &a);
      const int32_t need[5] = {a.n_local_kfs, a.n_points, a.n_fixed, a.n_poses, a.n_edges};
      if (G.rc == ASD_ERR_CAPACITY && attempt == 0 && need[0] > 0) { for (int k = 0; k < 5; ++k) cap[k] = need[k]; continue; }
      if (G.rc != ASD_OK) for (int k = 0; k < 5; ++k) cap[k] = 0;
      else for (int k = 0; k < 5; ++k) cap[k] = need[k];
      break;
    }
    G.lLocalKeyFrames.resize(cap[0]); G.lLocalMapPoints.resize(cap[1]); G.point_rank.resize(cap[1]); G.lFixedCameras.resize(cap[2]);
    G.pose_kfs.resize(cap[3]); G.pose_fixed.resize(cap[3]);
    G.e_point.resize(cap[4]); G.e_pose.resize(cap[4]); G.e_kf.resize(cap[4]); G.e_idx.resize(cap[4]); G.e_octave.resize(cap[4]);
    G.Xw.resize(wantXw ? 3 * (size_t)cap[1] : 0);
    return G;
  }

  // What LocalBundleAdjustment leaves behind, for the caller's own objects: the local keyframes' poses, the points' positions and seats.
  struct LocalBAResult {
    int rc = ASD_OK;
    bool stopped = false;             // pbStopFlag was set at :597: nothing was optimised and nothing written
    bool second_round = true;         // false: pbStopFlag was set at :606 (bDoMore = false)
    LocalBAGraph graph;
    std::vector<uint8_t> erase;       // per edge: chi2 > 5.991 || !isDepthPositive (:664)
    int32_t n_erased = 0;
    std::vector<int32_t> bad_rows;    // the points EraseObservation turned bad, in the order it happened
    std::vector<float> Tcw, Ow;       // [lLocalKeyFrames][16], [..][3]: pKF->SetPose(Converter::toCvMat(SE3quat)) (:701-707)
    std::vector<int32_t> rows, mpRefKF;   // the points written back (:712-732: not GetGlobalMapFlag()), their seats after the erasures
    std::vector<float> Xw;            // [rows][3]: pMP->SetWorldPos
    std::vector<uint8_t> status;      // asd_update_normal_and_depth's: 1 for a point that just turned bad
    asd_ba_result ba{};
  };
  // void static LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap)  (Optimizer.cc:415-734) over the resident tables: graph ->
  // asd_ba_problem -> asd_local_ba -> erase policy (asd_local_ba_apply) -> WriteBack.  `view` is the caller's map:
  //   const float* Tcw(int32_t kf)      pKFi->GetPose(), 16 floats           bool fixed(int32_t kf)     pKFi->GetGlobalMapFlag() (:490)
  //   const float* keysUn(int32_t kf)   mvKeysUn[i].pt as [N][2]            const float* K()           fx, fy, cx, cy (:581-584)
  //   bool global(int32_t row)          pMP->GetGlobalMapFlag()              int32_t refKF(int32_t row) mpRefKF->mnId
  //   bool inTable(int32_t kf)          the caller has put the keyframe into the observation table (a neighbour it has not is legal)
  // The stop flag is read where the reference reads it: at :597 in front of the optimisation, and at :606 behind the first round -- for
  // that the two rounds run as two asd_local_ba calls (5 + 0 and 0 + 10 iterations: a round without iterations leaves the estimate as it
  // is), which is done only when a flag is given.  The caller assigns Tcw, Xw, mpRefKF and the bad flags of bad_rows to its own objects.
  template <class View>
  static LocalBAResult LocalBundleAdjustment(Context& c, int32_t kf, const std::vector<int32_t>& neigh, const View& view, const bool* pbStopFlag = nullptr) {
    LocalBAResult R;
    R.graph = LocalBundleAdjustmentGraph(c, kf, neigh, true);
    const LocalBAGraph& G = R.graph;
    if ((R.rc = G.rc) != ASD_OK) return R;
    const size_t P = G.pose_kfs.size(), L = G.lLocalMapPoints.size(), E = G.e_kf.size();
    float scale[ASD_MAX_LEVELS], inv_scale[ASD_MAX_LEVELS], sigma2[ASD_MAX_LEVELS], inv_sigma2[ASD_MAX_LEVELS];
    int32_t per_level[ASD_MAX_LEVELS];
    if ((R.rc = asd_get_scale_tables(c.get(), scale, inv_scale, sigma2, inv_sigma2, per_level)) != ASD_OK) return R;
    std::vector<double> poses(7 * P + 1), points(G.Xw), e_obs(2 * E + 1), e_info(E + 1), chi2(E + 1);
    std::vector<uint8_t> fixed(P + 1), dpos(E + 1), out1(E + 1);
    std::vector<int32_t> row_of_rank(L + 1);
    for (size_t i = 0; i < L; ++i) row_of_rank[G.point_rank[i]] = G.lLocalMapPoints[i];
    for (size_t i = 0; i < P; ++i) {
      asd_tcw_to_pose7(view.Tcw(G.pose_kfs[i]), poses.data() + 7 * i);                                           // :488, :501
      fixed[i] = G.pose_fixed[i] || G.pose_kfs[i] == 0 || view.fixed(G.pose_kfs[i]);                             // :490, :503
    }
    for (size_t e = 0; e < E; ++e) {
      const float* pt = view.keysUn(G.e_kf[e]) + 2 * (size_t)G.e_idx[e];
      e_obs[2 * e] = pt[0]; e_obs[2 * e + 1] = pt[1];                                                            // :563
      const float invSigma2 = inv_sigma2[G.e_octave[e]];
      e_info[e] = view.global(row_of_rank[G.e_point[e]]) ? 10.0 * (double)invSigma2 : (double)invSigma2;         // :570-575
    }
    if (pbStopFlag && *pbStopFlag) { R.stopped = true; return R; }                                               // :597-599
    asd_ba_problem pr{};
    pr.n_poses = (int32_t)P; pr.n_points = (int32_t)L; pr.n_edges = (int32_t)E;
    pr.poses = poses.data(); pr.fixed = fixed.data(); pr.points = points.data();
    pr.e_point = G.e_point.data(); pr.e_pose = G.e_pose.data(); pr.e_obs = e_obs.data(); pr.e_info = e_info.data();
    for (int k = 0; k < 4; ++k) pr.K[k] = view.K()[k];
    R.ba.edge_chi2 = chi2.data(); R.ba.edge_depth_pos = dpos.data(); R.ba.edge_outlier1 = out1.data();
    if (!pbStopFlag) {
      pr.its_first = 5; pr.its_second = 10;                                                                      // :602, :648
      if ((R.rc = asd_local_ba(c.get(), &pr, &R.ba)) != ASD_OK) return R;
    } else {
      pr.its_first = 5; pr.its_second = 0;
      if ((R.rc = asd_local_ba(c.get(), &pr, &R.ba)) != ASD_OK) return R;
      if (*pbStopFlag) R.second_round = false;                                                                   // :606-608
      else {
        const double chi2_first = R.ba.chi2_first;
        const int32_t iters_first = R.ba.iters_first;
        pr.its_first = 0; pr.its_second = 10;
        if ((R.rc = asd_local_ba(c.get(), &pr, &R.ba)) != ASD_OK) return R;
        R.ba.chi2_first = chi2_first; R.ba.iters_first = iters_first;
      }
    }
    R.ba.edge_chi2 = nullptr; R.ba.edge_depth_pos = nullptr; R.ba.edge_outlier1 = nullptr;   // (they pointed into this function's vectors)
    R.erase.assign(E, 0);
    for (size_t e = 0; e < E; ++e) R.erase[e] = chi2[e] > 5.991 || !dpos[e];                                     // :664
    std::vector<int32_t> new_ref(L + 1), bad(65);
    asd_ba_apply_args ap{};
    ap.n_edges = (int32_t)E; ap.erase = R.erase.data(); ap.apply = 1; ap.n_points = (int32_t)L; ap.new_ref = new_ref.data();
    ap.bad_capacity = 64; ap.bad_rows = bad.data();
    R.rc = asd_local_ba_apply(c.get(), &ap);
    if (R.rc == ASD_ERR_CAPACITY && ap.n_bad > ap.bad_capacity) {
      bad.assign((size_t)ap.n_bad + 1, 0);
      ap.bad_capacity = ap.n_bad; ap.bad_rows = bad.data();
      R.rc = asd_local_ba_apply(c.get(), &ap);
    }
    if (R.rc != ASD_OK) return R;
    R.n_erased = ap.n_erased;
    R.bad_rows.assign(bad.begin(), bad.begin() + ap.n_bad);
    // mpRefKF is re-seated when its own observation was erased (MapPoint.cc:131-132): then it ends at the lowest id left
    std::vector<int32_t> seat(L);
    for (size_t i = 0; i < L; ++i) seat[i] = view.refKF(G.lLocalMapPoints[i]);
    std::vector<int32_t> local_of_rank(L + 1);
    for (size_t i = 0; i < L; ++i) local_of_rank[G.point_rank[i]] = (int32_t)i;
    std::vector<uint8_t> seat_erased(L + 1, 0);
    for (size_t e = 0; e < E; ++e)
      if (R.erase[e] && G.e_kf[e] == seat[local_of_rank[G.e_point[e]]]) seat_erased[local_of_rank[G.e_point[e]]] = 1;
    for (size_t i = 0; i < L; ++i) if (seat_erased[i] && new_ref[i] >= 0) seat[i] = new_ref[i];
    // :701-707, then :712-732
    const size_t nLocal = G.lLocalKeyFrames.size();
    R.Tcw.assign(16 * nLocal, 0.f); R.Ow.assign(3 * nLocal, 0.f);
    for (size_t k = 0; k < nLocal; ++k) {
      const size_t i = std::lower_bound(G.pose_kfs.begin(), G.pose_kfs.end(), G.lLocalKeyFrames[k]) - G.pose_kfs.begin();
      float* T = R.Tcw.data() + 16 * k;
      asd_pose7_to_tcw(poses.data() + 7 * i, T);
      for (int r = 0; r < 3; ++r) R.Ow[3 * k + r] = -(T[r] * T[3] + T[4 + r] * T[7] + T[8 + r] * T[11]);   // Ow = -Rcw.t() * tcw, in f32 (KeyFrame.cc:228-230)
    }
    std::vector<int32_t> table_kfs;   // the centres go to the keyframes the table holds
    std::vector<float> table_Ow;
    for (size_t k = 0; k < nLocal; ++k) {
      if (!view.inTable(G.lLocalKeyFrames[k])) continue;
      table_kfs.push_back(G.lLocalKeyFrames[k]);
      table_Ow.insert(table_Ow.end(), R.Ow.begin() + 3 * k, R.Ow.begin() + 3 * k + 3);
    }
    for (size_t i = 0; i < L; ++i) {
      const int32_t row = G.lLocalMapPoints[i];
      if (view.global(row)) continue;                                                                            // :715-716
      R.rows.push_back(row); R.mpRefKF.push_back(seat[i]);
      for (int k = 0; k < 3; ++k) R.Xw.push_back((float)points[3 * (size_t)G.point_rank[i] + k]);                // Converter::toCvMat(Vector3d): CV_32F
    }
    R.rc = WriteBack(c, table_kfs, table_Ow, R.rows, R.mpRefKF, R.Xw, &R.status);
    return R;
  }
};

// ---- Tracking (Tracking.cc): the two per-frame stages as one submission each ------------------------------------------------
// The reference runs matcher.SearchByProjection and Optimizer::PoseOptimization back to back in TrackWithMotionModel (:664-723)
// and in TrackLocalMap (:725-736 with SearchLocalPoints :803-851); asd_track_motion_model / asd_track_local_points do the pair
// behind one synchronisation and return the same bits as the two calls (tests/test_track_chain.py).
class PnPsolver;
struct Tracking {
  // One pass of the loop of Tracking::Relocalization (:1156-1249) over the live PnPsolvers; defined behind asd::PnPsolver below.
  template <class TailFn>
  static int RelocalizationRound(Context& c, std::vector<PnPsolver*>& vpPnPsolvers, std::vector<bool>& vbDiscarded, int nIterations, TailFn tail);

  // The tail of Tracking::CreateInitialMapMonocular behind GlobalBundleAdjustemnt(mpMap, 20) (Tracking.cc:539-565), on the host:
  // medianDepth = pKFini->ComputeSceneMedianDepth(2) (KeyFrame.cc:909-937: z = Rcw.row(2) . Xw + tz over the keyframe's map points --
  // cv::Mat::dot accumulates the f32 products in double -- sorted, element (n - 1) / 2); false for the reference's "Wrong
  // initialization" (medianDepth < 0 or fewer than 50 tracked points in pKFcur, :542 -- upstream ORB-SLAM2 asks for 100, this
  // reference for 50), else pKFcur's translation and every map point of pKFini times 1 / medianDepth, in f32.  iniPoints[i] = index
  // into Xw of pKFini's map point at keypoint i, -1 = none (GetMapPointMatches: a point listed twice is scaled twice, as there).
  static bool InitialMapScale(const float TcwIni[16], float TcwCur[16], const std::vector<int32_t>& iniPoints, std::vector<float>& Xw,
                              int nTrackedCur, float* medianDepth_out = nullptr, int minTracked = 50) {
    std::vector<float> vDepths;
    for (int32_t l : iniPoints)
      if (l >= 0)
        vDepths.push_back((float)(((double)TcwIni[8] * Xw[3 * l] + (double)TcwIni[9] * Xw[3 * l + 1] + (double)TcwIni[10] * Xw[3 * l + 2]) + (double)TcwIni[11]));
    if (vDepths.empty()) return false;   // (the reference reads vDepths[0] of an empty vector)
    std::sort(vDepths.begin(), vDepths.end());
    const float medianDepth = vDepths[(vDepths.size() - 1) / 2];
    const float invMedianDepth = 1.0f / medianDepth;
    if (medianDepth_out) *medianDepth_out = medianDepth;
    if (medianDepth < 0 || nTrackedCur < minTracked) return false;                                  // :542-548
    for (int r = 0; r < 3; ++r) TcwCur[r * 4 + 3] = TcwCur[r * 4 + 3] * invMedianDepth;             // :551-554
    for (int32_t l : iniPoints)
      if (l >= 0) for (int k = 0; k < 3; ++k) Xw[3 * l + k] = Xw[3 * l + k] * invMedianDepth;       // :557-565
    return true;
  }

  // bool Tracking::TrackWithMotionModel(): Cur.mTcw holds the motion-model prediction on entry (mVelocity * mLastFrame.mTcw, :677).
  // `points` = LastFrame's map points indexed like LastFrame.mvKeysUn (null where there is none).  Writes Cur.mvpMapPoints,
  // Cur.mvbOutlier and Cur.mTcw, discards outliers like :704-719 and returns nmatchesMap >= 10 (:723); *nmatches_out gets the
  // matcher's count of the accepted search.
  static bool TrackWithMotionModel(Context& c, FrameView& Cur, const FrameView& Last, const std::vector<const MapPointView*>& points,
                                   const Camera& K, bool checkOrientation = true, int* nmatches_out = nullptr, int* ninliers_out = nullptr) {
    const int nl = Last.N(), nc = Cur.N();
    std::vector<uint8_t> has(nl, 0), obs(nl, 1);
    std::vector<float> Xw((size_t)nl * 3, 0.f), desc((size_t)nl * ASD_DESC_DIM, 0.f);
    for (int i = 0; i < nl; ++i)
      if (points[i]) {
        has[i] = 1;
        obs[i] = points[i]->nObs > 0;
        for (int k = 0; k < 3; ++k) Xw[3 * i + k] = points[i]->Xw[k];
        for (int k = 0; k < ASD_DESC_DIM; ++k) desc[(size_t)i * ASD_DESC_DIM + k] = points[i]->descriptor[k];
      }
    const float Kv[4] = {K.fx, K.fy, K.cx, K.cy};
    std::vector<int32_t> match(nc, -1);
    std::vector<uint8_t> outl(std::max(nc, 1), 0);
    double pose[7], pose_in[7];
    asd_tcw_to_pose7(Cur.mTcw, pose_in);
    int32_t n = 0, ninl = 0;
    float th = 15.f;                                                   // :673-675 (monocular)
    for (int attempt = 0; attempt < 2; ++attempt, th *= 2) {           // :679-687: a second search with 2*th when fewer than 20 matches
      for (int k = 0; k < 7; ++k) pose[k] = pose_in[k];
      if (asd_track_motion_model(c.get(), Cur.slot, Last.slot, has.data(), Xw.data(), desc.data(), Cur.mTcw, Kv, th, checkOrientation, obs.data(),
                                 pose, match.data(), &n, outl.data(), &ninl) != ASD_OK)
        return false;
      if (n >= 20) break;
    }
    if (nmatches_out) *nmatches_out = n;
    if (ninliers_out) *ninliers_out = ninl;
    Cur.mvpMapPoints.assign(nc, -1);
    Cur.mvbOutlier.assign(nc, 0);
    if (n < 20) return false;                                          // :689-690
    asd_pose7_to_tcw(pose, Cur.mTcw);
    int nmatchesMap = 0;
    for (int j = 0; j < nc; ++j) {
      if (match[j] < 0) continue;
      if (outl[j]) continue;                                           // :708-716: the map point is dropped from the frame
      Cur.mvpMapPoints[j] = Last.mvpMapPoints[match[j]];
      if (points[match[j]]->nObs > 0) ++nmatchesMap;                   // :717-718
    }
    return nmatchesMap >= 10;
  }

  // Tracking::SearchLocalPoints + Optimizer::PoseOptimization (TrackLocalMap's numeric body): `local` = mvpLocalMapPoints not
  // already in the frame, `ids` their map-point ids, `cur_points` the points the frame already holds (indexed like mvKeysUn,
  // null where none).  Returns the inlier count; writes Cur.mvpMapPoints (new matches), mvbOutlier and mTcw.
  static int TrackLocalMap(Context& c, FrameView& Cur, const std::vector<MapPointView>& local, const std::vector<int32_t>& ids,
                           const std::vector<const MapPointView*>& cur_points, const Camera& K, float th = 1.f, float nnratio = 0.8f) {
    const int n = (int)local.size(), nc = Cur.N();
    std::vector<float> Xw((size_t)n * 3), nrm((size_t)n * 3), mind(n), maxd(n), desc((size_t)n * ASD_DESC_DIM), curX((size_t)nc * 3, 0.f);
    std::vector<uint8_t> obs(n, 1), occupied(nc, 0), outl(std::max(nc, 1), 0);
    for (int m = 0; m < n; ++m) {
      for (int k = 0; k < 3; ++k) { Xw[3 * m + k] = local[m].Xw[k]; nrm[3 * m + k] = local[m].normal[k]; }
      mind[m] = local[m].mfMinDistance; maxd[m] = local[m].mfMaxDistance;
      obs[m] = local[m].nObs > 0;
      for (int k = 0; k < ASD_DESC_DIM; ++k) desc[(size_t)m * ASD_DESC_DIM + k] = local[m].descriptor[k];
    }
    for (int j = 0; j < nc; ++j)
      if (cur_points[j]) { occupied[j] = 1; for (int k = 0; k < 3; ++k) curX[3 * j + k] = cur_points[j]->Xw[k]; }
    const float Kv[4] = {K.fx, K.fy, K.cx, K.cy};
    std::vector<int32_t> match(nc, -1);
    double pose[7];
    asd_tcw_to_pose7(Cur.mTcw, pose);
    int32_t nm = 0, ninl = 0;
    if (asd_track_local_points(c.get(), Cur.slot, n, Xw.data(), nrm.data(), mind.data(), maxd.data(), desc.data(), Cur.mTcw, Kv, 0.5f,
                               occupied.data(), curX.data(), th, nnratio, obs.data(), pose, match.data(), &nm, outl.data(), &ninl) != ASD_OK)
      return 0;
    asd_pose7_to_tcw(pose, Cur.mTcw);
    Cur.mvpMapPoints.resize(nc, -1);
    Cur.mvbOutlier.assign(nc, 0);
    for (int j = 0; j < nc; ++j) {
      if (match[j] >= 0) Cur.mvpMapPoints[j] = ids[match[j]];
      Cur.mvbOutlier[j] = outl[j];
    }
    return ninl;
  }

  // void Tracking::UpdateLocalMap() (:871-879 = UpdateLocalKeyFrames :907-1015 + UpdateLocalPoints :881-905) together with the skip
  // loop of SearchLocalPoints (:827-841), over the context's observation table (asd_map_*; INTEGRATION.md says where the map's own
  // methods keep it current).  All views are flat: map points are bank rows, keyframes their mnId.
  struct LocalMap {
    std::vector<int32_t> mvpLocalKeyFrames;     // in: the current list (kept when nobody votes); out: the new one
    int32_t mpReferenceKF = -1;                 // in / out: replaced by pKFmax when somebody voted (:1010-1014)
    std::vector<int32_t> mvpLocalMapPoints;     // out, in order
    std::vector<int32_t> vpSearch;              // out: the points SearchLocalPoints goes on to project, in order; asd_track_local_points_map
                                                // searches exactly these (its match_cur indexes this list)
  };
  // curMapPoints = mCurrentFrame.mvpMapPoints as bank rows after the motion-model stage's outlier drop (-1 = none); seenPoints = the rows
  // of the points that drop stamped with mnLastFrameSeen (:705-707).  Returns asd_update_local_map's status; the library's capacity
  // answer is followed by one repetition with the counts it asked for.
  static int UpdateLocalMap(Context& c, const std::vector<int32_t>& curMapPoints, const std::vector<int32_t>& seenPoints, LocalMap& L,
                            int maxKeyFrames = 80) {
    const std::vector<int32_t> prev = L.mvpLocalKeyFrames;
    std::vector<int32_t> kfs(std::max<size_t>(256, prev.size())), rows(1 << 16), srch(1 << 16);
    asd_local_map_args a{};
    a.n_cur = (int32_t)curMapPoints.size(); a.cur_rows = curMapPoints.data();
    a.n_seen = (int32_t)seenPoints.size(); a.seen_rows = seenPoints.data();
    a.n_prev = (int32_t)prev.size(); a.prev_kfs = prev.data();
    a.max_kfs = maxKeyFrames;
    int rc = ASD_OK;
    for (int attempt = 0; attempt < 2; ++attempt) {
      a.kf_capacity = (int32_t)kfs.size(); a.local_kfs = kfs.data();
      a.row_capacity = (int32_t)rows.size(); a.local_rows = rows.data();
      a.search_capacity = (int32_t)srch.size(); a.search_rows = srch.data();
      rc = asd_update_local_map(c.get(), &a);
      if (rc != ASD_ERR_CAPACITY || (a.n_local_kfs <= 0 && a.n_local <= 0)) break;   // (a capacity answer of another kind carries no counts)
      kfs.resize(std::max<size_t>(kfs.size(), a.n_local_kfs)); rows.resize(std::max<size_t>(rows.size(), a.n_local)); srch.resize(std::max<size_t>(srch.size(), a.n_search));
    }
    if (rc != ASD_OK) return rc;
    L.mvpLocalKeyFrames.assign(kfs.begin(), kfs.begin() + a.n_local_kfs);
    if (a.ref_kf >= 0) L.mpReferenceKF = a.ref_kf;
    L.mvpLocalMapPoints.assign(rows.begin(), rows.begin() + a.n_local);
    L.vpSearch.assign(srch.begin(), srch.begin() + a.n_search);
    return ASD_OK;
  }
};

// ---- KeyFrame (KeyFrame.h; src/vslam/src/KeyFrame.cc) ---------------------------------------------
struct KeyFrame {
  struct Connections {
    int rc = ASD_OK;
    std::vector<int32_t> kfs, weights;                       // mConnectedKeyFrameWeights = KFcounter, ascending id
    std::vector<int32_t> mvpOrderedConnectedKeyFrames, mvOrderedWeights;
    int32_t pKFmax = -1; int nmax = 0;
    // GetBestCovisibilityKeyFrames(10) (KeyFrame.cc:372-379): what asd_map_kf_links takes as `cov`
    std::vector<int32_t> Best(size_t N = 10) const {
      return std::vector<int32_t>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + std::min(N, mvpOrderedConnectedKeyFrames.size()));
    }
  };
  // void KeyFrame::UpdateConnections() (KeyFrame.cc:533-637) for keyframe mnId: KFcounter from the device (asd_map_shared_counts: :541-573),
  // then the reference's rules on the host (:577-636): th = 15, the fall-back to the maximum, sort of (weight, keyframe) pairs ascending
  // and push_front -- so equal weights come out higher id first --, pKFmax as the first strictly larger count in ascending id.  An
  // empty KFcounter changes nothing (:577-578: "This should not happen").  The caller applies AddConnection(this, weight) to the listed
  // keyframes (:605, :617) and the spanning-tree step (:637-646: mpParent = mvpOrderedConnectedKeyFrames.front() on the first connection).
  static Connections UpdateConnections(Context& c, int32_t mnId, int th = 15) {
    Connections R;
    int32_t n = 0;
    std::vector<int32_t> kfs(256), cnt(256);
    R.rc = asd_map_shared_counts(c.get(), mnId, (int32_t)kfs.size(), kfs.data(), cnt.data(), &n);
    if (R.rc == ASD_ERR_CAPACITY && n > (int32_t)kfs.size()) {
      kfs.resize(n); cnt.resize(n);
      R.rc = asd_map_shared_counts(c.get(), mnId, n, kfs.data(), cnt.data(), &n);
    }
    if (R.rc != ASD_OK || n == 0) return R;
    R.kfs.assign(kfs.begin(), kfs.begin() + n);
    R.weights.assign(cnt.begin(), cnt.begin() + n);
    std::vector<std::pair<int, int32_t>> vPairs;
    for (int32_t i = 0; i < n; ++i) {
      if (cnt[i] > R.nmax) { R.nmax = cnt[i]; R.pKFmax = kfs[i]; }
      if (cnt[i] >= th) vPairs.emplace_back(cnt[i], kfs[i]);
    }
    if (vPairs.empty()) vPairs.emplace_back(R.nmax, R.pKFmax);
    std::sort(vPairs.begin(), vPairs.end());
    for (size_t i = vPairs.size(); i-- > 0;) { R.mvpOrderedConnectedKeyFrames.push_back(vPairs[i].second); R.mvOrderedWeights.push_back(vPairs[i].first); }
    return R;
  }

  // void KeyFrame::SetPose(const cv::Mat& Tcw) (KeyFrame.cc:221-235), the part the resident tables keep: Ow = GetCameraCenter() of the
  // keyframes `ids` as the caller's own SetPose computed them ([ids][3], f32).  Batched: LocalBA, GBA and the essential graph rewrite many poses.
  static int SetPose(Context& c, const std::vector<int32_t>& ids, const std::vector<float>& Ow) {
    if (Ow.size() != 3 * ids.size()) return ASD_ERR_INVALID;
    return asd_map_kf_centers(c.get(), (int32_t)ids.size(), ids.data(), Ow.data());
  }
};

// ---- MapPoint (MapPoint.h; src/vslam/src/MapPoint.cc) ---------------------------------------------
struct MapPoint {
  struct NormalAndDepth {
    int rc = ASD_OK;
    std::vector<float> mNormalVector, mfMinDistance, mfMaxDistance;   // [rows][3], [rows], [rows]: what the attribute bank now holds
    std::vector<uint8_t> status;                                      // 0 updated, 1 bad, 2 no observations, 3 mpRefKF does not observe the point
  };
  // void MapPoint::UpdateNormalAndDepth() (MapPoint.cc:361-407) for the points `rows` (bank rows, distinct) with refKFs = mpRefKF->mnId,
  // over the observation table, the keyframes' centres (KeyFrame::SetPose above) and octaves, and the attribute bank, which is rewritten in
  // place.  Xw (null or [rows][3]): MapPoint::SetWorldPos directly in front, as the optimizers' write-backs have it.
  static NormalAndDepth UpdateNormalAndDepth(Context& c, const std::vector<int32_t>& rows, const std::vector<int32_t>& refKFs,
                                             const std::vector<float>* Xw = nullptr) {
    NormalAndDepth R;
    if (refKFs.size() != rows.size() || (Xw && Xw->size() != 3 * rows.size())) { R.rc = ASD_ERR_INVALID; return R; }
    const size_t n = rows.size();
    R.mNormalVector.assign(3 * n, 0.f); R.mfMinDistance.assign(n, 0.f); R.mfMaxDistance.assign(n, 0.f); R.status.assign(n, 0);
    asd_normal_depth_args a{};
    a.n = (int32_t)n; a.rows = rows.data(); a.ref_kf = refKFs.data(); a.Xw = Xw ? Xw->data() : nullptr;
    a.normal = R.mNormalVector.data(); a.min_dist = R.mfMinDistance.data(); a.max_dist = R.mfMaxDistance.data(); a.status = R.status.data();
    R.rc = asd_update_normal_and_depth(c.get(), &a);
    return R;
  }
};

// ---- ORBmatcher::Fuse's side effects and MapPoint::Replace over the observation table (asd_fuse_apply) ----------------------------
// What the reference does with bestIdx (ORBmatcher.cc:939-955, :1065-1079, LoopClosing.cc:540-555, :619-627; MapPoint.cc:206-244), in its
// order, on the context's table: the host keeps no observation lists for it.  From action and other follow, in order, the pairs the host
// owes mpReplaced / IncreaseFound / IncreaseVisible for, and the points whose ComputeDistinctiveDescriptors Replace (and mode 2's
// AddMapPoint branch) calls.
struct FuseOutcome {
  int rc = ASD_OK;
  std::vector<uint8_t> action;                                   // asd_fuse_apply's codes, per candidate
  std::vector<int32_t> other, obsCand, obsOther, nMoved, nDropped;
  int nFused = 0;
  std::vector<int32_t> bestIdx;                                  // what the search half chose (the search-plus-apply forms fill it)
  std::vector<std::pair<int32_t, int32_t>> replaced;             // (loser, winner): loser->Replace(winner), in the reference's order
  std::vector<int32_t> winners;                                  // ComputeDistinctiveDescriptors is due for these, in order
  bool Changed() const { for (const uint8_t a : action) if (a >= 1 && a <= 3) return true; return false; }
};
inline FuseOutcome FuseApply(Context& c, int32_t kfId, int mode, const std::vector<int32_t>& rows, const std::vector<int32_t>& bestIdx, bool apply = true) {
  FuseOutcome R;
  if (rows.size() != bestIdx.size()) { R.rc = ASD_ERR_INVALID; return R; }
  const size_t n = rows.size();
  R.action.assign(n, 0); R.other.assign(n, -1); R.obsCand.assign(n, 0); R.obsOther.assign(n, 0); R.nMoved.assign(n, 0); R.nDropped.assign(n, 0);
  asd_fuse_apply_args a{};
  a.kf = kfId; a.mode = mode; a.n = (int32_t)n; a.cand = rows.data(); a.best_idx = bestIdx.data(); a.apply = apply ? 1 : 0;
  a.action = R.action.data(); a.other = R.other.data(); a.obs_cand = R.obsCand.data(); a.obs_other = R.obsOther.data();
  a.n_moved = R.nMoved.data(); a.n_dropped = R.nDropped.data();
  R.rc = asd_fuse_apply(c.get(), &a);
  if (R.rc != ASD_OK) return R;
  R.nFused = a.n_fused;
  for (size_t i = 0; i < n; ++i) {
    if (R.action[i] == 2) { R.replaced.emplace_back(rows[i], R.other[i]); R.winners.push_back(R.other[i]); }
    else if (R.action[i] == 3) { R.replaced.emplace_back(R.other[i], rows[i]); R.winners.push_back(rows[i]); }
    else if (R.action[i] == 1 && mode == 2) R.winners.push_back(rows[i]);   // LoopClosing.cc:552
  }
  return R;
}
// KeyFrame::GetMapPointMatches() from the table (asd_map_get)
inline int GetMapPointMatches(Context& c, int32_t kfId, std::vector<int32_t>& rows) {
  int32_t n = 0;
  rows.resize(2048);
  int rc = asd_map_get(c.get(), kfId, (int32_t)rows.size(), rows.data(), &n);
  if (rc == ASD_ERR_CAPACITY && n > (int32_t)rows.size()) { rows.resize(n); rc = asd_map_get(c.get(), kfId, n, rows.data(), &n); }
  rows.resize(rc == ASD_OK ? n : 0);
  return rc;
}
// the distinct not-bad points of the keyframes' rows in order (asd_map_points): vpFuseCandidates, the gathering loop of mvpLoopMapPoints
inline int GetMapPointsOf(Context& c, const std::vector<int32_t>& kfs, std::vector<int32_t>& rows) {
  int32_t n = 0;
  rows.resize(65536);
  int rc = asd_map_points(c.get(), (int32_t)kfs.size(), kfs.data(), (int32_t)rows.size(), rows.data(), &n);
  if (rc == ASD_ERR_CAPACITY && n > (int32_t)rows.size()) { rows.resize(n); rc = asd_map_points(c.get(), (int32_t)kfs.size(), kfs.data(), n, rows.data(), &n); }
  rows.resize(rc == ASD_OK ? n : 0);
  return rc;
}

inline int ORBmatcher::FuseSearchInput(Context& c, int32_t kfId, const std::vector<MapPointView>& points, const std::vector<int32_t>& rows,
                                       std::vector<uint8_t>& valid, std::vector<float>& Xw, std::vector<float>& nrm, std::vector<float>& mind,
                                       std::vector<float>& maxd, std::vector<float>& desc) {
  if (points.size() != rows.size()) return ASD_ERR_INVALID;
  std::vector<int32_t> inKF;
  const int rc = GetMapPointMatches(c, kfId, inKF);
  if (rc != ASD_OK) return rc;
  std::sort(inKF.begin(), inKF.end());
  const size_t n = rows.size();
  valid.assign(n, 0); Xw.assign(3 * n, 0.f); nrm.assign(3 * n, 0.f); mind.assign(n, 0.f); maxd.assign(n, 0.f); desc.assign(n * ASD_DESC_DIM, 0.f);
  for (size_t i = 0; i < n; ++i) {
    if (rows[i] < 0 || std::binary_search(inKF.begin(), inKF.end(), rows[i]) || !points[i].descriptor) continue;
    valid[i] = 1;
    for (int k = 0; k < 3; ++k) { Xw[3 * i + k] = points[i].Xw[k]; nrm[3 * i + k] = points[i].normal[k]; }
    mind[i] = points[i].mfMinDistance; maxd[i] = points[i].mfMaxDistance;
    for (int k = 0; k < ASD_DESC_DIM; ++k) desc[i * ASD_DESC_DIM + k] = points[i].descriptor[k];
  }
  return ASD_OK;
}
inline FuseOutcome ORBmatcher::Fuse(Context& c, int32_t kfId, const FrameView& KF, const std::vector<MapPointView>& points,
                                    const std::vector<int32_t>& rows, const Camera& K, float th) {
  FuseOutcome R;
  std::vector<uint8_t> valid;
  std::vector<float> Xw, nrm, mind, maxd, desc;
  if ((R.rc = FuseSearchInput(c, kfId, points, rows, valid, Xw, nrm, mind, maxd, desc)) != ASD_OK) return R;
  const int n = (int)rows.size();
  std::vector<int32_t> bestIdx(n, -1);
  std::vector<float> bd(n);
  const float Kv[4] = {K.fx, K.fy, K.cx, K.cy};
  if (n > 0 && (R.rc = asd_fuse_search(c.get(), KF.slot, n, valid.data(), Xw.data(), nrm.data(), mind.data(), maxd.data(), desc.data(), KF.mTcw, Kv, th,
                                       bestIdx.data(), bd.data())) != ASD_OK)
    return R;
  R = FuseApply(c, kfId, 0, rows, bestIdx, true);
  R.bestIdx = bestIdx;
  return R;
}

// OPTIONAL: Optimizer::LocalBundleAdjustment on the library's lane.  The reference calls it IN LINE (Tracking.cc:797 ->
// LocalMapping::DoMapping, LocalMapping.cc:89; no mapping thread exists in this fork) -- that is asd::Optimizer::LocalBundleAdjustment /
// asd_local_ba.  Submit returns at once (problem / result stay owned by the library), Tracking goes on against the PRE-BA map, Wait
// returns the run's status: upstream ORB-SLAM2's concurrency, a different data dependency from this reference.
struct LocalMapping {
  static int LocalBundleAdjustmentSubmit(Context& c, asd_ba_problem* problem, asd_ba_result* result) { return asd_local_ba_submit(c.get(), problem, result); }
  static int LocalBundleAdjustmentWait(Context& c) { return asd_local_ba_wait(c.get()); }
  static bool Busy(Context& c) { return asd_local_ba_poll(c.get()) == 1; }

  // void LocalMapping::KeyFrameCulling() (LocalMapping.cc:739-809, monocular) over the context's observation table, whose rows carry their
  // keypoints' octaves (asd_map_put_octaves).  cand = mpCurrentKeyFrame->GetVectorCovisibleKeyFrames() as ids in its order; flags per
  // candidate: bit0 = GetGlobalMapFlag(), bit1 = mbNotErase.  The in-loop SetBadFlag's effect on the observations is part of the call
  // (include/asd_slam.h); with apply the table is left as the cull leaves the map.  INTEGRATION.md lists what stays the caller's.
  struct Culling {
    int rc = ASD_OK;
    std::vector<uint8_t> decision;                       // 0 kept, 1 SetBadFlag took effect, 2 mbToBeErased only, 3 skipped
    std::vector<int32_t> nMPs, nRedundantObservations;
    std::vector<int32_t> badPoints;                      // bank rows of the points EraseObservation turned bad, in the order it happened
  };
  static Culling KeyFrameCulling(Context& c, const std::vector<int32_t>& cand, const std::vector<uint8_t>& flags, bool apply) {
    Culling R;
    if (flags.size() != cand.size()) { R.rc = ASD_ERR_INVALID; return R; }
    const size_t n = cand.size();
    R.decision.assign(n, 0); R.nMPs.assign(n, 0); R.nRedundantObservations.assign(n, 0);
    R.badPoints.resize(256);
    asd_kf_culling_args a{};
    a.n_cand = (int32_t)n; a.cand = cand.data(); a.cand_flags = flags.data(); a.apply = apply ? 1 : 0;
    a.decision = R.decision.data(); a.n_mps = R.nMPs.data(); a.n_redundant = R.nRedundantObservations.data();
    for (int attempt = 0; attempt < 2; ++attempt) {
      a.bad_capacity = (int32_t)R.badPoints.size(); a.bad_rows = R.badPoints.data();
      R.rc = asd_keyframe_culling(c.get(), &a);
      if (R.rc != ASD_ERR_CAPACITY || a.n_bad <= a.bad_capacity) break;   // (a capacity answer of another kind carries no count)
      R.badPoints.resize(a.n_bad);
    }
    R.badPoints.resize(R.rc == ASD_OK ? a.n_bad : 0);
    return R;
  }

  // void LocalMapping::MapPointCulling() (:261-297) over mlpRecentAddedMapPoints as flat records, Observations() from the table.  Returns
  // which records to SetBadFlag (the caller does that to its MapPoint and, for the table, asd_map_point_bad and the entries' asd_map_set) and
  // the surviving list.
  static MapPointCullingResult MapPointCulling(Context& c, const std::vector<RecentMapPoint>& recent, int32_t nCurrentKFid) {
    std::vector<int32_t> rows(recent.size()), obs(recent.size());
    for (size_t i = 0; i < recent.size(); ++i) rows[i] = recent[i].row;
    const int rc = asd_map_observations(c.get(), (int32_t)rows.size(), rows.data(), obs.data());
    if (rc != ASD_OK) { MapPointCullingResult R; R.rc = rc; R.recent = recent; return R; }
    return MapPointCullingRule(recent, obs, nCurrentKFid, 2);
  }

  // void LocalMapping::SearchInNeighbors() (:557-636), the part between vpTargetKFs and the tail, in the reference's per-call order
  // (:587-617): vpMapPointMatches from the table once (asd_map_get); per target ORBmatcher::Fuse = search + apply; vpFuseCandidates from
  // the table as those applies left it (asd_map_points); ORBmatcher::Fuse into the current keyframe.  `view` is the caller's map:
  // view.KF(mnId) -> const FrameView& (slot, pose) and view.MP(row) -> MapPointView of a bank row, read anew for every search.
  // onReplaced(winners) is called after every apply that replaced or added something and before the next search, so the caller can
  // refresh the descriptors MapPoint::Replace recomputes.  vpTargetKFs (:563-582) is the caller's: the table's ten links do not hold
  // GetBestCovisibilityKeyFrames(20).  The tail (:620-635) is ComputeDistinctiveDescriptors, asd::MapPoint::UpdateNormalAndDepth and
  // asd::KeyFrame::UpdateConnections.
  struct Neighbors {
    int rc = ASD_OK;
    std::vector<int32_t> vpMapPointMatches, vpFuseCandidates;
    std::vector<FuseOutcome> perTarget;
    FuseOutcome intoCurrent;
  };
  template <class MapView, class ReplacedFn>
  static Neighbors SearchInNeighbors(Context& c, int32_t currentKfId, const std::vector<int32_t>& vpTargetKFs, const MapView& view, ReplacedFn onReplaced,
                                     const Camera& K, float th = 3.f) {
    Neighbors R;
    if ((R.rc = GetMapPointMatches(c, currentKfId, R.vpMapPointMatches)) != ASD_OK) return R;
    auto points_of = [&](const std::vector<int32_t>& rows) {
      std::vector<MapPointView> pts(rows.size(), MapPointView{});
      for (size_t i = 0; i < rows.size(); ++i) if (rows[i] >= 0) pts[i] = view.MP(rows[i]);
      return pts;
    };
    for (const int32_t kf : vpTargetKFs) {                                                   // :588-593
      R.perTarget.push_back(ORBmatcher::Fuse(c, kf, view.KF(kf), points_of(R.vpMapPointMatches), R.vpMapPointMatches, K, th));
      if ((R.rc = R.perTarget.back().rc) != ASD_OK) return R;
      if (!R.perTarget.back().winners.empty()) onReplaced(R.perTarget.back().winners);
    }
    if ((R.rc = GetMapPointsOf(c, vpTargetKFs, R.vpFuseCandidates)) != ASD_OK) return R;    // :599-615
    R.intoCurrent = ORBmatcher::Fuse(c, currentKfId, view.KF(currentKfId), points_of(R.vpFuseCandidates), R.vpFuseCandidates, K, th);   // :617
    R.rc = R.intoCurrent.rc;
    if (R.rc == ASD_OK && !R.intoCurrent.winners.empty()) onReplaced(R.intoCurrent.winners);
    return R;
  }
};

// DBoW2::BowVector as asd_compute_bow hands it out: word ids ascending, one value per word
struct BowVector {
  std::vector<int32_t> id;
  std::vector<double> val;
  int size() const { return (int)id.size(); }
};

// ---- KeyFrameDatabase (KeyFrameDatabase.h; src/vslam/src/KeyFrameDatabase.cc) -----------------
// Keyframes are named by their mnId.  The BowVectors live in HBM inside the context; the reference's per-keyframe query fields
// (mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore) live with them, so the KeyFrame class needs none
// of them any more.  One database per Context.
class KeyFrameDatabase {
 public:
  // KeyFrameDatabase(const ORBVocabulary& voc) (:34-38): scoring -1 = the scoring of the vocabulary loaded with asd_voc_load
  explicit KeyFrameDatabase(Context& c, int scoring = -1) : c_(c) {
    if (asd_kfdb_clear(c_.get(), scoring) != ASD_OK) throw std::runtime_error(c_.error());
    scoring_ = scoring;
  }
  int add(int32_t mnId, const BowVector& mBowVec, bool bGlobalMapFlag) {                                    // :41-47
    return asd_kfdb_add(c_.get(), mnId, mBowVec.size(), mBowVec.id.data(), mBowVec.val.data(), bGlobalMapFlag ? 1 : 0);
  }
  int erase(int32_t mnId) { return asd_kfdb_erase(c_.get(), mnId); }                                        // :49-70
  int clear() { return asd_kfdb_clear(c_.get(), scoring_); }                                                // :72-76
  // vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore, bool only_global_map) (:80-204).  vConnected =
  // pKF->GetConnectedKeyFrames() as ids; neighbours(id) = GetBestCovisibilityKeyFrames(10) of keyframe id, as ids (at most 10 are read)
  template <class NeighboursFn>
  std::vector<int32_t> DetectLoopCandidates(const BowVector& mBowVec, const std::vector<int32_t>& vConnected, float minScore,
                                            bool only_global_map, NeighboursFn neighbours) {
    return run(0, [&](int32_t cap, int32_t* kf, float* sc, int32_t* n) {
      return asd_kfdb_query_loop(c_.get(), mBowVec.size(), mBowVec.id.data(), mBowVec.val.data(), (int32_t)vConnected.size(), vConnected.data(),
                                 minScore, only_global_map ? 1 : 0, cap, kf, sc, n);
    }, neighbours);
  }
  // vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F, bool only_global_map) (:206-322)
  template <class NeighboursFn>
  std::vector<int32_t> DetectRelocalizationCandidates(const BowVector& mBowVec, bool only_global_map, NeighboursFn neighbours) {
    return run(1, [&](int32_t cap, int32_t* kf, float* sc, int32_t* n) {
      return asd_kfdb_query_reloc(c_.get(), mBowVec.size(), mBowVec.id.data(), mBowVec.val.data(), only_global_map ? 1 : 0, cap, kf, sc, n);
    }, neighbours);
  }
 private:
  template <class QueryFn, class NeighboursFn>
  std::vector<int32_t> run(int mode, QueryFn query, NeighboursFn neighbours) {
    int64_t dbg[5] = {0, 0, 0, 0, 0};
    asd_debug_kfdb(c_.get(), dbg);
    const int32_t cap = (int32_t)dbg[0];   // live entries: no list is longer
    std::vector<int32_t> kf(cap + 1), cand(cap + 1);
    std::vector<float> sc(cap + 1);
    int32_t n = 0, nc = 0;
    if (query(cap, kf.data(), sc.data(), &n) != ASD_OK) return {};
    std::vector<int32_t> neigh((size_t)n * 10 + 1, -1);
    for (int32_t i = 0; i < n; ++i) {
      const std::vector<int32_t> v = neighbours(kf[i]);
      for (size_t k = 0; k < v.size() && k < 10; ++k) neigh[(size_t)i * 10 + k] = v[k];
    }
    if (asd_kfdb_select(c_.get(), mode, n, neigh.data(), cap, cand.data(), &nc) != ASD_OK) return {};
    cand.resize(nc);
    return cand;
  }
  Context& c_;
  int scoring_ = -1;
};

// ---- DUtils::Random as Sim3Solver uses it (src/dbow2/DUtils/Random.cpp:47-50) ----------------------------------------------
// A stream of raw rand() values.  The reference calls rand() three times per RANSAC iteration, at the moment the iteration runs; a
// batched iterate() has to draw 3 x nIterations values ahead and, on an early return after iteration k, has used only 3 x (k + 1)
// of them.  The stream therefore takes the unused values back (GiveBack) and hands them out first next time: the sequence of raw
// values the solvers consume is the reference's for the same seed.  The source defaults to ::rand and can be replaced.
class DrawStream {
 public:
  explicit DrawStream(std::function<int()> source = [] { return std::rand(); }, double rand_max = (double)RAND_MAX)
      : source_(std::move(source)), rand_max_(rand_max) {}
  int Next() {
    if (pending_.empty()) return source_();
    const int v = pending_.front();
    pending_.pop_front();
    return v;
  }
  // int RandomInt(int min, int max) of the raw value r: int(((double)r / ((double)RAND_MAX + 1.0)) * d) + min
  int RandomInt(int raw, int min, int max) const {
    const int d = max - min + 1;
    return int(((double)raw / (rand_max_ + 1.0)) * d) + min;
  }
  // raw values taken with Next() and not used, in the order they were taken; they must be the LAST values handed out
  void GiveBack(const int* raw, size_t n) { pending_.insert(pending_.begin(), raw, raw + n); }
  size_t Pending() const { return pending_.size(); }
 private:
  std::function<int()> source_;
  double rand_max_;
  std::deque<int> pending_;
};

// The random numbers of one batched call: K per iteration, drawn ahead of the call and handed to it as the RandomInt values; what the
// call did not consume goes back to the stream.  Sim3Solver, PnPsolver and Initializer draw through it.
class DrawBatch {
 public:
  // n_iter x K calls of stream.Next() in iteration order, draw i of an iteration as RandomInt(0, N - 1 - i) (vAvailableIndices.size() - 1);
  // returns the [n_iter][K] table for the problem's `draws`
  const int32_t* Draw(DrawStream& stream, int n_iter, int K, int N) {
    stream_ = &stream;
    raw_.resize((size_t)K * n_iter);
    randi_.resize((size_t)K * n_iter);
    for (int k = 0; k < n_iter; ++k)
      for (int i = 0; i < K; ++i) {
        raw_[(size_t)K * k + i] = stream.Next();
        randi_[(size_t)K * k + i] = stream.RandomInt(raw_[(size_t)K * k + i], 0, N - 1 - i);
      }
    return randi_.data();
  }
  // the first `used` raw values were consumed: the tail goes back to the stream
  void Keep(size_t used) {
    if (stream_) stream_->GiveBack(raw_.data() + used, raw_.size() - used);
    last_raw_.assign(raw_.begin(), raw_.begin() + used);
    raw_.clear();
  }
  // Draw undone: every random number back to the stream
  void Cancel() {
    if (stream_) stream_->GiveBack(raw_.data(), raw_.size());
    raw_.clear();
  }
  const std::vector<int>& LastRawConsumed() const { return last_raw_; }   // the raw values the last Keep kept (test aid)
 private:
  DrawStream* stream_ = nullptr;
  std::vector<int> raw_, last_raw_;
  std::vector<int32_t> randi_;
};

// ---- Sim3Solver (Sim3Solver.h:36-128; src/vslam/src/Sim3Solver.cc) -----------------------------------------------------------
// The RANSAC iterations run on the device (asd_sim3_ransac); this class keeps what the reference's object keeps between iterate()
// calls: the gathered correspondences, mnIterations, mnBestInliers and the best model.  iterate() = Begin + asd_sim3_ransac + End;
// the two halves are public so that several solvers can share one call (LoopClosing::ComputeSim3 below).
class Sim3Solver {
 public:
  // Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const vector<MapPoint*>& vpMatched12, bool bFixScale)  (:37-112).  vpMatched12[i1] = pKF2's
  // map point id matched to pKF1's keypoint i1 (-1 = NULL), vnIdx2[i1] = its keypoint in pKF2 (pMP2->GetIndexInKeyFrame(pKF2)), as
  // SearchByBoW(KF, KF) leaves them; mvpMapPoints[i] >= 0 stands for "a map point that is not bad", and pMP1->GetIndexInKeyFrame(pKF1) is
  // i1.  vLevelSigma2_1 / _2 = mvLevelSigma2.  mvnMaxError1 / 2 are vector<size_t> in the reference (Sim3Solver.h:78-79), so the
  // 9.210 * sigma2 of :87-88 is stored truncated to an integer and compared as a float (:356): that is what is stored here.
  Sim3Solver(Context& c, const FrameView& KF1, const FrameView& KF2, const std::vector<int32_t>& vpMatched12, const std::vector<int32_t>& vnIdx2,
             const std::vector<MapPointView>& points, const Camera& K1, const Camera& K2, const std::vector<float>& vLevelSigma2_1,
             const std::vector<float>& vLevelSigma2_2, bool bFixScale, DrawStream& draws)
      : ctx_(c.get()), draws_(&draws), mbFixScale(bFixScale), mK1(K1), mK2(K2) {
    mN1 = (int)vpMatched12.size();
    auto to_camera = [](const float* T, const float* X, std::vector<float>& out) {   // Rcw * X3Dw + tcw in f32 (:95, :98)
      for (int r = 0; r < 3; ++r) out.push_back((T[r * 4] * X[0] + T[r * 4 + 1] * X[1] + T[r * 4 + 2] * X[2]) + T[r * 4 + 3]);
    };
    for (int i1 = 0; i1 < mN1; ++i1) {                                                // :62-103
      if (vpMatched12[i1] < 0) continue;
      const int id1 = KF1.mvpMapPoints.size() == (size_t)KF1.N() ? KF1.mvpMapPoints[i1] : -1;
      if (id1 < 0) continue;                                                          // :69-73
      const int indexKF2 = vnIdx2[i1];
      if (indexKF2 < 0) continue;                                                     // :78-79
      const float sigmaSquare1 = vLevelSigma2_1[KF1.mvKeysUn[i1].octave], sigmaSquare2 = vLevelSigma2_2[KF2.mvKeysUn[indexKF2].octave];
      mvnMaxError1.push_back((float)(size_t)(9.210 * sigmaSquare1));                  // :87-88 into vector<size_t>
      mvnMaxError2.push_back((float)(size_t)(9.210 * sigmaSquare2));
      mvnIndices1.push_back((size_t)i1);
      to_camera(KF1.mTcw, points[id1].Xw, mvX3Dc1);
      to_camera(KF2.mTcw, points[vpMatched12[i1]].Xw, mvX3Dc2);
    }
    SetRansacParameters();                                                            // :111
  }
  // the gathered vectors directly (tests, or a caller that gathers itself).  ctx may be null for a solver that is only stepped through
  // Begin / End
  Sim3Solver(asd_ctx* ctx, int N1, std::vector<size_t> vnIndices1, std::vector<float> vX3Dc1, std::vector<float> vX3Dc2,
             std::vector<float> vnMaxError1, std::vector<float> vnMaxError2, const Camera& K1, const Camera& K2, bool bFixScale, DrawStream& draws)
      : ctx_(ctx), draws_(&draws), mbFixScale(bFixScale), mK1(K1), mK2(K2), mN1(N1), mvnIndices1(std::move(vnIndices1)),
        mvX3Dc1(std::move(vX3Dc1)), mvX3Dc2(std::move(vX3Dc2)), mvnMaxError1(std::move(vnMaxError1)), mvnMaxError2(std::move(vnMaxError2)) {
    SetRansacParameters();
  }

  // void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)  (:114-138)
  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    N = (int)mvnIndices1.size();
    mRansacMaxIts = asd_sim3_ransac_max_iterations(N, probability, minInliers, maxIterations);
    mnIterations = 0;
  }

  // cv::Mat iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers)  (:140-207).  Returns true where the reference
  // returns a non-empty mBestT12 (GetEstimatedT12); false with an empty matrix.  A failed device call counts as bNoMore.
  bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    asd_sim3_ransac_problem p;
    if (!Begin(nIterations, p)) { bNoMore = true; vbInliers.assign(mN1, false); nInliers = 0; return false; }
    if (asd_sim3_ransac(ctx_, 1, &p) != ASD_OK) { Cancel(); bNoMore = true; vbInliers.assign(mN1, false); nInliers = 0; return false; }
    return End(p, bNoMore, vbInliers, nInliers);
  }
  // cv::Mat find(vector<bool>& vbInliers12, int& nInliers)  (:209-213)
  bool find(std::vector<bool>& vbInliers12, int& nInliers) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
  }
  const float* GetEstimatedRotation() const { return mBestRotation; }        // row-major 3x3 (:367-370)
  const float* GetEstimatedTranslation() const { return mBestTranslation; }  // (:372-375)
  float GetEstimatedScale() const { return mBestScale; }                     // (:377-380)
  const float* GetEstimatedT12() const { return mBestT12; }                  // mBestT12, row-major 4x4
  const std::vector<size_t>& GetIndices1() const { return mvnIndices1; }
  int GetIterations() const { return mnIterations; }
  int GetBestInliers() const { return mnBestInliers; }
  int GetMaxIterations() const { return mRansacMaxIts; }
  int GetN() const { return N; }

  // The first half of iterate(): fills `p` for asd_sim3_ransac with the iterations the reference's loop would start (:158) and draws
  // their 3 random numbers each from the stream (:168).  false: N < mRansacMinInliers (:146-150, bNoMore), nothing was drawn.
  // p points into this object: it must not be moved or destroyed, nor Begin called again, before End or Cancel.
  bool Begin(int nIterations, asd_sim3_ransac_problem& p) {
    p = asd_sim3_ransac_problem{};
    if (N < mRansacMinInliers) return false;
    const int n_iter = std::max(0, std::min(nIterations, mRansacMaxIts - mnIterations));
    p.draws = batch_.Draw(*draws_, n_iter, 3, N);
    inliers_.assign((size_t)N + 1, 0);
    p.n = N;
    p.X1c = mvX3Dc1.data(); p.X2c = mvX3Dc2.data(); p.max_err1 = mvnMaxError1.data(); p.max_err2 = mvnMaxError2.data();
    const float k1[4] = {mK1.fx, mK1.fy, mK1.cx, mK1.cy}, k2[4] = {mK2.fx, mK2.fy, mK2.cx, mK2.cy};
    for (int i = 0; i < 4; ++i) { p.K1[i] = k1[i]; p.K2[i] = k2[i]; }
    p.fix_scale = mbFixScale; p.min_inliers = mRansacMinInliers; p.n_iter = n_iter;
    p.best_inliers = mnBestInliers;
    p.inliers = inliers_.data();
    return true;
  }
  // The second half: what the iterations changed in the object, the unused random numbers back to the stream, iterate()'s outputs
  bool End(const asd_sim3_ransac_problem& p, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
    bNoMore = false;
    vbInliers.assign(mN1, false);
    nInliers = 0;
    batch_.Keep((size_t)3 * p.iterations_done);
    mnIterations += p.iterations_done;
    mnBestInliers = p.best_inliers;
    if (p.best_updated) {                                                             // :185-190
      for (int i = 0; i < 9; ++i) mBestRotation[i] = p.R12[i];
      for (int i = 0; i < 3; ++i) mBestTranslation[i] = p.t12[i];
      for (int i = 0; i < 16; ++i) mBestT12[i] = p.T12[i];
      mBestScale = p.s12;
    }
    if (p.found) {                                                                    // :192-199
      nInliers = p.n_inliers;
      for (int i = 0; i < N; ++i)
        if (inliers_[i]) vbInliers[mvnIndices1[i]] = true;
      return true;
    }
    if (mnIterations >= mRansacMaxIts) bNoMore = true;                                // :203-204
    return false;
  }
  // Begin undone: every random number back to the stream, the object as it was (the reference would not have called iterate())
  void Cancel() { batch_.Cancel(); }
  const std::vector<int>& LastRawConsumed() const { return batch_.LastRawConsumed(); }   // the raw values the last End kept (test aid)

 private:
  asd_ctx* ctx_;
  DrawStream* draws_;
  bool mbFixScale;
  Camera mK1, mK2;
  int mN1 = 0, N = 0;
  std::vector<size_t> mvnIndices1;
  std::vector<float> mvX3Dc1, mvX3Dc2, mvnMaxError1, mvnMaxError2;
  double mRansacProb = 0.99;
  int mRansacMinInliers = 6, mRansacMaxIts = 300, mnIterations = 0, mnBestInliers = 0;
  float mBestRotation[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, mBestTranslation[3] = {0, 0, 0}, mBestScale = 1.f;
  float mBestT12[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  DrawBatch batch_;
  std::vector<uint8_t> inliers_;
};

// ---- PnPsolver (PnPsolver.h; src/vslam/src/PnPsolver.cc) -----------------------------------------------------------------------
// The EPnP RANSAC iterations run on the device (asd_pnp_ransac); this class keeps what the reference's object keeps between iterate()
// calls: the gathered correspondences, mnIterations, mnBestInliers, mvbBestInliers and mBestTcw.  iterate() = Begin + asd_pnp_ransac +
// End; the two halves are public so that several solvers can share one call (Tracking::RelocalizationRound below).  Four random numbers
// per iteration come from the DrawStream; the unused ones go back in front of the generator.
class PnPsolver {
 public:
  // PnPsolver(const Frame& F, const vector<MapPoint*>& vpMapPointMatches)  (:67-110).  vpMapPointMatches[i] = the map point id matched to
  // F's keypoint i (-1 = NULL; a bad map point is the caller's to leave out, :85), vLevelSigma2 = F.mvLevelSigma2.
  PnPsolver(Context& c, const FrameView& F, const std::vector<int32_t>& vpMapPointMatches, const std::vector<MapPointView>& points, const Camera& K,
            const std::vector<float>& vLevelSigma2, DrawStream& draws)
      : ctx_(c.get()), draws_(&draws), mK(K) {
    mNF = (int)vpMapPointMatches.size();
    for (int i = 0; i < mNF; ++i) {                                                   // :79-101
      if (vpMapPointMatches[i] < 0) continue;
      const asd_keypoint& kp = F.mvKeysUn[i];
      mvP2D.push_back(kp.x); mvP2D.push_back(kp.y);                                   // :89
      mvSigma2.push_back(vLevelSigma2[kp.octave]);                                    // :90
      for (int k = 0; k < 3; ++k) mvP3Dw.push_back(points[vpMapPointMatches[i]].Xw[k]);   // :92-93
      mvKeyPointIndices.push_back((size_t)i);                                         // :95
    }
    SetRansacParameters();                                                            // :109
  }
  // the gathered vectors directly (tests, or a caller that gathers itself).  ctx may be null for a solver that is only stepped through
  // Begin / End
  PnPsolver(asd_ctx* ctx, int NF, std::vector<size_t> vKeyPointIndices, std::vector<float> vP3Dw, std::vector<float> vP2D, std::vector<float> vSigma2,
            const Camera& K, DrawStream& draws)
      : ctx_(ctx), draws_(&draws), mK(K), mNF(NF), mvKeyPointIndices(std::move(vKeyPointIndices)), mvP3Dw(std::move(vP3Dw)), mvP2D(std::move(vP2D)),
        mvSigma2(std::move(vSigma2)) {
    SetRansacParameters();
  }

  // void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4,
  //                          float th2 = 5.991)  (:121-157).  minSet must be 4 (ASD_PNP_MIN_SET): the only value the reference passes
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f,
                           float th2 = 5.991f) {
    N = (int)mvKeyPointIndices.size();
    int32_t mi = minInliers, its = 1;
    asd_pnp_ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon, &mi, &its);
    mRansacMinInliers = mi;
    mRansacMaxIts = its;
    mvMaxError.resize(mvSigma2.size());
    for (size_t i = 0; i < mvSigma2.size(); ++i) mvMaxError[i] = mvSigma2[i] * th2;   // :156, an f32 product
  }

  // cv::Mat iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers)  (:165-258).  Returns true where the reference
  // returns a non-empty matrix, Tcw (row-major 4x4) = mRefinedTcw (:235) or, at the last iteration, mBestTcw (:253).  A failed device call
  // counts as bNoMore.
  bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, float* Tcw) {
    asd_pnp_ransac_problem p;
    if (!Begin(nIterations, p)) { bNoMore = true; vbInliers.clear(); nInliers = 0; return false; }
    if (asd_pnp_ransac(ctx_, 1, &p) != ASD_OK) { Cancel(); bNoMore = true; vbInliers.clear(); nInliers = 0; return false; }
    return End(p, bNoMore, vbInliers, nInliers, Tcw);
  }
  // cv::Mat find(vector<bool>& vbInliers, int& nInliers)  (:159-163)
  bool find(std::vector<bool>& vbInliers, int& nInliers, float* Tcw) {
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers, Tcw);
  }
  int GetIterations() const { return mnIterations; }
  int GetBestInliers() const { return mnBestInliers; }
  int GetMaxIterations() const { return mRansacMaxIts; }
  int GetMinInliers() const { return mRansacMinInliers; }
  int GetN() const { return N; }
  const float* GetBestTcw() const { return mBestTcw; }
  const std::vector<size_t>& GetKeyPointIndices() const { return mvKeyPointIndices; }

  // The first half of iterate(): fills `p` for asd_pnp_ransac and draws the 4 random numbers of every iteration the call may run from the
  // stream (:193).  The loop condition of :182 joins its two limits with OR -- mnIterations < mRansacMaxIts || nCurrentIterations <
  // nIterations -- so a call that returns no refined model runs max(nIterations, mRansacMaxIts - mnIterations) iterations.  false:
  // N < mRansacMinInliers (:173-177, bNoMore), nothing was drawn.  p points into this object: it must not be moved or destroyed, nor Begin
  // called again, before End or Cancel.
  bool Begin(int nIterations, asd_pnp_ransac_problem& p) {
    p = asd_pnp_ransac_problem{};
    if (N < mRansacMinInliers) return false;
    const int n_iter = std::max(0, std::max(nIterations, mRansacMaxIts - mnIterations));
    p.draws = batch_.Draw(*draws_, n_iter, 4, N);
    inliers_.assign((size_t)N + 1, 0);
    best_mask_.assign((size_t)N + 1, 0);
    p.n = N;
    p.P3Dw = mvP3Dw.data(); p.P2D = mvP2D.data(); p.max_err = mvMaxError.data();
    p.K[0] = mK.fx; p.K[1] = mK.fy; p.K[2] = mK.cx; p.K[3] = mK.cy;
    p.min_inliers = mRansacMinInliers; p.n_iter = n_iter;
    p.best_inliers = mnBestInliers;
    p.best_mask = best_mask_.data();
    p.inliers = inliers_.data();
    return true;
  }
  // The second half: what the iterations changed in the object, the unused random numbers back to the stream, iterate()'s outputs.
  // `problem` = the position of p in the asd_pnp_ransac call that ran it.
  // A solver that is iterated again after it returned its refined model (Relocalization does that when the tail turns the pose down and
  // bNoMore is not set): the reference calls Refine() at the next iteration that passes :209; where that iteration does not beat the best
  // model, Refine() runs on the same mvbBestInliers, succeeds again and the same refined model comes back at that iteration.  The device's
  // walk knows no Refine of an earlier call, so this case is settled here from the iteration counts of the call (asd_debug_pnp_ransac).
  bool End(const asd_pnp_ransac_problem& p, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, float* Tcw, int problem = 0) {
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;
    int done = p.iterations_done;
    bool again = false;
    if (refined_ok_ && ctx_)
      for (int k = 0; k < p.iterations_done; ++k) {
        asd_pnp_ransac_debug d;
        if (asd_debug_pnp_ransac(ctx_, problem, k, &d) != ASD_OK) break;
        if (d.count < mRansacMinInliers) continue;                                    // :209
        if (d.count <= mnBestInliers) { again = true; done = k + 1; }                 // :212 not taken, :226 on the same set
        break;
      }
    batch_.Keep((size_t)4 * done);
    mnIterations += done;
    if (again) {
      nInliers = mnRefinedInliers;
      vbInliers.assign(mNF, false);
      for (int i = 0; i < N; ++i)
        if (mvbRefinedInliers[i]) vbInliers[mvKeyPointIndices[i]] = true;
      for (int i = 0; i < 16; ++i) Tcw[i] = mRefinedTcw[i];
      return true;
    }
    mnBestInliers = p.best_inliers;
    if (p.best_updated) {                                                             // :214-223; otherwise the previous mask and matrix stay
      mvbBestInliers.assign(best_mask_.begin(), best_mask_.begin() + N);
      for (int i = 0; i < 16; ++i) mBestTcw[i] = p.best_Tcw[i];
      refined_ok_ = false;                                                            // its Refine failed, unless found says otherwise
    }
    if (p.found) {                                                                    // :226-236
      refined_ok_ = true;
      mnRefinedInliers = p.n_inliers;
      mvbRefinedInliers.assign(inliers_.begin(), inliers_.begin() + N);
      for (int i = 0; i < 16; ++i) mRefinedTcw[i] = p.Tcw[i];
      nInliers = p.n_inliers;
      vbInliers.assign(mNF, false);
      for (int i = 0; i < N; ++i)
        if (inliers_[i]) vbInliers[mvKeyPointIndices[i]] = true;
      for (int i = 0; i < 16; ++i) Tcw[i] = p.Tcw[i];
      return true;
    }
    if (mnIterations >= mRansacMaxIts) {                                              // :241-255 (always true behind the loop of :182)
      bNoMore = true;
      if (mnBestInliers >= mRansacMinInliers && (int)mvbBestInliers.size() == N) {
        nInliers = mnBestInliers;
        vbInliers.assign(mNF, false);
        for (int i = 0; i < N; ++i)
          if (mvbBestInliers[i]) vbInliers[mvKeyPointIndices[i]] = true;
        for (int i = 0; i < 16; ++i) Tcw[i] = mBestTcw[i];
        return true;
      }
    }
    return false;
  }
  // whether End(p, ..., problem) will consume fewer iterations than p supplied (the solvers behind it in a shared call then drew numbers
  // that are not theirs)
  bool ReturnsEarly(const asd_pnp_ransac_problem& p, int problem = 0) const {
    if (p.found && p.iterations_done < p.n_iter) return true;
    if (refined_ok_ && ctx_)
      for (int k = 0; k < p.iterations_done; ++k) {
        asd_pnp_ransac_debug d;
        if (asd_debug_pnp_ransac(ctx_, problem, k, &d) != ASD_OK) break;
        if (d.count < mRansacMinInliers) continue;
        return d.count <= mnBestInliers && k + 1 < p.n_iter;
      }
    return false;
  }
  // Begin undone: every random number back to the stream, the object as it was (the reference would not have called iterate())
  void Cancel() { batch_.Cancel(); }
  const std::vector<int>& LastRawConsumed() const { return batch_.LastRawConsumed(); }   // the raw values the last End kept (test aid)

 private:
  asd_ctx* ctx_;
  DrawStream* draws_;
  Camera mK;
  int mNF = 0, N = 0;
  std::vector<size_t> mvKeyPointIndices;
  std::vector<float> mvP3Dw, mvP2D, mvSigma2, mvMaxError;
  int mRansacMinInliers = 8, mRansacMaxIts = 300, mnIterations = 0, mnBestInliers = 0;
  std::vector<uint8_t> mvbBestInliers, mvbRefinedInliers;
  float mBestTcw[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, mRefinedTcw[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  int mnRefinedInliers = 0;
  bool refined_ok_ = false;   // Refine() on the present mvbBestInliers succeeded (an earlier call returned its model)
  DrawBatch batch_;
  std::vector<uint8_t> inliers_, best_mask_;
};

// One pass of the loop of Tracking::Relocalization (Tracking.cc:1156-1249): every live solver fills its problem in candidate order, ONE
// asd_pnp_ransac runs them all, and the results are applied in candidate order: iterate()'s outputs (:1169), bNoMore -> discarded
// (:1172-1176), and where a pose came back the tail :1176-1247 -- tail(i, Tcw, vbInliers, nInliers) -> bMatch, the caller's
// PoseOptimization / SearchByProjection rounds.  At the first candidate whose tail reports bMatch the solvers behind it are cancelled,
// last first, so that the stream hands their random numbers out again in the order they were drawn; its position is returned (-1: no
// match in this pass).  The reference's pass is sequential: a solver that returned its refined model before its last supplied iteration
// has numbers left that the solver behind it would have consumed, so behind such a candidate whose tail says no the pass goes on with a
// call of its own for the rest.
template <class TailFn>
int Tracking::RelocalizationRound(Context& c, std::vector<PnPsolver*>& vpPnPsolvers, std::vector<bool>& vbDiscarded, int nIterations, TailFn tail) {
  const int nKFs = (int)vpPnPsolvers.size();
  for (int from = 0; from < nKFs;) {
    std::vector<int> who;
    std::vector<asd_pnp_ransac_problem> probs;
    for (int i = from; i < nKFs; ++i) {
      if (vbDiscarded[i]) continue;
      asd_pnp_ransac_problem p;
      if (!vpPnPsolvers[i]->Begin(nIterations, p)) { vbDiscarded[i] = true; continue; }   // N < mRansacMinInliers: bNoMore at once
      who.push_back(i);
      probs.push_back(p);
    }
    if (who.empty()) return -1;
    if (asd_pnp_ransac(c.get(), (int32_t)probs.size(), probs.data()) != ASD_OK) {
      for (size_t k = who.size(); k-- > 0;) { vpPnPsolvers[who[k]]->Cancel(); vbDiscarded[who[k]] = true; }
      return -1;
    }
    // results in candidate order.  A solver that returned before its last supplied iteration has numbers left that the solver behind it
    // would have consumed: everything behind it is cancelled (last first), then its own End hands its unused numbers back in front
    size_t stop = who.size();
    for (size_t k = 0; k < who.size(); ++k) {
      if (vpPnPsolvers[who[k]]->ReturnsEarly(probs[k], (int)k)) {
        stop = k;
        for (size_t b = who.size(); b-- > k + 1;) vpPnPsolvers[who[b]]->Cancel();
      }
      bool bNoMore = false;
      std::vector<bool> vbInliers;
      int nInliers = 0;
      float Tcw[16];
      const bool got = vpPnPsolvers[who[k]]->End(probs[k], bNoMore, vbInliers, nInliers, Tcw, (int)k);
      if (bNoMore) vbDiscarded[who[k]] = true;
      if (got && tail(who[k], (const float*)Tcw, vbInliers, nInliers)) {
        if (stop == who.size())
          for (size_t b = who.size(); b-- > k + 1;) vpPnPsolvers[who[b]]->Cancel();
        return who[k];
      }
      if (stop < who.size()) break;
    }
    if (stop >= who.size()) return -1;
    from = who[stop] + 1;
  }
  return -1;
}

// LoopClosing::ComputeSim3 (LoopClosing.cc:269-423): every search, the RANSAC and the refinement run behind the C ABI.  Two forms:
// ComputeSim3 over the candidate list with asd::Sim3Solver (:291-377), and ComputeSim3Candidate, the numeric body for ONE candidate with
// the Sim3 handed in by a callback (a caller that keeps a solver of its own).  Both end in the same tail (Sim3Tail: :359-375, :415).
struct LoopClosing {
  // LoopClosing::SearchAndFuse (LoopClosing.cc:603-629) for ONE keyframe of CorrectedPosesMap: ORBmatcher::Fuse(pKF, cvScw,
  // mvpLoopMapPoints, 4, vpReplacePoints) -- its search half is asd_fuse_search_sim3, with valid[i] = "a point, and not in spAlreadyFound"
  // from the keyframe's row in the table; a bad point is dropped by the apply's gate -- then its own additions and the Replace loop of
  // :619-627 (asd_fuse_apply mode 1).  points[i] is the view of bank row rows[i] (ignored where rows[i] < 0); Scw row-major 4x4.
  static FuseOutcome SearchAndFuse(Context& c, int32_t kfId, const FrameView& KF, const float Scw[16], const std::vector<MapPointView>& points,
                                   const std::vector<int32_t>& rows, const Camera& K, float th = 4.f) {
    FuseOutcome R;
    std::vector<uint8_t> valid;
    std::vector<float> Xw, nrm, mind, maxd, desc;
    if ((R.rc = ORBmatcher::FuseSearchInput(c, kfId, points, rows, valid, Xw, nrm, mind, maxd, desc)) != ASD_OK) return R;
    const int n = (int)rows.size();
    std::vector<int32_t> bestIdx(n, -1);
    std::vector<float> bd(n);
    const float Kv[4] = {K.fx, K.fy, K.cx, K.cy};
    if (n > 0 && (R.rc = asd_fuse_search_sim3(c.get(), KF.slot, Scw, n, valid.data(), Xw.data(), nrm.data(), mind.data(), maxd.data(), desc.data(), Kv, th,
                                              bestIdx.data(), bd.data())) != ASD_OK)
      return R;
    R = FuseApply(c, kfId, 1, rows, bestIdx, true);
    R.bestIdx = bestIdx;
    return R;
  }
  // the loop-fusion block of CorrectLoop (LoopClosing.cc:540-555): vpCurrentMatchedPoints[i] = mvpCurrentMatchedPoints[i] as a bank row,
  // -1 = NULL
  static FuseOutcome FuseMatchedPoints(Context& c, int32_t currentKfId, const std::vector<int32_t>& vpCurrentMatchedPoints) {
    std::vector<int32_t> bestIdx(vpCurrentMatchedPoints.size());
    for (size_t i = 0; i < bestIdx.size(); ++i) bestIdx[i] = vpCurrentMatchedPoints[i] >= 0 ? (int32_t)i : -1;
    return FuseApply(c, currentKfId, 2, vpCurrentMatchedPoints, bestIdx, true);
  }

  // LoopClosing::DetectLoop's lowest score to a connected keyframe (LoopClosing.cc:154-168): vConnected = the ids of
  // mpCurrentKF->GetVectorCovisibleKeyFrames() that are not bad (all of them must be in the database); 1 when there is none.
  // The result is DetectLoopCandidates' minScore (:171).
  static float DetectLoopMinScore(Context& c, const BowVector& CurrentBowVec, const std::vector<int32_t>& vConnected) {
    float minScore = 1;
    std::vector<double> score(vConnected.size() + 1);
    if (asd_kfdb_score(c.get(), CurrentBowVec.size(), CurrentBowVec.id.data(), CurrentBowVec.val.data(), (int32_t)vConnected.size(),
                       vConnected.data(), score.data()) != ASD_OK)
      return minScore;
    for (size_t i = 0; i < vConnected.size(); ++i) {
      const float s = (float)score[i];
      if (s < minScore) minScore = s;
    }
    return minScore;
  }
  struct Result { bool bMatch = false; int iMatched = -1; int nBoW = 0, nSim3 = 0, nInliers = 0, nTotalMatches = 0; double g2oScm[8] = {0, 0, 0, 1, 0, 0, 0, 1}; };
  // `points` = the caller's map point table (ids as in mvpMapPoints); vpLoopMapPoints = ids of the points of the loop keyframe and
  // its neighbours (:393-412); vpCurrentMatchedPoints[i] = id matched to the current keyframe's keypoint i on return.
  template <class Sim3SolverFn>
  static Result ComputeSim3Candidate(Context& c, const FrameView& CurrentKF, const ORBmatcher::FeatVec& fvCur, const FrameView& KF,
                                     const ORBmatcher::FeatVec& fvKF, const std::vector<MapPointView>& points,
                                     const std::vector<int32_t>& vpLoopMapPoints, const Camera& K, const std::vector<float>& invLevelSigma2,
                                     bool bFixScale, Sim3SolverFn solver, std::vector<int32_t>& vpCurrentMatchedPoints) {
    Result r;
    ORBmatcher matcher(c, 0.85f, true);                                                   // :277
    std::vector<int32_t> vpMatches, vnIdx2;
    r.nBoW = matcher.SearchByBoW(CurrentKF, fvCur, KF, fvKF, vpMatches, vnIdx2);          // :304
    if (r.nBoW < 20) return r;                                                            // :305
    float s = 1.f, R[9], t[3];
    if (!solver(vpMatches, vnIdx2, &s, R, t)) return r;                                   // :337 (the caller keeps only the RANSAC inliers, :349-354)
    return Sim3Tail(c, CurrentKF, KF, points, vpLoopMapPoints, K, invLevelSigma2, bFixScale, r, vpMatches, vnIdx2, s, R, t, vpCurrentMatchedPoints);
  }

  // What follows a Sim3 from RANSAC for one candidate (:359-375, :415): SearchBySim3, OptimizeSim3, and for a match mScw and
  // SearchByProjection(KF, Scw).  vpMatches / vnIdx2 = the matches the RANSAC kept (:349-354); r carries nBoW.
  static Result Sim3Tail(Context& c, const FrameView& CurrentKF, const FrameView& KF, const std::vector<MapPointView>& points,
                         const std::vector<int32_t>& vpLoopMapPoints, const Camera& K, const std::vector<float>& invLevelSigma2, bool bFixScale,
                         Result r, std::vector<int32_t> vpMatches, std::vector<int32_t> vnIdx2, float s, const float* R, const float* t,
                         std::vector<int32_t>& vpCurrentMatchedPoints) {
    // matcher.SearchBySim3(mpCurrentKF, pKF, vpMapPointMatches, s, R, t, 7.5)  (:359)
    const int n1 = CurrentKF.N(), n2 = KF.N();
    auto gather = [&](const FrameView& F, std::vector<uint8_t>& has, std::vector<float>& Xw, std::vector<float>& mind, std::vector<float>& maxd,
                      std::vector<float>& desc) {
      has.assign(F.N(), 0); Xw.assign((size_t)F.N() * 3, 0.f); mind.assign(F.N(), 0.f); maxd.assign(F.N(), 0.f); desc.assign((size_t)F.N() * ASD_DESC_DIM, 0.f);
      for (int i = 0; i < F.N(); ++i) {
        const int id = F.mvpMapPoints.size() == (size_t)F.N() ? F.mvpMapPoints[i] : -1;
        if (id < 0) continue;
        has[i] = 1;
        for (int k = 0; k < 3; ++k) Xw[3 * i + k] = points[id].Xw[k];
        mind[i] = points[id].mfMinDistance; maxd[i] = points[id].mfMaxDistance;
        for (int k = 0; k < ASD_DESC_DIM; ++k) desc[(size_t)i * ASD_DESC_DIM + k] = points[id].descriptor[k];
      }
    };
    std::vector<uint8_t> has1, has2;
    std::vector<float> X1, X2, mn1, mx1, mn2, mx2, d1, d2;
    gather(CurrentKF, has1, X1, mn1, mx1, d1);
    gather(KF, has2, X2, mn2, mx2, d2);
    for (int i = 0; i < n1; ++i)                                                          // vbAlreadyMatched1 / 2 (ORBmatcher.cc:1118-1134)
      if (vpMatches[i] >= 0) { has1[i] = 0; if (vnIdx2[i] >= 0) has2[vnIdx2[i]] = 0; }
    std::vector<int32_t> m12(n1, -1);
    int32_t nfound = 0;
    const float Kv[4] = {K.fx, K.fy, K.cx, K.cy};
    if (asd_match_sim3(c.get(), CurrentKF.slot, KF.slot, has1.data(), has2.data(), X1.data(), X2.data(), mn1.data(), mx1.data(), mn2.data(), mx2.data(),
                       d1.data(), d2.data(), CurrentKF.mTcw, KF.mTcw, s, R, t, Kv, 7.5f, m12.data(), &nfound) != ASD_OK)
      return r;
    for (int i = 0; i < n1; ++i)
      if (m12[i] >= 0 && m12[i] < n2) { vpMatches[i] = KF.mvpMapPoints[m12[i]]; vnIdx2[i] = m12[i]; }
    r.nSim3 = nfound;
    // g2o::Sim3 gScm(R, t, s); Optimizer::OptimizeSim3(mpCurrentKF, pKF, vpMapPointMatches, gScm, 10, mbFixScale)  (:361-362)
    double q[4];
    {
      double pose[7];
      const float T[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1};
      asd_tcw_to_pose7(T, pose);
      for (int k = 0; k < 4; ++k) q[k] = pose[k];
    }
    double S[8] = {q[0], q[1], q[2], q[3], t[0], t[1], t[2], s};
    r.nInliers = Optimizer::OptimizeSim3(c, CurrentKF, KF, points, vpMatches, vnIdx2, S, 10.f, bFixScale, K, K, invLevelSigma2, invLevelSigma2);
    for (int k = 0; k < 8; ++k) r.g2oScm[k] = S[k];
    if (r.nInliers < 20) return r;                                                        // :364
    r.bMatch = true;
    // mg2oScw = gScm * gSmw, gSmw = (pKF's rotation, translation, 1)  (:368-370); mScw = Converter::toCvMat(mg2oScw) = [s R | t]
    float Scw[16];
    {
      const double pose[7] = {S[0], S[1], S[2], S[3], 0, 0, 0};
      float Rm[16];
      asd_pose7_to_tcw(pose, Rm);
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
          double a = 0;
          for (int k = 0; k < 3; ++k) a += (double)Rm[i * 4 + k] * KF.mTcw[k * 4 + j];
          Scw[i * 4 + j] = (float)(S[7] * a);
        }
        double b = 0;
        for (int k = 0; k < 3; ++k) b += (double)Rm[i * 4 + k] * KF.mTcw[k * 4 + 3];
        Scw[i * 4 + 3] = (float)(S[7] * b + S[4 + i]);
      }
      Scw[12] = Scw[13] = Scw[14] = 0.f; Scw[15] = 1.f;
    }
    // matcher.SearchByProjection(mpCurrentKF, mScw, mvpLoopMapPoints, mvpCurrentMatchedPoints, 10)  (:415)
    const int nl = (int)vpLoopMapPoints.size();
    std::vector<uint8_t> valid(nl, 1);
    std::vector<float> Xl((size_t)nl * 3), nrm((size_t)nl * 3), mnl(nl), mxl(nl), dl((size_t)nl * ASD_DESC_DIM);
    std::vector<int32_t> matched_kp(n1, -1);
    for (int m = 0; m < nl; ++m) {
      const MapPointView& P = points[vpLoopMapPoints[m]];
      for (int k = 0; k < 3; ++k) { Xl[3 * m + k] = P.Xw[k]; nrm[3 * m + k] = P.normal[k]; }
      mnl[m] = P.mfMinDistance; mxl[m] = P.mfMaxDistance;
      for (int k = 0; k < ASD_DESC_DIM; ++k) dl[(size_t)m * ASD_DESC_DIM + k] = P.descriptor[k];
      for (int i = 0; i < n1; ++i) if (vpMatches[i] == vpLoopMapPoints[m]) valid[m] = 0;  // spAlreadyFound (ORBmatcher.cc:321)
    }
    for (int i = 0; i < n1; ++i) if (vpMatches[i] >= 0) matched_kp[i] = nl;                // occupied on entry
    int32_t nproj = 0;
    if (asd_match_project_sim3(c.get(), CurrentKF.slot, Scw, nl, valid.data(), Xl.data(), nrm.data(), mnl.data(), mxl.data(), dl.data(), Kv, 10,
                               matched_kp.data(), &nproj) != ASD_OK)
      return r;
    vpCurrentMatchedPoints = vpMatches;
    for (int i = 0; i < n1; ++i)
      if (matched_kp[i] >= 0 && matched_kp[i] < nl) vpCurrentMatchedPoints[i] = vpLoopMapPoints[matched_kp[i]];
    for (int i = 0; i < n1; ++i) r.nTotalMatches += vpCurrentMatchedPoints[i] >= 0;        // :418-423
    return r;
  }

  // One round of the loop of :322-377 over the live solvers from position `from` on, as ONE asd_sim3_ransac call: every solver draws its
  // nIterations in candidate order and iterates.  The reference's round is sequential: when solver i returns a model, the solvers behind
  // it have not iterated yet -- their random numbers go back to the stream (last solver first, so that the stream hands them out in the
  // order they were drawn) and their state stays as it was in front of the round.  Returns the position of the first solver that
  // returned a model (vbInliers / nInliers are its outputs), or -1 when none did.  Solvers that reached their last iteration are
  // marked discarded (:339-343).
  static int Sim3Round(Context& c, std::vector<Sim3Solver*>& vpSim3Solvers, std::vector<bool>& vbDiscarded, int from, int nIterations,
                       std::vector<bool>& vbInliers, int& nInliers) {
    std::vector<int> who;
    std::vector<asd_sim3_ransac_problem> probs;
    for (int i = from; i < (int)vpSim3Solvers.size(); ++i) {
      if (vbDiscarded[i]) continue;
      asd_sim3_ransac_problem p;
      if (!vpSim3Solvers[i]->Begin(nIterations, p)) { vbDiscarded[i] = true; continue; }   // N < mRansacMinInliers: bNoMore at once
      who.push_back(i);
      probs.push_back(p);
    }
    if (who.empty()) return -1;
    if (asd_sim3_ransac(c.get(), (int32_t)probs.size(), probs.data()) != ASD_OK) {
      for (size_t k = who.size(); k-- > 0;) { vpSim3Solvers[who[k]]->Cancel(); vbDiscarded[who[k]] = true; }
      return -1;
    }
    size_t first = who.size();
    for (size_t k = 0; k < who.size(); ++k)
      if (probs[k].found) { first = k; break; }
    for (size_t k = who.size(); k-- > first + 1;) vpSim3Solvers[who[k]]->Cancel();
    int hit = -1;
    // (End gives the unused numbers of the solver that returned back LAST: they were drawn in front of those of the solvers behind it)
    for (size_t k = std::min(first + 1, who.size()); k-- > 0;) {
      bool bNoMore = false;
      std::vector<bool> inl;
      int nInl = 0;
      const bool got = vpSim3Solvers[who[k]]->End(probs[k], bNoMore, inl, nInl);
      if (bNoMore) vbDiscarded[who[k]] = true;
      if (got) { hit = who[k]; vbInliers = inl; nInliers = nInl; }
    }
    return hit;
  }

  // bool LoopClosing::ComputeSim3()  (:269-423) over mvpEnoughConsistentCandidates = vpCandidates (with their FeatureVectors).  A Sim3Solver
  // with SetRansacParameters(0.99, 20, 300) per candidate with 20 BoW matches or more (:304-315); rounds of 5 iterations per live
  // candidate (:337) until one gives a Sim3 that survives SearchBySim3 + OptimizeSim3 with 20 inliers (:364) or every candidate is
  // discarded.  loopPoints(i) = the ids of the map points of candidate i and its neighbours (:393-412), asked for the matched candidate only.
  // Result::iMatched = position of mpMatchedKF in vpCandidates (-1: no match).
  template <class LoopPointsFn>
  static Result ComputeSim3(Context& c, const FrameView& CurrentKF, const ORBmatcher::FeatVec& fvCur, const std::vector<const FrameView*>& vpCandidates,
                            const std::vector<const ORBmatcher::FeatVec*>& vfvCandidates, const std::vector<MapPointView>& points,
                            LoopPointsFn loopPoints, const Camera& K, const std::vector<float>& levelSigma2, const std::vector<float>& invLevelSigma2,
                            bool bFixScale, DrawStream& draws, std::vector<int32_t>& vpCurrentMatchedPoints) {
    const int nInitialCandidates = (int)vpCandidates.size();
    ORBmatcher matcher(c, 0.85f, true);                                                   // :277
    std::vector<Sim3Solver*> vpSim3Solvers(nInitialCandidates, nullptr);
    std::vector<std::vector<int32_t>> vvpMapPointMatches(nInitialCandidates), vvnIdx2(nInitialCandidates);
    std::vector<int> vnBoW(nInitialCandidates, 0);
    std::vector<bool> vbDiscarded(nInitialCandidates, false);
    for (int i = 0; i < nInitialCandidates; ++i) {                                        // :291-318
      vnBoW[i] = matcher.SearchByBoW(CurrentKF, fvCur, *vpCandidates[i], *vfvCandidates[i], vvpMapPointMatches[i], vvnIdx2[i]);
      if (vnBoW[i] < 20) { vbDiscarded[i] = true; continue; }
      vpSim3Solvers[i] = new Sim3Solver(c, CurrentKF, *vpCandidates[i], vvpMapPointMatches[i], vvnIdx2[i], points, K, K, levelSigma2, levelSigma2,
                                        bFixScale, draws);
      vpSim3Solvers[i]->SetRansacParameters(0.99, 20, 300);
    }
    Result r;
    auto live = [&] { int n = 0; for (int i = 0; i < nInitialCandidates; ++i) n += !vbDiscarded[i]; return n; };
    while (live() > 0 && !r.bMatch) {                                                     // :322
      for (int from = 0; from < nInitialCandidates && !r.bMatch;) {                       // :324: one pass over the candidates
        std::vector<bool> vbInliers;
        int nInliers = 0;
        const int i = Sim3Round(c, vpSim3Solvers, vbDiscarded, from, 5, vbInliers, nInliers);
        if (i < 0) break;
        std::vector<int32_t> vpMapPointMatches(vvpMapPointMatches[i].size(), -1), vnIdx2(vvpMapPointMatches[i].size(), -1);   // :349-354
        for (size_t j = 0; j < vbInliers.size(); ++j)
          if (vbInliers[j]) { vpMapPointMatches[j] = vvpMapPointMatches[i][j]; vnIdx2[j] = vvnIdx2[i][j]; }
        Result ri;
        ri.nBoW = vnBoW[i];
        ri = Sim3Tail(c, CurrentKF, *vpCandidates[i], points, loopPoints(i), K, invLevelSigma2, bFixScale, ri, vpMapPointMatches, vnIdx2,
                      vpSim3Solvers[i]->GetEstimatedScale(), vpSim3Solvers[i]->GetEstimatedRotation(), vpSim3Solvers[i]->GetEstimatedTranslation(),
                      vpCurrentMatchedPoints);
        ri.iMatched = ri.bMatch ? i : -1;
        r = ri;
        from = i + 1;                                                                     // no match (:364): the candidates behind i still iterate this round
      }
    }
    for (Sim3Solver* p : vpSim3Solvers) delete p;
    return r;
  }
};

// MapPoint::ComputeDistinctiveDescriptors for a batch of map points (MapPoint.cc:271-338): observations[s] = the
// descriptors (128 f32 each) of map point s's observations; returns the chosen observation index per map point
inline int ComputeDistinctiveDescriptors(Context& c, const std::vector<std::vector<const float*>>& observations, std::vector<int32_t>& best) {
  std::vector<int32_t> start(observations.size() + 1, 0);
  for (size_t s = 0; s < observations.size(); ++s) start[s + 1] = start[s] + (int32_t)observations[s].size();
  std::vector<float> desc((size_t)start.back() * ASD_DESC_DIM);
  for (size_t s = 0; s < observations.size(); ++s)
    for (size_t k = 0; k < observations[s].size(); ++k)
      for (int q = 0; q < ASD_DESC_DIM; ++q) desc[((size_t)start[s] + k) * ASD_DESC_DIM + q] = observations[s][k][q];
  best.assign(observations.size(), 0);
  return asd_distinctive_descriptor_batch(c.get(), (int32_t)observations.size(), start.data(), desc.data(), best.data());
}

// ---- vocabulary / local mapping (ORBVocabulary.h:34, Frame.cc:289-296, LocalMapping.cc:299-519) ---
// void Frame::ComputeBoW(): BowVector (word id -> weight) and FeatureVector (node id at levelsup = 4 -> keypoints)
inline int ComputeBoW(Context& c, const FrameView& F, std::vector<std::pair<int32_t, double>>& mBowVec, ORBmatcher::FeatVec& mFeatVec,
                      int levelsup = 4) {
  const int N = F.N();
  std::vector<int32_t> bid(N + 1);
  std::vector<double> bval(N + 1);
  mFeatVec.node.assign(N + 1, 0); mFeatVec.start.assign(N + 1, 0); mFeatVec.idx.assign(N + 1, 0);
  int32_t nw = 0, nn = 0;
  const int rc = asd_compute_bow(c.get(), F.slot, nullptr, N, levelsup, bid.data(), bval.data(), &nw, mFeatVec.node.data(),
                                 mFeatVec.start.data(), mFeatVec.idx.data(), &nn);
  if (rc != ASD_OK) return rc;
  mBowVec.clear();
  for (int k = 0; k < nw; ++k) mBowVec.emplace_back(bid[k], bval[k]);
  mFeatVec.node.resize(nn);
  mFeatVec.start.resize(nn + 1);
  mFeatVec.idx.resize(mFeatVec.start[nn]);
  return ASD_OK;
}

// LocalMapping::CreateNewMapPoints, per-match body (:386-523): x3D[3*i..] and ok[i] for every matched pair
inline int TriangulateMatches(Context& c, const FrameView& KF1, const FrameView& KF2, const Camera& K1, const Camera& K2,
                              const std::vector<std::pair<size_t, size_t>>& vMatchedIndices, std::vector<float>& x3D,
                              std::vector<uint8_t>& ok) {
  const int n = (int)vMatchedIndices.size();
  std::vector<int32_t> i1(n), i2(n);
  for (int i = 0; i < n; ++i) { i1[i] = (int32_t)vMatchedIndices[i].first; i2[i] = (int32_t)vMatchedIndices[i].second; }
  x3D.assign((size_t)3 * n, 0.f);
  ok.assign(n, 0);
  int32_t nnew = 0;
  const float k1[4] = {K1.fx, K1.fy, K1.cx, K1.cy}, k2[4] = {K2.fx, K2.fy, K2.cx, K2.cy};
  if (asd_triangulate_pairs(c.get(), KF1.slot, KF2.slot, n, i1.data(), i2.data(), KF1.mTcw, KF2.mTcw, k1, k2, x3D.data(), ok.data(), &nnew) != ASD_OK)
    return 0;
  return nnew;
}

// ---- Initializer (Initializer.h:36-100; src/vslam/src/Initializer.cc) --------------------------------------------------------------
// DUtils::Random::SeedRandOnce(0) (Random.cpp:38-45, called at Initializer.cc:84): one flag for the whole process; the first Initialize
// calls srand(0), every later one -- of this or of another Initializer -- goes on with the sequence.
inline void SeedRandOnce(int seed) {
  static bool already_seeded = false;
  if (!already_seeded) {
    std::srand((unsigned)seed);
    already_seeded = true;
  }
}

struct Point3f { float x, y, z; };

// The whole of Initialize runs on the device (asd_initialize); this class keeps what the reference's object keeps (mvKeys1, mK, mSigma,
// mMaxIterations) and makes the draws: 8 x mMaxIterations calls of rand() per Initialize, in the reference's order (:86-101).
class Initializer {
 public:
  // Initializer(const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200)  (:33-42); mK is the frame's in the reference
  Initializer(asd_ctx* ctx, const FrameView& ReferenceFrame, const Camera& K, float sigma = 1.0f, int iterations = 200)
      : ctx_(ctx), mK(K), mSigma(sigma), mMaxIterations(iterations) {
    mvKeys1.reserve(2 * ReferenceFrame.mvKeysUn.size());
    for (const asd_keypoint& k : ReferenceFrame.mvKeysUn) { mvKeys1.push_back(k.x); mvKeys1.push_back(k.y); }
  }
  // the draws of one Initialize over N matches (:84-100): RandomInt(0, vAvailableIndices.size() - 1) eight times per iteration
  std::vector<int32_t> Draw(int N) {
    SeedRandOnce(0);
    const int32_t* draws = batch_.Draw(stream_, mMaxIterations, 8, N);
    batch_.Keep((size_t)8 * mMaxIterations);   // Initialize runs every iteration
    return std::vector<int32_t>(draws, draws + (size_t)8 * mMaxIterations);
  }
  // bool Initialize(const Frame& CurrentFrame, const vector<int>& vMatches12, cv::Mat& R21, cv::Mat& t21, vector<cv::Point3f>& vP3D,
  //                 vector<bool>& vbTriangulated)  (:43-120).  R21 (row major) and t21 are written only when it returns true; vP3D and
  // vbTriangulated are then indexed by the keypoint of the reference frame.  Fewer than eight matches return false without drawing
  // (the reference's sampling is undefined there; Tracking.cc:428 asks for 100).
  bool Initialize(const FrameView& CurrentFrame, const std::vector<int>& vMatches12, float R21[9], float t21[3], std::vector<Point3f>& vP3D,
                  std::vector<bool>& vbTriangulated) {
    std::vector<float> keys2;
    keys2.reserve(2 * CurrentFrame.mvKeysUn.size());
    for (const asd_keypoint& k : CurrentFrame.mvKeysUn) { keys2.push_back(k.x); keys2.push_back(k.y); }
    const int n1 = (int)(mvKeys1.size() / 2);
    std::vector<int32_t> m12(n1, -1);
    int N = 0;
    for (int i = 0; i < n1 && i < (int)vMatches12.size(); ++i) { m12[i] = vMatches12[i]; N += vMatches12[i] >= 0; }
    if (N < 8) return false;
    mvDraws = Draw(N);
    std::vector<float> P3D((size_t)3 * n1);
    std::vector<uint8_t> tri(n1), inlH(N), inlF(N);
    asd_initializer_problem p{};
    p.n1 = n1; p.keys1 = mvKeys1.data(); p.n2 = (int)(keys2.size() / 2); p.keys2 = keys2.data(); p.matches12 = m12.data();
    p.K[0] = mK.fx; p.K[1] = mK.fy; p.K[2] = mK.cx; p.K[3] = mK.cy;
    p.sigma = mSigma; p.n_iter = mMaxIterations; p.draws = mvDraws.data();
    p.min_parallax = 1.0f; p.min_triangulated = 50;   // :115-117
    p.P3D = P3D.data(); p.triangulated = tri.data(); p.inliers_H = inlH.data(); p.inliers_F = inlF.data();
    if (asd_initialize(ctx_, 1, &p) != ASD_OK) throw std::runtime_error(asd_last_error(ctx_));
    mLast = p;
    if (!p.ok) return false;
    for (int i = 0; i < 9; ++i) R21[i] = p.R21[i];
    for (int i = 0; i < 3; ++i) t21[i] = p.t21[i];
    vP3D.resize(n1);
    vbTriangulated.assign(n1, false);
    for (int i = 0; i < n1; ++i) { vP3D[i] = Point3f{P3D[3 * i], P3D[3 * i + 1], P3D[3 * i + 2]}; vbTriangulated[i] = tri[i] != 0; }
    return true;
  }
  const std::vector<int32_t>& LastDraws() const { return mvDraws; }
  const asd_initializer_problem& Last() const { return mLast; }   // SH, SF, model, n_matches of the last Initialize (its pointers are stale)
 private:
  asd_ctx* ctx_;
  Camera mK;
  float mSigma;
  int mMaxIterations;
  std::vector<float> mvKeys1;
  std::vector<int32_t> mvDraws;
  asd_initializer_problem mLast{};
  DrawStream stream_;   // ::rand
  DrawBatch batch_;
};

}  // namespace asd
