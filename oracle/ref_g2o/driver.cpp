// driver.cpp -- flat-array entry points over the REFERENCE's vendored g2o (compiled in place by the
// Makefile next to this file).  TEST INFRASTRUCTURE ONLY: produces tests/golden/ba_*.npz and serves as
// the "reference" CPU baseline in bench.py.  Graph construction and schedules follow
// /root/reference/src/vslam/src/Optimizer.cc:241-404 (PoseOptimization) and :470-671
// (LocalBundleAdjustment) with the pointer graph replaced by the flat arrays of include/asd_slam.h.
// Signatures match oracle/oracle.h (orc_pose_optimize / orc_local_ba) so one ctypes wrapper drives both.
#include <cmath>
#include <cstdint>
#include <vector>

#include "g2o/core/block_solver.h"
#include "g2o/core/hyper_graph_action.h"
#include "g2o/core/optimization_algorithm_levenberg.h"
#include "g2o/core/robust_kernel_impl.h"
#include "g2o/solvers/linear_solver_dense.h"
#include "g2o/types/types_six_dof_expmap.h"

struct ref_ba_out { double chi2_first, chi2_second; int32_t iters_first, iters_second, trials_first, trials_second; };

// Revision of this driver's entry points, read by oracle/pyoracle.py (RefG2O.abi).  A library built from an older driver has no
// such symbol (revision 1): ref_local_ba without the trial counts, the trace or the edge errors computed ahead of an its1 = 0 round.
// Revision 2 has no ref_pose_optimize_trace.
extern "C" int ref_driver_abi() { return 3; }

// The Levenberg trace of the last ref_local_ba, per round (ref_local_ba_trace reads it):
//  - per iteration, from a post-iteration action: the trials it took (levenbergIteration()), the lambda it left behind
//    (currentLambda()) and activeRobustChi2() over the stored errors -- those of its last trial, accepted or not;
//  - per computeActiveErrors call, from a compute-error action, which runs IN FRONT of the computation: activeRobustChi2() of the
//    errors the previous call stored.  A round makes 1 + trials calls per iteration (levenberg.cpp:74, :119), so entry j + 1 is the
//    chi2 after call j, and the post-iteration chi2 of the round's last iteration closes the list.
// Neither action recomputes anything: the estimate, the stored errors and the Levenberg state are what they would be without them.
struct LmIter { double trials, lambda, chi2; };
static std::vector<LmIter> g_iters[2];
static std::vector<double> g_calls[2];
static int g_round = 0;

// The same two actions trace ref_pose_optimize, per round of Optimizer.cc:335-403 (ref_pose_optimize_trace reads it), next to what the
// driver itself sees between the rounds: the active edges after initializeOptimization(0), what optimize(10) returned, and the
// re-classification's nBad, flag changes and distance from the 5.991 gate.
struct PoseRound {
  int active, ret, n_bad, changed, reinlier, gate_edge;
  double pose[7], gate_margin;
};
static std::vector<LmIter> g_piters[4];
static std::vector<double> g_pcalls[4];
static PoseRound g_pround[4];
static int g_prounds = 0;

namespace {
struct PostIteration : g2o::HyperGraphAction {
  g2o::OptimizationAlgorithmLevenberg* lm;
  std::vector<LmIter>* sink;   // [round]
  PostIteration(g2o::OptimizationAlgorithmLevenberg* a, std::vector<LmIter>* s) : lm(a), sink(s) {}
  g2o::HyperGraphAction* operator()(const g2o::HyperGraph* graph, Parameters* = 0) {
    const g2o::SparseOptimizer* o = static_cast<const g2o::SparseOptimizer*>(graph);
    sink[g_round].push_back(LmIter{(double)lm->levenbergIteration(), lm->currentLambda(), o->activeRobustChi2()});
    return this;
  }
};
struct ComputeErrors : g2o::HyperGraphAction {
  std::vector<double>* sink;   // [round]
  explicit ComputeErrors(std::vector<double>* s) : sink(s) {}
  g2o::HyperGraphAction* operator()(const g2o::HyperGraph* graph, Parameters* = 0) {
    sink[g_round].push_back(static_cast<const g2o::SparseOptimizer*>(graph)->activeRobustChi2());
    return this;
  }
};
}  // namespace

static g2o::SE3Quat from7(const double* p) {
  return g2o::SE3Quat(Eigen::Quaterniond(p[3], p[0], p[1], p[2]), Eigen::Vector3d(p[4], p[5], p[6]));
}
static void to7(const g2o::SE3Quat& T, double* p) {
  const Eigen::Quaterniond& q = T.rotation();
  p[0] = q.x(); p[1] = q.y(); p[2] = q.z(); p[3] = q.w();
  p[4] = T.translation()[0]; p[5] = T.translation()[1]; p[6] = T.translation()[2];
}

extern "C" int ref_pose_optimize(double* pose7, int n, const double* Xw, const double* obs, const double* inv_sigma2,
                                 const double* K, uint8_t* outlier) {
  g2o::SparseOptimizer optimizer;
  g2o::OptimizationAlgorithmLevenberg* solver = new g2o::OptimizationAlgorithmLevenberg(
      new g2o::BlockSolver_6_3(new g2o::LinearSolverDense<g2o::BlockSolver_6_3::PoseMatrixType>()));
  optimizer.setAlgorithm(solver);
  int nInitialCorrespondences = 0;
  const g2o::SE3Quat T0 = from7(pose7);
  g2o::VertexSE3Expmap* vSE3 = new g2o::VertexSE3Expmap();
  vSE3->setEstimate(T0);
  vSE3->setId(0);
  vSE3->setFixed(false);
  optimizer.addVertex(vSE3);
  std::vector<g2o::EdgeSE3ProjectXYZOnlyPose*> vpEdgesMono;
  const float deltaMono = sqrt(5.991);
  for (int i = 0; i < n; i++) {
    nInitialCorrespondences++;
    outlier[i] = false;
    Eigen::Matrix<double, 2, 1> o;
    o << obs[2 * i], obs[2 * i + 1];
    g2o::EdgeSE3ProjectXYZOnlyPose* e = new g2o::EdgeSE3ProjectXYZOnlyPose();
    e->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(0)));
    e->setMeasurement(o);
    e->setInformation(Eigen::Matrix2d::Identity() * inv_sigma2[i]);
    g2o::RobustKernelHuber* rk = new g2o::RobustKernelHuber;
    e->setRobustKernel(rk);
    rk->setDelta(deltaMono);
    e->fx = K[0]; e->fy = K[1]; e->cx = K[2]; e->cy = K[3];
    e->Xw[0] = Xw[3 * i]; e->Xw[1] = Xw[3 * i + 1]; e->Xw[2] = Xw[3 * i + 2];
    optimizer.addEdge(e);
    vpEdgesMono.push_back(e);
  }
  g_prounds = 0;
  for (int r = 0; r < 4; ++r) { g_piters[r].clear(); g_pcalls[r].clear(); }
  if (nInitialCorrespondences < 3) return 0;
  const float chi2Mono[4] = {5.991, 5.991, 5.991, 5.991};
  const int its[4] = {10, 10, 10, 10};
  int nBad = 0;
  PostIteration post(solver, g_piters);
  ComputeErrors calls(g_pcalls);
  optimizer.addPostIterationAction(&post);
  optimizer.addComputeErrorAction(&calls);
  for (size_t it = 0; it < 4; it++) {
    PoseRound& tr = g_pround[it];
    g_round = (int)it;
    vSE3->setEstimate(T0);
    optimizer.initializeOptimization(0);
    tr.active = (int)optimizer.activeEdges().size();
    tr.ret = optimizer.optimize(its[it]);
    g_pcalls[it].push_back(optimizer.activeRobustChi2());   // closes the list: the chi2 the round's last computeActiveErrors left
    to7(vSE3->estimate(), tr.pose);
    tr.changed = tr.reinlier = 0;
    tr.gate_margin = 1e300;
    tr.gate_edge = -1;
    nBad = 0;
    for (size_t i = 0, iend = vpEdgesMono.size(); i < iend; i++) {
      g2o::EdgeSE3ProjectXYZOnlyPose* e = vpEdgesMono[i];
      if (outlier[i]) e->computeError();
      const float chi2 = e->chi2();
      const double margin = std::fabs(e->chi2() - (double)chi2Mono[it]) / (double)chi2Mono[it];
      if (!(margin >= tr.gate_margin)) { tr.gate_margin = margin; tr.gate_edge = (int)i; }   // (a NaN margin is kept: it fails every test)
      const bool was = outlier[i];
      if (chi2 > chi2Mono[it]) { outlier[i] = true; e->setLevel(1); nBad++; }
      else { outlier[i] = false; e->setLevel(0); }
      tr.changed += was != (bool)outlier[i];
      tr.reinlier += was && !outlier[i];
      if (it == 2) e->setRobustKernel(0);
    }
    tr.n_bad = nBad;
    g_prounds = (int)it + 1;
    if (optimizer.edges().size() < 10) break;
  }
  optimizer.removePostIterationAction(&post);
  optimizer.removeComputeErrorAction(&calls);
  g2o::VertexSE3Expmap* vr = static_cast<g2o::VertexSE3Expmap*>(optimizer.vertex(0));
  to7(vr->estimate(), pose7);
  return nInitialCorrespondences - nBad;
}

// The trace of the last ref_pose_optimize's round `round`; returns the number of rounds it ran (0: fewer than 3 edges), -1 for a round
// it did not run.  hdr[6] = {active edges at initializeOptimization(0), what optimize(10) returned (-1: no active vertex), nBad,
// flags the re-classification changed, of those outlier -> inlier, the edge nearest to the 5.991 gate}; misc[8] = {the estimate
// behind optimize(): 7, that edge's |chi2 - 5.991| / 5.991 as the re-classification read it}; trials[<= 10] per iteration
// (levenbergIteration()); calls[n_calls <= 110]: activeRobustChi2 after each computeActiveErrors of the round, in order (an iteration
// makes 1 + trials calls, levenberg.cpp:74, :119).  The compute-error action runs in front of the computation, so it reads what the
// call before it stored: its first reading predates the round and is dropped, the reading behind optimize() closes the list.
extern "C" int ref_pose_optimize_trace(int round, int32_t* hdr, double* misc, int32_t* trials, int32_t* n_iters, double* calls,
                                       int32_t* n_calls) {
  if (round < 0 || round >= g_prounds) return -1;
  const PoseRound& tr = g_pround[round];
  hdr[0] = tr.active; hdr[1] = tr.ret; hdr[2] = tr.n_bad; hdr[3] = tr.changed; hdr[4] = tr.reinlier; hdr[5] = tr.gate_edge;
  for (int q = 0; q < 7; ++q) misc[q] = tr.pose[q];
  misc[7] = tr.gate_margin;
  *n_iters = (int32_t)g_piters[round].size();
  for (size_t i = 0; i < g_piters[round].size() && i < 10; ++i) trials[i] = (int32_t)g_piters[round][i].trials;
  const std::vector<double>& c = g_pcalls[round];
  const size_t n = c.size() > 1 && tr.ret > 0 ? c.size() - 1 : 0;   // (a round without an active vertex computes nothing)
  *n_calls = (int32_t)n;
  for (size_t i = 0; i < n && i < 110; ++i) calls[i] = c[i + 1];
  return g_prounds;
}

extern "C" int ref_local_ba(int n_poses, int n_points, int n_edges, double* poses, const uint8_t* fixed, double* points,
                            const int32_t* e_point, const int32_t* e_pose, const double* e_obs, const double* e_info,
                            const double* K, int its1, int its2, double* edge_chi2, uint8_t* edge_depth_pos,
                            uint8_t* edge_outlier1, ref_ba_out* out) {
  g2o::SparseOptimizer optimizer;
  g2o::OptimizationAlgorithmLevenberg* solver = new g2o::OptimizationAlgorithmLevenberg(
      new g2o::BlockSolver_6_3(new g2o::LinearSolverDense<g2o::BlockSolver_6_3::PoseMatrixType>()));
  optimizer.setAlgorithm(solver);
  // keyframe vertices: id = pose index (poses arrive ordered by ascending KF id)
  for (int p = 0; p < n_poses; ++p) {
    g2o::VertexSE3Expmap* vSE3 = new g2o::VertexSE3Expmap();
    vSE3->setEstimate(from7(poses + 7 * p));
    vSE3->setId(p);
    vSE3->setFixed(fixed[p] != 0);
    optimizer.addVertex(vSE3);
  }
  const int maxKFid = n_poses - 1;
  const float thHuberMono = sqrt(5.991);
  std::vector<g2o::EdgeSE3ProjectXYZ*> vpEdgesMono(n_edges);
  for (int l = 0; l < n_points; ++l) {
    g2o::VertexSBAPointXYZ* vPoint = new g2o::VertexSBAPointXYZ();
    vPoint->setEstimate(Eigen::Vector3d(points[3 * l], points[3 * l + 1], points[3 * l + 2]));
    vPoint->setId(l + maxKFid + 1);
    vPoint->setMarginalized(true);
    vPoint->setFixed(false);
    optimizer.addVertex(vPoint);
  }
  for (int k = 0; k < n_edges; ++k) {
    Eigen::Matrix<double, 2, 1> o;
    o << e_obs[2 * k], e_obs[2 * k + 1];
    g2o::EdgeSE3ProjectXYZ* e = new g2o::EdgeSE3ProjectXYZ();
    e->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(e_point[k] + maxKFid + 1)));
    e->setVertex(1, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(e_pose[k])));
    e->setMeasurement(o);
    e->setInformation(Eigen::Matrix2d::Identity() * e_info[k]);
    g2o::RobustKernelHuber* rk = new g2o::RobustKernelHuber;
    e->setRobustKernel(rk);
    rk->setDelta(thHuberMono);
    e->fx = K[0]; e->fy = K[1]; e->cx = K[2]; e->cy = K[3];
    optimizer.addEdge(e);
    vpEdgesMono[k] = e;
  }
  // every edge's error at the input estimate.  optimize() computes the active errors at the start of its first iteration, so this
  // changes nothing when its1 >= 1; with its1 = 0 it computes none, and the gating below would read errors that were never
  // computed (uninitialised memory: two runs of one problem disagree).  The oracle and asd_local_ba gate on these.
  for (int k = 0; k < n_edges; ++k) vpEdgesMono[k]->computeError();
  PostIteration post(solver, g_iters);
  ComputeErrors calls(g_calls);
  optimizer.addPostIterationAction(&post);
  optimizer.addComputeErrorAction(&calls);
  for (int r = 0; r < 2; ++r) { g_iters[r].clear(); g_calls[r].clear(); }
  g_round = 0;
  optimizer.initializeOptimization();
  out->iters_first = optimizer.optimize(its1);
  out->chi2_first = optimizer.activeRobustChi2();  // from the edges' stored errors, nothing recomputed
  for (int k = 0; k < n_edges; ++k) {
    g2o::EdgeSE3ProjectXYZ* e = vpEdgesMono[k];
    const bool bad = e->chi2() > 5.991 || !e->isDepthPositive();
    edge_outlier1[k] = bad;
    if (bad) e->setLevel(1);
    e->setRobustKernel(0);
  }
  g_round = 1;
  optimizer.initializeOptimization(0);
  out->iters_second = optimizer.optimize(its2);
  optimizer.removePostIterationAction(&post);
  optimizer.removeComputeErrorAction(&calls);
  int trials[2] = {0, 0};
  for (int r = 0; r < 2; ++r)
    for (const LmIter& it : g_iters[r]) trials[r] += (int)it.trials;
  out->trials_first = trials[0];
  out->trials_second = trials[1];
  for (int k = 0; k < n_edges; ++k) {
    g2o::EdgeSE3ProjectXYZ* e = vpEdgesMono[k];
    edge_chi2[k] = e->chi2();
    edge_depth_pos[k] = e->isDepthPositive();
  }
  out->chi2_second = optimizer.activeChi2();
  for (int p = 0; p < n_poses; ++p)
    to7(static_cast<g2o::VertexSE3Expmap*>(optimizer.vertex(p))->estimate(), poses + 7 * p);
  for (int l = 0; l < n_points; ++l) {
    const Eigen::Vector3d& x = static_cast<g2o::VertexSBAPointXYZ*>(optimizer.vertex(l + maxKFid + 1))->estimate();
    points[3 * l] = x[0]; points[3 * l + 1] = x[1]; points[3 * l + 2] = x[2];
  }
  return 0;
}

// the trace of the last ref_local_ba's round `round`: iters[n_iters][3] = {trials, lambda, chi2} per iteration, calls[n_calls] = the
// compute-error action's readings (see g_calls).  With null buffers only the counts are returned.
extern "C" int ref_local_ba_trace(int round, double* iters, int32_t* n_iters, double* calls, int32_t* n_calls) {
  if (round < 0 || round > 1) return -1;
  *n_iters = (int32_t)g_iters[round].size();
  *n_calls = (int32_t)g_calls[round].size();
  if (iters)
    for (size_t i = 0; i < g_iters[round].size(); ++i) {
      iters[3 * i] = g_iters[round][i].trials; iters[3 * i + 1] = g_iters[round][i].lambda; iters[3 * i + 2] = g_iters[round][i].chi2;
    }
  if (calls)
    for (size_t i = 0; i < g_calls[round].size(); ++i) calls[i] = g_calls[round][i];
  return 0;
}
