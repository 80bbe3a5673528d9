// Driver of tests/golden/make_gba_golden.py: Optimizer::BundleAdjustment (reference src/vslam/src/Optimizer.cc:51-237) on the
// reference's own vendored g2o.  The graph of :57-173 is rebuilt from the flat arrays of asd_gba_problem: a VertexSE3Expmap per pose
// (id = pose index, the poses arrive by ascending keyframe id), then per point -- in point order, as the loop of :96-162 goes -- a
// marginalised VertexSBAPointXYZ with id = point index + maxKFid + 1, its edges in the caller's order, and the vertex removed again
// when it got none (:153-157).  Then initializeOptimization(); optimize(nIterations) (:172-173).  Compiled by the generator, together
// with the reference's g2o sources, into a temporary directory; nothing built from it is kept.
//
// Two entries that differ only in the solver: gba_ref_sparse is the reference's BlockSolverX + LinearSolverEigen (:59-61),
// gba_ref_dense is BlockSolver_6_3 + LinearSolverDense -- the same normal equations, factored densely, which is how the device
// factors them.
//
// Besides the result it reports, without changing the run: what optimize() returned, the trials of each iteration
// (levenbergIteration(), from a post-iteration action), activeRobustChi2() of the stored errors, and the time of :172-173.
// Every edge's error is computed once at the input estimate in front of the run: optimize() does that itself at the start of its
// first iteration, and a run without one (nIterations = 0, nothing to optimise) would otherwise report errors nobody computed.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <vector>

#include "g2o/core/block_solver.h"
#include "g2o/core/hyper_graph_action.h"
#include "g2o/core/optimization_algorithm_levenberg.h"
#include "g2o/core/robust_kernel_impl.h"
#include "g2o/solvers/linear_solver_dense.h"
#include "g2o/solvers/linear_solver_eigen.h"
#include "g2o/types/types_six_dof_expmap.h"

namespace {
struct PostIteration : g2o::HyperGraphAction {
  g2o::OptimizationAlgorithmLevenberg* lm;
  std::vector<int>* sink;
  PostIteration(g2o::OptimizationAlgorithmLevenberg* a, std::vector<int>* s) : lm(a), sink(s) {}
  g2o::HyperGraphAction* operator()(const g2o::HyperGraph*, Parameters* = 0) {
    sink->push_back(lm->levenbergIteration());
    return this;
  }
};

g2o::SE3Quat from7(const double* p) {
  return g2o::SE3Quat(Eigen::Quaterniond(p[3], p[0], p[1], p[2]), Eigen::Vector3d(p[4], p[5], p[6]));
}
void to7(const g2o::SE3Quat& T, double* p) {
  const Eigen::Quaterniond& q = T.rotation();
  p[0] = q.x(); p[1] = q.y(); p[2] = q.z(); p[3] = q.w();
  p[4] = T.translation()[0]; p[5] = T.translation()[1]; p[6] = T.translation()[2];
}

// info[4] = {optimize()'s return, iterations the action saw, trials in all, vertices the optimiser kept (points removed at :155 are
// gone)}; trials[cap] per iteration (-1 behind the last); dout[2] = {activeRobustChi2 of the stored errors, seconds of :172-173}
int run(g2o::OptimizationAlgorithmLevenberg* solver, int n_poses, int n_points, int n_edges, double* poses, const uint8_t* fixed,
        double* points, const int32_t* e_point, const int32_t* e_pose, const double* e_obs, const double* e_info, const double* K,
        int n_iterations, int robust, double* edge_chi2, int32_t* info, int32_t* trials, int cap, double* dout) {
  g2o::SparseOptimizer optimizer;
  optimizer.setAlgorithm(solver);
  for (int p = 0; p < n_poses; ++p) {
    g2o::VertexSE3Expmap* vSE3 = new g2o::VertexSE3Expmap();
    vSE3->setEstimate(from7(poses + 7 * p));
    vSE3->setId(p);
    vSE3->setFixed(fixed[p] != 0);
    optimizer.addVertex(vSE3);
  }
  const int maxKFid = n_poses - 1;
  const float thHuber2D = sqrt(5.99);
  std::vector<std::vector<int> > of_point(n_points);
  for (int k = 0; k < n_edges; ++k) of_point[e_point[k]].push_back(k);
  std::vector<g2o::EdgeSE3ProjectXYZ*> edges(n_edges, (g2o::EdgeSE3ProjectXYZ*)0);
  std::vector<uint8_t> not_included(n_points, 0);
  for (int l = 0; l < n_points; ++l) {
    g2o::VertexSBAPointXYZ* vPoint = new g2o::VertexSBAPointXYZ();
    vPoint->setEstimate(Eigen::Vector3d(points[3 * l], points[3 * l + 1], points[3 * l + 2]));
    const int id = l + maxKFid + 1;
    vPoint->setId(id);
    vPoint->setMarginalized(true);
    optimizer.addVertex(vPoint);
    int nEdges = 0;
    for (size_t q = 0; q < of_point[l].size(); ++q) {
      const int k = of_point[l][q];
      nEdges++;
      Eigen::Matrix<double, 2, 1> obs;
      obs << e_obs[2 * k], e_obs[2 * k + 1];
      g2o::EdgeSE3ProjectXYZ* e = new g2o::EdgeSE3ProjectXYZ();
      e->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(id)));
      e->setVertex(1, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(e_pose[k])));
      e->setMeasurement(obs);
      e->setInformation(Eigen::Matrix2d::Identity() * e_info[k]);
      if (robust) {
        g2o::RobustKernelHuber* rk = new g2o::RobustKernelHuber;
        e->setRobustKernel(rk);
        rk->setDelta(thHuber2D);
      }
      e->fx = K[0]; e->fy = K[1]; e->cx = K[2]; e->cy = K[3];
      optimizer.addEdge(e);
      edges[k] = e;
    }
    if (nEdges == 0) {
      optimizer.removeVertex(vPoint);
      not_included[l] = 1;
    }
  }
  for (int k = 0; k < n_edges; ++k) edges[k]->computeError();
  std::vector<int> per_iteration;
  PostIteration post(solver, &per_iteration);
  optimizer.addPostIterationAction(&post);
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  optimizer.initializeOptimization();
  const int ret = optimizer.optimize(n_iterations);
  dout[1] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  optimizer.removePostIterationAction(&post);
  info[0] = ret;
  info[1] = (int32_t)per_iteration.size();
  info[2] = 0;
  info[3] = (int32_t)optimizer.vertices().size();
  for (int q = 0; q < cap; ++q) trials[q] = -1;
  for (size_t q = 0; q < per_iteration.size(); ++q) {
    info[2] += per_iteration[q];
    if ((int)q < cap) trials[q] = per_iteration[q];
  }
  dout[0] = optimizer.activeEdges().empty() ? 0.0 : optimizer.activeRobustChi2();
  for (int k = 0; k < n_edges; ++k) edge_chi2[k] = edges[k]->chi2();
  for (int p = 0; p < n_poses; ++p)
    to7(static_cast<g2o::VertexSE3Expmap*>(optimizer.vertex(p))->estimate(), poses + 7 * p);
  for (int l = 0; l < n_points; ++l) {
    if (not_included[l]) continue;
    const Eigen::Vector3d& x = static_cast<g2o::VertexSBAPointXYZ*>(optimizer.vertex(l + maxKFid + 1))->estimate();
    points[3 * l] = x[0]; points[3 * l + 1] = x[1]; points[3 * l + 2] = x[2];
  }
  return 0;
}
}  // namespace

#define GBA_ARGS                                                                                                                    \
  int n_poses, int n_points, int n_edges, double *poses, const uint8_t *fixed, double *points, const int32_t *e_point,             \
      const int32_t *e_pose, const double *e_obs, const double *e_info, const double *K, int n_iterations, int robust,              \
      double *edge_chi2, int32_t *info, int32_t *trials, int cap, double *dout
#define GBA_PASS                                                                                                                    \
  n_poses, n_points, n_edges, poses, fixed, points, e_point, e_pose, e_obs, e_info, K, n_iterations, robust, edge_chi2, info,       \
      trials, cap, dout

extern "C" int gba_ref_sparse(GBA_ARGS) {
  return run(new g2o::OptimizationAlgorithmLevenberg(
                 new g2o::BlockSolverX(new g2o::LinearSolverEigen<g2o::BlockSolverX::PoseMatrixType>())),
             GBA_PASS);
}

extern "C" int gba_ref_dense(GBA_ARGS) {
  return run(new g2o::OptimizationAlgorithmLevenberg(
                 new g2o::BlockSolver_6_3(new g2o::LinearSolverDense<g2o::BlockSolver_6_3::PoseMatrixType>())),
             GBA_PASS);
}
