// Driver of tests/golden/make_sim3_golden.py: Optimizer::OptimizeSim3 (reference src/vslam/src/Optimizer.cc:1002-1194) on the
// reference's own vendored g2o.  The graph of :1004-1131 is rebuilt from flat arrays -- one pair per correspondence the reference adds
// edges for -- and the schedule of :1133-1193 runs as written there.  Compiled by the generator, together with the reference's g2o
// sources, into a temporary directory; nothing built from it is kept.
//
// Besides the result it reports, without changing the run:
//  - per round, the active edges after initializeOptimization(), what optimize() returned, the trials of each iteration
//    (levenbergIteration(), from a post-iteration action) and whether the round ended on a rejected trial: the estimate that the
//    round's last computeActiveErrors evaluated (seen by a compute-error action, which runs in front of the computation) is not, bit
//    for bit, the estimate optimize() left -- the trial was popped, the edges' stored errors are still the trial's;
//  - the smallest |chi2 / th2 - 1| over every chi2 either re-classification read.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <vector>

#include "g2o/core/block_solver.h"
#include "g2o/core/hyper_graph_action.h"
#include "g2o/core/optimization_algorithm_levenberg.h"
#include "g2o/core/robust_kernel_impl.h"
#include "g2o/solvers/linear_solver_dense.h"
#include "g2o/types/types_seven_dof_expmap.h"

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

struct ComputeErrors : g2o::HyperGraphAction {
  const g2o::VertexSim3Expmap* v;
  double* at;   // [8]: the estimate the last computeActiveErrors evaluated
  ComputeErrors(const g2o::VertexSim3Expmap* v_, double* at_) : v(v_), at(at_) {}
  g2o::HyperGraphAction* operator()(const g2o::HyperGraph*, Parameters* = 0) {
    for (int k = 0; k < 8; ++k) at[k] = v->estimate()[k];
    return this;
  }
};
}  // namespace

// sim3[8] in/out: qx qy qz qw tx ty tz s.  info[8] = nBad, early return, per round: active edges, optimize()'s return, ended on a
// rejected trial (-1 where the round did not run).  trials[2][10]: trials per iteration, -1 beyond.  dinfo[2] = gate margin, seconds.
extern "C" int sim3_ref_optimize(double* sim3, int n, const double* P1c, const double* P2c, const double* obs1, const double* obs2,
                                 const double* inv_sigma2_1, const double* inv_sigma2_2, const double* K1, const double* K2,
                                 float th2, int fix_scale, uint8_t* keep, int32_t* info, int32_t* trials, double* dinfo) {
  const auto t_start = std::chrono::steady_clock::now();
  g2o::SparseOptimizer optimizer;
  g2o::OptimizationAlgorithmLevenberg* solver = new g2o::OptimizationAlgorithmLevenberg(
      new g2o::BlockSolverX(new g2o::LinearSolverDense<g2o::BlockSolverX::PoseMatrixType>()));
  optimizer.setAlgorithm(solver);

  g2o::VertexSim3Expmap* vSim3 = new g2o::VertexSim3Expmap();
  vSim3->_fix_scale = fix_scale != 0;
  vSim3->setEstimate(g2o::Sim3(Eigen::Quaterniond(sim3[3], sim3[0], sim3[1], sim3[2]), Eigen::Vector3d(sim3[4], sim3[5], sim3[6]), sim3[7]));
  vSim3->setId(0);
  vSim3->setFixed(false);
  vSim3->_principle_point1[0] = K1[2];
  vSim3->_principle_point1[1] = K1[3];
  vSim3->_focal_length1[0] = K1[0];
  vSim3->_focal_length1[1] = K1[1];
  vSim3->_principle_point2[0] = K2[2];
  vSim3->_principle_point2[1] = K2[3];
  vSim3->_focal_length2[0] = K2[0];
  vSim3->_focal_length2[1] = K2[1];
  optimizer.addVertex(vSim3);

  std::vector<g2o::EdgeSim3ProjectXYZ*> vpEdges12;
  std::vector<g2o::EdgeInverseSim3ProjectXYZ*> vpEdges21;
  const float deltaHuber = sqrt(th2);
  int nCorrespondences = 0;
  for (int i = 0; i < n; i++) {
    const int id1 = 2 * i + 1;
    const int id2 = 2 * (i + 1);
    g2o::VertexSBAPointXYZ* vPoint1 = new g2o::VertexSBAPointXYZ();
    vPoint1->setEstimate(Eigen::Vector3d(P1c[3 * i], P1c[3 * i + 1], P1c[3 * i + 2]));
    vPoint1->setId(id1);
    vPoint1->setFixed(true);
    optimizer.addVertex(vPoint1);
    g2o::VertexSBAPointXYZ* vPoint2 = new g2o::VertexSBAPointXYZ();
    vPoint2->setEstimate(Eigen::Vector3d(P2c[3 * i], P2c[3 * i + 1], P2c[3 * i + 2]));
    vPoint2->setId(id2);
    vPoint2->setFixed(true);
    optimizer.addVertex(vPoint2);
    nCorrespondences++;
    keep[i] = 1;

    Eigen::Matrix<double, 2, 1> o1;
    o1 << obs1[2 * i], obs1[2 * i + 1];
    g2o::EdgeSim3ProjectXYZ* e12 = new g2o::EdgeSim3ProjectXYZ();
    e12->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(id2)));
    e12->setVertex(1, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(0)));
    e12->setMeasurement(o1);
    e12->setInformation(Eigen::Matrix2d::Identity() * inv_sigma2_1[i]);
    g2o::RobustKernelHuber* rk1 = new g2o::RobustKernelHuber;
    e12->setRobustKernel(rk1);
    rk1->setDelta(deltaHuber);
    optimizer.addEdge(e12);

    Eigen::Matrix<double, 2, 1> o2;
    o2 << obs2[2 * i], obs2[2 * i + 1];
    g2o::EdgeInverseSim3ProjectXYZ* e21 = new g2o::EdgeInverseSim3ProjectXYZ();
    e21->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(id1)));
    e21->setVertex(1, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(0)));
    e21->setMeasurement(o2);
    e21->setInformation(Eigen::Matrix2d::Identity() * inv_sigma2_2[i]);
    g2o::RobustKernelHuber* rk2 = new g2o::RobustKernelHuber;
    e21->setRobustKernel(rk2);
    rk2->setDelta(deltaHuber);
    optimizer.addEdge(e21);

    vpEdges12.push_back(e12);
    vpEdges21.push_back(e21);
  }

  for (int k = 0; k < 8; ++k) info[k] = -1;
  for (int k = 0; k < 20; ++k) trials[k] = -1;
  double margin = 1e300;
  auto gate = [&](double chi2) {
    const double m = std::fabs(chi2 / (double)th2 - 1.0);
    if (!(m >= margin)) margin = m;   // (a NaN is kept: it fails every test)
  };
  std::vector<int> its;
  PostIteration post(solver, &its);
  optimizer.addPostIterationAction(&post);
  double at[8];
  ComputeErrors calls(vSim3, at);
  optimizer.addComputeErrorAction(&calls);
  auto report_round = [&](int r, int ret) {
    info[2 + 3 * r] = (int)optimizer.activeEdges().size();
    info[3 + 3 * r] = ret;
    bool moved = false;
    for (int k = 0; k < 8; ++k) moved |= at[k] != vSim3->estimate()[k];
    info[4 + 3 * r] = ret > 0 && moved ? 1 : 0;
    for (size_t k = 0; k < its.size() && k < 10; ++k) trials[10 * r + k] = its[k];
    its.clear();
  };
  auto finish = [&](int ret) {
    optimizer.removePostIterationAction(&post);
    optimizer.removeComputeErrorAction(&calls);
    dinfo[0] = margin;
    dinfo[1] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    return ret;
  };

  optimizer.initializeOptimization();
  const int ret0 = optimizer.optimize(5);
  report_round(0, ret0);

  int nBad = 0;
  for (size_t i = 0; i < vpEdges12.size(); i++) {
    g2o::EdgeSim3ProjectXYZ* e12 = vpEdges12[i];
    g2o::EdgeInverseSim3ProjectXYZ* e21 = vpEdges21[i];
    if (!e12 || !e21) continue;
    gate(e12->chi2());
    gate(e21->chi2());
    if (e12->chi2() > th2 || e21->chi2() > th2) {
      keep[i] = 0;
      optimizer.removeEdge(e12);
      optimizer.removeEdge(e21);
      vpEdges12[i] = static_cast<g2o::EdgeSim3ProjectXYZ*>(NULL);
      vpEdges21[i] = static_cast<g2o::EdgeInverseSim3ProjectXYZ*>(NULL);
      nBad++;
    }
  }
  info[0] = nBad;
  int nMoreIterations;
  if (nBad > 0)
    nMoreIterations = 10;
  else
    nMoreIterations = 5;
  info[1] = nCorrespondences - nBad < 10 ? 1 : 0;
  if (nCorrespondences - nBad < 10) return finish(0);

  optimizer.initializeOptimization();
  const int ret1 = optimizer.optimize(nMoreIterations);
  report_round(1, ret1);

  int nIn = 0;
  for (size_t i = 0; i < vpEdges12.size(); i++) {
    g2o::EdgeSim3ProjectXYZ* e12 = vpEdges12[i];
    g2o::EdgeInverseSim3ProjectXYZ* e21 = vpEdges21[i];
    if (!e12 || !e21) continue;
    gate(e12->chi2());
    gate(e21->chi2());
    if (e12->chi2() > th2 || e21->chi2() > th2)
      keep[i] = 0;
    else
      nIn++;
  }
  const g2o::Sim3 S = static_cast<g2o::VertexSim3Expmap*>(optimizer.vertex(0))->estimate();
  sim3[0] = S.rotation().x(); sim3[1] = S.rotation().y(); sim3[2] = S.rotation().z(); sim3[3] = S.rotation().w();
  sim3[4] = S.translation()[0]; sim3[5] = S.translation()[1]; sim3[6] = S.translation()[2];
  sim3[7] = S.scale();
  return finish(nIn);
}
