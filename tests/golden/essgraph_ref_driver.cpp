// Driver of tests/golden/make_essgraph_golden.py: Optimizer::OptimizeEssentialGraph (reference src/vslam/src/Optimizer.cc:737-1000)
// on the reference's own vendored g2o.  The graph of :743-939 is rebuilt from flat keyframe views (the arrays of
// synth.essential_graph: row = position in GetAllKeyFrames(); the reference's sets and maps of KeyFrame* are walked in the order the
// views list them): a VertexSim3Expmap per keyframe with id = mnId, the LoopConnections edges, then per keyframe its spanning-tree
// edge, its loop edges and its covisibility edges, with the rules as written there.  Then initializeOptimization(); optimize(its)
// (:942-943), the pose recovery (:947-966) and the map-point correction (:968-999).  Compiled by the generator, together with the
// reference's g2o sources, into a temporary directory; nothing built from it is kept.
//
// Two solvers: the reference's BlockSolver_7_3 + LinearSolverEigen (:746-748), and BlockSolver_7_3 + LinearSolverDense -- the same
// normal equations factored densely, as the device factors them.
//
// Besides the result it reports, without changing the run: the edge list with its measurements and the entry estimates vScw, what
// optimize() returned, the trials of each iteration (levenbergIteration(), from a post-iteration action), activeChi2() and every
// edge's chi2() of the stored errors, and the time of :942-943.  Every edge's error is computed once at the entry estimate in front
// of the run (see gba_ref_driver.cpp).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <map>
#include <set>
#include <vector>

#include "g2o/core/block_solver.h"
#include "g2o/core/hyper_graph_action.h"
#include "g2o/core/optimization_algorithm_levenberg.h"
#include "g2o/solvers/linear_solver_dense.h"
#include "g2o/solvers/linear_solver_eigen.h"
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

// in front of every computeActiveErrors: activeChi2() of the errors stored so far, i.e. of the evaluation before
struct ChiLog : g2o::HyperGraphAction {
  g2o::SparseOptimizer* opt;
  std::vector<double>* sink;
  ChiLog(g2o::SparseOptimizer* o, std::vector<double>* s) : opt(o), sink(s) {}
  g2o::HyperGraphAction* operator()(const g2o::HyperGraph*, Parameters* = 0) {
    sink->push_back(opt->activeEdges().empty() ? 0.0 : opt->activeChi2());
    return this;
  }
};

g2o::Sim3 from8(const double* p) {
  return g2o::Sim3(Eigen::Quaterniond(p[3], p[0], p[1], p[2]), Eigen::Vector3d(p[4], p[5], p[6]), p[7]);
}
void to8(const g2o::Sim3& S, double* p) {
  for (int k = 0; k < 8; ++k) p[k] = S[k];
}
}  // namespace

// hdr[8] = {keyframes, map points, LoopConnections entries, pLoopKF row, pCurKF row, bFixScale, iterations, dense solver}
// info[5] = {optimize()'s return, iterations the action saw, trials in all, edges}; trials[cap] per iteration (-1 behind the last);
// dout[2] = {activeChi2 of the stored errors, seconds of :942-943}.  evals[evals_cap]: activeChi2 behind every computeActiveErrors of the
// run in order (the head of each iteration, then each of its trials), info[4] = their number.  Returns -1 when edge_cap is too small.
extern "C" int essgraph_ref(const int32_t* hdr, const int64_t* mnId, const float* Tcw, const int32_t* parent, const int32_t* child_start,
                            const int32_t* child, const int32_t* loop_start, const int32_t* loop, const int32_t* cov_start,
                            const int32_t* cov, const int32_t* cov_w, const uint8_t* corrected, const double* corrected_sim3,
                            const uint8_t* noncorrected, const double* noncorrected_sim3, const int32_t* lc_kf, const int32_t* lc_start,
                            const int32_t* lc, const float* mp_Xw, const int32_t* mp_ref, const int64_t* mp_corrected_by,
                            const int64_t* mp_corrected_ref, int32_t edge_cap, int32_t* e_i, int32_t* e_j, double* e_meas,
                            double* sim3_in, double* sim3_out, float* Tiw_out, float* mp_out, double* edge_chi2, int32_t* info,
                            int32_t* trials, int32_t cap, double* dout, double* evals, int32_t evals_cap) {
  const int nKF = hdr[0], nMP = hdr[1], nLC = hdr[2], loopRow = hdr[3], curRow = hdr[4], its = hdr[6];
  const bool bFixScale = hdr[5] != 0, dense = hdr[7] != 0;
  g2o::SparseOptimizer optimizer;
  optimizer.setVerbose(false);
  g2o::OptimizationAlgorithmLevenberg* solver =
      dense ? new g2o::OptimizationAlgorithmLevenberg(new g2o::BlockSolver_7_3(new g2o::LinearSolverDense<g2o::BlockSolver_7_3::PoseMatrixType>()))
            : new g2o::OptimizationAlgorithmLevenberg(new g2o::BlockSolver_7_3(new g2o::LinearSolverEigen<g2o::BlockSolver_7_3::PoseMatrixType>()));
  solver->setUserLambdaInit(1e-16);
  optimizer.setAlgorithm(solver);

  long nMaxKFid = 0;
  std::map<long, int> row_of_id;
  for (int i = 0; i < nKF; ++i) { nMaxKFid = std::max<long>(nMaxKFid, mnId[i]); row_of_id[mnId[i]] = i; }
  std::vector<g2o::Sim3, Eigen::aligned_allocator<g2o::Sim3> > vScw(nMaxKFid + 1);
  std::vector<g2o::Sim3, Eigen::aligned_allocator<g2o::Sim3> > vCorrectedSwc(nMaxKFid + 1);
  const int minFeat = 100;
  // KeyFrame::GetWeight: the weight of a connected keyframe, 0 otherwise
  auto GetWeight = [&](int a, int b) {
    for (int k = cov_start[a]; k < cov_start[a + 1]; ++k) if (cov[k] == b) return (int)cov_w[k];
    return 0;
  };

  // Set KeyFrame vertices (:765-800)
  for (int i = 0; i < nKF; i++) {
    g2o::VertexSim3Expmap* VSim3 = new g2o::VertexSim3Expmap();
    const int nIDi = (int)mnId[i];
    if (corrected[i]) {
      vScw[nIDi] = from8(corrected_sim3 + 8 * i);
      VSim3->setEstimate(vScw[nIDi]);
    } else {
      Eigen::Matrix<double, 3, 3> Rcw;
      Eigen::Matrix<double, 3, 1> tcw;
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Rcw(r, c) = Tcw[16 * i + 4 * r + c];
        tcw(r) = Tcw[16 * i + 4 * r + 3];
      }
      g2o::Sim3 Siw(Rcw, tcw, 1.0);
      vScw[nIDi] = Siw;
      VSim3->setEstimate(Siw);
    }
    if (i == loopRow) VSim3->setFixed(true);
    VSim3->setId(nIDi);
    VSim3->setMarginalized(false);
    VSim3->_fix_scale = bFixScale;
    optimizer.addVertex(VSim3);
    to8(vScw[nIDi], sim3_in + 8 * i);
  }

  std::set<std::pair<long unsigned int, long unsigned int> > sInsertedEdges;
  const Eigen::Matrix<double, 7, 7> matLambda = Eigen::Matrix<double, 7, 7>::Identity();
  std::vector<g2o::EdgeSim3*> edges;
  std::vector<std::pair<int, int> > rows;
  auto add = [&](long idI, long idJ, const g2o::Sim3& Sji) {
    g2o::EdgeSim3* e = new g2o::EdgeSim3();
    e->setVertex(1, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(idJ)));
    e->setVertex(0, dynamic_cast<g2o::OptimizableGraph::Vertex*>(optimizer.vertex(idI)));
    e->setMeasurement(Sji);
    e->information() = matLambda;
    optimizer.addEdge(e);
    edges.push_back(e);
    rows.push_back(std::make_pair(row_of_id[idI], row_of_id[idJ]));
  };

  // Set Loop edges (:808-836)
  for (int m = 0; m < nLC; ++m) {
    const int i = lc_kf[m];
    const long unsigned int nIDi = mnId[i];
    const g2o::Sim3 Siw = vScw[nIDi];
    const g2o::Sim3 Swi = Siw.inverse();
    for (int k = lc_start[m]; k < lc_start[m + 1]; ++k) {
      const int j = lc[k];
      const long unsigned int nIDj = mnId[j];
      if ((nIDi != (long unsigned int)mnId[curRow] || nIDj != (long unsigned int)mnId[loopRow]) && GetWeight(i, j) < minFeat) continue;
      const g2o::Sim3 Sjw = vScw[nIDj];
      const g2o::Sim3 Sji = Sjw * Swi;
      add(nIDi, nIDj, Sji);
      sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
    }
  }

  // Set normal edges (:839-939)
  for (int i = 0; i < nKF; i++) {
    const int nIDi = (int)mnId[i];
    g2o::Sim3 Swi;
    if (noncorrected[i]) Swi = from8(noncorrected_sim3 + 8 * i).inverse();
    else Swi = vScw[nIDi].inverse();
    const int pa = parent[i];
    // Spanning tree edge
    if (pa >= 0) {
      const int nIDj = (int)mnId[pa];
      g2o::Sim3 Sjw;
      if (noncorrected[pa]) Sjw = from8(noncorrected_sim3 + 8 * pa);
      else Sjw = vScw[nIDj];
      g2o::Sim3 Sji = Sjw * Swi;
      add(nIDi, nIDj, Sji);
    }
    // Loop edges
    std::set<int> sLoopEdges(loop + loop_start[i], loop + loop_start[i + 1]);
    for (int k = loop_start[i]; k < loop_start[i + 1]; ++k) {
      const int l = loop[k];
      if (mnId[l] < mnId[i]) {
        g2o::Sim3 Slw;
        if (noncorrected[l]) Slw = from8(noncorrected_sim3 + 8 * l);
        else Slw = vScw[mnId[l]];
        g2o::Sim3 Sli = Slw * Swi;
        add(nIDi, mnId[l], Sli);
      }
    }
    // Covisibility graph edges: GetCovisiblesByWeight(minFeat) is the head of the ordered list with weight >= minFeat
    for (int k = cov_start[i]; k < cov_start[i + 1] && cov_w[k] >= minFeat; ++k) {
      const int nb = cov[k];
      const bool hasChild = std::find(child + child_start[i], child + child_start[i + 1], nb) != child + child_start[i + 1];
      if (nb != pa && !hasChild && !sLoopEdges.count(nb)) {
        if (mnId[nb] < mnId[i]) {
          if (sInsertedEdges.count(std::make_pair((long unsigned int)std::min(mnId[i], mnId[nb]), (long unsigned int)std::max(mnId[i], mnId[nb]))))
            continue;
          g2o::Sim3 Snw;
          if (noncorrected[nb]) Snw = from8(noncorrected_sim3 + 8 * nb);
          else Snw = vScw[mnId[nb]];
          g2o::Sim3 Sni = Snw * Swi;
          add(nIDi, mnId[nb], Sni);
        }
      }
    }
  }
  const int nE = (int)edges.size();
  if (nE > edge_cap) return -1;
  for (int k = 0; k < nE; ++k) {
    e_i[k] = rows[k].first; e_j[k] = rows[k].second;
    to8(edges[k]->measurement(), e_meas + 8 * k);
    edges[k]->computeError();
  }

  // Optimize! (:942-943)
  std::vector<int> per_iteration;
  PostIteration post(solver, &per_iteration);
  optimizer.addPostIterationAction(&post);
  std::vector<double> chi_before;
  ChiLog chilog(&optimizer, &chi_before);
  const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  optimizer.initializeOptimization();
  optimizer.addComputeErrorAction(&chilog);
  const int ret = optimizer.optimize(its);
  optimizer.removeComputeErrorAction(&chilog);
  dout[1] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  optimizer.removePostIterationAction(&post);
  info[0] = ret;
  info[1] = (int32_t)per_iteration.size();
  info[2] = 0;
  info[3] = nE;
  for (int q = 0; q < cap; ++q) trials[q] = -1;
  for (size_t q = 0; q < per_iteration.size(); ++q) {
    info[2] += per_iteration[q];
    if ((int)q < cap) trials[q] = per_iteration[q];
  }
  dout[0] = optimizer.activeEdges().empty() ? 0.0 : optimizer.activeChi2();
  for (int k = 0; k < nE; ++k) edge_chi2[k] = edges[k]->chi2();
  // evaluation k was logged in front of evaluation k + 1; the last one is what is stored now
  info[4] = (int32_t)chi_before.size();
  for (int k = 0; k < evals_cap; ++k) evals[k] = k + 1 < (int)chi_before.size() ? chi_before[k + 1] : (k + 1 == (int)chi_before.size() ? dout[0] : 0.0);

  // SE3 Pose Recovering. Sim3:[sR t;0 1] -> SE3:[R t/s;0 1] (:947-966)
  for (int i = 0; i < nKF; i++) {
    const int nIDi = (int)mnId[i];
    g2o::VertexSim3Expmap* VSim3 = static_cast<g2o::VertexSim3Expmap*>(optimizer.vertex(nIDi));
    g2o::Sim3 CorrectedSiw = VSim3->estimate();
    to8(CorrectedSiw, sim3_out + 8 * i);
    vCorrectedSwc[nIDi] = CorrectedSiw.inverse();
    Eigen::Matrix3d eigR = CorrectedSiw.rotation().toRotationMatrix();
    Eigen::Vector3d eigt = CorrectedSiw.translation();
    double s = CorrectedSiw.scale();
    eigt *= (1. / s);
    float* T = Tiw_out + 16 * i;   // Converter::toCvSE3: CV_32F
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) T[4 * r + c] = (float)eigR(r, c);
      T[4 * r + 3] = (float)eigt(r);
    }
    T[12] = T[13] = T[14] = 0.f;
    T[15] = 1.f;
  }

  // Correct points (:968-999)
  for (int i = 0; i < nMP; i++) {
    int nIDr;
    if (mp_corrected_by[i] == mnId[curRow]) nIDr = (int)mp_corrected_ref[i];
    else nIDr = (int)mnId[mp_ref[i]];
    g2o::Sim3 Srw = vScw[nIDr];
    g2o::Sim3 correctedSwr = vCorrectedSwc[nIDr];
    Eigen::Matrix<double, 3, 1> eigP3Dw;
    eigP3Dw << mp_Xw[3 * i], mp_Xw[3 * i + 1], mp_Xw[3 * i + 2];
    Eigen::Matrix<double, 3, 1> eigCorrectedP3Dw = correctedSwr.map(Srw.map(eigP3Dw));
    for (int k = 0; k < 3; ++k) mp_out[3 * i + k] = (float)eigCorrectedP3Dw(k);
  }
  return 0;
}
