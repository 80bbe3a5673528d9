// ba_structure.h -- the active structure of a bundle adjustment round, built on the host.  Plain C++17, no HIP: LocalBA's host path
// (ASD_BA_STRUCT=host, more than 32 free poses, duplicate observations), BundleAdjustment and host/test_ba_structure.cpp share it.
//
// g2o's initializeOptimization + buildStructure (sparse_optimizer.cpp:206-267, 166-190; block_solver.hpp:117-300) as the solver keeps
// them: h-indices of the free poses / active landmarks, the edges grouped by landmark (CSR) and ordered by pose h-index inside a
// landmark (fixed poses, -1, first; equal poses in edge order), every free pose's edge list, and per upper block (i <= j) of the
// reduced pose system the list of edge pairs (a, b) that meet in it.  The k_ba_struct_* kernels (ba.hip) produce the same lists.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// Where each table sits in the structure block (sblk on the device, h_sblk pinned on the host): byte offsets, 256-byte aligned.  The
// counts may be upper bounds (the device-built path sizes by P, L, E); a caller's own tables go behind `bytes` with place().
struct BaStructLayout {
  size_t bytes = 0;
  size_t act, pose_h, pt_h, pose_of_h, pt_of_h, pt_start, ps_start, ps_edges, ps_h, blk_i, blk_j, pair_start, pairs, pair_h;
  size_t place(size_t n) { const size_t o = bytes; bytes += (std::max<size_t>(n, 1) + 255) / 256 * 256; return o; }
  // nps: entries of ps_edges / ps_h; pairs are int2
  BaStructLayout(size_t P, size_t L, size_t nPf, size_t nLa, size_t Ea, size_t nps, size_t nblk, size_t npairs) {
    act = place(Ea * 4); pose_h = place(P * 4); pt_h = place(L * 4); pose_of_h = place(nPf * 4); pt_of_h = place(nLa * 4);
    pt_start = place((nLa + 1) * 4); ps_start = place((nPf + 1) * 4); ps_edges = place(nps * 4); ps_h = place(nps * 4);
    blk_i = place(nblk * 4); blk_j = place(nblk * 4); pair_start = place((nblk + 1) * 4); pairs = place(npairs * 8); pair_h = place(npairs * 4);
  }
};

struct BaStructure {
  int P = 0, L = 0, nPf = 0, nLa = 0, Ea = 0, nblk = 0;
  size_t npairs = 0;
  bool all_blocks = true;

  // Step 1: the vertex tables, the landmark CSR and the pair count of every upper block; afterwards nPf, nLa, Ea and npairs are known.
  void count(int P_, int L_, int E, const int* e_pose, const int* e_point, const uint8_t* fixed, bool all = true) {
    P = P_; L = L_; Ea = E;
    std::vector<uint8_t> pa(P, 0), la(L, 0);
    for (int e = 0; e < E; ++e) { pa[e_pose[e]] = 1; la[e_point[e]] = 1; }
    pose_h.assign(P, -1); pt_h.assign(L, -1); pose_of_h.clear(); pt_of_h.clear();
    for (int p = 0; p < P; ++p) if (pa[p] && !fixed[p]) { pose_h[p] = (int)pose_of_h.size(); pose_of_h.push_back(p); }
    for (int l = 0; l < L; ++l) if (la[l]) { pt_h[l] = (int)pt_of_h.size(); pt_of_h.push_back(l); }
    nPf = (int)pose_of_h.size(); nLa = (int)pt_of_h.size();
    pt_start.assign(nLa + 1, 0);
    for (int e = 0; e < E; ++e) ++pt_start[pt_h[e_point[e]] + 1];
    for (int h = 0; h < nLa; ++h) pt_start[h + 1] += pt_start[h];
    act.assign(Ea, 0);
    ph_of_k.assign(Ea, -1);   // pose h-index of the k-th edge in act order (-1 = fixed pose)
    std::vector<int> cursor(pt_start.begin(), pt_start.end() - 1);
    for (int e = 0; e < E; ++e) act[cursor[pt_h[e_point[e]]]++] = e;
    for (int h = 0; h < nLa; ++h) {   // stable insertion sort: a landmark has a handful of observations
      const int s0 = pt_start[h], s1 = pt_start[h + 1];
      for (int a = s0; a < s1; ++a) ph_of_k[a] = pose_h[e_pose[act[a]]];
      for (int a = s0 + 1; a < s1; ++a) {
        const int ea = act[a], pa_ = ph_of_k[a];
        int b = a - 1;
        while (b >= s0 && ph_of_k[b] > pa_) { act[b + 1] = act[b]; ph_of_k[b + 1] = ph_of_k[b]; --b; }
        act[b + 1] = ea; ph_of_k[b + 1] = pa_;
      }
    }
    ps_start.assign(nPf + 1, 0);
    for (int k = 0; k < Ea; ++k) if (ph_of_k[k] >= 0) ++ps_start[ph_of_k[k] + 1];
    for (int h = 0; h < nPf; ++h) ps_start[h + 1] += ps_start[h];
    // pairs per upper block, blocks numbered row-major over the upper triangle: block id = row_off[i] + j
    row_off.assign(nPf, 0);
    for (int i = 0; i < nPf; ++i) row_off[i] = i * nPf - i * (i - 1) / 2 - i;
    cnt.assign((size_t)nPf * (nPf + 1) / 2, 0);
    npairs = 0;
    for_each_pair([&](int q, int, int, int, bool twice) { cnt[q] += 1 + twice; npairs += 1 + twice; });
    select_blocks(all);
  }

  // Which upper blocks get a slot.  true: every one, also those no landmark connects (LocalBA and the LDS solver forms rewrite the whole
  // packed system on every trial); false: the diagonal blocks and the off-diagonal blocks with at least one pair (a map's covisibility
  // is banded).  count() ends with it; BundleAdjustment, which decides from nPf, calls it once more.
  void select_blocks(bool all) {
    all_blocks = all;
    nblk = 0;
    for (int i = 0; i < nPf; ++i)
      for (int j = i; j < nPf; ++j) nblk += all || i == j || cnt[row_off[i] + j] > 0;
  }

  BaStructLayout layout() const { return BaStructLayout(P, L, nPf, nLa, Ea, ps_start[nPf], nblk, npairs); }

  // Step 2: every table at its offset in `base` (lay.bytes long); the per-pose lists, the blocks and the pair lists are written in place.
  void fill(char* base, const BaStructLayout& lay) const {
    auto put = [&](size_t o, const std::vector<int>& v) { if (!v.empty()) memcpy(base + o, v.data(), v.size() * 4); };
    auto tab = [&](size_t o) { return reinterpret_cast<int*>(base + o); };
    put(lay.act, act); put(lay.pose_h, pose_h); put(lay.pt_h, pt_h); put(lay.pose_of_h, pose_of_h); put(lay.pt_of_h, pt_of_h);
    put(lay.pt_start, pt_start); put(lay.ps_start, ps_start);
    // per free pose: its edges (k indices) in k order, and the landmark of each
    int* ps_edges = tab(lay.ps_edges); int* ps_h = tab(lay.ps_h);
    std::vector<int> cursor(ps_start.begin(), ps_start.end() - 1);
    for (int h = 0; h < nLa; ++h)
      for (int k = pt_start[h]; k < pt_start[h + 1]; ++k)
        if (ph_of_k[k] >= 0) { const int o = cursor[ph_of_k[k]]++; ps_edges[o] = k; ps_h[o] = h; }
    // the selected blocks in row-major order; cursor: where the next pair of upper block q goes
    int* blk_i = tab(lay.blk_i); int* blk_j = tab(lay.blk_j); int* pair_start = tab(lay.pair_start);
    cursor.assign(cnt.size(), -1);
    int c = 0;
    pair_start[0] = 0;
    for (int i = 0; i < nPf; ++i)
      for (int j = i; j < nPf; ++j) {
        const int q = row_off[i] + j;
        if (!all_blocks && i != j && cnt[q] == 0) continue;
        blk_i[c] = i; blk_j[c] = j;
        cursor[q] = pair_start[c];
        pair_start[c + 1] = pair_start[c] + cnt[q];
        ++c;
      }
    // two edges of one pose (a duplicate observation): k_ba_schur adds Y_a B_b^T for a pair, and the diagonal block needs both cross
    // terms, Y_a B_b^T + Y_b B_a^T -- the transposed block of an off-diagonal pair is written from the same sum
    int* pairs = tab(lay.pairs); int* pair_h = tab(lay.pair_h);   // pairs: int2 (a, b)
    for_each_pair([&](int q, int h, int a, int b, bool twice) {
      int o = cursor[q]++;
      pairs[2 * o] = a; pairs[2 * o + 1] = b; pair_h[o] = h;
      if (twice) { o = cursor[q]++; pairs[2 * o] = b; pairs[2 * o + 1] = a; pair_h[o] = h; }
    });
  }

 private:
  std::vector<int> pose_h, pt_h, pose_of_h, pt_of_h, pt_start, act, ph_of_k, ps_start, row_off, cnt;

  // f(upper block, landmark, a, b, twice) for every two edges a <= b (act positions) of one landmark that both go to free poses
  template <class F>
  void for_each_pair(F f) const {
    for (int h = 0; h < nLa; ++h) {
      const int s1 = pt_start[h + 1];
      int a = pt_start[h];
      while (a < s1 && ph_of_k[a] < 0) ++a;   // fixed poses sort first
      for (; a < s1; ++a)
        for (int b = a; b < s1; ++b) f(row_off[ph_of_k[a]] + ph_of_k[b], h, a, b, b != a && ph_of_k[b] == ph_of_k[a]);
    }
  }
};
