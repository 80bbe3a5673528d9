// kfdb_query_cpu.cpp -- the loop query the way the CPU implementation runs it (KeyFrameDatabase::DetectLoopCandidates: inverted
// file as std::list per word, BowVector as std::map, L1 score by merging the two maps), for the comparison in tools/kfdb_query_time.py.
//   g++ -O2 -std=c++17 -o kfdb_query_cpu kfdb_query_cpu.cpp ;  kfdb_query_cpu data.bin reps
// data.bin (written by kfdb_query_time.py): int32 n_words_in_vocabulary, n_entries, n_queries; per entry and then per query:
// int32 n, int32 id[n], f64 val[n].  Prints the mean wall time of one query in ms and a checksum of the candidates.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <map>
#include <set>
#include <vector>

typedef std::map<unsigned, double> Bow;
struct KF { int id; Bow bow; long query = -1; int words = 0; float score = 0; };

static double l1(const Bow& v1, const Bow& v2) {
  Bow::const_iterator a = v1.begin(), b = v2.begin();
  double score = 0;
  while (a != v1.end() && b != v2.end()) {
    if (a->first == b->first) { score += fabs(a->second - b->second) - fabs(a->second) - fabs(b->second); ++a; ++b; }
    else if (a->first < b->first) a = v1.lower_bound(b->first);
    else b = v2.lower_bound(a->first);
  }
  return -score / 2.0;
}

static Bow read_bow(FILE* f) {
  int32_t n = 0;
  if (fread(&n, 4, 1, f) != 1) exit(2);
  std::vector<int32_t> id(n);
  std::vector<double> val(n);
  if (n && (fread(id.data(), 4, n, f) != (size_t)n || fread(val.data(), 8, n, f) != (size_t)n)) exit(2);
  Bow b;
  for (int i = 0; i < n; ++i) b[id[i]] = val[i];
  return b;
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  const int reps = atoi(argv[2]);
  int32_t hdr[3];
  if (fread(hdr, 4, 3, f) != 3) return 2;
  std::vector<std::list<KF*>> inverted(hdr[0]);
  std::vector<KF> kfs(hdr[1]);
  for (int i = 0; i < hdr[1]; ++i) {
    kfs[i].id = i;
    kfs[i].bow = read_bow(f);
    for (const auto& w : kfs[i].bow) inverted[w.first].push_back(&kfs[i]);
  }
  std::vector<Bow> queries;
  for (int i = 0; i < hdr[2]; ++i) queries.push_back(read_bow(f));
  fclose(f);
  long stamp = 0, checksum = 0;
  const float minScore = 0.01f;
  const auto t0 = std::chrono::steady_clock::now();
  for (int r = 0; r < reps; ++r) {
    const Bow& q = queries[r % queries.size()];
    ++stamp;
    std::list<KF*> sharing;
    for (const auto& w : q)
      for (KF* k : inverted[w.first]) {
        if (k->query != stamp) { k->words = 0; k->query = stamp; sharing.push_back(k); }
        k->words++;
      }
    int maxCommon = 0;
    for (KF* k : sharing) if (k->words > maxCommon) maxCommon = k->words;
    const int minCommon = maxCommon * 0.6f;
    std::list<std::pair<float, KF*>> scored;
    for (KF* k : sharing)
      if (k->words > minCommon) {
        const float si = l1(q, k->bow);
        k->score = si;
        if (si >= minScore) scored.push_back(std::make_pair(si, k));
      }
    std::list<std::pair<float, KF*>> acc;
    float bestAcc = minScore;
    for (const auto& sm : scored) {
      float best = sm.first, a = sm.first;
      KF* bk = sm.second;
      for (int d = -5; d <= 5; ++d) {
        const int j = sm.second->id + d;
        if (d == 0 || j < 0 || j >= hdr[1]) continue;
        KF* k2 = &kfs[j];
        if (k2->query == stamp && k2->words > minCommon) { a += k2->score; if (k2->score > best) { bk = k2; best = k2->score; } }
      }
      acc.push_back(std::make_pair(a, bk));
      if (a > bestAcc) bestAcc = a;
    }
    std::set<KF*> added;
    for (const auto& am : acc)
      if (am.first > 0.55f * bestAcc && !added.count(am.second)) { added.insert(am.second); checksum += am.second->id + 1; }
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps;
  printf("{\"cpu_query_ms\": %.4f, \"reps\": %d, \"checksum\": %ld}\n", ms, reps, checksum);
  return 0;
}
