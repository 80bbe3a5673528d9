// test_initializer.cpp -- probe for asd::Initializer (asd_adapters.hpp); tests/test_initializer_host.py reads its output.
//
//   test_initializer --draws ITERATIONS N0 N1 ...
//     no device.  One Initializer per Nk, in order, in this process: prints "draws" and the 8 x ITERATIONS RandomInt results of each.  The
//     first srand(0)s (SeedRandOnce), the later ones continue the rand() sequence.
//   test_initializer PROBLEM_FILE
//     on the device.  The file (text; floats as C99 hex): "ncalls", then per call "n1 n2 sigma iterations", K[4], keys1[2 n1], keys2[2 n2],
//     matches12[n1].  One Initializer and one Initialize per call, in order.  Prints JSON per call: ok, model, SH, SF, R21, t21, the
//     triangulated flags, P3D and the draws.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "asd_adapters.hpp"

namespace {

asd::FrameView frame_of(const std::vector<float>& keys) {
  asd::FrameView f;
  f.mvKeysUn.resize(keys.size() / 2);
  for (size_t i = 0; i < f.mvKeysUn.size(); ++i) { f.mvKeysUn[i] = asd_keypoint{}; f.mvKeysUn[i].x = keys[2 * i]; f.mvKeysUn[i].y = keys[2 * i + 1]; }
  return f;
}

int draws_mode(int argc, char** argv) {
  if (argc < 4) return 2;
  const int iterations = atoi(argv[2]);
  const asd::Camera K{1, 1, 0, 0};
  for (int a = 3; a < argc; ++a) {
    asd::Initializer init(nullptr, asd::FrameView{}, K, 1.0f, iterations);
    printf("draws");
    for (int32_t d : init.Draw(atoi(argv[a]))) printf(" %d", d);
    printf("\n");
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "--draws")) return draws_mode(argc, argv);
  if (argc < 2) { fprintf(stderr, "usage: %s PROBLEM_FILE | --draws ITERATIONS N0 N1 ...\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int ncalls = 0;
  if (fscanf(f, "%d", &ncalls) != 1 || ncalls < 1) return 2;
  try {
    asd::Context ctx(500, 1.2f, 8, 20, 7, 640, 480);
    printf("[");
    for (int c = 0; c < ncalls; ++c) {
      int n1 = 0, n2 = 0, iterations = 0;
      float sigma = 0;
      asd::Camera K{};
      if (fscanf(f, "%d %d %a %d", &n1, &n2, &sigma, &iterations) != 4) return 2;
      if (fscanf(f, "%a %a %a %a", &K.fx, &K.fy, &K.cx, &K.cy) != 4) return 2;
      std::vector<float> k1(2 * n1), k2(2 * n2);
      std::vector<int> m(n1);
      for (float& x : k1) if (fscanf(f, "%a", &x) != 1) return 2;
      for (float& x : k2) if (fscanf(f, "%a", &x) != 1) return 2;
      for (int& x : m) if (fscanf(f, "%d", &x) != 1) return 2;
      asd::Initializer init(ctx.get(), frame_of(k1), K, sigma, iterations);
      float R21[9] = {0}, t21[3] = {0};
      std::vector<asd::Point3f> vP3D;
      std::vector<bool> vbTriangulated;
      const bool ok = init.Initialize(frame_of(k2), m, R21, t21, vP3D, vbTriangulated);
      printf("%s{\"ok\": %d, \"model\": %d, \"SH\": \"%a\", \"SF\": \"%a\", \"R21\": [", c ? ", " : "", (int)ok, init.Last().model,
             (double)init.Last().SH, (double)init.Last().SF);
      for (int i = 0; ok && i < 9; ++i) printf("%s\"%a\"", i ? ", " : "", (double)R21[i]);
      printf("], \"t21\": [");
      for (int i = 0; ok && i < 3; ++i) printf("%s\"%a\"", i ? ", " : "", (double)t21[i]);
      printf("], \"triangulated\": [");
      for (size_t i = 0; i < vbTriangulated.size(); ++i) printf("%s%d", i ? ", " : "", (int)vbTriangulated[i]);
      printf("], \"P3D\": [");
      for (size_t i = 0; i < vP3D.size(); ++i) printf("%s\"%a\", \"%a\", \"%a\"", i ? ", " : "", (double)vP3D[i].x, (double)vP3D[i].y, (double)vP3D[i].z);
      printf("], \"draws\": [");
      for (size_t i = 0; i < init.LastDraws().size(); ++i) printf("%s%d", i ? ", " : "", init.LastDraws()[i]);
      printf("]}");
    }
    printf("]\n");
    fclose(f);
    return 0;
  } catch (const std::exception& e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}
