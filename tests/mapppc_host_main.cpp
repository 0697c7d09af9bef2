// Host driver of the per-column part of MDFIT-PPC v1 (csrc/mdfit_mapppc.h:
// mid_p and worst_position, plain C++) for tests/test_map_ppc.py: plain g++, no
// HIP.  argv[1]: a file holding the number of items, then per item "R" and 30
// triples "has gt eq" -- stdout: the 30 mid-p values (nan where has = 0),
// worst, p_worst, n_low and n_points, the doubles as C hex floats.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../metadamage_amd/csrc/mdfit_mapppc.h"

int main(int argc, char** argv) {
  namespace mc = mdfit::mapppc;
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int count = 0;
  if (std::fscanf(f, "%d", &count) != 1) return 2;
  for (int i = 0; i < count; ++i) {
    int R = 0;
    if (std::fscanf(f, "%d", &R) != 1) return 2;
    if (R < mdfit::mappred::kMinPred || R > mdfit::mappred::kMaxPred) return 2;
    // exactly the lengths the routine is given: a sanitizer sees any access beyond them
    std::vector<uint32_t> cnt((size_t)mc::kNCols * 2);
    std::vector<int> has((size_t)mc::kNCols);
    for (int col = 0; col < mc::kNCols; ++col)
      if (std::fscanf(f, "%d %u %u", &has[(size_t)col], &cnt[(size_t)col * 2], &cnt[(size_t)col * 2 + 1]) != 3) return 2;
    const uint32_t(*c2)[2] = reinterpret_cast<const uint32_t(*)[2]>(cnt.data());
    const mc::Worst w = mc::worst_position(c2, [&](int col) { return has[(size_t)col] != 0; }, R);
    for (int col = 0; col < mc::kNCols; ++col)
      std::printf("%a ", has[(size_t)col] ? mc::mid_p(c2[col][0], c2[col][1], R) : (double)NAN);
    std::printf("%d %a %a %a\n", w.worst, w.p_worst, w.n_low, w.n_points);
  }
  std::fclose(f);
  return 0;
}
