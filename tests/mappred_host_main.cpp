// Host driver of the resampling and the median / HPDI of MDFIT-PPRED v1
// (csrc/mdfit_mappred.h with its one-lane policy) for tests/test_map_pred.py:
// plain g++, no HIP.  argv[1]: a file holding the number of items, then per
// item either "r S R" and the S weights as C hex floats -- stdout: the R
// indices and n_distinct --, or "m R N" (N as a C hex float) and the R counts
// -- stdout: median, lower and upper as C hex floats.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../metadamage_amd/csrc/mdfit_mappred.h"

int main(int argc, char** argv) {
  namespace mq = mdfit::mappred;
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int count = 0;
  if (std::fscanf(f, "%d", &count) != 1) return 2;
  for (int i = 0; i < count; ++i) {
    char kind = 0;
    if (std::fscanf(f, " %c", &kind) != 1) return 2;
    if (kind == 'r') {
      int S = 0, R = 0;
      if (std::fscanf(f, "%d %d", &S, &R) != 2) return 2;
      if (S < mdfit::mappsis::kMinDraws || S > mdfit::mappsis::kMaxDraws || R < mq::kMinPred || R > mq::kMaxPred)
        return 2;
      // exactly the lengths the routine is given: a sanitizer sees any access beyond them
      std::vector<double> c((size_t)S);
      std::vector<int> idx((size_t)R);
      for (auto& v : c)
        if (std::fscanf(f, "%la", &v) != 1) return 2;
      const int nd = mq::resample_host(c.data(), S, R, idx.data());
      for (int r = 0; r < R; ++r) std::printf("%d ", idx[(size_t)r]);
      std::printf("%d\n", nd);
    } else if (kind == 'm') {
      int R = 0;
      double Nn = 0.0;
      if (std::fscanf(f, "%d %la", &R, &Nn) != 2) return 2;
      if (R < mq::kMinPred || R > mq::kMaxPred) return 2;
      std::vector<uint32_t> v((size_t)mq::sort_len(R));
      for (int r = 0; r < R; ++r)
        if (std::fscanf(f, "%u", &v[(size_t)r]) != 1) return 2;
      double m3[3];
      mq::median_hpdi_host(v.data(), R, Nn, m3);
      std::printf("%a %a %a\n", m3[0], m3[1], m3[2]);
    } else {
      return 2;
    }
  }
  std::fclose(f);
  return 0;
}
