// Host driver of the weighted order statistics of MDFIT-QUANT v1
// (csrc/mdfit_mapquant.h with its one-lane policy) for tests/test_map_quant.py:
// plain g++, no HIP.  argv[1]: a file holding n, then per series S, d0, its S
// values and its S weights as C hex floats (or nan, inf, -inf); stdout per
// series: the 8 fields of the result.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../metadamage_amd/csrc/mdfit_mapquant.h"

int main(int argc, char** argv) {
  namespace mq = mdfit::mapquant;
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n = 0;
  if (std::fscanf(f, "%d", &n) != 1) return 2;
  for (int i = 0; i < n; ++i) {
    int S = 0;
    double d0 = 0.0;
    if (std::fscanf(f, "%d %la", &S, &d0) != 2 || S < mdfit::mappsis::kMinDraws || S > mdfit::mappsis::kMaxDraws)
      return 2;
    // exactly the buffers' lengths: a sanitizer sees any access beyond them
    std::vector<double> v((size_t)S), w((size_t)S), sv((size_t)mq::sort_len(S));
    std::vector<int> si((size_t)mq::sort_len(S));
    std::vector<uint64_t> cum((size_t)S);
    for (int j = 0; j < S; ++j)
      if (std::fscanf(f, "%la", &v[(size_t)j]) != 1) return 2;
    for (int j = 0; j < S; ++j)
      if (std::fscanf(f, "%la", &w[(size_t)j]) != 1) return 2;
    double res[mq::kNRes];
    mq::series_stats_host(v.data(), w.data(), S, d0, sv.data(), si.data(), cum.data(), res);
    for (int j = 0; j < mq::kNRes; ++j) std::printf("%s%a", j ? " " : "", res[j]);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
