// Host driver of the PSIS-LOO arithmetic (csrc/mdfit_nutsloo.h with its one-lane
// policy) for tests/test_nuts_loo.py: built with g++ under the address and
// undefined-behaviour sanitizers.  argv[1]: a file holding n, then per series S
// and its S pointwise log-likelihoods as C hex floats (or nan, inf, -inf);
// stdout: elpd and khat of each series as hex floats.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../metadamage_amd/csrc/mdfit_nutsloo.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n = 0;
  if (std::fscanf(f, "%d", &n) != 1) return 2;
  for (int i = 0; i < n; ++i) {
    int S = 0;
    if (std::fscanf(f, "%d", &S) != 1 || S < 2 || S > 4096) return 2;
    // exactly the work buffer's length: the sanitizer sees any access beyond it
    std::vector<double> work((size_t)mdfit::nutsloo::work_len(S));
    for (int j = 0; j < S; ++j) {
      double l = 0.0;
      if (std::fscanf(f, "%la", &l) != 1) return 2;
      work[(size_t)j] = -l;
    }
    double elpd = 0.0, khat = 0.0;
    mdfit::nutsloo::psis_point_host(work.data(), S, &elpd, &khat);
    std::printf("%a %a\n", elpd, khat);
  }
  std::fclose(f);
  return 0;
}
