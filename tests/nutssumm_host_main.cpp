// Host driver of the posterior summary's arithmetic (csrc/mdfit_nutssumm.h with
// its one-lane policy) for tests/test_nuts_summary.py: built with g++ under the
// address and undefined-behaviour sanitizers.  argv[1]: a file holding n, then
// per case S, pmd (0/1), the chain status and the S x 4 draws as C hex floats;
// stdout: the 16 fields of each record as hex floats.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../metadamage_amd/csrc/mdfit_nutssumm.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n = 0;
  if (std::fscanf(f, "%d", &n) != 1) return 2;
  for (int i = 0; i < n; ++i) {
    int S = 0, pmd = 0;
    double status = 0.0, rec[MDFIT_NNUTSSUMM];
    if (std::fscanf(f, "%d %d %la", &S, &pmd, &status) != 3 || S < 2 || S > 4096) return 2;
    // the draws 32-byte aligned, as a workspace row is
    double* x = (double*)std::aligned_alloc(32, (size_t)S * 4 * sizeof(double));
    if (!x) return 2;
    for (int j = 0; j < 4 * S; ++j)
      if (std::fscanf(f, "%la", &x[j]) != 1) return 2;
    std::vector<double> work((size_t)mdfit::nutssumm::sort_len(S));
    mdfit::nutssumm::summary_row_host(x, S, pmd != 0, status, work.data(), rec);
    std::free(x);
    for (int k = 0; k < MDFIT_NNUTSSUMM; ++k) std::printf("%a%c", rec[k], k + 1 < MDFIT_NNUTSSUMM ? ' ' : '\n');
  }
  std::fclose(f);
  return 0;
}
