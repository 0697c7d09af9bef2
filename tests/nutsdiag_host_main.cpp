// Host driver of the sampling diagnostics' per-series arithmetic
// (csrc/mdfit_nutsdiag.h with its one-lane policy) for tests/test_nuts_diag.py:
// built with g++ under the address and undefined-behaviour sanitizers.  stdin:
// n, then per case S, pmd (0/1), the chain status and the S x 4 draws as C hex
// floats; stdout: the 12 fields of each record as hex floats.
#include <cstdio>
#include <vector>

#include "../metadamage_amd/csrc/mdfit_nutsdiag.h"

int main() {
  int n = 0;
  if (std::scanf("%d", &n) != 1) return 2;
  for (int i = 0; i < n; ++i) {
    int S = 0, pmd = 0;
    double status = 0.0, rec[MDFIT_NNUTSDIAG];
    if (std::scanf("%d %d %la", &S, &pmd, &status) != 3 || S < 2 || S > 4096) return 2;
    std::vector<double> x((size_t)4 * S), work((size_t)S);
    for (double& v : x)
      if (std::scanf("%la", &v) != 1) return 2;
    mdfit::nutsdiag::diag_row_host(x.data(), S, pmd != 0, status, work.data(), rec);
    for (int k = 0; k < MDFIT_NNUTSDIAG; ++k) std::printf("%a%c", rec[k], k + 1 < MDFIT_NNUTSDIAG ? ' ' : '\n');
  }
  return 0;
}
