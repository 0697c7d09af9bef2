// Host driver of the 4x4 Laplace routine (csrc/mdfit_laplace.h, its plain-C++
// part) for tests/test_laplace.py: built with g++ under the address and
// undefined-behaviour sanitizers.  stdin: n, then per case the free mask, the
// packed upper triangle of H (10), J (4) and D_max as C hex floats; stdout: the
// 8 fields of each record as hex floats.
#include <cstdio>

#include "../metadamage_amd/csrc/mdfit_laplace.h"

int main() {
  int n = 0;
  if (std::scanf("%d", &n) != 1) return 2;
  for (int i = 0; i < n; ++i) {
    unsigned mask = 0;
    double H[10], J[4], dmax = 0.0, rec[MDFIT_NLAPLACE];
    if (std::scanf("%u", &mask) != 1) return 2;
    for (double& h : H)
      if (std::scanf("%la", &h) != 1) return 2;
    for (double& j : J)
      if (std::scanf("%la", &j) != 1) return 2;
    if (std::scanf("%la", &dmax) != 1) return 2;
    mdfit::laplace::laplace4(H, mask, J, dmax, rec);
    for (int k = 0; k < MDFIT_NLAPLACE; ++k) std::printf("%a%c", rec[k], k + 1 < MDFIT_NLAPLACE ? ' ' : '\n');
  }
  return 0;
}
