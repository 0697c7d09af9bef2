// Host driver of the pointwise accumulation and the row record of MDFIT-WAIC
// v1 (csrc/mdfit_mapwaic.h with its one-lane policy) for
// tests/test_map_waic.py: plain g++, no HIP.  argv[1]: a file holding the
// number of series, then per series S, n (15 or 30), khat, its S normalised
// weights, its S x n log-pmf values and its n shifts as C hex floats (or nan,
// inf, -inf); stdout per series: the n lppd_i, the n p_i and the 8 fields of
// the record (free mask 15; n_infeasible: the weights that are 0).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../metadamage_amd/csrc/mdfit_mapwaic.h"

int main(int argc, char** argv) {
  namespace mw = mdfit::mapwaic;
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int count = 0;
  if (std::fscanf(f, "%d", &count) != 1) return 2;
  for (int i = 0; i < count; ++i) {
    int S = 0, n = 0;
    double khat = 0.0;
    if (std::fscanf(f, "%d %d %la", &S, &n, &khat) != 3) return 2;
    if (S < mdfit::mappsis::kMinDraws || S > mdfit::mappsis::kMaxDraws || n < 1 || n > mw::kMaxPts) return 2;
    // exactly the lengths the routine is given: a sanitizer sees any access beyond them
    std::vector<double> wt((size_t)S), l((size_t)S * n), l0((size_t)n), lppd((size_t)n), p((size_t)n);
    for (auto& v : wt)
      if (std::fscanf(f, "%la", &v) != 1) return 2;
    for (auto& v : l)
      if (std::fscanf(f, "%la", &v) != 1) return 2;
    for (auto& v : l0)
      if (std::fscanf(f, "%la", &v) != 1) return 2;
    double n_inf = 0.0;
    for (double v : wt) n_inf += v == 0.0 ? 1.0 : 0.0;
    mw::waic_points_host(wt.data(), S, n, l.data(), l0.data(), lppd.data(), p.data());
    double rec[MDFIT_NMAPWAIC];
    mw::waic_row_host(lppd.data(), p.data(), n, wt.data(), S, khat, n_inf, 15u, rec);
    for (int j = 0; j < n; ++j) std::printf("%a ", lppd[(size_t)j]);
    for (int j = 0; j < n; ++j) std::printf("%a ", p[(size_t)j]);
    for (int j = 0; j < MDFIT_NMAPWAIC; ++j) std::printf("%a ", rec[j]);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
