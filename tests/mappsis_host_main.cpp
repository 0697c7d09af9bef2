// Host driver of the importance-weight smoothing and the estimates of
// MDFIT-PSIS v1 (csrc/mdfit_mappsis.h with its one-lane policy) for
// tests/test_map_psis.py: plain g++, no HIP.  argv[1]: a file holding n, then
// per series S, its S raw log-weights and its S x 4 draws (q, A, c, phi) as C
// hex floats (or nan, inf, -inf); stdout per series: valid, khat, the S
// weights and the 16 fields of the record (free mask 15).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../metadamage_amd/csrc/mdfit_mappsis.h"

int main(int argc, char** argv) {
  namespace mp = mdfit::mappsis;
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n = 0;
  if (std::fscanf(f, "%d", &n) != 1) return 2;
  for (int i = 0; i < n; ++i) {
    int S = 0;
    if (std::fscanf(f, "%d", &S) != 1 || S < mp::kMinDraws || S > mp::kMaxDraws) return 2;
    // exactly the work buffer's length: a sanitizer sees any access beyond it
    std::vector<double> work((size_t)mp::work_len(S));
    std::vector<double> draws((size_t)S * 4);
    for (int j = 0; j < S; ++j)
      if (std::fscanf(f, "%la", &work[(size_t)j]) != 1) return 2;
    for (int j = 0; j < 4 * S; ++j)
      if (std::fscanf(f, "%la", &draws[(size_t)j]) != 1) return 2;
    double khat = 0.0, n_inf = 0.0, rec[MDFIT_NMAPPSIS];
    const bool ok = mp::psis_weights_host(work.data(), S, &khat, &n_inf);
    if (ok) mp::psis_estimates_host(work.data(), S, draws.data(), khat, n_inf, 15u, rec);
    else mp::invalid_row(rec, 15u);
    std::printf("%d %a", ok ? 1 : 0, khat);
    for (int j = 0; j < S; ++j) std::printf(" %a", ok ? work[(size_t)j] : std::nan(""));
    for (int j = 0; j < MDFIT_NMAPPSIS; ++j) std::printf(" %a", rec[j]);
    std::printf("\n");
  }
  std::fclose(f);
  return 0;
}
