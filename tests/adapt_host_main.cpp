// Host driver of the proposal refit of MDFIT-ADAPT v1 (csrc/mdfit_mapadapt.h
// with its one-lane policy) for tests/test_map_adapt.py: plain g++, no HIP.
// argv[1]: a file holding n, then per series S, the free mask, the c-held flag,
// K[4], its S weights and its S x 4 draws (logit q, logit A, c, log delta) as C
// hex floats (or nan, inf, -inf); stdout per series: ok, m[4], d[4], F[4][4]
// (row-major) and the exponential's rate.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../metadamage_amd/csrc/mdfit_mapadapt.h"

int main(int argc, char** argv) {
  namespace ma = mdfit::mapadapt;
  namespace mp = mdfit::mappsis;
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n = 0;
  if (std::fscanf(f, "%d", &n) != 1) return 2;
  for (int i = 0; i < n; ++i) {
    int S = 0, mask = 0, cheld = 0;
    double K[4];
    if (std::fscanf(f, "%d %d %d", &S, &mask, &cheld) != 3 || S < mp::kMinDraws || S > mp::kMaxDraws) return 2;
    for (int j = 0; j < 4; ++j)
      if (std::fscanf(f, "%la", &K[j]) != 1) return 2;
    // exactly S weights and S x 4 draws: a sanitizer sees any access beyond them
    std::vector<double> w((size_t)S), u((size_t)S * 4);
    for (int j = 0; j < S; ++j)
      if (std::fscanf(f, "%la", &w[(size_t)j]) != 1) return 2;
    for (int j = 0; j < 4 * S; ++j)
      if (std::fscanf(f, "%la", &u[(size_t)j]) != 1) return 2;
    ma::Refit r;
    const bool ok = ma::refit_host(w.data(), S, u.data(), (unsigned)mask & 15u, cheld != 0, K, &r);
    std::printf("%d", ok ? 1 : 0);
    for (int j = 0; j < 4; ++j) std::printf(" %a", ok ? r.m[j] : std::nan(""));
    for (int j = 0; j < 4; ++j) std::printf(" %a", ok ? r.d[j] : std::nan(""));
    for (int j = 0; j < 4; ++j)
      for (int p = 0; p < 4; ++p) std::printf(" %a", ok ? r.F[j][p] : std::nan(""));
    std::printf(" %a\n", ok ? r.gc : std::nan(""));
  }
  std::fclose(f);
  return 0;
}
