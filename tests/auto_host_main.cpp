// Host driver of MDFIT-AUTO v1 (csrc/mdfit_auto.h: the routing rule and the
// composition, the device kernel's own functions) for tests/test_auto.py: plain
// g++ on tests/host_shim, no HIP.  argv[1]: a binary file holding int64 T, then
// int32 status[T], double psis[T][3][16], double waic[T][7][8], double
// out[T][80]; argv[2]: the file written: int32 route[T], double out[T][80].
#include <cstdint>
#include <cstdio>
#include <vector>

#include <hip/hip_runtime.h>

#include "../metadamage_amd/csrc/mdfit_auto.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t T = 0;
  if (std::fread(&T, sizeof(T), 1, f) != 1 || T < 0 || T > (1 << 20)) return 2;
  const size_t n = (size_t)T;
  // exactly the lengths the routine is given: a sanitizer sees any access beyond them
  std::vector<int32_t> status(n), route(n);
  std::vector<double> psis(n * 3 * MDFIT_NMAPPSIS), waic(n * 7 * MDFIT_NMAPWAIC), out(n * MDFIT_NOUT);
  if (std::fread(status.data(), sizeof(int32_t), n, f) != n) return 2;
  if (std::fread(psis.data(), sizeof(double), psis.size(), f) != psis.size()) return 2;
  if (std::fread(waic.data(), sizeof(double), waic.size(), f) != waic.size()) return 2;
  if (std::fread(out.data(), sizeof(double), out.size(), f) != out.size()) return 2;
  std::fclose(f);
  for (int64_t t = 0; t < T; ++t)
    mdfit::autoroute::route_one(t, status.data(), psis.data(), waic.data(), out.data(), route.data());
  std::FILE* g = std::fopen(argv[2], "wb");
  if (!g) return 2;
  if (std::fwrite(route.data(), sizeof(int32_t), n, g) != n) return 2;
  if (std::fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) return 2;
  return std::fclose(g) == 0 ? 0 : 2;
}
