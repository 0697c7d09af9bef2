// Host driver of MDFIT-AUTO v1.1 (csrc/mdfit_auto.h: route_pred_one, the device
// kernel's own function) for tests/test_auto_pred.py: plain g++ on
// tests/host_shim, no HIP.  argv[1]: a binary file holding int64 T, int64
// with_pred (0: pred is NULL), then int32 status[T], double psis[T][3][16],
// double waic[T][7][8], double prec[T][16], float ppred[T][90], double
// out[T][80] and, with_pred, float pred[T][90]; argv[2]: the file written:
// int32 route[T], double out[T][80] and, with_pred, float pred[T][90].
#include <cstdint>
#include <cstdio>
#include <vector>

#include <hip/hip_runtime.h>

#include "../metadamage_amd/csrc/mdfit_auto.h"

template <class T>
static bool rd(std::FILE* f, std::vector<T>& v) {
  return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
}
template <class T>
static bool wr(std::FILE* f, const std::vector<T>& v) {
  return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t T = 0, with_pred = 0;
  if (std::fread(&T, sizeof(T), 1, f) != 1 || T < 0 || T > (1 << 20)) return 2;
  if (std::fread(&with_pred, sizeof(with_pred), 1, f) != 1) return 2;
  const size_t n = (size_t)T;
  // exactly the lengths the routine is given: a sanitizer sees any access beyond them
  std::vector<int32_t> status(n), route(n);
  std::vector<double> psis(n * 3 * MDFIT_NMAPPSIS), waic(n * 7 * MDFIT_NMAPWAIC), prec(n * MDFIT_NMAPPRED),
      out(n * MDFIT_NOUT);
  std::vector<float> ppred(n * MDFIT_NPRED * 30), pred(with_pred ? n * MDFIT_NPRED * 30 : 0);
  if (!rd(f, status) || !rd(f, psis) || !rd(f, waic) || !rd(f, prec) || !rd(f, ppred) || !rd(f, out) || !rd(f, pred))
    return 2;
  std::fclose(f);
  for (int64_t t = 0; t < T; ++t)
    mdfit::autoroute::route_pred_one(t, status.data(), psis.data(), waic.data(), prec.data(), ppred.data(), out.data(),
                                     with_pred ? pred.data() : nullptr, route.data());
  std::FILE* g = std::fopen(argv[2], "wb");
  if (!g) return 2;
  if (!wr(g, route) || !wr(g, out) || !wr(g, pred)) return 2;
  return std::fclose(g) == 0 ? 0 : 2;
}
