// Host build of csrc/mdfit_special.h (tests/test_special_host.py): the
// unmodified header through the include-path stand-in tests/host_shim/hip/
// hip_runtime.h, compiled by g++ -ffp-contract=off.  Every fusion in the header
// is an explicit fma, so the functions without a reciprocal (flog_t, fexp_t,
// fexp) run the device's arithmetic; the reciprocal's seed is 1.0 / x here.
//
//   special_host <file> : the file holds "which n" and then n lines "x x2" of
//   hex floats (or nan / inf / -inf); prints primitive `which` (enum
//   mdfit_primitive_id) at each as a hex float, one per line.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../metadamage_amd/csrc/mdfit_primitive.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s <file>\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "r");
  if (f == nullptr) {
    std::perror(argv[1]);
    return 2;
  }
  int which = 0;
  long n = 0;
  if (std::fscanf(f, "%d %ld", &which, &n) != 2 || which < 1 || which >= MDFIT_P_COUNT || n < 0) {
    std::fprintf(stderr, "bad header\n");
    return 2;
  }
  std::vector<double> x((size_t)n), x2((size_t)n);
  char a[64], b[64];
  for (long i = 0; i < n; ++i) {
    if (std::fscanf(f, "%63s %63s", a, b) != 2) {
      std::fprintf(stderr, "short file at element %ld\n", i);
      return 2;
    }
    x[(size_t)i] = std::strtod(a, nullptr);
    x2[(size_t)i] = std::strtod(b, nullptr);
  }
  std::fclose(f);
  for (long i = 0; i < n; ++i) std::printf("%a\n", mdfit::primitive_eval(which, x[(size_t)i], x2[(size_t)i]));
  return 0;
}
