// Host build of csrc/mdfit_special.h (tests/test_eval_trim_host.py), as
// tests/special_host_main.cpp: the unmodified header through tests/host_shim,
// g++ -ffp-contract=off.  Prints, for every point, the bits of the forms that
// must agree (the test compares the columns):
//
//   eval_trim_host <mode> <file> : the file holds n and then n lines "x x2" of
//   hex floats; one output line per point, the columns as 16 hex digits.
//     lg3   : lg3<false>.l | l, psi, psi1 of lg3<true>, each followed by the
//             same of the form with flog's special-case tail (kPos off)
//     log   : flog(x), flog_pos(x)                      (x finite and > 0)
//     prod  : P = x (x+1) ... (x+9) as lg3 forms it, flog(P), the one-select form
//     sel   : flog(x), the one-select form at x itself  (x >= 0: 0, subnormals)
//     lrise : lrise(x, x2), lrise_lg(x, x2, lgam(x2))
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../metadamage_amd/csrc/mdfit_special.h"

static unsigned long long bits(double v) {
  unsigned long long b;
  std::memcpy(&b, &v, 8);
  return b;
}

static double one_select(double P) { return P == 0.0 ? -INFINITY : mdfit::flog_pos(P); }

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <mode> <file>\n", argv[0]);
    return 2;
  }
  const char* mode = argv[1];
  std::FILE* f = std::fopen(argv[2], "r");
  if (f == nullptr) {
    std::perror(argv[2]);
    return 2;
  }
  long n = 0;
  if (std::fscanf(f, "%ld", &n) != 1 || n < 0) {
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
  for (long i = 0; i < n; ++i) {
    const double v = x[(size_t)i], w = x2[(size_t)i];
    double o[10];
    int k = 0;
    if (std::strcmp(mode, "lg3") == 0) {
      const mdfit::LG3 t = mdfit::lg3<true>(v);
      const mdfit::LG3 u = mdfit::lg3<true, false, false>(v);
      o[k++] = mdfit::lg3<false>(v).l;
      o[k++] = t.l;
      o[k++] = u.l;
      o[k++] = t.p, o[k++] = u.p;
      o[k++] = t.q, o[k++] = u.q;
    } else if (std::strcmp(mode, "log") == 0) {
      o[k++] = mdfit::flog(v);
      o[k++] = mdfit::flog_pos(v);
    } else if (std::strcmp(mode, "prod") == 0) {
      double P = v;
      for (int j = 1; j < 10; ++j) P = P * (v + (double)j);
      o[k++] = P;
      o[k++] = mdfit::flog(P);
      o[k++] = one_select(P);
    } else if (std::strcmp(mode, "sel") == 0) {
      o[k++] = mdfit::flog(v);
      o[k++] = one_select(v);
    } else if (std::strcmp(mode, "lrise") == 0) {
      o[k++] = mdfit::lrise(v, w);
      o[k++] = mdfit::lrise_lg(v, w, mdfit::lgam(w));
    } else {
      std::fprintf(stderr, "unknown mode %s\n", mode);
      return 2;
    }
    for (int j = 0; j < k; ++j) std::printf("%016llx%c", bits(o[j]), j + 1 < k ? ' ' : '\n');
  }
  return 0;
}
