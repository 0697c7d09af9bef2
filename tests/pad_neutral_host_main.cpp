// Host build of csrc/mdfit_model.h (tests/test_pad_neutral_host.py): the
// unmodified header through tests/host_shim_lanes, g++ -ffp-contract=off.
// Evaluates point_accum<true> on the 32 lanes of one slot (two rows of 16, lane
// 15 of each a pad) beside the form it replaces -- every lane, the pads
// included, evaluating lg3 at its own y + a, N - y + b, a and b -- and, for
// null_row, beside the form without the broadcast (every lane its own lg3(a),
// lg3(b)).
//
//   pad_neutral_host <file> : the file holds n and then n cases, each
//     pmd accf null_row whole_pair q A c phi      (flags 0 / 1, hex floats)
//     32 lines "y N"                               (hex floats; lanes 15, 31: 0 0)
//   one output line per lane: case, lane, then 17 columns (the 16 accumulators
//   and the returned log-likelihood, 16 hex digits each) of the header's form,
//   of the replaced form, and of the form without the broadcast.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../metadamage_amd/csrc/mdfit_model.h"

using namespace mdfit;

static unsigned long long bits(double v) {
  unsigned long long b;
  std::memcpy(&b, &v, 8);
  return b;
}

// point_accum<true> as it was before the pad's neutral argument
static double point_accum_replaced(const PointData& pd, const Theta& th, double acc[kNAcc], int accf, bool null_row,
                                   bool whole_pair, bool broadcast) {
  const PointArgs pa = point_args(pd, th);
  const LG3 t3 = lg3<true>(pd.N + th.phi);
  const LG3 t6 = rowb3<15>(t3);
  const LG3 t1 = lg3<true>(pd.y + pa.a);
  const LG3 t2 = lg3<true>(pd.N - pd.y + pa.b);
  LG3 t4, t5;
  if (null_row && broadcast) {
    t4 = rowb3<15>(t1);
    t5 = rowb3<15>(t2);
  } else if (whole_pair && !null_row) {
    const bool odd = (threadIdx.x & 16) != 0;
    const LG3 mine = lg3<true>(odd ? pa.b : pa.a);
    const LG3 other = {xrow(mine.l), xrow(mine.p), xrow(mine.q)};
    t4 = odd ? other : mine;
    t5 = odd ? mine : other;
  } else {
    t4 = lg3<true>(pa.a);
    t5 = lg3<true>(pa.b);
  }
  return point_finish(pd, th, pa, t1, t2, t3, t4, t5, t6, acc, accf);
}

struct Case {
  int pmd, accf, null_row, whole_pair;
  double q, A, c, phi;
  double y[32], N[32];
};

static Theta theta_of(const Case& k) {
  Theta th;
  th.q = k.q;
  th.omq = 1.0 - k.q;
  th.iomq = 1.0 / th.omq;
  th.phi = k.phi;
  th.delta = k.phi - 2.0;
  th.lprior = 0.0;
  if (k.pmd) {
    th.A = k.A;
    th.JA = k.A * (1.0 - k.A);
    th.c = k.c;
    th.iomc = 1.0 / (1.0 - k.c);
  } else {
    th.A = th.JA = th.c = 0.0;
    th.iomc = 1.0;
  }
  return th;
}

// form 0: the header's; 1: the replaced one; 2: the replaced one without the broadcast
static void run(const Case& k, int form, double out[32][kNAcc + 1]) {
  mdfit_shim::Lanes& l = mdfit_shim::lanes();
  for (int lane = 0; lane < 64; ++lane) l.rec[lane].clear();
  const Theta th = theta_of(k);
  for (int pass = 0; pass < 2; ++pass) {
    l.pass = pass;
    for (int lane = 0; lane < 32; ++lane) {
      l.seq[lane] = 0;
      threadIdx.x = (unsigned)lane;
      PointData pd;
      pd.valid = (lane & 15) < kNHalf;
      pd.pmd = k.pmd;
      pd.k = pd.valid ? (lane & 15) : 0;
      pd.y = pd.valid ? k.y[lane] : 0.0;
      pd.N = pd.valid ? k.N[lane] : 0.0;
      double acc[kNAcc];
      for (int j = 0; j < kNAcc; ++j) acc[j] = 0.0;
      double ell;
      if (form == 0) ell = point_accum<true>(pd, th, acc, k.accf, k.null_row != 0, k.whole_pair != 0);
      else ell = point_accum_replaced(pd, th, acc, k.accf, k.null_row != 0, k.whole_pair != 0, form == 1);
      for (int j = 0; j < kNAcc; ++j) out[lane][j] = acc[j];
      out[lane][kNAcc] = ell;
    }
  }
}

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
  long n = 0;
  if (std::fscanf(f, "%ld", &n) != 1 || n < 0) {
    std::fprintf(stderr, "bad header\n");
    return 2;
  }
  char a[4][64];
  for (long i = 0; i < n; ++i) {
    Case k;
    if (std::fscanf(f, "%d %d %d %d %63s %63s %63s %63s", &k.pmd, &k.accf, &k.null_row, &k.whole_pair, a[0], a[1], a[2],
                    a[3]) != 8) {
      std::fprintf(stderr, "short file at case %ld\n", i);
      return 2;
    }
    k.q = std::strtod(a[0], nullptr);
    k.A = std::strtod(a[1], nullptr);
    k.c = std::strtod(a[2], nullptr);
    k.phi = std::strtod(a[3], nullptr);
    for (int lane = 0; lane < 32; ++lane) {
      if (std::fscanf(f, "%63s %63s", a[0], a[1]) != 2) {
        std::fprintf(stderr, "short file at case %ld, lane %d\n", i, lane);
        return 2;
      }
      k.y[lane] = std::strtod(a[0], nullptr);
      k.N[lane] = std::strtod(a[1], nullptr);
    }
    static double o[3][32][kNAcc + 1];
    for (int form = 0; form < 3; ++form) run(k, form, o[form]);
    for (int lane = 0; lane < 32; ++lane) {
      std::printf("%ld %d", i, lane);
      for (int form = 0; form < 3; ++form)
        for (int j = 0; j <= kNAcc; ++j) std::printf(" %016llx", bits(o[form][lane][j]));
      std::printf("\n");
    }
  }
  std::fclose(f);
  return 0;
}
