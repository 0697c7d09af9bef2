// Host driver of MDFIT-EVID v1 (csrc/mdfit_mapevid.h with its one-lane policy)
// for tests/test_map_evidence.py: plain g++, no HIP.  argv[1]: a file holding
// the number of items, then per item either
//   w S  and its S raw log-weights  -> stdout: logz se khat (mdfit_log_mean_weight's), or
//   p    and the 32 words of a proposal -> stdout: K_prop (proposal_constant),
// numbers as C hex floats (or nan, inf, -inf).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../metadamage_amd/csrc/mdfit_mapevid.h"

int main(int argc, char** argv) {
  namespace me = mdfit::mapevid;
  namespace mp = mdfit::mappsis;
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int count = 0;
  if (std::fscanf(f, "%d", &count) != 1) return 2;
  for (int i = 0; i < count; ++i) {
    char kind = 0;
    if (std::fscanf(f, " %c", &kind) != 1) return 2;
    if (kind == 'w') {
      int S = 0;
      if (std::fscanf(f, "%d", &S) != 1 || S < mp::kMinDraws || S > mp::kMaxDraws) return 2;
      // exactly the length the routine is given: a sanitizer sees any access beyond it
      std::vector<double> work((size_t)mp::work_len(S));
      for (int t = 0; t < S; ++t)
        if (std::fscanf(f, "%la", &work[(size_t)t]) != 1) return 2;
      double logz, se, khat;
      me::log_mean_weight_host(work.data(), S, &logz, &se, &khat);
      std::printf("%a %a %a\n", logz, se, khat);
    } else if (kind == 'p') {
      std::vector<double> P((size_t)mp::kNPar);
      for (auto& v : P)
        if (std::fscanf(f, "%la", &v) != 1) return 2;
      std::printf("%a\n", me::proposal_constant(P.data()));
    } else {
      return 2;
    }
  }
  std::fclose(f);
  return 0;
}
