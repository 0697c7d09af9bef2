// mdfit_mapppc.hip — the posterior predictive check's kernel (mdfit_map_ppc and
// mdfit_map_ppc_adapt, MDFIT-PPC v1) as a translation unit of
// its own, compiled with MachineLICM off as the adapting predictive kernel's
// unit is and for its reason (mdfit_mappred_adapt.hip).  mdfit.hip keeps the
// C-ABI entries, which check the arguments and call launch.
#define MDFIT_NO_HELPER_KERNELS 1  // (the one-wave helper kernels of the headers live in mdfit.hip)
#include "mdfit_host.h"
#include "mdfit_mapppc.h"

namespace mdfit::mapppc {

int launch(bool adapting, const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
           int64_t n_taxa, int S, int R, int adapt_rounds, uint64_t seed, int64_t index_base, float* ppos, double* rec,
           double* adapt, int32_t* index, uint32_t* counts, double* disc, hipStream_t s) {
  const double tau = mappsis::khat_threshold(S);
  if (adapting) {
    hipLaunchKernelGGL(map_ppc_kernel<true>, dim3((unsigned)n_taxa), dim3(mdfit::kWave), lds_bytes(S, R), s, y, N, out,
                       status, n_taxa, S, R, seed, index_base, tau, ppos, rec, index, counts, disc, adapt_rounds, adapt);
    return mdfit::host::check_launch("map_ppc_kernel<adapt>");
  }
  hipLaunchKernelGGL(map_ppc_kernel<false>, dim3((unsigned)n_taxa), dim3(mdfit::kWave), lds_bytes(S, R), s, y, N, out,
                     status, n_taxa, S, R, seed, index_base, tau, ppos, rec, index, counts, disc, 0, (double*)nullptr);
  return mdfit::host::check_launch("map_ppc_kernel");
}

}  // namespace mdfit::mapppc
