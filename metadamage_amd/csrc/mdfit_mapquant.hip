// mdfit_mapquant.hip — the weighted order statistics' kernels (mdfit_map_quant,
// mdfit_map_quant_adapt and the helper mdfit_weighted_order_stats, MDFIT-QUANT
// v1) as a translation unit of its own, compiled with
// MachineLICM off as the posterior predictive check's unit is and for its
// reason (mdfit_mapppc.hip; profiles/map_quant_resources.txt).  mdfit.hip keeps
// the C-ABI entries, which check the arguments and call launch.
#define MDFIT_NO_HELPER_KERNELS 1  // (the one-wave helper kernels of the headers live in mdfit.hip)
#include "mdfit_host.h"
#include "mdfit_mapquant.h"

namespace mdfit::mapquant {

int launch(bool adapting, const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
           int64_t n_taxa, int S, int adapt_rounds, uint64_t seed, int64_t index_base, double d0, double* quant,
           double* adapt, double* values, hipStream_t s) {
  const double tau = mappsis::khat_threshold(S);
  const size_t lds = (size_t)work_len(S) * sizeof(double);
  if (adapting) {
    hipLaunchKernelGGL(map_quant_kernel<true>, dim3((unsigned)n_taxa), dim3(mdfit::kWave), lds, s, y, N, out, status,
                       n_taxa, S, seed, index_base, tau, d0, quant, values, adapt_rounds, adapt);
    return mdfit::host::check_launch("map_quant_kernel<adapt>");
  }
  hipLaunchKernelGGL(map_quant_kernel<false>, dim3((unsigned)n_taxa), dim3(mdfit::kWave), lds, s, y, N, out, status,
                     n_taxa, S, seed, index_base, tau, d0, quant, values, 0, (double*)nullptr);
  return mdfit::host::check_launch("map_quant_kernel");
}

int launch_series(const double* v, const double* w, int64_t n_series, int S, double d0, double* res, hipStream_t s) {
  hipLaunchKernelGGL(weighted_order_stats_kernel, dim3((unsigned)n_series), dim3(mdfit::kWave),
                     (size_t)work_len(S) * sizeof(double), s, v, w, n_series, S, d0, res);
  return mdfit::host::check_launch("weighted_order_stats_kernel");
}

}  // namespace mdfit::mapquant
