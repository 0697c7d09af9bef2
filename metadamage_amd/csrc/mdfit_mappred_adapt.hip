// mdfit_mappred_adapt.hip — the adapting instantiation of the predictive kernel
// (mdfit_map_pred_adapt, MDFIT-AUTO v1.1) as a translation
// unit of its own, compiled with MachineLICM off as the NUTS unit is: with the
// rounds' refit inlined into map_pred_kernel, the constants MachineLICM hoists
// out of the row loop stay live across the refit's calls and the kernel takes
// 256 VGPRs + 22 AGPRs (1 wave/SIMD) in the MAP unit; here 162, no scratch.
// mdfit.hip keeps the plain instantiation and the C-ABI entry, which checks
// the arguments and calls launch_adapt.
#define MDFIT_NO_HELPER_KERNELS 1  // (the one-wave helper kernels of the headers live in mdfit.hip)
#include "mdfit_host.h"
#include "mdfit_mappred.h"

namespace mdfit::mappred {

int launch_adapt(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status, int64_t n_taxa, int S,
                 int R, int adapt_rounds, uint64_t seed, int64_t index_base, float* ppred, double* rec, double* adapt,
                 int32_t* index, uint32_t* counts, hipStream_t s) {
  const int tc = tile_cols(S, R);
  hipLaunchKernelGGL(map_pred_kernel<true>, dim3((unsigned)n_taxa), dim3(mdfit::kWave), lds_bytes(S, R, tc), s, y, N,
                     out, status, n_taxa, S, R, tc, seed, index_base, mappsis::khat_threshold(S), ppred, rec, index,
                     counts, adapt_rounds, adapt);
  return mdfit::host::check_launch("map_pred_kernel<adapt>");
}

}  // namespace mdfit::mappred
