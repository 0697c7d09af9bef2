// mdfit_host.h — host-side helpers shared by the translation units of
// libmdfit.so (mdfit.hip: C-ABI + MAP kernels, mdfit_nuts.hip: sampling mode,
// mdfit_mappred_adapt.hip: the adapting predictive kernel, mdfit_mapppc.hip:
// the posterior predictive check, mdfit_mapquant.hip: the weighted order
// statistics).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/mdfit.h"

namespace mdfit {
constexpr int kWave = 64;
constexpr int kQueues = 8;  // one work queue per XCD (blockIdx % 8 share an XCD)
}  // namespace mdfit

namespace mdfit::host {
extern thread_local char g_err[512];
// record an argument / launch error for mdfit_last_error(); returns code
int set_err(int code, const char* msg);
// hipGetLastError after a launch -> 0 or the hipError_t (message recorded)
int check_launch(const char* what);

// optional HIP-event timing (mdfit_profile_enable): slot 1 / 2 bracket the
// dominant kernel of the call
void prof_mark(int slot, hipStream_t s);

// persistent grid: no more waves than can be resident at once (so every
// wave starts immediately and pulls work until its queue is drained), a
// multiple of the 8 queues
// (cap_per_cu > 0: at most that many waves per CU; force_per_cu > 0: exactly
// that many -- development A/B; MDFIT_DEV_GRID prints the sizing)
template <typename K>
int64_t fit_grid(K kernel, int64_t ntask, int fits_per_wave, int cap_per_cu = 0, int force_per_cu = 0) {
  int dev = 0, n_cu = 256, per_cu = 8;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0)
    n_cu = 256;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kWave, 0) != hipSuccess || per_cu <= 0)
    per_cu = 8;
  if (cap_per_cu > 0 && cap_per_cu < per_cu) per_cu = cap_per_cu;
  const int api = per_cu;
  if (force_per_cu > 0) per_cu = force_per_cu;
  const int64_t want = (ntask + fits_per_wave - 1) / fits_per_wave;
  const int64_t cap = (int64_t)n_cu * per_cu;
  int64_t g = want < cap ? want : cap;
  g = ((g + kQueues - 1) / kQueues) * kQueues;
  if (std::getenv("MDFIT_DEV_GRID")) {
    hipFuncAttributes fa{};
    (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kernel));
    int lds_cu = 0;
    (void)hipDeviceGetAttribute(&lds_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev);
    std::fprintf(stderr, "fit_grid: n_cu %d occupancy-api %d per_cu %d lds/block %zu regs %d lds/cu %d -> grid %lld\n",
                 n_cu, api, per_cu, fa.sharedSizeBytes, fa.numRegs, lds_cu, (long long)g);
  }
  return g < kQueues ? kQueues : g;
}
}  // namespace mdfit::host

namespace mdfit::host {
// MDFIT_DEBUG_POISON_LDS=1 (tests): NaN into every CU's LDS on stream s
// (mdfit_poison_lds) -- called before each LDS-using kernel of a call
void debug_poison(hipStream_t s);
}  // namespace mdfit::host

namespace mdfit::mappred {
// mdfit_map_pred_adapt's launch (mdfit_mappred_adapt.hip: map_pred_kernel<true>
// in a unit of its own flags); the arguments are checked by the caller
int launch_adapt(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status, int64_t n_taxa, int S,
                 int R, int adapt_rounds, uint64_t seed, int64_t index_base, float* ppred, double* rec, double* adapt,
                 int32_t* index, uint32_t* counts, hipStream_t s);
}  // namespace mdfit::mappred

namespace mdfit::mapppc {
// mdfit_map_ppc's and mdfit_map_ppc_adapt's launch (mdfit_mapppc.hip: both
// instantiations of map_ppc_kernel); the arguments are checked by the caller
int launch(bool adapting, const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
           int64_t n_taxa, int S, int R, int adapt_rounds, uint64_t seed, int64_t index_base, float* ppos, double* rec,
           double* adapt, int32_t* index, uint32_t* counts, double* disc, hipStream_t s);
}  // namespace mdfit::mapppc

namespace mdfit::mapquant {
// mdfit_map_quant's and mdfit_map_quant_adapt's launch (mdfit_mapquant.hip:
// both instantiations of map_quant_kernel) and mdfit_weighted_order_stats';
// the arguments are checked by the caller
int launch(bool adapting, const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
           int64_t n_taxa, int S, int adapt_rounds, uint64_t seed, int64_t index_base, double d0, double* quant,
           double* adapt, double* values, hipStream_t s);
int launch_series(const double* v, const double* w, int64_t n_series, int S, double d0, double* res, hipStream_t s);
}  // namespace mdfit::mapquant

namespace mdfit::nuts {
// sampling mode (mdfit_nuts.hip): workspace = 256 B of queue counters, then
// the chains' samples double[T][6][num_samples][4] = (q, A, c, phi)
constexpr int64_t kSamplesOffset = 256;
int64_t workspace_bytes(int64_t n_taxa, int num_samples);
// register-only throughput probe of the chain kernel's potential evaluation
int peak_probe(int64_t n_waves, int iters, double* sink, hipStream_t s);
int potential(const int32_t* model, const int32_t* subset, const uint32_t* y, const uint32_t* N, const double* v,
              int64_t n, double* U, double* g, hipStream_t s);
// launches the chain and post-processing kernels (workspace already zeroed);
// taxon_index (device int64[n_taxa], or null): row t's streams are keyed by
// index_base + taxon_index[t] instead of index_base + t -- the INDEXED
// instantiations of both kernels (mdfit_fit_batch_indexed); null launches the
// plain ones
int fit_batch(const uint32_t* y, const uint32_t* N, const uint32_t* mm, int64_t n_taxa, const mdfit_opts& o,
              double* out, float* pred, int32_t* status, void* workspace, hipStream_t s,
              const int64_t* taxon_index = nullptr);
// MDFIT-DIAG v1 of the chains a finished fit_batch left in `workspace`: one
// launch, reads the draws and out's chain status slots, writes
// diag[n_taxa][6][MDFIT_NNUTSDIAG]
int diag(const void* workspace, const double* out, int64_t n_taxa, const mdfit_opts& o, double* diag_out,
         hipStream_t s);
// MDFIT-SUMM v1 of the same chains: one launch, reads the draws and out's chain
// status slots, writes summ[n_taxa][6][MDFIT_NNUTSSUMM]
int summary(const void* workspace, const double* out, int64_t n_taxa, const mdfit_opts& o, double* summ_out,
            hipStream_t s);
// MDFIT-LOO v1 of the same chains: one launch, reads y, N, the draws and out's
// chain status slots, writes loo[n_taxa][7][MDFIT_NNUTSLOO] and, unless null,
// pointwise[n_taxa][6][30][2]
int loo(const uint32_t* y, const uint32_t* N, const void* workspace, const double* out, int64_t n_taxa,
        const mdfit_opts& o, double* loo_out, double* pointwise, hipStream_t s);
// the post kernel alone (its tapped instantiation) on a workspace and chain
// diag slots (out's 4..7 per sub-fit) the caller filled: writes out, pred
// (unless null), status and the taps that are not null
int post(const uint32_t* y, const uint32_t* N, const uint32_t* mm, int64_t n_taxa, const mdfit_opts& o,
         const void* workspace, double* out, float* pred, int32_t* status, double* waic, uint32_t* counts,
         uint8_t* count_flags, hipStream_t s);
// steps 1-6 of MDFIT-LOO v1 on given series ll[n_series][S], one wave per series
int psis(const double* ll, int64_t n_series, int S, double* elpd, double* khat, hipStream_t s);
}  // namespace mdfit::nuts
