// mdfit_mapjoint.hip — mdfit_map_joint and mdfit_map_joint_adapt (DESIGN.md
// §3.18): the WAIC record of mdfit_map_waic, the evidence record of
// mdfit_map_evidence and the posterior record of mdfit_map_psis from one launch
// that forms each sub-fit's weights once.  A translation unit of its own, the
// entries included, so that mdfit.hip and the code objects of the three kernels
// it is measured against are the ones they were.
#define MDFIT_NO_HELPER_KERNELS 1  // (the one-wave helper kernels of the headers live in mdfit.hip)
#include "mdfit_host.h"
#include "mdfit_mapevid.h"

namespace mdfit::mapjoint {

using namespace mapis;

// One wave per taxon, its six sub-fits one after another in diagnostic-slot
// order, on map_waic_kernel's scaffolding.  Phases 1-3 are the core's
// (mdfit_mapis.h), called as map_waic_kernel calls them, so the weights in s_w,
// khat, n_inf, the level, the draws tap and the adapt record are that kernel's.
// Phase 4, per sub-fit, on the one set of weights: waic_points and waic_row
// (map_waic_kernel's), then K_prior - K_prop of the proposal that stands in
// s_par and evidence_row (map_evidence_kernel's), then, for the PMD slots 0, 2,
// 3, psis_estimates over the draws regenerated from the stream
// (map_psis_kernel's, rows 0, 1, 2 of psis).  Every row function is the
// existing one; the adapted bit and the best round go in as each kernel puts
// them.
//
// LDS: waic_points overlays its tile and accumulators on the work buffer from
// s_w + S on and leaves lppd_i and p_i in the static s_pt; it only reads s_w[0,
// S).  evidence_row and psis_estimates read s_w[0, S) and nothing behind it, and
// waic_row has read s_pt before they run, so nothing the overlay holds is live
// when they read the weights; s_pt stays untouched until the pointwise copy at
// the end of the sub-fit.  Dynamic LDS: mapwaic::lds_len(S) doubles (22,016 B
// at S = 1024, 11,048 B at S = 256); static: map_waic_kernel's 4,448 B and
// s_ev's 96 B.  Reads y, N, out and status only.
template <bool kAdapt>
__global__ __launch_bounds__(64) void map_joint_kernel(const uint32_t* __restrict__ gy,
                                                       const uint32_t* __restrict__ gN,
                                                       const double* __restrict__ out,
                                                       const int32_t* __restrict__ status, int64_t n_taxa, int S,
                                                       uint64_t seed, int64_t index_base, double tau,
                                                       double* __restrict__ waic, double* __restrict__ evid,
                                                       double* __restrict__ psis, double* __restrict__ pointwise,
                                                       double* __restrict__ draws, int adapt_rounds,
                                                       double* __restrict__ adapt) {
  namespace mw = mapwaic;
  namespace me = mapevid;
  namespace mp = mappsis;
  constexpr int kMaxPts = mw::kMaxPts;
  extern __shared__ double s_w[];
  __shared__ double s_y[kLD], s_N[kLD];
  __shared__ double s_par[MDFIT_NSUBFIT][kNPar];
  __shared__ double s_l0[kMaxPts], s_pt[2][kMaxPts];    // the current sub-fit's shift, lppd_i and p_i
  __shared__ double s_col[MDFIT_NSUBFIT + 1][kMaxPts];  // waic_i; row 6: PMD-forward | PMD-reverse
  __shared__ double s_ev[2][MDFIT_NSUBFIT];             // log Z and se of the rows (lane 0's)
  const int lane = threadIdx.x;
  const int64_t t = blockIdx.x;
  if (t >= n_taxa) return;
  double* rec = waic + t * (MDFIT_NSUBFIT + 1) * MDFIT_NMAPWAIC;
  double* erec = evid + t * (MDFIT_NSUBFIT + 1) * MDFIT_NMAPEVID;
  double* prec = psis + t * 3 * MDFIT_NMAPPSIS;
  double* pw = pointwise != nullptr ? pointwise + t * MDFIT_NSUBFIT * kMaxPts * 2 : nullptr;
  double* dr0 = draws != nullptr ? draws + t * MDFIT_NSUBFIT * (int64_t)S * 6 : nullptr;

  if (status[t] != MDFIT_OK) {  // wave-uniform: NaN statistics, flags 0
    if (lane < MDFIT_NSUBFIT + 1) {
      mw::invalid_row(rec + lane * MDFIT_NMAPWAIC, 0u);
      me::invalid_row(erec + lane * MDFIT_NMAPEVID, 0u);
    }
    if (lane < 3) mp::invalid_row(prec + lane * MDFIT_NMAPPSIS, 0u);
    if (pw != nullptr)
      for (int i = lane; i < MDFIT_NSUBFIT * kMaxPts * 2; i += 64) pw[i] = NAN;
    bad_status_fills<kAdapt>(dr0, (int64_t)MDFIT_NSUBFIT * S * 6, adapt, t);
    return;
  }
  load_counts(gy, gN, t, s_y, s_N);
  for (int x = lane; x < (MDFIT_NSUBFIT + 1) * kMaxPts; x += 64) (&s_col[0][0])[x] = NAN;

  // ---- phase 1: the modes, g and H there, the held sets ----
  proposals<true>(gy, gN, out, t, s_par);
  proposals<false>(gy, gN, out, t, s_par);
  __syncthreads();

  const PsisWave w;
  const uint64_t gtaxon = (uint64_t)(index_base + t);
  double* tile = s_w + S;
  double* s_acc = tile + mw::tile_len(64);
  double kmax = -INFINITY, emin = INFINITY, e_emin = INFINITY;
  bool all_ok = true, all_rel = true;
  for (int s = 0; s < MDFIT_NSUBFIT; ++s) {
    const bool pmd = s == 0 || s == 2 || s == 3;
    const int lo = (s == 3 || s == 5) ? kNHalf : 0, hi = s < 2 ? kNPos : lo + kNHalf;
    const int n = hi - lo;
    const double* P = s_par[s];
    const unsigned mask = (unsigned)P[kPMask];
    double* dr = dr0 != nullptr ? dr0 + (int64_t)s * S * 6 : nullptr;
    bool ok = P[kPValid] != 0.0;          // (wave-uniform)
    const int arow = s == 0 ? 0 : s - 1;  // a PMD sub-fit's row of the adapt record and of psis
    if (ok) {
      const Stream st = subfit_stream(seed, gtaxon, s);
      // ---- phases 2-3: the draws, the smoothed weights, the rounds ----
      const SubfitWeights sw = subfit_weights<kAdapt, true>(w, pmd, lo, hi, s_par[s], st, S, tau, adapt_rounds, s_y,
                                                            s_N, s_w, s_l0, dr);
      ok = sw.ok;
      if constexpr (kAdapt)
        if (pmd) adapt_row(adapt, t, arow, sw);
      draws_weights(dr, s_w, S, ok);
      if (ok) {
        // ---- phase 4a: the pointwise statistics, the waic row ----
        mw::waic_points(w, s_w, S, n, mw::StreamSource{P, st, pmd, lo, s_y, s_N}, s_l0, tile, s_acc, s_pt[0],
                        s_pt[1]);
        const double ess =
            mw::waic_row(w, s_pt[0], s_pt[1], n, s_w, S, sw.khat, sw.n_inf, tau, mask, rec + s * MDFIT_NMAPWAIC);
        if constexpr (kAdapt)
          if (sw.best > 0 && lane == 0) rec[s * MDFIT_NMAPWAIC + mw::kFlags] += (double)mapadapt::kAdaptedBit;
        kmax = fmax(kmax, sw.khat);
        emin = fmin(emin, ess);
        all_rel = all_rel && sw.khat <= tau;
        if (lane < n) {
          const double wv = -2.0 * (s_pt[0][lane] - s_pt[1][lane]);
          s_col[s][lo + lane] = wv;
          if (s == 2 || s == 3) s_col[MDFIT_NSUBFIT][lo + lane] = wv;
        }
        // ---- phase 4b: the constants of the round in LDS, the evidence row ----
        double K = 0.0;
        if (lane == 0) K = me::prior_constant(pmd) - me::proposal_constant(P);
        double* row = erec + s * MDFIT_NMAPEVID;
        const me::EvidenceStats e = me::evidence_row(w, s_w, S, sw.shift, sw.total, K, sw.khat, sw.n_inf, tau, mask, row);
        if (lane == 0) {
          s_ev[0][s] = e.log_z;
          s_ev[1][s] = e.se;
          if constexpr (kAdapt) {
            row[me::kRound] = (double)sw.best;
            if (sw.best > 0) row[me::kFlags] += (double)mapadapt::kAdaptedBit;
          }
        }
        e_emin = fmin(e_emin, e.ess);
        // ---- phase 4c: the posterior's estimates of a PMD sub-fit ----
        if (pmd) {
          double* prow = prec + arow * MDFIT_NMAPPSIS;
          mp::psis_estimates(w, s_w, S, mp::StreamDraws{P, st}, sw.khat, sw.n_inf, tau, mask, prow);
          if constexpr (kAdapt)
            if (sw.best > 0 && lane == 0) prow[mp::kFlags] += (double)mapadapt::kAdaptedBit;
        }
      }
    } else if (dr != nullptr) {
      nan_fill(dr, (int64_t)S * 6);
    }
    if constexpr (kAdapt)
      if (!ok && pmd) adapt_row_nan(adapt, t, arow);
    if (!ok) {
      all_ok = false;
      if (lane == 0) {
        mw::invalid_row(rec + s * MDFIT_NMAPWAIC, mask);
        me::invalid_row(erec + s * MDFIT_NMAPEVID, mask);
        s_ev[0][s] = NAN;
        s_ev[1][s] = NAN;
        if (pmd) mp::invalid_row(prec + arow * MDFIT_NMAPPSIS, mask);
      }
    }
    if (pw != nullptr && lane < 2 * kMaxPts) {
      const int col = lane >> 1;
      const bool in = ok && col >= lo && col < hi;
      pw[(s * kMaxPts) * 2 + lane] = in ? s_pt[lane & 1][col - lo] : NAN;
    }
    __syncthreads();  // (the next sub-fit overwrites s_w, s_l0 and s_pt)
  }
  // row 6 of waic: fits.py:194-227 on waic_i (an invalid row's column is NaN: its comparisons are)
  const double ns = nutsloo::n_sigma(w, s_col[0], s_col[1], kNPos);
  const double nsf = nutsloo::n_sigma(w, s_col[2], s_col[4], kNHalf);
  const double nsr = nutsloo::n_sigma(w, s_col[3] + kNHalf, s_col[5] + kNHalf, kNHalf);
  const double asy = nutsloo::n_sigma(w, s_col[0], s_col[MDFIT_NSUBFIT], kNPos);
  if (lane == 0) {
    double* r6 = rec + MDFIT_NSUBFIT * MDFIT_NMAPWAIC;
    r6[mw::kNSigma] = ns;
    r6[mw::kNSigmaForward] = nsf;
    r6[mw::kNSigmaReverse] = nsr;
    r6[mw::kAsymmetry] = asy;
    r6[mw::kKhatMax] = kmax > -INFINITY ? kmax : NAN;
    r6[mw::kEssMin] = emin < INFINITY ? emin : NAN;
    r6[6] = 0.0;
    r6[mw::kFlags] = (double)((all_ok ? mw::kValidBit : 0u) | (all_ok && all_rel ? mw::kReliableBit : 0u));
    // row 6 of evid, from the six rows' log Z and se
    me::compare_row(s_ev[0], s_ev[1], kmax > -INFINITY ? kmax : NAN, e_emin < INFINITY ? e_emin : NAN, all_ok, all_rel,
                    erec + MDFIT_NSUBFIT * MDFIT_NMAPEVID);
  }
}

template <bool kAdapt>
int launch(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status, int64_t n_taxa,
           int32_t num_draws, int32_t adapt_rounds, uint64_t seed, int64_t index_base, double* waic, double* evid,
           double* psis, double* adapt, double* pointwise, double* draws, void* hip_stream) {
  using host::set_err;
  // the importance sampler's argument checks, in the order its other entries make them
  if (n_taxa < 0) return set_err(MDFIT_E_ARG, "n_taxa < 0");
  if (num_draws < mappsis::kMinDraws || num_draws > mappsis::kMaxDraws)
    return set_err(MDFIT_E_ARG, "num_draws must be in [25, 1024]");
  if (adapt_rounds < 0 || adapt_rounds > mapadapt::kMaxRounds)
    return set_err(MDFIT_E_ARG, "adapt_rounds must be in [0, 4]");
  if (n_taxa == 0) return 0;
  if (!(y && N && out && status && waic && evid && psis)) return set_err(MDFIT_E_ARG, "null required pointer");
  if (n_taxa > ((int64_t)1 << 25)) return set_err(MDFIT_E_ARG, "n_taxa exceeds 2^25 per call");
  const int S = (int)num_draws;
  host::debug_poison((hipStream_t)hip_stream);
  hipLaunchKernelGGL(map_joint_kernel<kAdapt>, dim3((unsigned)n_taxa), dim3(mdfit::kWave),
                     (size_t)mapwaic::lds_len(S) * sizeof(double), (hipStream_t)hip_stream, y, N, out, status, n_taxa,
                     S, seed, index_base, mappsis::khat_threshold(S), waic, evid, psis, pointwise, draws,
                     (int)adapt_rounds, adapt);
  return host::check_launch(kAdapt ? "map_joint_kernel<adapt>" : "map_joint_kernel");
}

}  // namespace mdfit::mapjoint

extern "C" {

int mdfit_map_joint(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status, int64_t n_taxa,
                    int32_t num_draws, uint64_t seed, int64_t index_base, double* waic, double* evid, double* psis,
                    double* pointwise, double* draws, void* hip_stream) {
  return mdfit::mapjoint::launch<false>(y, N, out, status, n_taxa, num_draws, 0, seed, index_base, waic, evid, psis,
                                        nullptr, pointwise, draws, hip_stream);
}

int mdfit_map_joint_adapt(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                          int64_t n_taxa, int32_t num_draws, int32_t adapt_rounds, uint64_t seed, int64_t index_base,
                          double* waic, double* evid, double* psis, double* adapt, double* pointwise, double* draws,
                          void* hip_stream) {
  return mdfit::mapjoint::launch<true>(y, N, out, status, n_taxa, num_draws, adapt_rounds, seed, index_base, waic,
                                       evid, psis, adapt, pointwise, draws, hip_stream);
}

}  // extern "C"
