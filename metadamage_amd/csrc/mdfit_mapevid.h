// mdfit_mapevid.h — MDFIT-EVID v1 (mdfit_map_evidence): the
// marginal likelihood of each of the six sub-fits of a MAP fit from the
// importance weights of mdfit_mapwaic.h, and the Bayes factors PMD : null on
// them.  The raw log-weights lw_t = log p~(u_t) - log g(u_t) of a sub-fit are
// map_waic_kernel's, constants dropped; psis_weights_level smooths them and
// gives up what the normalisation drops, the shift c = max lw and the sum tot
// of the smoothed, shifted weights.  With the constants put back,
//   log Z = (K_prior - K_prop) + c + log(tot / S),
//   se    = sqrt(sum_t (w_t - 1/S)^2)     (= sqrt(1/ess - 1/S): sum w = 1)
// the delta-method standard error of the log of a mean of S weights.
//
// The row (evidence_row) is written once over a `lanes` policy, as
// mdfit_mapwaic.h: the kernel below runs it with the 64 lanes of a wave, a
// plain C++ program (g++, no HIP) with the one-lane policy
// (tests/mapevid_host_main.cpp).  Its sums are per-lane strided partials in
// ascending draw index plus the policy's reduction.
#pragma once

#include <cmath>
#include <cstdint>

#include "mdfit_mapwaic.h"

namespace mdfit::mapevid {

// record layout (MDFIT_NMAPEVID = 8 doubles per row); rows 0..5 the sub-fits
constexpr int kLogEvidence = 0, kSe = 1, kKhat = 2, kEss = 3, kNInfeasible = 4, kLogWMax = 5, kRound = 6, kFlags = 7;
// row 6, the comparisons
constexpr int kLogBf = 0, kLogBfForward = 1, kLogBfReverse = 2, kLogBfAsymmetry = 3, kLogBfSe = 4, kKhatMax = 5,
              kEssMin = 6;
constexpr unsigned kValidBit = 1u, kReliableBit = 2u;  // flags; rows 0..5: bits 2..5 coordinate (q, A, c, phi) free

using mappsis::kPCHeld;
using mappsis::kPD;
using mappsis::kPGc;
using mappsis::kPM;
using mappsis::kPMask;
using mappsis::OneLane;
using nutssumm::ns_nan;

// The constants psis_theta / null_theta leave out of the log prior: Beta(2, 3)
// on q (and A) 1 / B(2, 3) = 12, Beta(1, 9) on c 1 / B(1, 9) = 9, Exponential
// on delta its rate 1 / 1000 (the powers of q, A and 1 - c, -delta / 1000 and
// the Jacobian are in lj; the log-pmf is the full one).
constexpr double kLog12 = 2.4849066497880004, kLog9 = 2.1972245773362196, kLogRate = -6.907755278982137;
MDFIT_NS_FN double prior_constant(bool pmd) { return pmd ? ((kLog12 + kLog12) + kLog9) + kLogRate : kLog12 + kLogRate; }

// The constant psis_draw leaves out of lg, from the proposal's words P as they
// stand: the d free coordinates are u_j = m_j + P[kPD + j] sum_{p >= j} P[kPM +
// 4 p + j] t_p with t a d-variate Student-t (nu = 4) of unit scale, a triangular
// map whose log determinant is sum_free log P[kPD + j] + log P[kPM + 4 j + j];
// the initial proposal holds L^-1 in those words and a refitted one
// (mapadapt::next_proposal) F transposed, its scale in P[kPD], so one formula
// serves both.  A held c is e / P[kPGc], e standard exponential: its density
// adds log P[kPGc] (the centre's shift K c_s has unit determinant).
constexpr double kLog4Pi = 2.5310242469692907;
// lgamma((4 + d) / 2), d = 1..4; lgamma(nu / 2) = lgamma(2) = 0
constexpr double kLgamma25 = 0.2846828704729192, kLgamma3 = 0.6931471805599453, kLgamma35 = 1.2009736023470743,
                 kLgamma4 = 1.791759469228055;
MDFIT_NS_FN double proposal_constant(const double* P) {
  const unsigned mask = (unsigned)P[kPMask];
  int d = 0;
  double ldet = 0.0;
  for (int j = 0; j < 4; ++j) {
    if ((mask >> j) & 1u) {
      ++d;
      ldet += std::log(P[kPD + j]) + std::log(P[kPM + 4 * j + j]);
    }
  }
  const double lg = d == 4 ? kLgamma4 : (d == 3 ? kLgamma35 : (d == 2 ? kLgamma3 : (d == 1 ? kLgamma25 : 0.0)));
  double k = (lg - 0.5 * (double)d * kLog4Pi) - ldet;
  if (P[kPCHeld] != 0.0) k += std::log(P[kPGc]);
  return k;
}

struct EvidenceStats {
  double log_z, se, ess, log_w_max;
};

// The log of the mean weight and its standard error from the normalised weights
// wt[S] (shared by the lanes, written behind a barrier), the shift c and the
// sum tot of psis_weights_level and the constant K = K_prior - K_prop.  Every
// lane calls it and gets the same se and ess; log_z and log_w_max are those of
// the lane's own K.  Uniform weights have se = 0 exactly; ess is waic_row's
// arithmetic.
template <class L>
MDFIT_NS_FN EvidenceStats evidence_stats(const L& w, const double* wt, int S, double c, double tot, double K) {
  const int lane = w.lane(), nl = w.nlanes();
  const double u = 1.0 / (double)S;
  double s2 = 0.0, v = 0.0;
  for (int t = lane; t < S; t += nl) {
    const double wi = wt[t];
    s2 += wi * wi;
    const double dw = wi - u;
    v += dw * dw;
  }
  s2 = w.sum(s2);
  v = w.sum(v);
  EvidenceStats e;
  e.ess = 1.0 / s2;
  e.se = std::sqrt(v);
  e.log_w_max = K + c;
  e.log_z = e.log_w_max + std::log(tot / (double)S);
  return e;
}

// all-NaN record; flags: the free bits alone
MDFIT_NS_FN void invalid_row(double* rec, unsigned free_mask) {
  for (int k = 0; k < kFlags; ++k) rec[k] = ns_nan();
  rec[kFlags] = (double)((free_mask & 15u) << 2);
}

// One sub-fit's record.  Every lane calls it; lane 0, whose K counts, writes
// rec (round 0: the kernel puts the best round there).
template <class L>
MDFIT_NS_FN EvidenceStats evidence_row(const L& w, const double* wt, int S, double c, double tot, double K, double khat,
                                       double n_inf, double tau, unsigned free_mask, double* rec) {
  const EvidenceStats e = evidence_stats(w, wt, S, c, tot, K);
  if (w.lane() == 0) {
    rec[kLogEvidence] = e.log_z;
    rec[kSe] = e.se;
    rec[kKhat] = khat;
    rec[kEss] = e.ess;
    rec[kNInfeasible] = n_inf;
    rec[kLogWMax] = e.log_w_max;
    rec[kRound] = 0.0;
    rec[kFlags] = (double)(kValidBit | (khat <= tau ? kReliableBit : 0u) | ((free_mask & 15u) << 2));
  }
  return e;
}

// Row 6 from the rows' log Z and se (NaN in an invalid row: a comparison that
// needs it is NaN)
MDFIT_NS_FN void compare_row(const double lz[MDFIT_NSUBFIT], const double se[MDFIT_NSUBFIT], double khat_max,
                             double ess_min, bool all_ok, bool all_rel, double* r6) {
  r6[kLogBf] = lz[0] - lz[1];
  r6[kLogBfForward] = lz[2] - lz[4];
  r6[kLogBfReverse] = lz[3] - lz[5];
  r6[kLogBfAsymmetry] = lz[0] - (lz[2] + lz[3]);
  r6[kLogBfSe] = std::sqrt(se[0] * se[0] + se[1] * se[1]);
  r6[kKhatMax] = khat_max;
  r6[kEssMin] = ess_min;
  r6[kFlags] = (double)((all_ok ? kValidBit : 0u) | (all_ok && all_rel ? kReliableBit : 0u));
}

// Host form of mdfit_log_mean_weight: work holds mappsis::work_len(S) doubles,
// work[t] = lw_t on entry.  False (outputs NaN) where psis_weights refuses.
inline bool log_mean_weight_host(double* work, int S, double* logz, double* se, double* khat) {
  double n_inf, c, tot;
  const bool ok = mappsis::psis_weights_level(OneLane{}, work, S, *khat, n_inf, c, tot);
  if (!ok) {
    *logz = *se = *khat = ns_nan();
    return false;
  }
  const EvidenceStats e = evidence_stats(OneLane{}, work, S, c, tot, 0.0);
  *logz = e.log_z;
  *se = e.se;
  return true;
}

}  // namespace mdfit::mapevid

#if defined(__HIPCC__)
#include "mdfit_mapis.h"  // (the importance sampler's device core)

namespace mdfit::mapevid {

using namespace mapis;

// One wave per taxon, its six sub-fits one after another in diagnostic-slot
// order.  Phases 1-3 are the core's (mdfit_mapis.h), called as map_waic_kernel
// calls them: proposals<true> and <false>, then per sub-fit subfit_weights (the
// draws, the raw log-weights, psis_weights and, with kAdapt, the PMD rows'
// rounds).  Phase 4: lane 0 forms K_prior - K_prop from the proposal of the
// round whose weights stand in LDS, evidence_row the record; lane 0 then forms
// row 6 from the six rows' log Z and se in s_ev.  No pointwise tile: dynamic
// LDS is mappsis::work_len(S) doubles (22,016 B at S = 1024, 6,656 B at
// S = 256); static: 2,144 B.  Reads y, N, out and status only.
template <bool kAdapt>
__global__ __launch_bounds__(64) void map_evidence_kernel(const uint32_t* __restrict__ gy,
                                                          const uint32_t* __restrict__ gN,
                                                          const double* __restrict__ out,
                                                          const int32_t* __restrict__ status, int64_t n_taxa, int S,
                                                          uint64_t seed, int64_t index_base, double tau,
                                                          double* __restrict__ evid, double* __restrict__ draws,
                                                          int adapt_rounds, double* __restrict__ adapt) {
  extern __shared__ double s_w[];
  __shared__ double s_y[kLD], s_N[kLD];
  __shared__ double s_par[MDFIT_NSUBFIT][kNPar];
  __shared__ double s_ev[2][MDFIT_NSUBFIT];  // log Z and se of the rows (lane 0's)
  const int lane = threadIdx.x;
  const int64_t t = blockIdx.x;
  if (t >= n_taxa) return;
  double* rec = evid + t * (MDFIT_NSUBFIT + 1) * MDFIT_NMAPEVID;
  double* dr0 = draws != nullptr ? draws + t * MDFIT_NSUBFIT * (int64_t)S * 6 : nullptr;

  if (status[t] != MDFIT_OK) {  // wave-uniform: NaN statistics, flags 0
    if (lane < MDFIT_NSUBFIT + 1) invalid_row(rec + lane * MDFIT_NMAPEVID, 0u);
    bad_status_fills<kAdapt>(dr0, (int64_t)MDFIT_NSUBFIT * S * 6, adapt, t);
    return;
  }
  load_counts(gy, gN, t, s_y, s_N);

  // ---- phase 1: the modes, g and H there, the held sets ----
  proposals<true>(gy, gN, out, t, s_par);
  proposals<false>(gy, gN, out, t, s_par);
  __syncthreads();

  const PsisWave w;
  const uint64_t gtaxon = (uint64_t)(index_base + t);
  double kmax = -INFINITY, emin = INFINITY;
  bool all_ok = true, all_rel = true;
  for (int s = 0; s < MDFIT_NSUBFIT; ++s) {
    const bool pmd = s == 0 || s == 2 || s == 3;
    const int lo = (s == 3 || s == 5) ? kNHalf : 0, hi = s < 2 ? kNPos : lo + kNHalf;
    const double* P = s_par[s];
    const unsigned mask = (unsigned)P[kPMask];
    double* dr = dr0 != nullptr ? dr0 + (int64_t)s * S * 6 : nullptr;
    bool ok = P[kPValid] != 0.0;  // (wave-uniform)
    const int arow = s == 0 ? 0 : s - 1;  // a PMD sub-fit's row of the adapt record
    if (ok) {
      const Stream st = subfit_stream(seed, gtaxon, s);
      // ---- phases 2-3: the draws, the smoothed weights, the rounds ----
      const SubfitWeights sw = subfit_weights<kAdapt, false>(w, pmd, lo, hi, s_par[s], st, S, tau, adapt_rounds, s_y,
                                                             s_N, s_w, nullptr, dr);
      ok = sw.ok;
      if constexpr (kAdapt)
        if (pmd) adapt_row(adapt, t, arow, sw);
      draws_weights(dr, s_w, S, ok);
      if (ok) {
        // ---- phase 4: the constants of the round in LDS, the row ----
        double K = 0.0;
        if (lane == 0) K = prior_constant(pmd) - proposal_constant(P);
        double* row = rec + s * MDFIT_NMAPEVID;
        const EvidenceStats e = evidence_row(w, s_w, S, sw.shift, sw.total, K, sw.khat, sw.n_inf, tau, mask, row);
        if (lane == 0) {
          s_ev[0][s] = e.log_z;
          s_ev[1][s] = e.se;
          if constexpr (kAdapt) {
            row[kRound] = (double)sw.best;
            if (sw.best > 0) row[kFlags] += (double)mapadapt::kAdaptedBit;
          }
        }
        kmax = fmax(kmax, sw.khat);
        emin = fmin(emin, e.ess);
        all_rel = all_rel && sw.khat <= tau;
      }
    } else if (dr != nullptr) {
      nan_fill(dr, (int64_t)S * 6);
    }
    if constexpr (kAdapt)
      if (!ok && pmd) adapt_row_nan(adapt, t, arow);
    if (!ok) {
      all_ok = false;
      if (lane == 0) {
        invalid_row(rec + s * MDFIT_NMAPEVID, mask);
        s_ev[0][s] = NAN;
        s_ev[1][s] = NAN;
      }
    }
    __syncthreads();  // (the next sub-fit overwrites s_w)
  }
  if (lane == 0)
    compare_row(s_ev[0], s_ev[1], kmax > -INFINITY ? kmax : NAN, emin < INFINITY ? emin : NAN, all_ok, all_rel,
                rec + MDFIT_NSUBFIT * MDFIT_NMAPEVID);
}

// mdfit_log_mean_weight: one wave per series lw[row][0..S)
#ifndef MDFIT_NO_HELPER_KERNELS
__global__ __launch_bounds__(64) void log_mean_weight_kernel(const double* __restrict__ lw, int64_t n_series, int S,
                                                             double* __restrict__ logz, double* __restrict__ se,
                                                             double* __restrict__ khat) {
  extern __shared__ double s_w[];
  const int64_t row = blockIdx.x;
  if (row >= n_series) return;
  for (int x = threadIdx.x; x < S; x += 64) s_w[x] = lw[row * (int64_t)S + x];
  double k, ninf, c, tot;
  const bool ok = mappsis::psis_weights_level(PsisWave{}, s_w, S, k, ninf, c, tot);
  EvidenceStats e{NAN, NAN, NAN, NAN};
  if (ok) e = evidence_stats(PsisWave{}, s_w, S, c, tot, 0.0);  // (wave-uniform)
  if (threadIdx.x == 0) {
    logz[row] = e.log_z;
    se[row] = e.se;
    khat[row] = ok ? k : NAN;
  }
}
#endif  // MDFIT_NO_HELPER_KERNELS

}  // namespace mdfit::mapevid
#endif  // __HIPCC__
