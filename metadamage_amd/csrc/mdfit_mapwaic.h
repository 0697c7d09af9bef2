// mdfit_mapwaic.h — MDFIT-WAIC v1 (mdfit_map_waic): the
// reference's WAIC comparisons (n_sigma, n_sigma_forward, n_sigma_reverse,
// asymmetry; fits.py:147-227) of a MAP fit from importance-weighted draws.  The
// three PMD sub-fits are importance-sampled exactly as mdfit_mappsis.h does it
// (the same functions, mdfit_mapis.h, so the same bits); the three null sub-fits get a
// bivariate Student-t (nu = 4) proposal on (logit q, log delta) from one
// evaluation of the fit kernel's null objective at their mode.  Per sub-fit the
// Pareto-smoothed, normalised weights w_s and the pointwise log-pmf l_si give
//   lppd_i = log sum_s w_s exp(l_si),  p_i = sum_s w_s (l_si - sum_s w_s l_si)^2,
//   waic_i = -2 (lppd_i - p_i),
// and row 6 is nutsloo::n_sigma on those columns.
//
// The accumulation (waic_points) and the row record (waic_row) are written once
// over a `lanes` policy, as mdfit_mappsis.h: the kernel below runs them with
// the 64 lanes of a wave and the tile in LDS; a plain C++ program (g++, no HIP)
// runs them with the one-lane policy (tests/mapwaic_host_main.cpp).  A point's
// accumulators run over the draws in ascending index whatever the policy;
// the row's sums are per-lane strided partials plus the policy's reduction.
#pragma once

#include <cmath>
#include <cstdint>

#include "mdfit_mappsis.h"

namespace mdfit::mapwaic {

// record layout (MDFIT_NMAPWAIC = 8 doubles per row); rows 0..5 the sub-fits
constexpr int kElpd = 0, kPWaic = 1, kLppd = 2, kKhat = 3, kEss = 4, kNInfeasible = 5, kPWaicMax = 6, kFlags = 7;
// row 6, the comparisons
constexpr int kNSigma = 0, kNSigmaForward = 1, kNSigmaReverse = 2, kAsymmetry = 3, kKhatMax = 4, kEssMin = 5;
constexpr unsigned kValidBit = 1u, kReliableBit = 2u;  // flags; rows 0..5: bits 2..5 coordinate (q, A, c, phi) free
constexpr int kMaxPts = 30;    // the points of an all-position sub-fit
constexpr int kTileCols = 15;  // the columns of one tile: a forward or reverse half
// per-point accumulators acc[kNPtAcc][kMaxPts]: the running maximum of l, sum w
// exp(l - max), sum w (l - l0), sum w (l - l0)^2, the minimum of l
constexpr int kAMax = 0, kASe = 1, kAS1 = 2, kAS2 = 3, kAMin = 4, kNPtAcc = 5;

using mappsis::OneLane;
using nutssumm::ns_inf;
using nutssumm::ns_nan;

// the tile's length in doubles for a policy of nl lanes: kTileCols columns of
// nl draws, the leading dimension padded by one (LDS banks)
MDFIT_NS_FN int tile_len(int nl) { return kTileCols * (nl + 1); }
// the kernel's dynamic LDS in doubles: psis_weights' work buffer, whose part
// behind the S weights the tile and the accumulators overlay afterwards
MDFIT_NS_FN int lds_len(int S) {
  const int a = mappsis::work_len(S), b = S + tile_len(64) + kNPtAcc * kMaxPts;
  return a > b ? a : b;
}

// Pointwise lppd_i and p_i of one sub-fit's n <= kMaxPts points from the
// normalised weights wt[S] (shared by the lanes, written behind a barrier).
// src.draw(t) prepares draw t and src.fill(d, c0, nc, dst, ld) leaves its
// log-pmf at the points c0 .. c0 + nc - 1 in dst[c * ld], the same values at
// every call; a draw of weight 0 is never asked for.  l0[n]: a finite shift
// per point (the log-pmf at the mode) that keeps sum w (l - l0)^2 - (sum w (l -
// l0))^2 from cancelling.  tile: tile_len(nlanes) doubles, acc: kNPtAcc * kMaxPts
// doubles, both shared by the lanes.  Every lane calls it; on return lppd[i]
// and p[i], i < n, are written behind a barrier.  A point whose l is the same
// in every draw of positive weight has lppd_i = l and p_i = 0 exactly.
template <class L, class Src>
MDFIT_NS_FN void waic_points(const L& w, const double* wt, int S, int n, const Src& src, const double* l0,
                             double* tile, double* acc, double* lppd, double* p) {
  const int lane = w.lane(), nl = w.nlanes(), ld = nl + 1;
  for (int i = lane; i < n; i += nl) {
    acc[kAMax * kMaxPts + i] = -ns_inf();
    acc[kASe * kMaxPts + i] = 0.0;
    acc[kAS1 * kMaxPts + i] = 0.0;
    acc[kAS2 * kMaxPts + i] = 0.0;
    acc[kAMin * kMaxPts + i] = ns_inf();
  }
  w.sync();
  for (int base = 0; base < S; base += nl) {
    const int cnt = S - base < nl ? S - base : nl;
    const int t = base + lane;
    const bool mine = t < S && wt[t] > 0.0;
    decltype(src.draw(0)) d{};
    if (mine) d = src.draw(t);
    for (int c0 = 0; c0 < n; c0 += kTileCols) {
      const int nc = n - c0 < kTileCols ? n - c0 : kTileCols;
      if (mine) src.fill(d, c0, nc, tile + lane, ld);
      w.sync();
      for (int i = lane; i < nc; i += nl) {
        const int pt = c0 + i;
        double mx = acc[kAMax * kMaxPts + pt], se = acc[kASe * kMaxPts + pt], s1 = acc[kAS1 * kMaxPts + pt];
        double s2 = acc[kAS2 * kMaxPts + pt], mn = acc[kAMin * kMaxPts + pt];
        const double sh = l0[pt];
        for (int x = 0; x < cnt; ++x) {
          const double wi = wt[base + x];
          if (!(wi > 0.0)) continue;  // (the same for every lane)
          const double l = tile[i * ld + x];
          if (l > mx) {
            se = se * std::exp(mx - l) + wi;
            mx = l;
          } else {
            se += wi * std::exp(l - mx);
          }
          mn = std::fmin(mn, l);
          const double dl = l - sh;
          s1 += wi * dl;
          s2 += wi * (dl * dl);
        }
        acc[kAMax * kMaxPts + pt] = mx;
        acc[kASe * kMaxPts + pt] = se;
        acc[kAS1 * kMaxPts + pt] = s1;
        acc[kAS2 * kMaxPts + pt] = s2;
        acc[kAMin * kMaxPts + pt] = mn;
      }
      w.sync();
    }
  }
  for (int i = lane; i < n; i += nl) {
    const double mx = acc[kAMax * kMaxPts + i], mn = acc[kAMin * kMaxPts + i];
    const double s1 = acc[kAS1 * kMaxPts + i], s2 = acc[kAS2 * kMaxPts + i];
    const bool flat = mx == mn;
    const double v = s2 - s1 * s1;
    lppd[i] = flat ? mx : mx + std::log(acc[kASe * kMaxPts + i]);
    p[i] = flat ? 0.0 : (v > 0.0 ? v : 0.0);
  }
  w.sync();
}

// all-NaN record; flags: the free bits alone
MDFIT_NS_FN void invalid_row(double* rec, unsigned free_mask) {
  for (int k = 0; k < kFlags; ++k) rec[k] = ns_nan();
  rec[kFlags] = (double)((free_mask & 15u) << 2);
}

// One sub-fit's record from its n points' lppd[] and p[] and the weights
// wt[S] (shared by the lanes, written behind a barrier).  Every lane calls it
// and gets ess back; lane 0 writes rec.
template <class L>
MDFIT_NS_FN double waic_row(const L& w, const double* lppd, const double* p, int n, const double* wt, int S,
                            double khat, double n_inf, double tau, unsigned free_mask, double* rec) {
  const int lane = w.lane(), nl = w.nlanes();
  double se = 0.0, sp = 0.0, sl = 0.0, pm = -ns_inf();
  for (int i = lane; i < n; i += nl) {
    se += lppd[i] - p[i];
    sp += p[i];
    sl += lppd[i];
    pm = std::fmax(pm, p[i]);
  }
  se = w.sum(se);
  sp = w.sum(sp);
  sl = w.sum(sl);
  pm = w.max(pm);
  double s2 = 0.0;
  for (int t = lane; t < S; t += nl) {
    const double wi = wt[t];
    s2 += wi * wi;
  }
  s2 = w.sum(s2);
  const double ess = 1.0 / s2;
  if (lane == 0) {
    rec[kElpd] = se;
    rec[kPWaic] = sp;
    rec[kLppd] = sl;
    rec[kKhat] = khat;
    rec[kEss] = ess;
    rec[kNInfeasible] = n_inf;
    rec[kPWaicMax] = pm;
    rec[kFlags] = (double)(kValidBit | (khat <= tau ? kReliableBit : 0u) | ((free_mask & 15u) << 2));
  }
  return ess;
}

// the draws of the host form: the log-pmf l[S][n]
struct ArraySource {
  const double* l;
  int n;
  int draw(int t) const { return t; }
  void fill(int t, int c0, int nc, double* dst, int ld) const {
    for (int c = 0; c < nc; ++c) dst[c * ld] = l[(size_t)t * n + c0 + c];
  }
};

// Host form: lppd[n] and p[n] from weights wt[S], log-pmf l[S][n] and shifts l0[n].
inline void waic_points_host(const double* wt, int S, int n, const double* l, const double* l0, double* lppd,
                             double* p) {
  double tile[kTileCols * 2], acc[kNPtAcc * kMaxPts];
  waic_points(OneLane{}, wt, S, n, ArraySource{l, n}, l0, tile, acc, lppd, p);
}
inline double waic_row_host(const double* lppd, const double* p, int n, const double* wt, int S, double khat,
                            double n_inf, unsigned free_mask, double* rec) {
  return waic_row(OneLane{}, lppd, p, n, wt, S, khat, n_inf, mappsis::khat_threshold(S), free_mask, rec);
}

}  // namespace mdfit::mapwaic

#if defined(__HIPCC__)
#include "mdfit_mapis.h"  // (the importance sampler's device core)

namespace mdfit::mapwaic {

using namespace mapis;

// the kernel's draws for waic_points: regenerated from the stream; column lo +
// c of the counts in LDS is point c of the sub-fit
struct StreamSource {
  const double* P;
  Stream st;
  bool pmd;
  int lo;
  const double *s_y, *s_N;
  __device__ __forceinline__ DrawPt draw(int t) const { return draw_point(pmd, psis_draw(P, st, t)); }
  __device__ __forceinline__ void fill(const DrawPt& d, int c0, int nc, double* dst, int ld) const {
#pragma unroll 1
    for (int c = 0; c < nc; ++c) {
      const int col = lo + c0 + c;
      const int kk = col < kNHalf ? col : col - kNHalf;
      const double D = fma(d.A, powk(d.w, kk), d.c);
      dst[c * ld] = bb_logpmf(s_y[col], s_N[col], D, d.ph);
    }
  }
};

// One wave per taxon, its six sub-fits one after another in diagnostic-slot
// order.  Phases 1-3 are the core's (mdfit_mapis.h): proposals<true> and
// proposals<false>, then per sub-fit subfit_weights with the shift s_l0, the
// log-pmf at the centre of the proposal whose weights stand (with kAdapt,
// mdfit_map_waic_adapt, the PMD rows in the rounds of MDFIT-ADAPT v1, DESIGN.md
// §3.12; the null rows take one pass).  Phase 4 -- waic_points with the draws
// regenerated from the stream, 64 at a time through a tile of 15 columns that
// overlays the work buffer behind the weights (as the points' accumulators
// do), lane i < 15 walking point i's accumulators over the tile's draws in
// ascending order; then waic_row.  Row 6 is nutsloo::n_sigma on the waic_i
// columns, as nuts_loo_kernel's.  Dynamic LDS: lds_len(S) doubles (22,016 B at
// S = 1024, 11,048 B at S = 256); static: 4,448 B.  Reads y, N, out and status
// only.
template <bool kAdapt>
__global__ __launch_bounds__(64) void map_waic_kernel(const uint32_t* __restrict__ gy,
                                                      const uint32_t* __restrict__ gN,
                                                      const double* __restrict__ out,
                                                      const int32_t* __restrict__ status, int64_t n_taxa, int S,
                                                      uint64_t seed, int64_t index_base, double tau,
                                                      double* __restrict__ waic, double* __restrict__ pointwise,
                                                      double* __restrict__ draws, int adapt_rounds,
                                                      double* __restrict__ adapt) {
  extern __shared__ double s_w[];
  __shared__ double s_y[kLD], s_N[kLD];
  __shared__ double s_par[MDFIT_NSUBFIT][kNPar];
  __shared__ double s_l0[kMaxPts], s_pt[2][kMaxPts];    // the current sub-fit's shift, lppd_i and p_i
  __shared__ double s_col[MDFIT_NSUBFIT + 1][kMaxPts];  // waic_i; row 6: PMD-forward | PMD-reverse
  const int lane = threadIdx.x;
  const int64_t t = blockIdx.x;
  if (t >= n_taxa) return;
  double* rec = waic + t * (MDFIT_NSUBFIT + 1) * MDFIT_NMAPWAIC;
  double* pw = pointwise != nullptr ? pointwise + t * MDFIT_NSUBFIT * kMaxPts * 2 : nullptr;
  double* dr0 = draws != nullptr ? draws + t * MDFIT_NSUBFIT * (int64_t)S * 6 : nullptr;

  if (status[t] != MDFIT_OK) {  // wave-uniform: NaN statistics, flags 0
    if (lane < MDFIT_NSUBFIT + 1) invalid_row(rec + lane * MDFIT_NMAPWAIC, 0u);
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
  double* s_acc = tile + tile_len(64);
  double kmax = -INFINITY, emin = INFINITY;
  bool all_ok = true, all_rel = true;
  for (int s = 0; s < MDFIT_NSUBFIT; ++s) {
    const bool pmd = s == 0 || s == 2 || s == 3;
    const int lo = (s == 3 || s == 5) ? kNHalf : 0, hi = s < 2 ? kNPos : lo + kNHalf;
    const int n = hi - lo;
    const double* P = s_par[s];
    const unsigned mask = (unsigned)P[kPMask];
    double* dr = dr0 != nullptr ? dr0 + (int64_t)s * S * 6 : nullptr;
    bool ok = P[kPValid] != 0.0;  // (wave-uniform)
    const int arow = s == 0 ? 0 : s - 1;  // a PMD sub-fit's row of the adapt record
    if (ok) {
      const Stream st = subfit_stream(seed, gtaxon, s);
      const SubfitWeights sw = subfit_weights<kAdapt, true>(w, pmd, lo, hi, s_par[s], st, S, tau, adapt_rounds, s_y,
                                                            s_N, s_w, s_l0, dr);
      ok = sw.ok;
      const double khat = sw.khat, n_inf = sw.n_inf;
      const int best = sw.best;
      if constexpr (kAdapt)
        if (pmd) adapt_row(adapt, t, arow, sw);
      draws_weights(dr, s_w, S, ok);
      if (ok) {
        // ---- phase 4: the pointwise statistics, the row ----
        waic_points(w, s_w, S, n, StreamSource{P, st, pmd, lo, s_y, s_N}, s_l0, tile, s_acc, s_pt[0], s_pt[1]);
        const double ess = waic_row(w, s_pt[0], s_pt[1], n, s_w, S, khat, n_inf, tau, mask, rec + s * MDFIT_NMAPWAIC);
        if constexpr (kAdapt)
          if (best > 0 && lane == 0) rec[s * MDFIT_NMAPWAIC + kFlags] += (double)mapadapt::kAdaptedBit;
        kmax = fmax(kmax, khat);
        emin = fmin(emin, ess);
        all_rel = all_rel && khat <= tau;
        if (lane < n) {
          const double wv = -2.0 * (s_pt[0][lane] - s_pt[1][lane]);
          s_col[s][lo + lane] = wv;
          if (s == 2 || s == 3) s_col[MDFIT_NSUBFIT][lo + lane] = wv;
        }
      }
    } else if (dr != nullptr) {
      nan_fill(dr, (int64_t)S * 6);
    }
    if constexpr (kAdapt)
      if (!ok && pmd) adapt_row_nan(adapt, t, arow);
    if (!ok) {
      all_ok = false;
      if (lane == 0) invalid_row(rec + s * MDFIT_NMAPWAIC, mask);
    }
    if (pw != nullptr && lane < 2 * kMaxPts) {
      const int col = lane >> 1;
      const bool in = ok && col >= lo && col < hi;
      pw[(s * kMaxPts) * 2 + lane] = in ? s_pt[lane & 1][col - lo] : NAN;
    }
    __syncthreads();  // (the next sub-fit overwrites s_w, s_l0 and s_pt)
  }
  // row 6: fits.py:194-227 on waic_i (an invalid row's column is NaN: its comparisons are)
  const double ns = nutsloo::n_sigma(w, s_col[0], s_col[1], kNPos);
  const double nsf = nutsloo::n_sigma(w, s_col[2], s_col[4], kNHalf);
  const double nsr = nutsloo::n_sigma(w, s_col[3] + kNHalf, s_col[5] + kNHalf, kNHalf);
  const double asy = nutsloo::n_sigma(w, s_col[0], s_col[MDFIT_NSUBFIT], kNPos);
  if (lane == 0) {
    double* r6 = rec + MDFIT_NSUBFIT * MDFIT_NMAPWAIC;
    r6[kNSigma] = ns;
    r6[kNSigmaForward] = nsf;
    r6[kNSigmaReverse] = nsr;
    r6[kAsymmetry] = asy;
    r6[kKhatMax] = kmax > -INFINITY ? kmax : NAN;
    r6[kEssMin] = emin < INFINITY ? emin : NAN;
    r6[6] = 0.0;
    r6[kFlags] = (double)((all_ok ? kValidBit : 0u) | (all_ok && all_rel ? kReliableBit : 0u));
  }
}

}  // namespace mdfit::mapwaic
#endif  // __HIPCC__
