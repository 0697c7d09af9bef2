// mdfit_mapadapt.h — MDFIT-ADAPT v1 (mdfit_map_psis_adapt, mdfit_map_waic_adapt,
// DESIGN.md §3.12), steps 2-4: the Student-t proposal of a PMD sub-fit refitted
// to the smoothed weights of the draws it produced (importance-weighted moment
// matching, Paananen et al. 2021).  From the normalised weights w and the draws
// u = (logit q, logit A, c, log delta) come the weighted mean m and covariance
// C of the free coordinates' residuals rho_j = u_j - K_j c_s (K the shift of
// mdfit_mappsis.h's proposal, zero when c is free), the Jacobi scale d_j =
// sqrt(C_jj), the upper-triangular factor F of C_jm / (d_j d_m) = (F F')_jm and,
// with c held on 0, the exponential's new rate 1 / sum w c_s.
//
// Written once over a `lanes` policy, as mdfit_mappsis.h: a plain C++ program
// (g++, no HIP) runs it with the one-lane policy (tests/adapt_host_main.cpp).
// This header has no device part.  What runs it with the 64 lanes of a wave
// needs the core's wave policy and draw and lives in mdfit_mapis.h: StreamU and
// next_proposal inside the rounds of subfit_weights, and mdfit_adapt_proposal's
// one-wave kernel, mapadapt::adapt_proposal_kernel, at that header's end.  Every sum is a per-lane
// strided partial sum in ascending draw index followed by the policy's
// cross-lane reduction.
#pragma once

#include <cmath>

#include "mdfit_nutsloo.h"

namespace mdfit::mapadapt {

constexpr int kMaxRounds = 4;
constexpr double kPivMin = 1e-8;    // kLaplacePivMin's role: a pivot of the scaled covariance at or below it stops
constexpr unsigned kAdaptedBit = 64u;  // flags bit 6 of the psis and waic records: the best round is > 0
// the adapt record (MDFIT_NMAPADAPT = 4 doubles per PMD row)
constexpr int kKhat0 = 0, kEss0 = 1, kBestRound = 2, kRoundsTried = 3;

using nutsloo::OneLane;

// the refitted proposal: centre m (the residuals'), scale d, factor F[j][p]
// (p >= j; held coordinates: the identity's rows and columns, d = 1, m = 0),
// the held c's exponential rate gc (0 when c is free)
struct Refit {
  double m[4], d[4], F[4][4], gc;
};

// 1 / sum w^2 of normalised weights, psis_estimates' arithmetic
template <class L>
MDFIT_NS_FN double weights_ess(const L& w, const double* wt, int S) {
  const int lane = w.lane(), nl = w.nlanes();
  double s2 = 0.0;
  for (int t = lane; t < S; t += nl) {
    const double wi = wt[t];
    s2 += wi * wi;
  }
  s2 = w.sum(s2);
  return 1.0 / s2;
}

// Steps 2-4 of one round.  wt[S]: the best round's normalised weights (shared
// by the lanes, written behind a barrier); draw(t, u) gives u[4] of draw t, the
// same values at every call -- a draw of weight 0 takes no part, its values may
// be anything.  mask: the free coordinates (bit j); cheld: c is held on 0 and
// drawn from the exponential, c_s = u[2]; K[4]: the centre's shift.  Every lane
// calls it and gets the same r and return value.  False -- the round stops, r
// unspecified -- when some C_jj is not > 0, a pivot is <= kPivMin, c-bar is not
// > 0 or anything is not finite.
template <class L, class G>
MDFIT_NS_FN bool refit(const L& w, const double* wt, int S, const G& draw, unsigned mask, bool cheld, const double* K,
                       Refit& r) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int lane = w.lane(), nl = w.nlanes();
  bool fr[4];
  for (int j = 0; j < 4; ++j) fr[j] = ((mask >> j) & 1u) != 0u;
  // (K is read where it is used: four fewer doubles live across the draws)
  // 2. the weighted moments: the mean, then the covariance about it
  double m[4] = {0.0, 0.0, 0.0, 0.0}, cb = 0.0;
  for (int t = lane; t < S; t += nl) {
    const double wi = wt[t];
    double u[4];
    draw(t, u);
    if (wi > 0.0) {
      const double cs = cheld ? u[2] : 0.0;
      for (int j = 0; j < 4; ++j) m[j] += wi * (cheld ? u[j] - K[j] * cs : u[j]);
      cb += wi * cs;
    }
  }
  for (int j = 0; j < 4; ++j) m[j] = w.sum(m[j]);
  cb = w.sum(cb);
  double C[4][4];
  for (int j = 0; j < 4; ++j)
    for (int p = 0; p < 4; ++p) C[j][p] = 0.0;
  for (int t = lane; t < S; t += nl) {
    const double wi = wt[t];
    double u[4];
    draw(t, u);
    if (wi > 0.0) {
      const double cs = cheld ? u[2] : 0.0;
      double e[4];
      for (int j = 0; j < 4; ++j) e[j] = (cheld ? u[j] - K[j] * cs : u[j]) - m[j];
      for (int j = 0; j < 4; ++j)
        for (int p = j; p < 4; ++p) C[j][p] += wi * (e[j] * e[p]);
    }
  }
  for (int j = 0; j < 4; ++j)
    for (int p = j; p < 4; ++p) C[j][p] = w.sum(C[j][p]);
  // 3. the Jacobi scale and the factor, from the last free coordinate backwards
  bool ok = true;
  for (int j = 0; j < 4; ++j) {
    if (fr[j] && !(C[j][j] > 0.0)) ok = false;
    r.d[j] = (fr[j] && C[j][j] > 0.0) ? std::sqrt(C[j][j]) : 1.0;
    r.m[j] = fr[j] ? m[j] : 0.0;
  }
  for (int j = 0; j < 4; ++j)
    for (int p = 0; p < 4; ++p) r.F[j][p] = 0.0;
  for (int j = 3; j >= 0; --j) {
    if (!fr[j]) {
      r.F[j][j] = 1.0;
      continue;
    }
    // the pivot of column j (row j's entries behind it are complete), then the column above it
    double s = C[j][j] / (r.d[j] * r.d[j]);
    for (int p = j + 1; p < 4; ++p) s -= r.F[j][p] * r.F[j][p];
    if (!(s > kPivMin)) {
      ok = false;
      s = 1.0;
    }
    r.F[j][j] = std::sqrt(s);
    for (int i = j - 1; i >= 0; --i) {
      if (!fr[i]) continue;
      double v = C[i][j] / (r.d[i] * r.d[j]);
      for (int p = j + 1; p < 4; ++p) v -= r.F[i][p] * r.F[j][p];
      r.F[i][j] = v / r.F[j][j];
    }
  }
  r.gc = 0.0;
  if (cheld) {
    if (!(cb > 0.0)) ok = false;
    r.gc = 1.0 / cb;
    if (!std::isfinite(r.gc)) ok = false;
  }
  for (int j = 0; j < 4; ++j) {
    if (!std::isfinite(r.m[j]) || !std::isfinite(r.d[j])) ok = false;
    for (int p = 0; p < 4; ++p)
      if (!std::isfinite(r.F[j][p])) ok = false;
  }
  return ok;
}

// the draws of the host form: u[S][4]
struct ArrayDraws {
  const double* u;
  MDFIT_NS_FN void operator()(int t, double o[4]) const {
    for (int k = 0; k < 4; ++k) o[k] = u[4 * t + k];
  }
};

inline bool refit_host(const double* wt, int S, const double* u, unsigned mask, bool cheld, const double* K,
                       Refit* r) {
  return refit(OneLane{}, wt, S, ArrayDraws{u}, mask, cheld, K, *r);
}

}  // namespace mdfit::mapadapt

// (the proposal that is refitted and the bounds on S; behind the definitions above, which the HIP part of that
// header stands on through mdfit_mapis.h)
#include "mdfit_mappsis.h"
