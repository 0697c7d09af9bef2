// mdfit_nutsloo.h — MDFIT-LOO v1: Pareto-smoothed importance-
// sampling leave-one-out of one point's pointwise log-likelihood series (Vehtari,
// Gelman & Gabry 2017; Vehtari et al. 2024; the generalised Pareto fit of Zhang &
// Stephens 2009 with loo's priors), the per-sub-fit record built from the
// points' results, and the n_sigma comparison of two looic columns.
//
// The arithmetic is written once over a `lanes` policy, as mdfit_nutssumm.h:
// the loo kernel (mdfit_nuts.hip) runs it with the 64 lanes of a wave and the
// series in LDS; a plain C++ program (g++, no HIP) runs it with the one-lane
// policy below (tests/nutsloo_host_main.cpp).  Every sum is a per-lane strided
// partial sum in ascending index followed by the policy's cross-lane reduction,
// whose result every lane holds: every decision taken from one is uniform over
// the lanes, and a result depends on the policy alone, not on the grid.
// log, exp, log1p and expm1 are the platform's double-precision ones (the
// device library's on the GPU, libm's on the host).
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>

#include "mdfit_nutssumm.h"

namespace mdfit::nutsloo {

// record layout (MDFIT_NNUTSLOO = 8 doubles per row)
constexpr int kElpd = 0, kPLoo = 1, kElpdSe = 2, kKhatMax = 3, kKhatArgmax = 4, kNBad = 5, kLppd = 6, kFlags = 7;
// row 6, the comparisons
constexpr int kNSigma = 0, kNSigmaForward = 1, kNSigmaReverse = 2, kAsymmetry = 3, kAllKhatMax = 4, kAllNBad = 5;
constexpr double kValid = 1.0;  // flags bit 0
// S <= 4096: the tail holds M <= 192 draws and the grid m <= 43 points
constexpr int kMaxTail = 192, kMaxGrid = 43, kGridBuf = 96;

using nutssumm::ns_inf;
using nutssumm::ns_nan;
using nutssumm::sort_len;

// the one-lane policy: sequential sums in index order
struct OneLane : nutssumm::OneLane {
  MDFIT_NS_FN double max(double v) const { return v; }
};

// the work buffer's length for S draws: the sort buffer, the tail, the grid
MDFIT_NS_FN int work_len(int S) { return sort_len(S) + kMaxTail + kGridBuf; }

// floor(sqrt(n)), n >= 0
MDFIT_NS_FN int isqrt_floor(int n) {
  int q = (int)std::sqrt((double)n);
  while (q * q > n) --q;
  while ((q + 1) * (q + 1) <= n) ++q;
  return q;
}

// M = min(floor(S / 5), ceil(3 sqrt(S))), in integers
MDFIT_NS_FN int tail_len(int S) {
  const int f = isqrt_floor(9 * S);
  const int c = f * f == 9 * S ? f : f + 1;
  return S / 5 < c ? S / 5 : c;
}

// the k-hat above which a point counts as bad: min(1 - 1 / log10(S), 0.7)
inline double khat_threshold(int S) {
  const double t = 1.0 - 1.0 / std::log10((double)S);
  return t < 0.7 ? t : 0.7;
}

// One point.  buf holds work_len(S) doubles shared by the policy's lanes; on
// entry buf[t] = r_t = -l_t for t < S, each written by the lane t mod nlanes
// (no barrier of the caller's needed).  Every lane of the policy calls it and
// gets the same elpd and khat.  A series with a value that is not finite gives
// NaN for both.  On return the buffer may be rewritten at once.
template <class L>
MDFIT_NS_FN void psis_point(const L& w, double* buf, int S, double& elpd, double& khat) {
  const int lane = w.lane(), nl = w.nlanes();
  double* xs = buf + sort_len(S);
  double* g = xs + kMaxTail;
  // 1. r~ = r - max r, ascending
  double bad = 0.0, c = -ns_inf();
  for (int t = lane; t < S; t += nl) {
    const double v = buf[t];
    if (!std::isfinite(v)) bad = 1.0;
    c = std::fmax(c, v);
  }
  if (w.sum(bad) > 0.0) {  // (before the sort: the network orders finite values)
    elpd = khat = ns_nan();
    return;
  }
  c = w.max(c);
  for (int t = lane; t < S; t += nl) buf[t] -= c;
  w.sort(buf, S);
  // 2. the tail: the top M by rank, its cutoff the value below it
  const int M = tail_len(S);
  const int T0 = S - M;
  double eu = 0.0, sigma = 0.0;
  bool smooth = false;
  khat = ns_inf();  // 3. M < 5: no fit, no smoothing
  if (M >= 5) {
    eu = std::exp(buf[T0 - 1]);
    for (int j = lane; j < M; j += nl) {
      const double x = std::exp(buf[T0 + j]) - eu;
      xs[j] = x > 0.0 ? x : 0.0;  // (>= 0 by the order of r~; an exp that is monotone only to its last bit)
    }
    w.sync();
    const double xmax = xs[M - 1], xstar = xs[(M + 2) / 4 - 1];  // floor(M / 4 + 0.5) - 1
    if (xmax == 0.0) {
      khat = 0.0;  // a constant tail: uniform weights, nothing to diagnose
    } else if (xstar > 0.0) {
      // 4. Zhang & Stephens: the profile likelihood on a grid of theta, one lane per grid point
      const int m = 30 + isqrt_floor(M);
      for (int j = lane; j < m; j += nl) {
        const double theta = 1.0 / xmax + (1.0 - std::sqrt((double)m / ((double)j + 0.5))) / (3.0 * xstar);
        double kap = 0.0;
        for (int t = 0; t < M; ++t) kap += std::log1p(-theta * xs[t]);
        kap /= M;
        g[j] = theta;
        g[kMaxGrid + j] = M * (std::log(-theta / kap) - kap - 1.0);
      }
      w.sync();
      double part = 0.0;
      for (int j = lane; j < m; j += nl) {
        const double Lj = g[kMaxGrid + j];
        double s = 0.0;
        for (int i = 0; i < m; ++i) s += std::exp(g[kMaxGrid + i] - Lj);
        part += (1.0 / s) * g[j];
      }
      const double theta_hat = w.sum(part);
      part = 0.0;
      for (int t = lane; t < M; t += nl) part += std::log1p(-theta_hat * xs[t]);
      const double kap_hat = w.sum(part) / M;
      sigma = -kap_hat / theta_hat;
      khat = (M * kap_hat + 5.0) / (M + 10.0);
      smooth = std::isfinite(khat);
    }
    w.sync();  // (every lane has read the excesses; the smoothed tail overwrites them)
  }
  // 5. the tail's log weights replaced by the fitted distribution's quantiles, capped at 0
  if (smooth) {
    const bool tiny = std::fabs(khat) < 30.0 * std::numeric_limits<double>::epsilon();
    for (int j = lane; j < M; j += nl) {
      const double l1 = std::log1p(-((double)j + 0.5) / M);
      const double q = tiny ? -sigma * l1 : sigma * std::expm1(-khat * l1) / khat;
      const double wt = std::log(q + eu);
      xs[j] = wt < 0.0 ? wt : 0.0;
    }
    w.sync();
  }
  // 6. elpd = log sum exp(w~ - r~) - log sum exp(w~) - c, each sum shifted by its maximum
  double amax = -ns_inf(), bmax = -ns_inf();
  for (int j = lane; j < S; j += nl) {
    const double rt = buf[j], wt = (smooth && j >= T0) ? xs[j - T0] : rt;
    amax = std::fmax(amax, wt - rt);
    bmax = std::fmax(bmax, wt);
  }
  amax = w.max(amax);
  bmax = w.max(bmax);
  double sa = 0.0, sb = 0.0;
  for (int j = lane; j < S; j += nl) {
    const double rt = buf[j], wt = (smooth && j >= T0) ? xs[j - T0] : rt;
    sa += std::exp((wt - rt) - amax);
    sb += std::exp(wt - bmax);
  }
  sa = w.sum(sa);
  sb = w.sum(sb);
  elpd = (amax + std::log(sa)) - (bmax + std::log(sb)) - c;
  w.sync();  // (every lane has read buf and xs)
}

// all-NaN record with flags 0
MDFIT_NS_FN void invalid_row(double* rec) {
  for (int k = 0; k < kFlags; ++k) rec[k] = ns_nan();
  rec[kFlags] = 0.0;
}

// One sub-fit's record from its n points' elpd e[], lppd l[] and k-hat k[]
// (shared by the lanes, written behind a barrier); the first point is column
// col0.  Every lane calls it; lane 0 writes rec.  Returns k-hat's maximum and
// the bad count to every lane.
template <class L>
MDFIT_NS_FN void row_stats(const L& w, const double* e, const double* l, const double* k, int n, int col0, double tau,
                           double* rec, double& kmax_out, double& nbad_out) {
  const int lane = w.lane(), nl = w.nlanes();
  double se = 0.0, sl = 0.0, sp = 0.0, nb = 0.0, km = -ns_inf();
  for (int p = lane; p < n; p += nl) {
    se += e[p];
    sl += l[p];
    sp += l[p] - e[p];
    if (k[p] > tau) nb += 1.0;
    km = std::fmax(km, k[p]);
  }
  se = w.sum(se);
  sl = w.sum(sl);
  sp = w.sum(sp);
  nb = w.sum(nb);
  km = w.max(km);
  const double mean = se / n;
  double sv = 0.0, arg = -(double)nutssumm::kNoIndex;
  for (int p = lane; p < n; p += nl) {
    sv += (e[p] - mean) * (e[p] - mean);
    if (k[p] == km) arg = std::fmax(arg, -(double)(col0 + p));  // the lowest column among ties
  }
  sv = w.sum(sv) / n;
  arg = -w.max(arg);
  if (lane == 0) {
    rec[kElpd] = se;
    rec[kPLoo] = sp;
    rec[kElpdSe] = std::sqrt(n * sv);
    rec[kKhatMax] = km;
    rec[kKhatArgmax] = arg;
    rec[kNBad] = nb;
    rec[kLppd] = sl;
    rec[kFlags] = kValid;
  }
  kmax_out = km;
  nbad_out = nb;
}

// (sum b - sum a) / sqrt(n var(a - b)), var with ddof 0: the reference's
// n_sigma of a PMD column a against a null column b (fits.py:194-227)
template <class L>
MDFIT_NS_FN double n_sigma(const L& w, const double* a, const double* b, int n) {
  const int lane = w.lane(), nl = w.nlanes();
  double sd = 0.0, sa = 0.0, sb = 0.0;
  for (int p = lane; p < n; p += nl) {
    sd += a[p] - b[p];
    sa += a[p];
    sb += b[p];
  }
  const double md = w.sum(sd) / n;
  double sv = 0.0;
  for (int p = lane; p < n; p += nl) sv += ((a[p] - b[p]) - md) * ((a[p] - b[p]) - md);
  const double var = w.sum(sv) / n;
  return (w.sum(sb) - w.sum(sa)) / std::sqrt(n * var);
}

// Host form: work holds work_len(S) doubles, work[t] = -l_t on entry.
inline void psis_point_host(double* work, int S, double* elpd, double* khat) {
  psis_point(OneLane{}, work, S, *elpd, *khat);
}

}  // namespace mdfit::nutsloo
