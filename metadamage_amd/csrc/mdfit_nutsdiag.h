// mdfit_nutsdiag.h — MDFIT-DIAG v1: effective sample size,
// split R-hat and Monte Carlo standard error of one chain's series, the
// single-chain case of the published algorithms behind numpyro's
// effective_sample_size / split_gelman_rubin (Geyer's initial monotone
// sequence; Gelman et al., BDA3 §11.4-11.5), restated.
//
// The per-series arithmetic is written once over a `lanes` policy: the diag
// kernel (mdfit_nuts.hip) runs it with the 64 lanes of a wave over the sample
// index t and the centred series in LDS; a plain C++ program (g++, no HIP)
// runs it with the one-lane policy below (tests/nutsdiag_host_main.cpp).  Every
// sum is a per-lane strided partial sum followed by the policy's cross-lane
// reduction, so a record depends on the policy alone, not on the grid.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/mdfit.h"

#if defined(__HIPCC__)
#define MDFIT_ND_FN __host__ __device__ __forceinline__
#else
#define MDFIT_ND_FN inline
#endif

namespace mdfit::nutsdiag {

constexpr int kNSeries = 5;  // q, A, c, phi, D_max
// record layout (MDFIT_NNUTSDIAG = 12 doubles per sub-fit)
constexpr int kEss = 0, kRhat = 5, kMcse = 10, kFlags = 11;
constexpr double kValid = 1.0;  // flags bit 0

struct SeriesStats {
  double ess, rhat, mcse;
};

// the one-lane policy: sequential sums in index order
struct OneLane {
  MDFIT_ND_FN int lane() const { return 0; }
  MDFIT_ND_FN int nlanes() const { return 1; }
  MDFIT_ND_FN double sum(double v) const { return v; }
  MDFIT_ND_FN void sum2(double& a, double& b) const { (void)a, (void)b; }
  MDFIT_ND_FN void sync() const {}
};

MDFIT_ND_FN double nd_nan() { return std::nan(""); }

// Statistics of the series d[0..S) (raw draws on entry; overwritten with the
// centred series), S in [2, 4096].  Every lane of the policy calls it with the
// same arguments and gets the same result.
template <class L>
MDFIT_ND_FN SeriesStats series_stats(const L& w, double* d, int S) {
  SeriesStats r;
  r.ess = r.rhat = r.mcse = nd_nan();
  const int lane = w.lane(), nl = w.nlanes();
  // centred about the first draw, then about the mean of that: d_t = (x_t -
  // x_0) - mean(x - x_0).  Equal to x_t - mean(x) in exact arithmetic; a
  // constant series gives d = 0, so gamma_0 == 0, exactly, and a large common
  // offset cancels in x_t - x_0 before anything is rounded to its magnitude
  const double x0 = d[0];
  double s = 0.0;
  for (int t = lane; t < S; t += nl) s += d[t] - x0;
  const double mbar = w.sum(s) / S;
  w.sync();  // (every lane has read d[0])
  // centred series, gamma_0 and the halves' sums
  const int h = S / 2;
  double g0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int t = lane; t < S; t += nl) {
    const double v = (d[t] - x0) - mbar;
    d[t] = v;
    g0 = std::fma(v, v, g0);
    s1 += t < h ? v : 0.0;
    s2 += t >= S - h ? v : 0.0;
  }
  w.sync();
  g0 = w.sum(g0) / S;
  if (!(g0 > 0.0)) return r;  // constant (or non-finite) series: NaN
  // split R-hat: halves d[0:h) and d[S-h:S)
  w.sum2(s1, s2);
  const double mu1 = s1 / h, mu2 = s2 / h;
  double q1 = 0.0, q2 = 0.0;
  for (int t = lane; t < S; t += nl) {
    const double v = d[t];
    const double e1 = v - mu1, e2 = v - mu2;
    q1 = std::fma(t < h ? e1 : 0.0, e1, q1);
    q2 = std::fma(t >= S - h ? e2 : 0.0, e2, q2);
  }
  w.sum2(q1, q2);
  if (h >= 2) {
    const double W = 0.5 * (q1 / (h - 1) + q2 / (h - 1));
    const double dm = mu1 - mu2;
    const double B = 0.5 * dm * dm;  // variance (ddof 1) of the two half means
    if (W > 0.0) r.rhat = std::sqrt((W * (double)(h - 1) / (double)h + B) / W);
  }
  // Geyer's initial monotone sequence over lag pairs (2j, 2j + 1), stopped at
  // the first P_j <= 0: nothing after it contributes
  const double inv = 1.0 / (S - 1);
  double tau_sum = 0.0, prev = 0.0;
  for (int j = 0; j < h; ++j) {
    const int k0 = 2 * j, k1 = k0 + 1;
    double a0 = 0.0, a1 = 0.0;
    for (int t = lane; t < S - k0; t += nl) {
      const double v = d[t];
      a0 = std::fma(v, d[t + k0], a0);
      const int u = t + k1;
      a1 = std::fma(v, u < S ? d[u] : 0.0, a1);
    }
    w.sum2(a0, a1);
    const double rho0 = j == 0 ? 1.0 : (a0 / S) / g0 - inv;
    const double rho1 = (a1 / S) / g0 - inv;
    double P = rho0 + rho1;
    if (j > 0) {
      P = P > 0.0 ? P : 0.0;
      P = P < prev ? P : prev;
    }
    if (!(P > 0.0)) {
      if (j == 0) tau_sum = P;  // P_0 is kept as it is
      break;
    }
    tau_sum += P;
    prev = P;
  }
  const double tau = -1.0 + 2.0 * tau_sum;
  const double floor_tau = 1.0 / std::log10((double)S);  // ess <= S log10 S (Stan's cap)
  r.ess = S / (tau > floor_tau ? tau : floor_tau);
  r.mcse = std::sqrt(g0 * (double)S / (double)(S - 1) / r.ess);
  return r;
}

// all-NaN record with flags 0
MDFIT_ND_FN void invalid_row(double* rec) {
  for (int k = 0; k < kFlags; ++k) rec[k] = nd_nan();
  rec[kFlags] = 0.0;
}

// Host form of one sub-fit's record from its draws x[S][4] = (q, A, c, phi):
// pmd selects D_max = A + c (else q); work holds S doubles.
inline void diag_row_host(const double* x, int S, bool pmd, double chain_status, double* work, double* rec) {
  bool ok = chain_status == 0.0;
  for (int i = 0; i < 4 * S && ok; ++i) ok = std::isfinite(x[i]);
  if (!ok) {
    invalid_row(rec);
    return;
  }
  const OneLane w;
  for (int s = 0; s < kNSeries; ++s) {
    for (int t = 0; t < S; ++t)
      work[t] = s < 4 ? x[4 * t + s] : (pmd ? x[4 * t + 1] + x[4 * t + 2] : x[4 * t]);
    const SeriesStats r = series_stats(w, work, S);
    rec[kEss + s] = r.ess;
    rec[kRhat + s] = r.rhat;
    if (s == 4) rec[kMcse] = r.mcse;
  }
  rec[kFlags] = kValid;
}

}  // namespace mdfit::nutsdiag
