// mdfit_mappsis.h — MDFIT-PSIS v1 (mdfit_map_psis): an
// importance-sampled posterior around the MAP mode of each PMD sub-fit.  S
// draws from a Student-t (nu = 4) proposal built on the Laplace fit of
// mdfit_laplace.h are weighted by the density the sampling mode draws from,
// the weights are Pareto-smoothed (Vehtari et al. 2024, the tail rule and the
// generalised Pareto fit of mdfit_nutsloo.h), and the posterior means and
// standard deviations of q, A, c, phi and D_max come with the shape k-hat that
// says whether they can be trusted.
//
// The smoothing (psis_weights) and the estimates (psis_estimates) are written
// once over a `lanes` policy, as mdfit_nutsloo.h: the kernel below (whose draws,
// weights and rounds are the device core's, mdfit_mapis.h) runs them
// with the 64 lanes of a wave and the series in LDS; a plain C++ program (g++,
// no HIP) runs them with the one-lane policy (tests/mappsis_host_main.cpp).
// Every sum is a per-lane strided partial sum in ascending draw index followed
// by the policy's cross-lane reduction: a record depends on the policy alone,
// not on the grid.
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>

#include "mdfit_nutsloo.h"

namespace mdfit::mappsis {

// record layout (MDFIT_NMAPPSIS = 16 doubles per PMD sub-fit)
constexpr int kMean = 0, kStd = 5, kRhoAc = 10, kSignificance = 11, kKhat = 12, kEss = 13, kNInfeasible = 14,
              kFlags = 15;
constexpr unsigned kValidBit = 1u, kReliableBit = 2u;  // flags; bits 2..5: coordinate (q, A, c, phi) free
constexpr int kMinDraws = 25, kMaxDraws = 1024;
// S <= 1024: the tail holds M <= 96 draws and the grid m <= 39 points
constexpr int kMaxTail = 96, kMaxGrid = 48;
constexpr double kFloor = -800.0;  // an infeasible draw's rank value below the maximum: exp() of it is exactly 0
// one sub-fit's proposal, kNPar words in LDS: the centre u, the scale d, the
// factor M (psis_draw: draw_j = u_j + d_j sum_{p >= j} M[p][j] t_p), the centre's
// shift K with a held c, the held c's exponential rate, the free mask, valid,
// c held
constexpr int kPU = 0, kPD = 4, kPM = 8, kPK = 24, kPGc = 28, kPMask = 29, kPValid = 30, kPCHeld = 31, kNPar = 32;

using nutsloo::isqrt_floor;
using nutsloo::khat_threshold;
using nutsloo::tail_len;
using nutssumm::ns_inf;
using nutssumm::ns_nan;
using nutssumm::sort_len;

struct OneLane : nutsloo::OneLane {};

// the work buffer's length in doubles for S draws: the series, the sorted
// values, the tail's excesses, the grid, and the sorted draw indices (ints)
MDFIT_NS_FN int work_len(int S) { return S + sort_len(S) + kMaxTail + 2 * kMaxGrid + sort_len(S) / 2; }

// (value, draw index) ascending: the order of a stable sort by value
MDFIT_NS_FN bool pair_after(double va, int ia, double vb, int ib) { return va > vb || (va == vb && ia > ib); }

// Ascending bitonic sort of the pairs (v[p], ix[p]), p < S, by pair_after; v
// and ix hold sort_len(S) entries (the padding +inf ends beyond S - 1).
template <class L>
MDFIT_NS_FN void sort_pairs(const L& w, double* v, int* ix, int S) {
  const int lane = w.lane(), nl = w.nlanes();
  const int m = sort_len(S);
  for (int j = S + lane; j < m; j += nl) {
    v[j] = ns_inf();
    ix[j] = j;
  }
  w.sync();
  for (int k = 2; k <= m; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = lane; p < (m >> 1); p += nl) {
        const int x = ((p & ~(j - 1)) << 1) | (p & (j - 1)), y = x | j;
        const double a = v[x], b = v[y];
        const int ia = ix[x], ib = ix[y];
        const bool up = (x & k) == 0;
        if (pair_after(a, ia, b, ib) == up) {
          v[x] = b;
          v[y] = a;
          ix[x] = ib;
          ix[y] = ia;
        }
      }
      w.sync();
    }
  }
}

// Pareto-smoothed, normalised importance weights of one series.  buf holds
// work_len(S) doubles shared by the policy's lanes; on entry buf[t] = lw_t, the
// raw log-weight of draw t < S, each written by the lane t mod nlanes (no
// barrier of the caller's needed); -inf is an infeasible draw (weight 0).
// Every lane calls it and gets the same khat, n_inf and return value.  On a
// true return buf[t] is the weight of draw t, summing to 1.  False -- buf then
// unspecified, khat NaN -- when a value is NaN or +inf, or when the draw that
// sets the tail's cut-off is infeasible.  S in [kMinDraws, kMaxDraws].
// psis_weights_level is that routine; it also gives up the level that the
// normalisation drops (MDFIT-EVID v1, mdfit_mapevid.h): shift, the largest
// finite log-weight, and total, the sum of the smoothed weights exp(buf[t]) of
// step 6 before they are divided by it (an infeasible draw adds 0).  Both are
// unspecified on a false return.
template <class L>
MDFIT_NS_FN bool psis_weights_level(const L& w, double* buf, int S, double& khat, double& n_inf, double& shift,
                                    double& total) {
  const int lane = w.lane(), nl = w.nlanes();
  double* sv = buf + S;
  double* xs = sv + sort_len(S);
  double* g = xs + kMaxTail;
  int* si = reinterpret_cast<int*>(g + 2 * kMaxGrid);
  // 1. the largest log-weight; the infeasible draws
  double bad = 0.0, ninf = 0.0, c = -ns_inf();
  for (int t = lane; t < S; t += nl) {
    const double v = buf[t];
    if (v != v || v == ns_inf()) bad = 1.0;
    if (v == -ns_inf()) ninf += 1.0;
    else c = std::fmax(c, v);
  }
  bad = w.sum(bad);
  n_inf = w.sum(ninf);
  c = w.max(c);
  khat = ns_nan();
  shift = c;
  total = ns_nan();
  if (bad > 0.0 || !(c > -ns_inf())) return false;
  // 2. shifted by the maximum; the rank values (an infeasible draw: the floor), stably sorted
  for (int t = lane; t < S; t += nl) {
    const double v = buf[t];
    const bool inf = v == -ns_inf();
    const double r = inf ? v : v - c;
    buf[t] = r;
    sv[t] = inf ? kFloor : r;
    si[t] = t;
  }
  sort_pairs(w, sv, si, S);
  // 3. the tail: the top M by rank, its cut-off the value below it
  const int M = tail_len(S);  // >= 5: S >= 25
  const int T0 = S - M;
  if (buf[si[T0 - 1]] == -ns_inf()) return false;
  const double eu = std::exp(sv[T0 - 1]);
  for (int j = lane; j < M; j += nl) {
    const double x = std::exp(sv[T0 + j]) - eu;
    xs[j] = x > 0.0 ? x : 0.0;
  }
  w.sync();
  double sigma = 0.0;
  bool smooth = false;
  khat = ns_inf();
  const double xmax = xs[M - 1], xstar = xs[(M + 2) / 4 - 1];
  if (xmax == 0.0) {
    khat = 0.0;  // a constant tail: nothing to smooth or to diagnose
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
  w.sync();  // (every lane has read the excesses and the cut-off's draw)
  // 5. a draw of the tail takes the fitted quantile of its rank, capped at the largest raw weight
  if (smooth) {
    const bool tiny = std::fabs(khat) < 30.0 * std::numeric_limits<double>::epsilon();
    for (int j = lane; j < M; j += nl) {
      const double l1 = std::log1p(-((double)j + 0.5) / M);
      const double q = tiny ? -sigma * l1 : sigma * std::expm1(-khat * l1) / khat;
      const double wt = std::log(q + eu);
      buf[si[T0 + j]] = wt < 0.0 ? wt : 0.0;
    }
    w.sync();
  }
  // 6. normalised
  double part = 0.0;
  for (int t = lane; t < S; t += nl) part += std::exp(buf[t]);
  const double tot = w.sum(part);
  total = tot;
  for (int t = lane; t < S; t += nl) buf[t] = std::exp(buf[t]) / tot;
  w.sync();
  return true;
}
template <class L>
MDFIT_NS_FN bool psis_weights(const L& w, double* buf, int S, double& khat, double& n_inf) {
  double shift, total;
  return psis_weights_level(w, buf, S, khat, n_inf, shift, total);
}

// all-NaN record; flags: the free bits alone
MDFIT_NS_FN void invalid_row(double* rec, unsigned free_mask) {
  for (int k = 0; k < kFlags; ++k) rec[k] = ns_nan();
  rec[kFlags] = (double)((free_mask & 15u) << 2);
}

// One sub-fit's record from the normalised weights wt[S] (shared by the lanes,
// written behind a barrier) and the draws: draw(t, f) gives f[4] = (q, A, c,
// phi) of draw t, the same values at every call.  Every lane calls it; lane 0
// writes rec.
template <class L, class G>
MDFIT_NS_FN void psis_estimates(const L& w, const double* wt, int S, const G& draw, double khat, double n_inf,
                                double tau, unsigned free_mask, double* rec) {
  const int lane = w.lane(), nl = w.nlanes();
  double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, s2 = 0.0;
  for (int t = lane; t < S; t += nl) {
    const double wi = wt[t];
    double f[4];
    draw(t, f);
    const double D = f[1] + f[2];
    // (a weight of 0 takes no part: an infeasible draw's values may be anything)
    if (wi > 0.0) {
      for (int k = 0; k < 4; ++k) m[k] += wi * f[k];
      m[4] += wi * D;
    }
    s2 += wi * wi;
  }
  for (int k = 0; k < 5; ++k) m[k] = w.sum(m[k]);
  s2 = w.sum(s2);
  double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, cAc = 0.0;
  for (int t = lane; t < S; t += nl) {
    const double wi = wt[t];
    double f[4];
    draw(t, f);
    if (wi > 0.0) {
      const double d[5] = {f[0] - m[0], f[1] - m[1], f[2] - m[2], f[3] - m[3], (f[1] + f[2]) - m[4]};
      for (int k = 0; k < 5; ++k) v[k] += wi * (d[k] * d[k]);
      cAc += wi * (d[1] * d[2]);
    }
  }
  for (int k = 0; k < 5; ++k) v[k] = w.sum(v[k]);
  cAc = w.sum(cAc);
  if (lane == 0) {
    for (int k = 0; k < 5; ++k) {
      rec[kMean + k] = m[k];
      rec[kStd + k] = std::sqrt(v[k]);
    }
    rec[kRhoAc] = (v[1] > 0.0 && v[2] > 0.0) ? cAc / std::sqrt(v[1] * v[2]) : ns_nan();
    const double sd = std::sqrt(v[4]);
    rec[kSignificance] = sd > 0.0 ? m[4] / sd : ns_nan();
    rec[kKhat] = khat;
    rec[kEss] = 1.0 / s2;
    rec[kNInfeasible] = n_inf;
    rec[kFlags] = (double)(kValidBit | (khat <= tau ? kReliableBit : 0u) | ((free_mask & 15u) << 2));
  }
}

// the draws of the host form: f[S][4]
struct ArrayDraws {
  const double* f;
  void operator()(int t, double o[4]) const {
    for (int k = 0; k < 4; ++k) o[k] = f[4 * t + k];
  }
};

// Host form: work holds work_len(S) doubles, work[t] = lw_t on entry and the
// weights on a true return.
inline bool psis_weights_host(double* work, int S, double* khat, double* n_inf) {
  return psis_weights(OneLane{}, work, S, *khat, *n_inf);
}
inline void psis_estimates_host(const double* wt, int S, const double* f, double khat, double n_inf, unsigned free_mask,
                                double* rec) {
  psis_estimates(OneLane{}, wt, S, ArrayDraws{f}, khat, n_inf, khat_threshold(S), free_mask, rec);
}

}  // namespace mdfit::mappsis

#if defined(__HIPCC__)
#include "mdfit_mapis.h"  // (the importance sampler's device core)

namespace mdfit::mappsis {

using namespace mapis;

// the kernel's draws for psis_estimates: regenerated from the stream
struct StreamDraws {
  const double* P;
  Stream st;
  __device__ __forceinline__ void operator()(int t, double f[4]) const {
    const ThetaD th = psis_theta(psis_draw(P, st, t));
    f[0] = th.q;
    f[1] = th.A;
    f[2] = th.c;
    f[3] = th.delta + 2.0;
  }
};

// One wave per taxon, its three PMD sub-fits one after another.  Phases 1-3
// are the core's (mdfit_mapis.h): proposals<true> leaves each sub-fit's
// proposal in LDS by diagnostic slot, subfit_weights draws, weights and
// smooths (with kAdapt, mdfit_map_psis_adapt, in the rounds of MDFIT-ADAPT v1,
// DESIGN.md §3.12; adapt_rounds = 0 is the plain kernel's arithmetic).  Phase 4
// is psis_estimates with the draws regenerated from the stream.  Dynamic LDS:
// work_len(S) doubles (22,016 B at S = 1024, 6,656 B at S = 256); static:
// 1,536 B.  Reads y, N, out and status only.  adapt: [T][3][4], optional.
template <bool kAdapt>
__global__ __launch_bounds__(64) void map_psis_kernel(const uint32_t* __restrict__ gy,
                                                      const uint32_t* __restrict__ gN,
                                                      const double* __restrict__ out,
                                                      const int32_t* __restrict__ status, int64_t n_taxa, int S,
                                                      uint64_t seed, int64_t index_base, double tau,
                                                      double* __restrict__ psis, double* __restrict__ draws,
                                                      int adapt_rounds, double* __restrict__ adapt) {
  extern __shared__ double s_w[];
  __shared__ double s_y[kLD], s_N[kLD];
  __shared__ double s_par[4][kNPar];  // by diagnostic slot: 0, 2, 3 (1, the null fit's, unused)
  const int lane = threadIdx.x;
  const int64_t t = blockIdx.x;
  if (t >= n_taxa) return;
  double* dr0 = draws != nullptr ? draws + t * 3 * (int64_t)S * 6 : nullptr;

  if (status[t] != MDFIT_OK) {  // wave-uniform: NaN statistics, flags 0
    if (lane < 3) invalid_row(psis + (t * 3 + lane) * MDFIT_NMAPPSIS, 0u);
    bad_status_fills<kAdapt>(dr0, (int64_t)3 * S * 6, adapt, t);
    return;
  }
  load_counts(gy, gN, t, s_y, s_N);

  // ---- phase 1: the modes, g and H there, the held sets ----
  proposals<true>(gy, gN, out, t, s_par);
  __syncthreads();

  const PsisWave w;
  const uint64_t gtaxon = (uint64_t)(index_base + t);
  for (int s = 0; s < 3; ++s) {
    const int slot = s == 0 ? 0 : s + 1;  // the chain's sub-fit index: 0, 2, 3
    const double* P = s_par[slot];
    const unsigned mask = (unsigned)P[kPMask];
    double* rec = psis + (t * 3 + s) * MDFIT_NMAPPSIS;
    double* dr = dr0 != nullptr ? dr0 + (int64_t)s * S * 6 : nullptr;
    if (P[kPValid] == 0.0) {  // (wave-uniform)
      if (lane == 0) invalid_row(rec, mask);
      if (dr != nullptr) nan_fill(dr, (int64_t)S * 6);
      if constexpr (kAdapt) adapt_row_nan(adapt, t, s);
      continue;
    }
    const Stream st = subfit_stream(seed, gtaxon, slot);
    const int lo = s == 2 ? kNHalf : 0, hi = s == 1 ? kNHalf : kNPos;
    // ---- phases 2-3: the draws, the smoothed weights, the rounds ----
    const SubfitWeights sw = subfit_weights<kAdapt, false>(w, true, lo, hi, s_par[slot], st, S, tau, adapt_rounds, s_y,
                                                           s_N, s_w, nullptr, dr);
    // ---- phase 4: the estimates ----
    if (sw.ok) {
      psis_estimates(w, s_w, S, StreamDraws{P, st}, sw.khat, sw.n_inf, tau, mask, rec);
    } else if (lane == 0) {
      invalid_row(rec, mask);
    }
    if constexpr (kAdapt) {
      if (sw.ok && sw.best > 0 && lane == 0) rec[kFlags] += (double)mapadapt::kAdaptedBit;
      adapt_row(adapt, t, s, sw);
    }
    draws_weights(dr, s_w, S, sw.ok);
    __syncthreads();  // (the next sub-fit overwrites s_w)
  }
}

// mdfit_psis_weights: one wave per series lw[row][0..S)
#ifndef MDFIT_NO_HELPER_KERNELS  // (a second unit of libmdfit.so includes this header for the templates alone)
__global__ __launch_bounds__(64) void psis_weights_kernel(const double* __restrict__ lw, int64_t n_series, int S,
                                                          double* __restrict__ wout, double* __restrict__ khat) {
  extern __shared__ double s_w[];
  const int64_t row = blockIdx.x;
  if (row >= n_series) return;
  for (int x = threadIdx.x; x < S; x += 64) s_w[x] = lw[row * (int64_t)S + x];
  double k, ninf;
  const bool ok = psis_weights(PsisWave{}, s_w, S, k, ninf);
  for (int x = threadIdx.x; x < S; x += 64) wout[row * (int64_t)S + x] = ok ? s_w[x] : NAN;
  if (threadIdx.x == 0) khat[row] = ok ? k : NAN;
}
#endif  // MDFIT_NO_HELPER_KERNELS

}  // namespace mdfit::mappsis
#endif  // __HIPCC__
