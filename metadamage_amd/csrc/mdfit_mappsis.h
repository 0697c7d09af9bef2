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
// once over a `lanes` policy, as mdfit_nutsloo.h: the kernel below runs them
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
#include "mdfit_laplace.h"
#include "mdfit_model.h"

namespace mdfit::mappsis {

// the 64 lanes of a wave: per-lane strided partial sums, then a fixed
// butterfly; lane 0's value is broadcast, so every decision is wave-uniform
struct PsisWave {
  __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
  __device__ __forceinline__ int nlanes() const { return 64; }
  __device__ __forceinline__ double sum(double v) const {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return __shfl(v, 0, 64);
  }
  __device__ __forceinline__ double max(double v) const {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return __shfl(v, 0, 64);
  }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
};

// Philox4x32-10 in the sampler's stream layout (mdfit_nuts.hip: make_stream,
// block; restated here because that translation unit is closed to this one):
// key = seed, counter = (global taxon lo, hi + (sub-fit << 24), w2, w3).  The
// draws of this launch take w2 = kDomain + draw index, a range no chain draw
// uses (theirs: the iteration, and 0xFFFD0000.. 0xFFFFFFFF), and w3 = 0..3.
constexpr uint32_t kDomain = 0xFFFC0000u;

__device__ __forceinline__ uint4 philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0;
    c1 = lo1;
    c2 = n2;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}
__device__ __forceinline__ double u53(uint32_t a, uint32_t b) {  // [0, 1)
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

struct Stream {
  uint32_t k0, k1, c0, c1;
};

struct DrawU {
  double u0, u1, u2, u3, lg;
};

// Draw x of the proposal P: four Philox blocks -- two Box-Muller pairs, the
// chi-square's two uniforms, the exponential's uniform -- whatever the free
// set is.  u in (logit q, logit A, c, log delta), lg the log proposal density
// up to a constant.  (Not inlined and without contraction: every pass over the
// draws gets the same bits.)
__device__ __noinline__ DrawU psis_draw(const double* P, Stream st, int x) {
#pragma clang fp contract(off)
  const uint32_t w2 = kDomain + (uint32_t)x;
  double z[4];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const uint4 o = philox(st.k0, st.k1, st.c0, st.c1, w2, (uint32_t)b);
    const double u1 = 1.0 - u53(o.x, o.y), u2 = u53(o.z, o.w);
    double sn, cs;
    sincos(6.283185307179586 * u2, &sn, &cs);
    const double r = sqrt(-2.0 * log(u1));
    z[2 * b] = r * cs;
    z[2 * b + 1] = r * sn;
  }
  const uint4 o2 = philox(st.k0, st.k1, st.c0, st.c1, w2, 2u);
  const double chi2 = -2.0 * (log(1.0 - u53(o2.x, o2.y)) + log(1.0 - u53(o2.z, o2.w)));
  const uint4 o3 = philox(st.k0, st.k1, st.c0, st.c1, w2, 3u);
  const double e = -log(1.0 - u53(o3.x, o3.y));
  const unsigned mask = (unsigned)P[kPMask];
  const bool cheld = P[kPCHeld] != 0.0;
  const double sc = 1.0 / sqrt(chi2 / 4.0);
  double t[4], tt = 0.0;
  int d = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool fr = (mask >> j) & 1u;
    t[j] = fr ? z[j] * sc : 0.0;
    tt += t[j] * t[j];
    d += fr ? 1 : 0;
  }
  const double cs_ = cheld ? e / P[kPGc] : 0.0;
  double u[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double s = 0.0;
#pragma unroll
    for (int p = j; p < 4; ++p) s += P[kPM + 4 * p + j] * t[p];
    const double mj = cheld ? P[kPU + j] + P[kPK + j] * cs_ : P[kPU + j];
    u[j] = ((mask >> j) & 1u) ? mj + P[kPD + j] * s : P[kPU + j];
  }
  if (cheld) u[2] = cs_;
  DrawU r;
  r.u0 = u[0];
  r.u1 = u[1];
  r.u2 = u[2];
  r.u3 = u[3];
  r.lg = -0.5 * (4.0 + (double)d) * log1p(tt / 4.0) - (cheld ? e : 0.0);
  return r;
}

struct ThetaD {
  double q, omq, A, c, delta, lj;  // lj: log prior + log Jacobian
  bool feasible;
};

// the constrained parameters of a draw and log prior(q, A, c, delta) + log[q(1-q) A(1-A) delta]
__device__ __noinline__ ThetaD psis_theta(DrawU r) {
#pragma clang fp contract(off)
  ThetaD th;
  double omA, lq, l1mq, lA, l1mA;
  logit_parts(r.u0, th.q, th.omq, lq, l1mq);
  logit_parts(r.u1, th.A, omA, lA, l1mA);
  th.c = r.u2;
  th.delta = exp(r.u3);
  th.feasible = th.c >= 0.0 && th.A + th.c < 1.0;
  // Beta(2, 3) on q and A, Beta(1, 9) on c, Exponential(1000) on delta (§3.1), then the Jacobian
  th.lj = (2.0 * lq + 3.0 * l1mq) + (2.0 * lA + 3.0 * l1mA) + 8.0 * log1p(-th.c) - th.delta / 1000.0 + r.u3;
  return th;
}

// the Jacobi-scaled Cholesky factor of laplace::free_covariance once more, by
// its own arithmetic: d = diag(H_ff)^-1/2 and M = L^-1 (lower triangular; the
// rows and columns of held coordinates the identity's)
__device__ __forceinline__ void scaled_factor(const double H[10], unsigned free_mask, double d[4], double M[4][4]) {
  bool fr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    fr[j] = (free_mask >> j) & 1u;
    const double hjj = H[laplace::lidx(j, j)];
    d[j] = (fr[j] && hjj > 0.0) ? laplace::rsqrt_pos(hjj) : 1.0;
  }
  double L[4][4], iL[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int m = 0; m <= j; ++m) {
      double s;
      if (!fr[j] || !fr[m]) s = (j == m) ? 1.0 : 0.0;
      else s = H[laplace::lidx(m, j)] * d[j] * d[m];
#pragma unroll
      for (int p = 0; p < m; ++p) s -= L[j][p] * L[m][p];
      if (j == m) {
        const double sp = s > laplace::kLaplacePivMin ? s : 1.0;
        iL[j] = laplace::rsqrt_pos(sp);
        L[j][j] = sp * iL[j];
      } else {
        L[j][m] = s * iL[m];
      }
    }
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < m) {
        M[j][m] = 0.0;
      } else if (j == m) {
        M[j][m] = iL[j];
      } else {
        double s = 0.0;
#pragma unroll
        for (int p = m; p < j; ++p) s -= L[j][p] * M[p][m];
        M[j][m] = s * iL[j];
      }
    }
  }
}

}  // namespace mdfit::mappsis
#include "mdfit_mapadapt.h"  // (the refit of a round: needs psis_draw and the proposal's layout above)
namespace mdfit::mappsis {

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

// One wave per taxon, its three PMD sub-fits one after another.  Phase 1 is
// laplace_kernel's evaluation in its row layout (rows 0-1 the all-position
// fit, row 2 forward, row 3 reverse; the same device functions, so the free
// bits and the factorisation's validity are mdfit_map_laplace's); the writer
// lane of each sub-fit leaves its proposal in LDS.  Phase 2 puts the lanes
// over the draws: a lane draws u, walks its sub-fit's 15 or 30 points through
// bb_logpmf and leaves the raw log-weight in LDS.  Phase 3 is psis_weights,
// phase 4 psis_estimates with the draws regenerated from the stream.
// Dynamic LDS: work_len(S) doubles (22,016 B at S = 1024, 6,656 B at S = 256);
// static: 1,280 B.  Reads y, N, out and status only.
//
// kAdapt (mdfit_map_psis_adapt, MDFIT-ADAPT v1): phases 2-3
// run once per round.  A row whose khat is over tau gets its proposal refitted
// to the weighted draws (mdfit_mapadapt.h), in place in s_par[s] with the best
// round's 32 words kept one per lane in a register, and is drawn and smoothed
// again from the same stream; a round that lowers khat becomes the best one,
// any other ends the loop: the best proposal is put back and phases 2-3 run
// once more on it, which brings its weights back into the work buffer bit for
// bit (no second copy of the weights and no further LDS: the blocks per CU are
// the plain kernel's).  adapt_rounds = 0 is the plain kernel's arithmetic.
// adapt: [T][3][4], optional.
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
  __shared__ double s_par[3][kNPar];
  const int lane = threadIdx.x;
  const int64_t t = blockIdx.x;
  if (t >= n_taxa) return;
  const int row = lane >> 4, k = lane & 15;
  const int sub = row < 2 ? 0 : row - 1;
  const bool writer = k == 0 && row != 1;

  if (status[t] != MDFIT_OK) {  // wave-uniform: NaN statistics, flags 0
    if (lane < 3) invalid_row(psis + (t * 3 + lane) * MDFIT_NMAPPSIS, 0u);
    if (draws != nullptr)
      for (int64_t i = lane; i < (int64_t)3 * S * 6; i += 64) draws[t * 3 * S * 6 + i] = NAN;
    if constexpr (kAdapt)
      if (adapt != nullptr && lane < 12) adapt[t * 12 + lane] = NAN;
    return;
  }
  if (lane < kLD) {
    s_y[lane] = (double)gy[t * kLD + lane];
    s_N[lane] = (double)gN[t * kLD + lane];
  }

  // ---- phase 1: the mode, g and H there, the held set (laplace_kernel) ----
  const double* dg = out + t * MDFIT_NOUT + MDFIT_F_DIAG + MDFIT_DIAG_STRIDE * (row < 2 ? 0 : row);
  const double q = dg[0], A = dg[1], c = dg[2], phi = dg[3];
  const double x = k == 0 ? q : (k == 1 ? A : phi - 2.0);
  const double lx = flog(x), l1mx = flog1p(k < 2 ? -x : 0.0);
  const double v = lx - l1mx;
  double u[4] = {rowb<0>(v), rowb<1>(v), c, rowb<2>(v)};
#pragma unroll
  for (int j = 0; j < 4; ++j) u[j] = clampd(u[j], kULo[j], kUHi[j]);
  {
    PointData pd;
    pd.pmd = 1;
    pd.valid = k < kNHalf;
    pd.k = pd.valid ? k : 0;
    const int col = pd.valid ? (row & 1) * kNHalf + k : 0;
    pd.y = pd.valid ? (double)gy[t * kLD + col] : 0.0;
    pd.N = pd.valid ? (double)gN[t * kLD + col] : 0.0;
    const Theta th = make_theta<16>(true, u);
    double acc[kNAcc];
#pragma unroll
    for (int j = 0; j < kNAcc; ++j) acc[j] = 0.0;
    point_accum<true>(pd, th, acc);
#pragma unroll
    for (int j = 2; j < kNAcc; ++j) {
      const double s16 = gsum<16>(acc[j]);
      const double s32 = s16 + xrow(s16);
      acc[j] = row < 2 ? s32 : s16;
    }
    acc[0] = acc[1] = 0.0;
    Eval e;
    finish_eval(true, th, acc, e);
    bool fr[4];
    double dbind[4];
    free_set(true, u, e.g, e.H, INFINITY, fr, dbind);
    const unsigned mask = (fr[0] ? 1u : 0u) | (fr[1] ? 2u : 0u) | (fr[2] ? 4u : 0u) | (fr[3] ? 8u : 0u);
    double C[4][4];
    const bool lap_ok = laplace::free_covariance(e.H, mask, C);
    double d[4], M[4][4];
    scaled_factor(e.H, mask, d, M);
    // supported: q, A and phi free, c free or held on its lower bound
    const bool cheld = !fr[2];
    const bool c_low = u[2] - kULo[2] <= kEpsBind[2];
    const bool ok = lap_ok && fr[0] && fr[1] && fr[3] && (!cheld || c_low);
    if (writer) {
      double* P = s_par[sub];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        P[kPU + j] = u[j];
        P[kPD + j] = d[j];
        // the free block's centre moves with a held c: -C_ff H_fc
        double kj = 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m)
          if (m != 2) kj -= C[j][m] * e.H[m < 2 ? hidx(m, 2) : hidx(2, m)];
        P[kPK + j] = (cheld && j != 2) ? kj : 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m) P[kPM + 4 * j + m] = M[j][m];
      }
      P[kPGc] = e.g[2];
      P[kPMask] = (double)mask;
      P[kPValid] = ok ? 1.0 : 0.0;
      P[kPCHeld] = cheld ? 1.0 : 0.0;
    }
  }
  __syncthreads();

  const PsisWave w;
  const uint64_t gtaxon = (uint64_t)(index_base + t);
  for (int s = 0; s < 3; ++s) {
    const double* P = s_par[s];
    const unsigned mask = (unsigned)P[kPMask];
    double* rec = psis + (t * 3 + s) * MDFIT_NMAPPSIS;
    double* dr = draws != nullptr ? draws + (t * 3 + s) * (int64_t)S * 6 : nullptr;
    if (P[kPValid] == 0.0) {  // (wave-uniform)
      if (lane == 0) invalid_row(rec, mask);
      if (dr != nullptr)
        for (int i = lane; i < S * 6; i += 64) dr[i] = NAN;
      if constexpr (kAdapt)
        if (adapt != nullptr && lane < 4) adapt[(t * 3 + s) * 4 + lane] = NAN;
      continue;
    }
    Stream st;
    st.k0 = (uint32_t)seed;
    st.k1 = (uint32_t)(seed >> 32);
    st.c0 = (uint32_t)gtaxon;
    st.c1 = (uint32_t)(gtaxon >> 32) + ((uint32_t)(s == 0 ? 0 : s + 1) << 24);  // the chain's sub-fit index: 0, 2, 3
    const int lo = s == 2 ? kNHalf : 0, hi = s == 1 ? kNHalf : kNPos;
    // the rounds of MDFIT-ADAPT v1 (one pass without kAdapt): a round's proposal is written over the best one
    // in s_par[s], which lane j < 32 keeps word j of in `keep` and puts back when the round is dropped
    double khat, n_inf;
    bool okw;
    double k0 = NAN, ess0 = NAN, k_best = NAN, keep = 0.0;
    int best = 0, tried = 0;
    bool rerun = false;
    for (int rnd = 0;;) {
      // ---- phase 2: lanes over draws ----
      for (int i = lane; i < S; i += 64) {
        const DrawU r = psis_draw(P, st, i);
        const ThetaD th = psis_theta(r);
        double lw = -INFINITY;
        if (th.feasible) {
          const double ph = th.delta + 2.0;
          double ll = 0.0;
#pragma unroll 1
          for (int col = lo; col < hi; ++col) {
            const int kk = col < kNHalf ? col : col - kNHalf;
            const double D = fma(th.A, powk(th.omq, kk), th.c);
            ll += bb_logpmf(s_y[col], s_N[col], D, ph);
          }
          lw = (ll + th.lj) - r.lg;
        }
        s_w[i] = lw;
        if (dr != nullptr) {
          dr[i * 6 + 0] = r.u0;
          dr[i * 6 + 1] = r.u1;
          dr[i * 6 + 2] = r.u2;
          dr[i * 6 + 3] = r.u3;
          dr[i * 6 + 4] = lw;
        }
      }
      // ---- phase 3: the smoothed weights; phase 4: the estimates ----
      okw = psis_weights(w, s_w, S, khat, n_inf);
      if constexpr (!kAdapt) {
        break;
      } else {
        if (rerun) break;  // (the best round's weights are back in s_w, khat and n_inf its own)
        if (rnd == 0) {
          if (!okw) break;
          k0 = khat;
          ess0 = mapadapt::weights_ess(w, s_w, S);
        } else {
          tried = rnd;
          if (!(okw && isfinite(khat) && khat < k_best)) {  // 6. the round is dropped: the best one once more
            if (lane < kNPar) s_par[s][lane] = keep;
            __syncthreads();
            rerun = true;
            continue;
          }
          best = rnd;
        }
        k_best = khat;
        if (rnd == adapt_rounds || k_best <= tau) break;              // 1. the stop test
        if (lane < kNPar) keep = s_par[s][lane];
        if (!mapadapt::next_proposal(s_w, S, s_par[s], st)) break;  // 2-4. the refitted proposal, in place
        ++rnd;
      }
    }
    if (okw) {
      psis_estimates(w, s_w, S, StreamDraws{P, st}, khat, n_inf, tau, mask, rec);
    } else if (lane == 0) {
      invalid_row(rec, mask);
    }
    if constexpr (kAdapt) {
      if (lane == 0) {
        if (okw && best > 0) rec[kFlags] += (double)mapadapt::kAdaptedBit;
        if (adapt != nullptr) {
          double* ar = adapt + (t * 3 + s) * 4;
          ar[mapadapt::kKhat0] = k0;
          ar[mapadapt::kEss0] = ess0;
          ar[mapadapt::kBestRound] = okw ? (double)best : NAN;
          ar[mapadapt::kRoundsTried] = okw ? (double)tried : NAN;
        }
      }
    }
    if (dr != nullptr)
      for (int i = lane; i < S; i += 64) dr[i * 6 + 5] = okw ? s_w[i] : NAN;
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
