// mdfit_mapwaic.h — MDFIT-WAIC v1 (mdfit_map_waic): the
// reference's WAIC comparisons (n_sigma, n_sigma_forward, n_sigma_reverse,
// asymmetry; fits.py:147-227) of a MAP fit from importance-weighted draws.  The
// three PMD sub-fits are importance-sampled exactly as mdfit_mappsis.h does it
// (the same device functions, so the same bits); the three null sub-fits get a
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
namespace mdfit::mapwaic {

using mappsis::DrawU;
using mappsis::kNPar;
using mappsis::kPCHeld;
using mappsis::kPD;
using mappsis::kPGc;
using mappsis::kPK;
using mappsis::kPM;
using mappsis::kPMask;
using mappsis::kPU;
using mappsis::kPValid;
using mappsis::PsisWave;
using mappsis::Stream;
using mappsis::ThetaD;

// the constrained parameters of a null draw and log prior(q, delta) + log[q(1-q) delta]
// (A = c = 0; every draw is feasible)
__device__ __noinline__ ThetaD null_theta(DrawU r) {
#pragma clang fp contract(off)
  ThetaD th;
  double lq, l1mq;
  logit_parts(r.u0, th.q, th.omq, lq, l1mq);
  th.A = 0.0;
  th.c = 0.0;
  th.delta = exp(r.u3);
  th.feasible = true;
  // Beta(2, 3) on q, Exponential(1000) on delta (§3.1), then the Jacobian
  th.lj = (2.0 * lq + 3.0 * l1mq) - th.delta / 1000.0 + r.u3;
  return th;
}

// a draw ready for its points: D(k) = fma(A, w^k, c) -- a null draw has A = 0,
// w = 1 and c = q, so D = q exactly
struct DrawPt {
  double A, w, c, ph, lj;
  bool feasible;
};

__device__ __forceinline__ DrawPt draw_point(bool pmd, DrawU r) {
  DrawPt d;
  if (pmd) {
    const ThetaD th = mappsis::psis_theta(r);
    d.A = th.A;
    d.w = th.omq;
    d.c = th.c;
    d.ph = th.delta + 2.0;
    d.lj = th.lj;
    d.feasible = th.feasible;
  } else {
    const ThetaD th = null_theta(r);
    d.A = 0.0;
    d.w = 1.0;
    d.c = th.q;
    d.ph = th.delta + 2.0;
    d.lj = th.lj;
    d.feasible = true;
  }
  return d;
}

// the kernel's draws for waic_points: regenerated from the stream; column lo +
// c of the counts in LDS is point c of the sub-fit
struct StreamSource {
  const double* P;
  Stream st;
  bool pmd;
  int lo;
  const double *s_y, *s_N;
  __device__ __forceinline__ DrawPt draw(int t) const { return draw_point(pmd, mappsis::psis_draw(P, st, t)); }
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

// Phase 1 of map_psis_kernel (laplace_kernel's evaluation in its row layout),
// for the PMD sub-fits (kPmd: rows 0-1 diag slot 0, row 2 slot 2, row 3 slot 3;
// map_psis_kernel's statements, so its bits) or the null ones (slots 1, 4, 5:
// the fit kernel's null objective, the binding rule on q and delta alone, the
// 2x2 factorisation through the same 4x4 routines with A and c held).  The
// writer lane of each sub-fit leaves the proposal in s_par[slot].
template <bool kPmd>
__device__ __forceinline__ void proposals(const uint32_t* __restrict__ gy, const uint32_t* __restrict__ gN,
                                          const double* __restrict__ out, int64_t t, double (*s_par)[kNPar]) {
  const int lane = threadIdx.x;
  const int row = lane >> 4, k = lane & 15;
  const int slot = kPmd ? (row < 2 ? 0 : row) : (row < 2 ? 1 : row + 2);
  const bool writer = k == 0 && row != 1;
  const double* dg = out + t * MDFIT_NOUT + MDFIT_F_DIAG + MDFIT_DIAG_STRIDE * slot;
  const double q = dg[0], A = kPmd ? dg[1] : 0.5, c = kPmd ? dg[2] : 0.0, phi = dg[3];
  const double x = k == 0 ? q : (k == 1 ? A : phi - 2.0);
  const double lx = flog(x), l1mx = flog1p(k < 2 ? -x : 0.0);
  const double v = lx - l1mx;
  double u[4] = {rowb<0>(v), rowb<1>(v), c, rowb<2>(v)};
#pragma unroll
  for (int j = 0; j < 4; ++j) u[j] = clampd(u[j], kULo[j], kUHi[j]);
  PointData pd;
  pd.pmd = kPmd ? 1 : 0;
  pd.valid = k < kNHalf;
  pd.k = pd.valid ? k : 0;
  const int col = pd.valid ? (row & 1) * kNHalf + k : 0;
  pd.y = pd.valid ? (double)gy[t * kLD + col] : 0.0;
  pd.N = pd.valid ? (double)gN[t * kLD + col] : 0.0;
  const Theta th = make_theta<16>(kPmd, u);
  double acc[mdfit::kNAcc];
#pragma unroll
  for (int j = 0; j < mdfit::kNAcc; ++j) acc[j] = 0.0;
  point_accum<true>(pd, th, acc);
#pragma unroll
  for (int j = 2; j < mdfit::kNAcc; ++j) {
    const double s16 = gsum<16>(acc[j]);
    const double s32 = s16 + xrow(s16);
    acc[j] = row < 2 ? s32 : s16;
  }
  acc[0] = acc[1] = 0.0;
  Eval e;
  finish_eval(kPmd, th, acc, e);
  bool fr[4];
  double dbind[4];
  free_set(kPmd, u, e.g, e.H, INFINITY, fr, dbind);
  const unsigned mask = (fr[0] ? 1u : 0u) | (fr[1] ? 2u : 0u) | (fr[2] ? 4u : 0u) | (fr[3] ? 8u : 0u);
  double C[4][4];
  const bool lap_ok = laplace::free_covariance(e.H, mask, C);
  double d[4], M[4][4];
  mappsis::scaled_factor(e.H, mask, d, M);
  // supported: PMD -- q, A and phi free, c free or held on its lower bound;
  // null -- q and delta free
  const bool cheld = kPmd && !fr[2];
  const bool c_low = u[2] - kULo[2] <= kEpsBind[2];
  const bool ok = lap_ok && fr[0] && (!kPmd || fr[1]) && fr[3] && (!cheld || c_low);
  if (writer) {
    double* P = s_par[slot];
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

// What phases 2-3 leave of one sub-fit: ok, khat and n_inf are psis_weights'
// of the pass whose weights stand in s_w (the best round's), shift and total
// its level (psis_weights_level); k0, ess0, best and tried the adapt record.
struct SubfitWeights {
  bool ok;
  double khat, n_inf, shift, total, k0, ess0;
  int best, tried;
};

// Phases 2-3 of one sub-fit whose proposal P = s_par[s] is valid, shared by
// map_waic_kernel and map_evidence_kernel (mdfit_mapevid.h).  Phase 2 -- lanes
// over draws, the raw log-weight into s_w (map_psis_kernel's statements for a
// PMD row), u and the log-weight into dr when it is given; with kShift the
// log-pmf at the proposal's centre into s_l0 (waic_points' shift).  Phase 3 --
// psis_weights.  kAdapt: the rounds of MDFIT-ADAPT v1 for a PMD row (one pass
// otherwise): a round's proposal is written over the best one in P, which lane
// j < 32 keeps word j of in `keep` and puts back when the round is dropped.
template <bool kAdapt, bool kShift>
__device__ __forceinline__ SubfitWeights subfit_weights(const PsisWave& w, bool pmd, int lo, int hi, double* P,
                                                        Stream st, int S, double tau, int adapt_rounds,
                                                        const double* s_y, const double* s_N, double* s_w,
                                                        double* s_l0, double* dr) {
  const int lane = threadIdx.x;
  const int n = hi - lo;
  bool ok;
  double khat, n_inf, shift, total;
  double k0 = NAN, ess0 = NAN, k_best = NAN, keep = 0.0;
  int best = 0, tried = 0;
  bool rerun = false;
  for (int rnd = 0;;) {
    // ---- phase 2: lanes over draws ----
    for (int i = lane; i < S; i += 64) {
      const DrawU r = mappsis::psis_draw(P, st, i);
      double lw = -INFINITY;
      if (pmd) {
        const ThetaD th = mappsis::psis_theta(r);
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
      } else {
        const ThetaD th = null_theta(r);
        const double ph = th.delta + 2.0;
        double ll = 0.0;
#pragma unroll 1
        for (int col = lo; col < hi; ++col) ll += bb_logpmf(s_y[col], s_N[col], th.q, ph);
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
    if constexpr (kShift) {
      // the shift of the second moments: the log-pmf at the mode (lanes over points)
      if (lane < n) {
        DrawU m;
        m.u0 = P[kPU + 0];
        m.u1 = P[kPU + 1];
        m.u2 = P[kPU + 2];
        m.u3 = P[kPU + 3];
        m.lg = 0.0;
        const DrawPt d = draw_point(pmd, m);
        const int col = lo + lane;
        const int kk = col < kNHalf ? col : col - kNHalf;
        const double l = bb_logpmf(s_y[col], s_N[col], fma(d.A, powk(d.w, kk), d.c), d.ph);
        s_l0[lane] = isfinite(l) ? l : 0.0;
      }
    }
    // ---- phase 3: the smoothed weights ----
    ok = mappsis::psis_weights_level(w, s_w, S, khat, n_inf, shift, total);
    if constexpr (!kAdapt) {
      break;
    } else {
      if (!pmd || rerun) break;  // (rerun: the best round's weights are back in s_w, khat and n_inf its own)
      if (rnd == 0) {
        if (!ok) break;
        k0 = khat;
        ess0 = mapadapt::weights_ess(w, s_w, S);
      } else {
        tried = rnd;
        if (!(ok && isfinite(khat) && khat < k_best)) {  // 6. the round is dropped: the best one once more
          if (lane < kNPar) P[lane] = keep;
          __syncthreads();
          rerun = true;
          continue;
        }
        best = rnd;
      }
      k_best = khat;
      if (rnd == adapt_rounds || k_best <= tau) break;      // 1. the stop test
      if (lane < kNPar) keep = P[lane];
      if (!mapadapt::next_proposal(s_w, S, P, st)) break;  // 2-4. the refitted proposal, in place
      ++rnd;
    }
  }
  SubfitWeights r;
  r.ok = ok;
  r.khat = khat;
  r.n_inf = n_inf;
  r.shift = shift;
  r.total = total;
  r.k0 = k0;
  r.ess0 = ess0;
  r.best = best;
  r.tried = tried;
  return r;
}

// One wave per taxon, its six sub-fits one after another in diagnostic-slot
// order.  Phase 1 twice (proposals<true>, proposals<false>).  Per sub-fit
// (phases 2-3: subfit_weights above, shared with map_evidence_kernel):
// phase 2 -- lanes over draws, the raw log-weight into LDS (map_psis_kernel's
// statements for a PMD row); phase 3 -- psis_weights; phase 4 -- waic_points
// with the draws regenerated from the stream, 64 at a time through a tile of
// 15 columns that overlays the work buffer behind the weights (as the points'
// accumulators do), lane i < 15
// walking point i's accumulators over the tile's draws in ascending order;
// then waic_row.  Row 6 is nutsloo::n_sigma on the waic_i columns, as
// nuts_loo_kernel's.  Dynamic LDS: lds_len(S) doubles (22,016 B at S = 1024,
// 11,048 B at S = 256); static: 4,448 B.  Reads y, N, out and status only.
//
// kAdapt (mdfit_map_waic_adapt, MDFIT-ADAPT v1): the PMD rows'
// phases 2-3 run in map_psis_kernel<true>'s rounds, statement for statement, so
// their khat, ess, n_infeasible, flags and adapt record are its bits; the null
// rows take one pass.  The shift s_l0 is the log-pmf at the best round's centre.
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
    if (dr0 != nullptr)
      for (int64_t i = lane; i < (int64_t)MDFIT_NSUBFIT * S * 6; i += 64) dr0[i] = NAN;
    if constexpr (kAdapt)
      if (adapt != nullptr && lane < 12) adapt[t * 12 + lane] = NAN;
    return;
  }
  if (lane < kLD) {
    s_y[lane] = (double)gy[t * kLD + lane];
    s_N[lane] = (double)gN[t * kLD + lane];
  }
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
    if (ok) {
      Stream st;
      st.k0 = (uint32_t)seed;
      st.k1 = (uint32_t)(seed >> 32);
      st.c0 = (uint32_t)gtaxon;
      st.c1 = (uint32_t)(gtaxon >> 32) + ((uint32_t)s << 24);  // the chain's sub-fit index
      const SubfitWeights sw = subfit_weights<kAdapt, true>(w, pmd, lo, hi, s_par[s], st, S, tau, adapt_rounds, s_y,
                                                            s_N, s_w, s_l0, dr);
      ok = sw.ok;
      const double khat = sw.khat, n_inf = sw.n_inf, k0 = sw.k0, ess0 = sw.ess0;
      const int best = sw.best, tried = sw.tried;
      if constexpr (kAdapt) {
        if (pmd && adapt != nullptr && lane == 0) {
          double* ar = adapt + (t * 3 + (s == 0 ? 0 : s - 1)) * 4;
          ar[mapadapt::kKhat0] = k0;
          ar[mapadapt::kEss0] = ess0;
          ar[mapadapt::kBestRound] = ok ? (double)best : NAN;
          ar[mapadapt::kRoundsTried] = ok ? (double)tried : NAN;
        }
      }
      if (dr != nullptr)
        for (int i = lane; i < S; i += 64) dr[i * 6 + 5] = ok ? s_w[i] : NAN;
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
      for (int i = lane; i < S * 6; i += 64) dr[i] = NAN;
    }
    if constexpr (kAdapt)
      if (!ok && pmd && adapt != nullptr && lane < 4) adapt[(t * 3 + (s == 0 ? 0 : s - 1)) * 4 + lane] = NAN;
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
