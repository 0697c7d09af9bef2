// mdfit_mapis.h — the device core of the importance sampler behind
// mdfit_map_psis, mdfit_map_waic, mdfit_map_pred, mdfit_map_evidence and their
// _adapt forms: the wave policy, the Philox
// draw of a proposal, the proposals at the MAP modes (phase 1), the draws, raw
// log-weights, Pareto smoothing and MDFIT-ADAPT rounds of one sub-fit (phases
// 2-3), and the per-taxon and per-sub-fit scaffolding of the four kernels.
//
// The four kernels call these functions, so whatever a record takes from them
// is the same bits in every entry at the same (seed, index_base + taxon,
// sub-fit, num_draws, adapt_rounds): a sub-fit's khat, ess, n_infeasible, its
// valid / reliable / free / adapted flag bits, its draws tap and its adapt
// record.  The mode, g, H and the free set under a proposal are
// mdfit_map_laplace's (mode_eval, mdfit_laplace.h).
//
// Device only; included by the HIP parts of mdfit_mappsis.h, mdfit_mapwaic.h,
// mdfit_mappred.h and mdfit_mapevid.h.  What a plain C++ program can run --
// psis_weights, the refit, the rows -- stays in those headers and
// mdfit_mapadapt.h, over the `lanes` policy.
//
// Any of those headers, or this one, may be the first included: the core
// stands on mdfit_mappsis.h's host part and that header's HIP part stands on
// the core, so this file goes through mdfit_mappsis.h before its own guard and
// is entered from there.

#include "mdfit_mappsis.h"

#ifndef MDFIT_MAPIS_H
#define MDFIT_MAPIS_H

#include "mdfit_mapadapt.h"

#if defined(__HIPCC__)
#include "mdfit_laplace.h"
#include "mdfit_model.h"

namespace mdfit::mapis {

// the proposal's words (mdfit_mappsis.h)
using mappsis::kNPar;
using mappsis::kPCHeld;
using mappsis::kPD;
using mappsis::kPGc;
using mappsis::kPK;
using mappsis::kPM;
using mappsis::kPMask;
using mappsis::kPU;
using mappsis::kPValid;

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

// the stream of one sub-fit: slot is the chain's sub-fit index, the
// diagnostic slot 0..5 (the PMD sub-fits: 0, 2, 3)
__device__ __forceinline__ Stream subfit_stream(uint64_t seed, uint64_t gtaxon, int slot) {
  Stream st;
  st.k0 = (uint32_t)seed;
  st.k1 = (uint32_t)(seed >> 32);
  st.c0 = (uint32_t)gtaxon;
  st.c1 = (uint32_t)(gtaxon >> 32) + ((uint32_t)slot << 24);
  return st;
}

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
    const ThetaD th = psis_theta(r);
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

// ---- the scaffolding of a kernel: one wave per taxon, its sub-fits in turn ----

// the taxon's counts as doubles in LDS (read behind the caller's next barrier)
__device__ __forceinline__ void load_counts(const uint32_t* __restrict__ gy, const uint32_t* __restrict__ gN, int64_t t,
                                            double* s_y, double* s_N) {
  const int lane = threadIdx.x;
  if (lane < kLD) {
    s_y[lane] = (double)gy[t * kLD + lane];
    s_N[lane] = (double)gN[t * kLD + lane];
  }
}

// n NaN doubles at p, the wave over them
__device__ __forceinline__ void nan_fill(double* p, int64_t n) {
  for (int64_t i = threadIdx.x; i < n; i += 64) p[i] = NAN;
}

// What a taxon whose status is not MDFIT_OK gets beside its NaN record (the
// kernel's own): n NaN words of draws when the tap is asked for, and NaN in
// its three adapt rows.
template <bool kAdapt>
__device__ __forceinline__ void bad_status_fills(double* dr, int64_t n, double* adapt, int64_t t) {
  if (dr != nullptr) nan_fill(dr, n);
  if constexpr (kAdapt)
    if (adapt != nullptr && threadIdx.x < 12) adapt[t * 12 + threadIdx.x] = NAN;
}

// column 5 of a sub-fit's draws tap: the smoothed weights, NaN where psis_weights refused
__device__ __forceinline__ void draws_weights(double* dr, const double* s_w, int S, bool ok) {
  if (dr != nullptr)
    for (int i = threadIdx.x; i < S; i += 64) dr[i * 6 + 5] = ok ? s_w[i] : NAN;
}

// ---- phase 1: the proposals at the modes ----

// mode_eval (laplace_kernel's evaluation in its row layout) for the PMD
// sub-fits (kPmd: rows 0-1 diag slot 0, row 2 slot 2, row 3 slot 3) or the null
// ones (slots 1, 4, 5: the fit kernel's null objective, the binding rule on q
// and delta alone, the 2x2 factorisation through the same 4x4 routines with A
// and c held), then the factorisation.  The writer lane of each sub-fit leaves
// the proposal in s_par[slot]; read it behind a barrier.
template <bool kPmd>
__device__ __forceinline__ void proposals(const uint32_t* __restrict__ gy, const uint32_t* __restrict__ gN,
                                          const double* __restrict__ out, int64_t t, double (*s_par)[kNPar]) {
  const int lane = threadIdx.x;
  const int row = lane >> 4, k = lane & 15;
  const int slot = kPmd ? (row < 2 ? 0 : row) : (row < 2 ? 1 : row + 2);
  const bool writer = k == 0 && row != 1;
  ModeEval me;
  mode_eval<kPmd>(gy, gN, out + t * MDFIT_NOUT + MDFIT_F_DIAG + MDFIT_DIAG_STRIDE * slot, t, me);
  const double* u = me.u;
  const Eval& e = me.e;
  const unsigned mask = me.mask;
  const bool fr[4] = {(mask & 1u) != 0u, (mask & 2u) != 0u, (mask & 4u) != 0u, (mask & 8u) != 0u};
  double C[4][4];
  const bool lap_ok = laplace::free_covariance(e.H, mask, C);
  double d[4], M[4][4];
  scaled_factor(e.H, mask, d, M);
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

// ---- phases 2-3: the draws, the smoothed weights, the rounds ----

// the kernels' draws for mapadapt::refit: u regenerated from the stream
struct StreamU {
  const double* P;
  Stream st;
  __device__ __forceinline__ void operator()(int t, double u[4]) const {
    const DrawU r = psis_draw(P, st, t);
    u[0] = r.u0;
    u[1] = r.u1;
    u[2] = r.u2;
    u[3] = r.u3;
  }
};

// Steps 2-4 of an MDFIT-ADAPT round in a kernel: from the best round's proposal
// P (LDS), weights wt (LDS) and stream, the next round's proposal, written over
// P by lane 0 between two barriers when the refit succeeds (P is untouched when
// it does not).  The mask, the held set, K and the held coordinates' centre stay.
__device__ __forceinline__ bool next_proposal(const double* wt, int S, double* P, Stream st) {
  const unsigned mask = (unsigned)P[kPMask];
  const bool cheld = P[kPCHeld] != 0.0;
  mapadapt::Refit r;
  const bool ok = mapadapt::refit(PsisWave{}, wt, S, StreamU{P, st}, mask, cheld, P + kPK, r);
  __syncthreads();  // (every lane has drawn from P)
  if (ok && threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if ((mask >> j) & 1u) P[kPU + j] = r.m[j];
      P[kPD + j] = r.d[j];
#pragma unroll
      for (int p = 0; p < 4; ++p) P[kPM + 4 * p + j] = r.F[j][p];
    }
    if (cheld) P[kPGc] = r.gc;
  }
  __syncthreads();
  return ok;
}

// What phases 2-3 leave of one sub-fit: ok, khat and n_inf are psis_weights'
// of the pass whose weights stand in s_w (the best round's), shift and total
// its level (psis_weights_level); k0, ess0, best and tried the adapt record.
struct SubfitWeights {
  bool ok;
  double khat, n_inf, shift, total, k0, ess0;
  int best, tried;
};

// Phases 2-3 of one sub-fit whose proposal P = s_par[slot] is valid.  Phase 2
// -- lanes over draws: a lane draws u, walks its sub-fit's points lo .. hi - 1
// through bb_logpmf and leaves the raw log-weight in s_w; u and the log-weight
// go into dr when it is given; with kShift the log-pmf at the proposal's
// centre goes into s_l0 (waic_points' shift).  Phase 3 -- psis_weights.
// kAdapt: the rounds of MDFIT-ADAPT v1 for a PMD row (one
// pass otherwise).  A row whose khat is over tau gets its proposal refitted to
// the weighted draws, in place in P with the best round's 32 words kept one
// per lane in `keep`, and is drawn and smoothed again from the same stream; a
// round that lowers khat becomes the best one, any other ends the loop: the
// best proposal is put back and phases 2-3 run once more on it, which brings
// its weights back into s_w bit for bit (no second copy of the weights and no
// further LDS).  adapt_rounds = 0 is the plain pass's arithmetic.
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
      const DrawU r = psis_draw(P, st, i);
      double lw = -INFINITY;
      if (pmd) {
        const ThetaD th = psis_theta(r);
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
      if (rnd == adapt_rounds || k_best <= tau) break;  // 1. the stop test
      if (lane < kNPar) keep = P[lane];
      if (!next_proposal(s_w, S, P, st)) break;  // 2-4. the refitted proposal, in place
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

// Row `row` (0..2: PMD-all, forward, reverse) of the taxon's adapt record from
// the rounds of a sub-fit whose proposal was valid ...
__device__ __forceinline__ void adapt_row(double* adapt, int64_t t, int row, const SubfitWeights& sw) {
  if (adapt != nullptr && threadIdx.x == 0) {
    double* ar = adapt + (t * 3 + row) * 4;
    ar[mapadapt::kKhat0] = sw.k0;
    ar[mapadapt::kEss0] = sw.ess0;
    ar[mapadapt::kBestRound] = sw.ok ? (double)sw.best : NAN;
    ar[mapadapt::kRoundsTried] = sw.ok ? (double)sw.tried : NAN;
  }
}
// ... and of one that has no weights: NaN
__device__ __forceinline__ void adapt_row_nan(double* adapt, int64_t t, int row) {
  if (adapt != nullptr && threadIdx.x < 4) adapt[(t * 3 + row) * 4 + threadIdx.x] = NAN;
}

}  // namespace mdfit::mapis

namespace mdfit::mapadapt {

// mdfit_adapt_proposal: one wave per series
#ifndef MDFIT_NO_HELPER_KERNELS  // (a second unit of libmdfit.so includes this header for the templates alone)
__global__ __launch_bounds__(64) void adapt_proposal_kernel(const double* __restrict__ u, const double* __restrict__ wt,
                                                            const int32_t* __restrict__ mask,
                                                            const int32_t* __restrict__ cheld,
                                                            const double* __restrict__ K, int64_t n_series, int S,
                                                            double* __restrict__ outp, int32_t* __restrict__ okp) {
  extern __shared__ double s_w[];
  const int64_t row = blockIdx.x;
  if (row >= n_series) return;
  for (int x = threadIdx.x; x < S; x += 64) s_w[x] = wt[row * (int64_t)S + x];
  __syncthreads();
  Refit r;
  const bool ok = refit(mapis::PsisWave{}, s_w, S, ArrayDraws{u + row * (int64_t)S * 4}, (unsigned)mask[row] & 15u,
                        cheld[row] != 0, K + row * 4, r);
  if (threadIdx.x == 0) {
    double* o = outp + row * 25;
    for (int j = 0; j < 4; ++j) {
      o[j] = ok ? r.m[j] : NAN;
      o[4 + j] = ok ? r.d[j] : NAN;
      for (int p = 0; p < 4; ++p) o[8 + 4 * j + p] = ok ? r.F[j][p] : NAN;
    }
    o[24] = ok ? r.gc : NAN;
    okp[row] = ok ? 1 : 0;
  }
}
#endif  // MDFIT_NO_HELPER_KERNELS

}  // namespace mdfit::mapadapt
#endif  // __HIPCC__

#endif  // MDFIT_MAPIS_H
