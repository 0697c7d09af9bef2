// mdfit_mapppc.h — MDFIT-PPC v1 (mdfit_map_ppc): the
// posterior predictive check of the PMD fit on all positions (row 0, diagnostic
// slot 0) from the replicated counts that mdfit_map_pred draws.  Phases 1-4 are
// map_pred_kernel's through the same functions (mdfit_mapis.h, mappred::
// resample), so the weights, khat, ess, the index and the adapt record carry
// that kernel's row-0 bits; phase 5 draws the same predictive counts
// (mappred::predictive_count: jobs 0..29's keys) and, in place of a sort and a
// window, holds each replicate against the observed counts under its own theta:
// the largest squared standardised residual (an outlying position) and the
// signed strand difference of the residuals, as two posterior predictive
// p-values, and per column the upper mid-p of the observed count.
// mdfit_map_ppc_adapt is the same kernel with mdfit_mapadapt.h's proposal
// rounds around the importance sampling (map_ppc_kernel<true>).
//
// The record's selection over the 30 columns (worst_position) is written once
// as plain C++ (worst_position): lane 0 of the kernel runs it on the counts in
// LDS, and a plain C++ program can run it on an array.  Every count of the
// record is an integer count over the R draws; the two means go through
// PsisWave::sum, so a record depends on neither the grid nor the order.
#pragma once

#include <cmath>
#include <cstdint>

#include "mdfit_mappred.h"

namespace mdfit::mapppc {

// record layout (MDFIT_NMAPPPC = 12 doubles per taxon)
constexpr int kPOutlier = 0, kPStrand = 1, kTOutlier = 2, kTStrand = 3, kWorstPos = 4, kPWorst = 5, kNLow = 6,
              kNPoints = 7, kKhat = 8, kEss = 9, kNDistinct = 10, kFlags = 11;
constexpr unsigned kValidBit = 1u, kReliableBit = 2u, kNonCountBit = 8u;
constexpr int kNCols = 30;
constexpr double kLowP = 0.05;  // n_low counts the columns whose two-sided mid-p is below it

// the upper mid-p of a column from its counts over R draws: gt = #{rep > obs}, eq = #{rep = obs}
MDFIT_NS_FN double mid_p(uint32_t gt, uint32_t eq, int R) {
  return (2.0 * (double)gt + (double)eq) / (2.0 * (double)R);
}

// What the record takes from the per-column counts cnt[col] = {gt, eq} of the
// columns with N > 0 (has[col]): the column with the smallest two-sided mid-p
// 2 min(p, 1 - p) (the lowest index among equals), that value, the number of
// columns below kLowP and the number of columns.  worst = -1 without a column.
struct Worst {
  int worst;
  double p_worst, n_low, n_points;
};
template <class Has>
MDFIT_NS_FN Worst worst_position(const uint32_t (*cnt)[2], const Has& has, int R) {
  Worst r;
  r.worst = -1;
  r.p_worst = nutssumm::ns_nan();
  r.n_low = 0.0;
  r.n_points = 0.0;
#pragma unroll 1
  for (int col = 0; col < kNCols; ++col) {
    if (!has(col)) continue;
    const double p = mid_p(cnt[col][0], cnt[col][1], R);
    const double p2 = 2.0 * (p < 1.0 - p ? p : 1.0 - p);
    r.n_points += 1.0;
    if (p2 < kLowP) r.n_low += 1.0;
    if (r.worst < 0 || p2 < r.p_worst) {  // ascending col: only a strictly smaller value replaces
      r.worst = col;
      r.p_worst = p2;
    }
  }
  return r;
}

// the kernel's dynamic LDS in bytes: psis_weights' work buffer, whose part
// behind the S weights the index overlays afterwards
inline size_t lds_bytes(int S, int R) {
  const size_t a = (size_t)mappsis::work_len(S) * sizeof(double);
  const size_t b = (size_t)S * sizeof(double) + (size_t)R * sizeof(int);
  return a > b ? a : b;
}

}  // namespace mdfit::mapppc

#if defined(__HIPCC__)
namespace mdfit::mapppc {

using namespace mapis;
using mappred::kNoCount;

// the 64 lanes of a wave: PsisWave and an integer sum
struct PpcWave : PsisWave {
  __device__ __forceinline__ int isum(int v) const {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
  }
};

// D of column position k under theta, in predictive_count's arithmetic
__device__ __forceinline__ double damage_at(int k, double q, double A, double c) {
#pragma clang fp contract(off)
  double D = A * pow(1.0 - q, (double)k) + c;
  D = D < 0.0 ? 0.0 : (D > 1.0 ? 1.0 : D);
  return D;
}

// the standardised residuals of the observed and the replicated count of one
// column under theta: mu = N D, v = N D (1 - D)(phi + N) / (phi + 1); false
// when v is not > 0 (the column is skipped on both sides)
__device__ __forceinline__ bool residuals(double y, double yrep, double nn, double D, double phi, double& ro,
                                          double& rr) {
#pragma clang fp contract(off)
  const double mu = nn * D;
  const double v = nn * D * (1.0 - D) * (phi + nn) / (phi + 1.0);
  if (!(v > 0.0)) return false;
  const double sv = sqrt(v);
  ro = (y - mu) / sv;
  rr = (yrep - mu) / sv;
  return true;
}

// One wave per taxon.  Phases 1-4 are map_pred_kernel's for its row 0:
// proposals<true>, subfit_weights<kAdapt, false> on columns 0..29, ess,
// mappred::resample.  Phase 5 -- lanes over the R predictive draws: theta of
// draw idx[r] regenerated once (psis_draw, psis_theta), then the columns one
// after another; the per-draw maxima and strand sums stay in registers, and a
// column's two counts are a ballot's population count added by lane 0 (the
// lowest draw of a pass, so always active) into s_cnt.  Dynamic LDS:
// lds_bytes(S, R); static: 1,776 B.  Reads y, N, out and status only.
// adapt: [T][3][4], optional; rows 1 and 2 (not run) are NaN.
template <bool kAdapt>
__global__ __launch_bounds__(64) void map_ppc_kernel(const uint32_t* __restrict__ gy, const uint32_t* __restrict__ gN,
                                                     const double* __restrict__ out,
                                                     const int32_t* __restrict__ status, int64_t n_taxa, int S, int R,
                                                     uint64_t seed, int64_t index_base, double tau,
                                                     float* __restrict__ ppos, double* __restrict__ rec_out,
                                                     int32_t* __restrict__ index_tap,
                                                     uint32_t* __restrict__ counts_tap, double* __restrict__ disc_tap,
                                                     int adapt_rounds, double* __restrict__ adapt) {
  extern __shared__ double s_w[];
  __shared__ double s_y[kLD], s_N[kLD];
  __shared__ double s_par[4][kNPar];  // by diagnostic slot (proposals<true> writes 0, 2, 3; 0 is used)
  __shared__ uint32_t s_cnt[kNCols][2];  // #{rep > obs}, #{rep = obs} of each column
  const int lane = threadIdx.x;
  const int64_t t = blockIdx.x;
  if (t >= n_taxa) return;
  double* rec = rec_out + t * MDFIT_NMAPPPC;
  float* pp = ppos + t * kNCols;
  int32_t* itap = index_tap != nullptr ? index_tap + t * (int64_t)R : nullptr;
  uint32_t* ctap = counts_tap != nullptr ? counts_tap + t * kNCols * (int64_t)R : nullptr;
  double* dtap = disc_tap != nullptr ? disc_tap + t * 4 * (int64_t)R : nullptr;

  if (ctap != nullptr)
    for (int x = lane; x < kNCols * R; x += 64) ctap[x] = kNoCount;
  if (itap != nullptr)
    for (int x = lane; x < R; x += 64) itap[x] = -1;
  if (dtap != nullptr) nan_fill(dtap, 4 * (int64_t)R);
  if (lane < kNCols) {
    s_cnt[lane][0] = 0u;
    s_cnt[lane][1] = 0u;
  }
  const bool st_ok = status[t] == MDFIT_OK;  // (wave-uniform)
  if (!st_ok) bad_status_fills<kAdapt>(nullptr, 0, adapt, t);
  bool ok = false;
  double khat = NAN, ess = NAN, nd = NAN;
  double p_out = NAN, p_str = NAN, t_out = NAN, t_str = NAN;
  bool noncount = false, adapted = false;
  if (st_ok) {
    load_counts(gy, gN, t, s_y, s_N);
    // ---- phase 1: the modes, g and H there, the held sets ----
    proposals<true>(gy, gN, out, t, s_par);
    __syncthreads();
    const PpcWave w;
    double* P = s_par[0];
    const bool pvalid = P[kPValid] != 0.0;  // (wave-uniform)
    if (pvalid) {
      const Stream st = subfit_stream(seed, (uint64_t)(index_base + t), 0);
      // ---- phases 2-3: the draws, the smoothed weights, the rounds ----
      const SubfitWeights sw =
          subfit_weights<kAdapt, false>(w, true, 0, kNPos, P, st, S, tau, adapt_rounds, s_y, s_N, s_w, nullptr, nullptr);
      ok = sw.ok;
      if constexpr (kAdapt) {
        adapted = ok && sw.best > 0;
        adapt_row(adapt, t, 0, sw);
      }
      if (ok) {
        khat = sw.khat;
        double s2 = 0.0;
        for (int i = lane; i < S; i += 64) {
          const double wi = s_w[i];
          s2 += wi * wi;
        }
        s2 = w.sum(s2);
        ess = 1.0 / s2;
        // ---- phase 4: the index of each predictive draw ----
        int* s_idx = reinterpret_cast<int*>(s_w + S);
        nd = mappred::resample(w, s_w, S, R, s_idx);
        if (itap != nullptr)
          for (int r = lane; r < R; r += 64) itap[r] = s_idx[r];
        // ---- phase 5: lanes over the predictive draws ----
        int n_out = 0, n_str = 0;
        double sum_out = 0.0, sum_str = 0.0;
        for (int r = lane; r < R; r += 64) {
          const ThetaD th = psis_theta(psis_draw(P, st, s_idx[r]));
          const double phi = th.delta + 2.0;
          double max_o = 0.0, max_r = 0.0;                  // T_out of the observed / the replicated counts
          double fo = 0.0, fr = 0.0, bo = 0.0, br = 0.0;  // the strand sums: forward, reverse (backward)
#pragma unroll 1
          for (int col = 0; col < kNPos; ++col) {
            const double nn = s_N[col];
            if (!(nn > 0.0)) continue;  // (wave-uniform)
            const int kk = col < kNHalf ? col : col - kNHalf;
            const double yy = s_y[col];
            const int64_t c64 = mappred::predictive_count(st, r, col, kk, nn, th.q, th.A, th.c, phi);
            const bool isc = c64 >= 0;
            if (!isc) noncount = true;
            if (ctap != nullptr) ctap[col * (int64_t)R + r] = isc ? (uint32_t)c64 : kNoCount;
            const double yr = (double)c64;
            const unsigned long long bgt = __ballot(isc && yr > yy), beq = __ballot(isc && yr == yy);
            if (lane == 0) {
              s_cnt[col][0] += (uint32_t)__popcll(bgt);
              s_cnt[col][1] += (uint32_t)__popcll(beq);
            }
            double ro, rr;
            if (isc && residuals(yy, yr, nn, damage_at(kk, th.q, th.A, th.c), phi, ro, rr)) {
              max_o = fmax(max_o, ro * ro);
              max_r = fmax(max_r, rr * rr);
              if (col < kNHalf) {
                fo += ro;
                fr += rr;
              } else {
                bo += ro;
                br += rr;
              }
            }
          }
          const double so = fo - bo, sr = fr - br;
          n_out += max_r >= max_o ? 1 : 0;
          n_str += fabs(sr) >= fabs(so) ? 1 : 0;
          sum_out += max_o;
          sum_str += so;
          if (dtap != nullptr) {
            dtap[r * 4 + 0] = max_o;
            dtap[r * 4 + 1] = max_r;
            dtap[r * 4 + 2] = so;
            dtap[r * 4 + 3] = sr;
          }
        }
        noncount = __ballot(noncount) != 0ull;
        n_out = w.isum(n_out);
        n_str = w.isum(n_str);
        t_out = w.sum(sum_out) / (double)R;
        t_str = w.sum(sum_str) / (double)R;
        p_out = (double)n_out / (double)R;
        p_str = (double)n_str / (double)R;
      }
    }
    if constexpr (kAdapt) {
      if (!pvalid) adapt_row_nan(adapt, t, 0);
      adapt_row_nan(adapt, t, 1);
      adapt_row_nan(adapt, t, 2);
    }
  }
  __syncthreads();  // (s_cnt; s_N of a taxon that ran)
  const bool pvals = ok && !noncount;
  if (lane < kNCols)
    pp[lane] = (pvals && s_N[lane] > 0.0) ? (float)mid_p(s_cnt[lane][0], s_cnt[lane][1], R) : NAN;
  if (lane == 0) {
    if (!ok) {
#pragma unroll 1
      for (int x = 0; x < MDFIT_NMAPPPC; ++x) rec[x] = x == kFlags ? 0.0 : NAN;
    } else {
      bool fwd = false, rev = false;
#pragma unroll 1
      for (int col = 0; col < kNPos; ++col) {
        if (s_N[col] > 0.0) (col < kNHalf ? fwd : rev) = true;
      }
      const Worst wp = worst_position(s_cnt, [&](int col) { return s_N[col] > 0.0; }, R);
      rec[kPOutlier] = pvals ? p_out : NAN;
      rec[kPStrand] = pvals && fwd && rev ? p_str : NAN;
      rec[kTOutlier] = t_out;
      rec[kTStrand] = t_str;
      rec[kWorstPos] = pvals && wp.worst >= 0 ? (double)wp.worst : NAN;
      rec[kPWorst] = pvals ? wp.p_worst : NAN;
      rec[kNLow] = pvals ? wp.n_low : NAN;
      rec[kNPoints] = wp.n_points;
      rec[kKhat] = khat;
      rec[kEss] = ess;
      rec[kNDistinct] = nd;
      unsigned fl = (pvals ? kValidBit : 0u) | (khat <= tau ? kReliableBit : 0u) | (noncount ? kNonCountBit : 0u);
      if constexpr (kAdapt)
        if (adapted) fl |= mapadapt::kAdaptedBit;
      rec[kFlags] = (double)fl;
    }
  }
}

}  // namespace mdfit::mapppc
#endif  // __HIPCC__
