// mdfit_mappred.h — MDFIT-PPRED v1 (mdfit_map_pred): the
// reference's posterior predictive D_max columns and fit_predictions frame
// (fits.py:89-120) of a MAP fit from importance-weighted draws.  Each PMD
// sub-fit is importance-sampled exactly as mdfit_mappsis.h does it (the same
// functions, mdfit_mapis.h, so the same bits); its smoothed weights are resampled to R
// equally weighted draws by midpoint systematic resampling (no random number),
// and draw r of each of the sampler's 32 predictive jobs is the oracle's
// predictive_obs on theta of importance draw s(r), in the sampler's predictive
// Philox domain.  Median and numpyro's hpdi(0.68) of count / N follow.
// mdfit_map_pred_adapt (MDFIT-AUTO v1.1) is the same kernel
// with mdfit_mapadapt.h's proposal rounds around the importance sampling of a
// row (map_pred_kernel<true>, built in mdfit_mappred_adapt.hip).
//
// The resampling (resample), the u32 sort (sort_counts) and the median / HPDI
// (median_hpdi_counts) are written once over a `lanes` policy, as
// mdfit_mappsis.h: the kernel below runs them with the 64 lanes of a wave and
// the series in LDS; a plain C++ program (g++, no HIP) runs them with the
// one-lane policy (tests/mappred_host_main.cpp).  The cumulative weights are
// summed by one lane in ascending draw index whatever the policy; everything
// else is a selection, so a record depends on neither the policy nor the grid.
#pragma once

#include <cmath>
#include <cstdint>

#include "mdfit_mappsis.h"

namespace mdfit::mappred {

// record layout (MDFIT_NMAPPRED = 16 doubles per taxon)
constexpr int kDmax = 0, kDmaxLo = 1, kDmaxHi = 2, kDmaxForward = 3, kDmaxReverse = 4, kKhat = 5, kEss = 8,
              kNDistinct = 11, kNNonCount = 14, kFlags = 15;
constexpr unsigned kValidBit = 1u, kReliableBit = 2u;  // flags; bits 2..4: row 0..2 valid
constexpr int kMinPred = 25, kMaxPred = 1024;
constexpr int kNJobs = 32;  // columns 0..29 of PMD-all, column 0 under PMD-forward, under PMD-reverse
constexpr uint32_t kNoCount = 0xFFFFFFFFu;
constexpr int kMaxTile = 6;  // the most columns of row 0 one regenerated theta serves

using mappsis::OneLane;
using nutssumm::ns_inf;
using nutssumm::ns_nan;
using nutssumm::sort_len;

// Midpoint systematic resampling of the weights c[0..S) (>= 0, not all 0;
// shared by the lanes; the caller's last reads of them need no barrier of their
// own): c_s = c_{s-1} + w_s summed by lane 0 in ascending s and left in c,
// p_r = (r + 0.5) (c_{S-1} / R), idx[r] = the least s with c_s > p_r
// (np.searchsorted(np.cumsum(w), p, side="right")): a draw of weight 0 is never
// taken, and equal weights with R = S give idx[r] = r.  Every lane calls it and
// gets the number of different idx[r]; idx is written behind a barrier.
template <class L>
MDFIT_NS_FN double resample(const L& w, double* c, int S, int R, int* idx) {
  const int lane = w.lane(), nl = w.nlanes();
  w.sync();
  if (lane == 0) {
    double acc = 0.0;
    for (int s = 0; s < S; ++s) {
      acc += c[s];
      c[s] = acc;
    }
  }
  w.sync();
  const double step = c[S - 1] / (double)R;
  for (int r = lane; r < R; r += nl) {
    const double p = ((double)r + 0.5) * step;
    int lo = 0, hi = S;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (c[mid] > p) hi = mid;
      else lo = mid + 1;
    }
    idx[r] = lo < S ? lo : S - 1;  // (p_r < c_{S-1} by half a step: the bound is never used)
  }
  w.sync();
  double nd = 0.0;
  for (int r = lane; r < R; r += nl) nd += (r == 0 || idx[r] != idx[r - 1]) ? 1.0 : 0.0;  // (idx ascends)
  return w.sum(nd);
}

// Ascending bitonic sort of ncols columns of R counts each, column j at
// v + j * sort_len(R) (the padding kNoCount ends beyond R - 1): the network of
// mdfit_nutssumm.h's sort_series, every column's pairs in one pass per stage.
// The caller's writes of the counts need no barrier of their own.
template <class L>
MDFIT_NS_FN void sort_counts(const L& w, uint32_t* v, int R, int ncols) {
  const int lane = w.lane(), nl = w.nlanes();
  const int m = sort_len(R), half = m >> 1;
  for (int col = 0; col < ncols; ++col)
    for (int j = R + lane; j < m; j += nl) v[col * m + j] = kNoCount;
  w.sync();
  for (int k = 2; k <= m; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int pp = lane; pp < ncols * half; pp += nl) {
        const int col = pp / half, p = pp - col * half;
        const int x = ((p & ~(j - 1)) << 1) | (p & (j - 1)), y = x | j;
        uint32_t* vc = v + col * m;
        const uint32_t a = vc[x], b = vc[y];
        const bool up = (x & k) == 0;
        if ((a > b) == up) {
          vc[x] = b;
          vc[y] = a;
        }
      }
      w.sync();
    }
  }
}

// np.median and numpyro's hpdi(0.68) of the fractions c / Nn of the R sorted
// counts c (the oracle's median_hpdi on obs / N: the fractions formed after the
// sort, the narrowest window of int(0.68 R) + 1 draws, the lowest index among
// equals).  Every lane gets the same out3.
template <class L>
MDFIT_NS_FN void median_hpdi_counts(const L& w, const uint32_t* c, int R, double Nn, double out3[3]) {
  const int lane = w.lane(), nl = w.nlanes();
  out3[0] = (R & 1) ? (double)c[R / 2] / Nn : 0.5 * ((double)c[R / 2 - 1] / Nn + (double)c[R / 2] / Nn);
  const int len = (int)(0.68 * (double)R);
  const int n = R - len;
  double bw = ns_inf();
  int bi = nutssumm::kNoIndex;
  for (int i = lane; i < n; i += nl) {  // ascending i: only a strictly smaller width replaces
    const double wd = (double)c[i + len] / Nn - (double)c[i] / Nn;
    if (bi == nutssumm::kNoIndex || wd < bw) {
      bw = wd;
      bi = i;
    }
  }
  w.argmin(bw, bi);
  out3[1] = (double)c[bi] / Nn;
  out3[2] = (double)c[bi + len] / Nn;
}

// Host forms.  resample_host: c[S] the weights on entry (the cumulative weights
// on return), idx[R]; returns n_distinct.  median_hpdi_host: v holds
// sort_len(R) counts, the first R the unsorted draws.
inline int resample_host(double* c, int S, int R, int* idx) { return (int)resample(OneLane{}, c, S, R, idx); }
inline void median_hpdi_host(uint32_t* v, int R, double Nn, double out3[3]) {
  sort_counts(OneLane{}, v, R, 1);
  median_hpdi_counts(OneLane{}, v, R, Nn, out3);
}

// the kernel's dynamic LDS in bytes with a tile of tc columns: psis_weights'
// work buffer, whose part behind the S weights the index and the counts
// overlay afterwards
inline size_t lds_bytes(int S, int R, int tc) {
  const size_t a = (size_t)mappsis::work_len(S) * sizeof(double);
  const size_t b = (size_t)S * sizeof(double) + (size_t)R * sizeof(int) + (size_t)tc * sort_len(R) * sizeof(uint32_t);
  return a > b ? a : b;
}
// The tile: the most columns (<= kMaxTile, a divisor of 30 keeps the passes
// even) whose LDS stays within what map_psis_kernel's blocks per CU leave:
// eight blocks per CU by its registers (20,480 B each of the CU's 160 KB), or
// its own work buffer when that is larger.
inline int tile_cols(int S, int R) {
  constexpr size_t kStatic = 2560;  // (s_y, s_N, s_par, s_job, s_row: 2,400 B)
  const size_t work = (size_t)mappsis::work_len(S) * sizeof(double);
  const size_t cap = work + kStatic > 20480 ? work : 20480 - kStatic;
  int best = 1;
  for (int tc = 2; tc <= kMaxTile; ++tc)
    if (30 % tc == 0 && lds_bytes(S, R, tc) <= cap) best = tc;
  return best;
}

}  // namespace mdfit::mappred

#if defined(__HIPCC__)
#include "mdfit_mapis.h"  // (the importance sampler's device core)

namespace mdfit::mappred {

using namespace mapis;

// the 64 lanes of a wave: PsisWave and the (width, index) reduction
struct PredWave : PsisWave {
  __device__ __forceinline__ void argmin(double& wd, int& i) const {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double ow = __shfl_xor(wd, o, 64);
      const int oi = __shfl_xor(i, o, 64);
      if (oi != nutssumm::kNoIndex && (i == nutssumm::kNoIndex || nutssumm::window_before(ow, oi, wd, i))) {
        wd = ow;
        i = oi;
      }
    }
  }
};

// The sampler's sequential draws of one variate (oracle: ndraw; predictive
// draw convention 2): a block gives two uniforms -- words 0-1, then 2-3 -- or
// a Box-Muller pair of normals -- cos, then sin; the two kinds take blocks
// from one counter in the order they run dry.  Restated over this unit's
// primitives (mdfit_nuts.hip is closed to this unit) in the oracle's
// arithmetic: its divisions and 1 / sqrt, no reciprocal shared.
struct Draw {
  Stream st;
  uint32_t w2, w3;
  double uc = 0.0, nc = 0.0;  // the block's second uniform / normal
  bool uh = false, nh = false;
  __device__ __forceinline__ double uni() {
    if (uh) {
      uh = false;
      return uc;
    }
    const uint4 o = philox(st.k0, st.k1, st.c0, st.c1, w2, w3++);
    uc = u53(o.z, o.w);
    uh = true;
    return u53(o.x, o.y);
  }
  __device__ __forceinline__ double nrm() {
    if (nh) {
      nh = false;
      return nc;
    }
    const uint4 o = philox(st.k0, st.k1, st.c0, st.c1, w2, w3++);
    const double u1 = 1.0 - u53(o.x, o.y), u2 = u53(o.z, o.w);
    double sn, cs;
    sincos(6.283185307179586 * u2, &sn, &cs);
    const double r = sqrt(-2.0 * flog(u1));
    nc = r * sn;
    nh = true;
    return r * cs;
  }
};

// log of a Gamma(alpha, 1) draw (Marsaglia & Tsang; alpha < 1 boosted by u^(1/alpha))
__device__ __forceinline__ double log_gamma_draw(Draw& d, double alpha) {
  double boost = 0.0;
  if (alpha < 1.0) {
    boost = flog(1.0 - d.uni()) / alpha;
    alpha += 1.0;
  }
  const double dd = alpha - 1.0 / 3.0, cc = 1.0 / sqrt(9.0 * dd);
  for (int k = 0; k < 256; ++k) {
    const double x = d.nrm();
    double v = 1.0 + cc * x;
    if (v <= 0.0) continue;
    v = v * v * v;
    const double u = d.uni();
    if (u < 1.0 - 0.0331 * x * x * x * x) return flog(dd * v) + boost;
    if (flog(u) < 0.5 * x * x + dd * (1.0 - v + flog(v))) return flog(dd * v) + boost;
  }
  return flog(dd) + boost;
}

// Binomial(n, p): inversion for n min(p, 1 - p) < 10, else BTRS (Hormann 1993)
__device__ __forceinline__ double binomial_draw(Draw& d, double n, double p) {
  if (n <= 0.0 || p <= 0.0) return 0.0;
  if (p >= 1.0) return n;
  const bool flip = p > 0.5;
  const double pp = flip ? 1.0 - p : p, qq = 1.0 - pp;
  double k;
  if (n * pp < 10.0) {
    const double u = d.uni();
    double pmf = fexp(n * flog1p(-pp)), cdf = pmf;
    k = 0.0;
    const double ratio = pp / qq;
    while (u > cdf && k < n && k < 10000.0) {
      pmf *= (n - k) / (k + 1.0) * ratio;
      k += 1.0;
      cdf += pmf;
    }
  } else {
    const double spq = sqrt(n * pp * qq), bb = 1.15 + 2.53 * spq;
    const double aa = -0.0873 + 0.0248 * bb + 0.01 * pp, cc = n * pp + 0.5;
    const double vr = 0.92 - 4.2 / bb, alpha = (2.83 + 5.1 / bb) * spq;
    const double lpq = flog(pp / qq), m = floor((n + 1.0) * pp);
    const double hh = lgam(m + 1.0) + lgam(n - m + 1.0);
    k = floor(cc);
    for (int it = 0; it < 256; ++it) {
      const double u = d.uni() - 0.5, v = d.uni();
      const double us = 0.5 - fabs(u);
      const double kk = floor((2.0 * aa / us + bb) * u + cc);
      if (kk < 0.0 || kk > n) continue;
      if (us >= 0.07 && v <= vr) {
        k = kk;
        break;
      }
      const double lv = flog(v * alpha / (aa / (us * us) + bb));
      if (lv <= hh - lgam(kk + 1.0) - lgam(n - kk + 1.0) + (kk - m) * lpq) {
        k = kk;
        break;
      }
    }
  }
  return flip ? n - k : k;
}

// One predictive Beta-Binomial draw as its count (the oracle's predictive_obs
// with pmd = 1: draw r of column col, |z| - 1 = k, of theta = (q, A, c, phi)),
// -1 when it is no count in [0, Nn] (a NaN theta or p; at N = 2^32 - 1
// kNoCount is a count).  (Without contraction; its one call site is the column
// loop of phase 5, so inlining it repeats nothing and spares the call's frame:
// 8 B/lane of scratch otherwise.)
__device__ __forceinline__ int64_t predictive_count(Stream st, int r, int col, int k, double Nn, double q, double A,
                                                    double c, double phi) {
#pragma clang fp contract(off)
  double D = A * pow(1.0 - q, (double)k) + c;
  D = D < 0.0 ? 0.0 : (D > 1.0 ? 1.0 : D);
  Draw d{st, 0xFFFD0000u + (uint32_t)r, (uint32_t)col << 16};
  const double lx = log_gamma_draw(d, D * phi), ly = log_gamma_draw(d, (1.0 - D) * phi);
  const double p = 1.0 / (1.0 + fexp(ly - lx));
  const double obs = binomial_draw(d, Nn, p);
  return (obs >= 0.0 && obs <= Nn) ? (int64_t)obs : -1;
}

// One wave per taxon, its three PMD sub-fits one after another.  Phases 1-3
// are the core's (mdfit_mapis.h): proposals<true>, then per row subfit_weights
// -- the draws, the raw log-weights, psis_weights (with kAdapt,
// mdfit_map_pred_adapt, MDFIT-AUTO v1.1, DESIGN.md §3.13, in the rounds of
// MDFIT-ADAPT v1: afterwards the best round's proposal is in s_par[slot] and its
// weights are in the work buffer, so the phases below run unchanged and draw
// from the best proposal) -- then ess by psis_estimates' sum.  Phase 4 --
// resample: the cumulative weights over the weights, the index behind them;
// phase 5 -- lanes over the R predictive draws, theta of draw idx[r]
// regenerated from the stream (psis_draw, psis_theta: phase 2's bits) once per
// tile of tc columns of row 0, or for the one column of rows 1 and 2, the
// counts into the tile behind the index; phase 6 -- sort_counts and
// median_hpdi_counts per column.  Dynamic LDS: lds_bytes(S, R, tc); static:
// 2,400 B.  Reads y, N, out and status only.  adapt: [T][3][4], optional.
template <bool kAdapt>
__global__ __launch_bounds__(64) void map_pred_kernel(const uint32_t* __restrict__ gy,
                                                      const uint32_t* __restrict__ gN,
                                                      const double* __restrict__ out,
                                                      const int32_t* __restrict__ status, int64_t n_taxa, int S,
                                                      int R, int tc, uint64_t seed, int64_t index_base, double tau,
                                                      float* __restrict__ ppred, double* __restrict__ rec_out,
                                                      int32_t* __restrict__ index_tap,
                                                      uint32_t* __restrict__ counts_tap, int adapt_rounds,
                                                      double* __restrict__ adapt) {
  extern __shared__ double s_w[];
  __shared__ double s_y[kLD], s_N[kLD];
  __shared__ double s_par[4][kNPar];   // by diagnostic slot: 0, 2, 3 (1, the null fit's, unused)
  __shared__ double s_job[kNJobs][3];  // median, lower, upper of each job
  __shared__ double s_row[3][4];       // khat, ess, n_distinct, valid of each row
  const int lane = threadIdx.x;
  const int64_t t = blockIdx.x;
  if (t >= n_taxa) return;
  double* rec = rec_out + t * MDFIT_NMAPPRED;
  float* pp = ppred != nullptr ? ppred + t * (MDFIT_NPRED * kNPos) : nullptr;
  int32_t* itap = index_tap != nullptr ? index_tap + t * 3 * (int64_t)R : nullptr;
  uint32_t* ctap = counts_tap != nullptr ? counts_tap + t * kNJobs * (int64_t)R : nullptr;

  for (int x = lane; x < kNJobs * 3; x += 64) (&s_job[0][0])[x] = NAN;
  if (ctap != nullptr)
    for (int x = lane; x < kNJobs * R; x += 64) ctap[x] = kNoCount;
  if (itap != nullptr)
    for (int x = lane; x < 3 * R; x += 64) itap[x] = -1;
  if (status[t] != MDFIT_OK) {  // wave-uniform: NaN everywhere, flags 0
    if (lane < MDFIT_NMAPPRED) rec[lane] = lane == kFlags ? 0.0 : NAN;
    if (pp != nullptr)
      for (int x = lane; x < MDFIT_NPRED * kNPos; x += 64) pp[x] = NAN;
    bad_status_fills<kAdapt>(nullptr, 0, adapt, t);
    return;
  }
  load_counts(gy, gN, t, s_y, s_N);

  // ---- phase 1: the modes, g and H there, the held sets ----
  proposals<true>(gy, gN, out, t, s_par);
  __syncthreads();

  const PredWave w;
  const uint64_t gtaxon = (uint64_t)(index_base + t);
  const int m = sort_len(R);
  int* s_idx = reinterpret_cast<int*>(s_w + S);
  uint32_t* s_c = reinterpret_cast<uint32_t*>(s_idx + R);
  double n_noncount = 0.0;
  bool adapted = false;  // (kAdapt: some valid row's best round is > 0; wave-uniform)
#pragma unroll 1
  for (int row = 0; row < 3; ++row) {
    const int slot = row == 0 ? 0 : row + 1;  // the chain's sub-fit index: 0, 2, 3
    const double* P = s_par[slot];
    bool ok = P[kPValid] != 0.0;  // (wave-uniform)
    double khat = NAN, ess = NAN, nd = NAN;
    if (ok) {
      const Stream st = subfit_stream(seed, gtaxon, slot);
      const int lo = row == 2 ? kNHalf : 0, hi = row == 1 ? kNHalf : kNPos;
      // ---- phases 2-3: the draws, the smoothed weights, the rounds ----
      const SubfitWeights sw = subfit_weights<kAdapt, false>(w, true, lo, hi, s_par[slot], st, S, tau, adapt_rounds,
                                                             s_y, s_N, s_w, nullptr, nullptr);
      ok = sw.ok;
      khat = sw.khat;
      if constexpr (kAdapt) {
        adapted = adapted || (ok && sw.best > 0);
        adapt_row(adapt, t, row, sw);
      }
      if (ok) {
        double s2 = 0.0;
        for (int i = lane; i < S; i += 64) {
          const double wi = s_w[i];
          s2 += wi * wi;
        }
        s2 = w.sum(s2);
        ess = 1.0 / s2;
        // ---- phase 4: the index of each predictive draw ----
        nd = resample(w, s_w, S, R, s_idx);
        if (itap != nullptr)
          for (int r = lane; r < R; r += 64) itap[row * R + r] = s_idx[r];
        // ---- phases 5 and 6: the counts of a tile of columns, their summaries ----
        const int ncols = row == 0 ? kNPos : 1;
#pragma unroll 1
        for (int c0 = 0; c0 < ncols; c0 += tc) {
          const int nc = ncols - c0 < tc ? ncols - c0 : tc;
          unsigned badm = 0u;
          for (int r = lane; r < R; r += 64) {
            const ThetaD th = psis_theta(psis_draw(P, st, s_idx[r]));
            const double phi = th.delta + 2.0;
#pragma unroll 1
            for (int j = 0; j < nc; ++j) {
              const int col = c0 + j;  // (rows 1 and 2: column 0 of data_forward, fits.py:343-348)
              const int job = row == 0 ? col : kNPos + row - 1;
              const int kk = col < kNHalf ? col : col - kNHalf;
              const double nn = s_N[col];
              uint32_t cnt = kNoCount;
              if (nn > 0.0) {
                const int64_t c64 = predictive_count(st, r, col, kk, nn, th.q, th.A, th.c, phi);
                if (c64 < 0) badm |= 1u << j;
                else cnt = (uint32_t)c64;
                if (ctap != nullptr) ctap[job * (int64_t)R + r] = cnt;
              }
              s_c[j * m + r] = cnt;
            }
          }
#pragma unroll
          for (int o = 32; o >= 1; o >>= 1) badm |= (unsigned)__shfl_xor((int)badm, o, 64);
          sort_counts(w, s_c, R, nc);
          for (int j = 0; j < nc; ++j) {
            const int col = c0 + j;
            const int job = row == 0 ? col : kNPos + row - 1;
            const double nn = s_N[col];
            double m3[3] = {NAN, NAN, NAN};
            if (nn > 0.0) {  // (wave-uniform, as badm)
              if ((badm >> j) & 1u) n_noncount += 1.0;
              else median_hpdi_counts(w, s_c + j * m, R, nn, m3);
            }
            if (lane == 0) {
              s_job[job][0] = m3[0];
              s_job[job][1] = m3[1];
              s_job[job][2] = m3[2];
            }
          }
          __syncthreads();  // (the next tile overwrites s_c)
        }
      }
    }
    if constexpr (kAdapt)
      if (P[kPValid] == 0.0) adapt_row_nan(adapt, t, row);
    if (lane == 0) {
      s_row[row][0] = khat;
      s_row[row][1] = ess;
      s_row[row][2] = nd;
      s_row[row][3] = ok ? 1.0 : 0.0;
    }
    __syncthreads();  // (the next row overwrites s_w)
  }
  if (pp != nullptr)
    for (int x = lane; x < MDFIT_NPRED * kNPos; x += 64) pp[x] = (float)s_job[x % kNPos][x / kNPos];
  if (lane == 0) {
    rec[kDmax] = s_job[0][0];
    rec[kDmaxLo] = s_job[0][1];
    rec[kDmaxHi] = s_job[0][2];
    rec[kDmaxForward] = s_job[kNPos][0];
    rec[kDmaxReverse] = s_job[kNPos + 1][0];
    bool all_ok = true, all_rel = true;
    unsigned fl = 0u;
#pragma unroll
    for (int row = 0; row < 3; ++row) {
      const bool okr = s_row[row][3] != 0.0;
      rec[kKhat + row] = s_row[row][0];
      rec[kEss + row] = s_row[row][1];
      rec[kNDistinct + row] = s_row[row][2];
      all_ok = all_ok && okr;
      all_rel = all_rel && okr && s_row[row][0] <= tau;
      fl |= okr ? 4u << row : 0u;
    }
    rec[kNNonCount] = n_noncount;
    rec[kFlags] = (double)(fl | (all_ok ? kValidBit : 0u) | (all_ok && all_rel ? kReliableBit : 0u));
    if constexpr (kAdapt)
      if (adapted) rec[kFlags] += (double)mapadapt::kAdaptedBit;
  }
}

// mdfit_resample: one wave per series w[row][0..S)
#ifndef MDFIT_NO_HELPER_KERNELS  // (a second unit of libmdfit.so includes this header for the templates alone)
__global__ __launch_bounds__(64) void resample_kernel(const double* __restrict__ wt, int64_t n_series, int S, int R,
                                                      int32_t* __restrict__ idx, int32_t* __restrict__ n_distinct) {
  extern __shared__ double s_w[];
  const int64_t row = blockIdx.x;
  if (row >= n_series) return;
  int* s_idx = reinterpret_cast<int*>(s_w + S);
  for (int x = threadIdx.x; x < S; x += 64) s_w[x] = wt[row * (int64_t)S + x];
  const double nd = resample(PredWave{}, s_w, S, R, s_idx);
  for (int x = threadIdx.x; x < R; x += 64) idx[row * (int64_t)R + x] = s_idx[x];
  if (threadIdx.x == 0) n_distinct[row] = (int32_t)nd;
}
#endif  // MDFIT_NO_HELPER_KERNELS

}  // namespace mdfit::mappred
#endif  // __HIPCC__
