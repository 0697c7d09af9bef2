// mdfit_mapquant.h — MDFIT-QUANT v1 (mdfit_map_quant): the
// order statistics of the importance-weighted posterior that mdfit_map_psis
// forms: per PMD sub-fit the weighted median, 68 % highest-posterior-density
// interval, 5 % and 95 % quantiles and P(D_max > d0) of D_max, the median and
// interval of q, the medians of A, c and phi.  They are what
// mdfit_nuts_summary reads from a chain's draws (mdfit_nutssumm.h:
// order_stats), taken from weighted draws: with equal weights every rule below
// is that header's rule.
//
// All mass arithmetic is in integers: a weight becomes k = rint(w 2^52), the
// masses are sums of k, and every comparison of a mass with a share of the
// total is an integer comparison (100 mass > 68 K, never a floating 0.68 K).
// So a selection depends on neither the policy nor the order of a scan, and the
// statistics are selections and single operations on draws.  The arithmetic is
// written once over a `lanes` policy, as mdfit_mappsis.h: the kernel runs it
// with the 64 lanes of a wave and the series in LDS, a plain C++ program (g++,
// no HIP) with the one-lane policy (tests/mapquant_host_main.cpp).
#pragma once

#include <cmath>
#include <cstdint>

#include "mdfit_mapis.h"  // (mdfit_mappsis.h's host part and mdfit_mapadapt.h; the device core under hipcc)

namespace mdfit::mapquant {

// record layout (MDFIT_NMAPQUANT = 16 doubles per PMD sub-fit)
constexpr int kDMedian = 0, kDLo = 1, kDHi = 2, kDQ05 = 3, kDQ95 = 4, kDPAbove = 5, kQMedian = 6, kQLo = 7, kQHi = 8,
              kAMedian = 9, kCMedian = 10, kPhiMedian = 11, kKhat = 12, kEss = 13, kNWindow = 14, kFlags = 15;
// the result of one series (mdfit_weighted_order_stats: 8 doubles)
constexpr int kRMedian = 0, kRLo = 1, kRHi = 2, kRQ05 = 3, kRQ95 = 4, kRPAbove = 5, kRNWindow = 6, kROk = 7, kNRes = 8;
constexpr int kNSeries = 5;        // D_max, q, A, c, phi: the order of the values tap
constexpr double kScale = 4503599627370496.0;  // 2^52
constexpr int kNoIndex = nutssumm::kNoIndex;

using mappsis::sort_pairs;
using nutssumm::ns_inf;
using nutssumm::ns_nan;
using nutssumm::sort_len;
using nutssumm::window_before;

// the one-lane policy: mappsis' with the integer sum, the integer scan and the
// window's argmin
struct OneLane : mappsis::OneLane {
  MDFIT_NS_FN uint64_t usum(uint64_t v) const { return v; }
  // inclusive scan over the lanes on top of carry; carry becomes the total
  MDFIT_NS_FN uint64_t uscan(uint64_t v, uint64_t& carry) const {
    carry += v;
    return carry;
  }
};

// the work buffers of one series beside the weights: the sort's values and
// draw indices (sort_len(S) each) and the masses' prefix sums (S)
struct Work {
  double* sv;
  int* si;
  uint64_t* cum;
};

// the fixed-point weight of a draw: w in [0, 1] (anything else, a NaN
// included, counts as 0 here; weights_ok tells them apart)
MDFIT_NS_FN uint64_t fixed_weight(double w) { return (w > 0.0 && w <= 1.0) ? (uint64_t)std::rint(w * kScale) : 0u; }
MDFIT_NS_FN bool weight_ok(double w) { return w >= 0.0 && w <= 1.0; }

// a * c for c <= 100 without overflow, as (high, low 32 bits): lexicographic order is numeric order
struct Wide {
  uint64_t hi, lo;
};
MDFIT_NS_FN Wide times(uint64_t a, uint64_t c) {
  const uint64_t l = (a & 0xffffffffull) * c, h = (a >> 32) * c;
  Wide r;
  r.hi = h + (l >> 32);
  r.lo = l & 0xffffffffull;
  return r;
}
MDFIT_NS_FN bool wide_gt(Wide a, Wide b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }
MDFIT_NS_FN bool wide_ge(Wide a, Wide b) { return !wide_gt(b, a); }

// the first j in [from, S) with pc * (cum[j] - base) >= (strict: >) pk * K; S when there is none
MDFIT_NS_FN int first_mass(const uint64_t* cum, int from, int S, uint64_t base, uint64_t pc, uint64_t pk, uint64_t K,
                           bool strict) {
  const Wide need = times(K, pk);
  int lo = from, hi = S;  // the answer is in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const Wide got = times(cum[mid] - base, pc);
    if (strict ? wide_gt(got, need) : wide_ge(got, need)) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

struct Stats {
  double median, lo, hi, q05, q95, p_above, n_window;
  bool ok;
};

MDFIT_NS_FN Stats invalid_stats() {
  Stats r;
  r.median = r.lo = r.hi = r.q05 = r.q95 = r.p_above = r.n_window = ns_nan();
  r.ok = false;
  return r;
}

// The order statistics of one weighted series: value(t) is the value of draw
// t < S (the same at every call), wt[S] the weights (shared by the lanes,
// written behind a barrier).  Every lane calls it with the same arguments and
// gets the same result.  full: the interval, the two quantiles and the
// exceedance too (else the median alone; the other fields NaN).  Not ok -- all
// NaN -- when the weights' masses sum to 0 or a draw with mass is not finite.
// On return the lanes have passed a barrier behind their last read of wk.
template <class L, class V>
MDFIT_NS_FN Stats order_stats(const L& w, const double* wt, int S, const V& value, double d0, bool full,
                              const Work& wk) {
  const int lane = w.lane(), nl = w.nlanes();
  // 1. the keys: a draw without mass sorts last, whatever its value holds
  uint64_t ksum = 0u, above = 0u, bad = 0u;
  for (int t = lane; t < S; t += nl) {
    const uint64_t k = fixed_weight(wt[t]);
    const double v = value(t);
    if (k > 0u) {
      if (!std::isfinite(v)) bad += 1u;
      else if (v > d0) above += k;
    }
    ksum += k;
    wk.sv[t] = k > 0u ? v : ns_inf();
    wk.si[t] = t;
  }
  const uint64_t K = w.usum(ksum);
  bad = w.usum(bad);
  above = w.usum(above);
  if (K == 0u || bad > 0u) return invalid_stats();  // (wave-uniform; nothing of wk is read)
  // 2. ascending by (value, draw index); the masses' inclusive prefix sums in that order
  sort_pairs(w, wk.sv, wk.si, S);
  uint64_t carry = 0u;
  for (int base = 0; base < S; base += nl) {
    const int j = base + lane;
    const uint64_t c = w.uscan(j < S ? fixed_weight(wt[wk.si[j]]) : (uint64_t)0u, carry);
    if (j < S) wk.cum[j] = c;
  }
  w.sync();
  const uint64_t* cum = wk.cum;
  const double* v = wk.sv;
  Stats r = invalid_stats();
  r.ok = true;
  // 3. the median: the mean of the first draws to reach and to pass half the mass
  r.median = 0.5 * (v[first_mass(cum, 0, S, 0u, 2u, 1u, K, false)] + v[first_mass(cum, 0, S, 0u, 2u, 1u, K, true)]);
  if (full) {
    r.q05 = v[first_mass(cum, 0, S, 0u, 100u, 5u, K, false)];
    r.q95 = v[first_mass(cum, 0, S, 0u, 100u, 95u, K, false)];
    r.p_above = (double)above / (double)K;
    // 4. the narrowest window holding more than 68 % of the mass: lanes over its first draw
    double bw = ns_inf();
    int bi = kNoIndex;
    for (int i = lane; i < S; i += nl) {  // ascending i: only a strictly smaller width replaces
      const uint64_t before = i > 0 ? cum[i - 1] : (uint64_t)0u;
      if (cum[i] == before) break;  // (a draw without mass: so is every later one)
      const int j = first_mass(cum, i, S, before, 100u, 68u, K, true);
      if (j == S) break;  // (the mass from i on is too small: so it is from every later draw)
      const double wd = v[j] - v[i];
      if (bi == kNoIndex || wd < bw) {
        bw = wd;
        bi = i;
      }
    }
    int wi = bi;
    w.argmin(bw, wi);  // (window_before: the smaller width, else the smaller first draw; draw 0 always has a window)
    const int j = first_mass(cum, wi, S, wi > 0 ? cum[wi - 1] : (uint64_t)0u, 100u, 68u, K, true);
    r.lo = v[wi];
    r.hi = v[j];
    r.n_window = (double)(j - wi + 1);  // (draws with mass are a prefix of the order)
  }
  w.sync();  // (every lane has read wk; the next series overwrites it)
  return r;
}

// Host form on given values v[S] and weights w[S]: res[kNRes].  ok = 0 and NaN
// also when a weight is outside [0, 1] or NaN.  work: sort_len(S) doubles,
// sort_len(S) ints and S 64-bit words.
struct ArrayValues {
  const double* v;
  MDFIT_NS_FN double operator()(int t) const { return v[t]; }
};
MDFIT_NS_FN void stats_result(const Stats& s, double* res) {
  res[kRMedian] = s.median;
  res[kRLo] = s.lo;
  res[kRHi] = s.hi;
  res[kRQ05] = s.q05;
  res[kRQ95] = s.q95;
  res[kRPAbove] = s.p_above;
  res[kRNWindow] = s.n_window;
  res[kROk] = s.ok ? 1.0 : 0.0;
}
template <class L>
MDFIT_NS_FN void series_stats(const L& w, const double* v, const double* wt, int S, double d0, const Work& wk,
                              double* res) {
  const int lane = w.lane(), nl = w.nlanes();
  uint64_t badw = 0u;
  for (int t = lane; t < S; t += nl)
    if (!weight_ok(wt[t])) badw += 1u;
  badw = w.usum(badw);
  const Stats s = badw > 0u ? invalid_stats() : order_stats(w, wt, S, ArrayValues{v}, d0, true, wk);
  if (lane == 0) stats_result(s, res);
}
inline void series_stats_host(const double* v, const double* wt, int S, double d0, double* sv, int* si, uint64_t* cum,
                              double* res) {
  series_stats(OneLane{}, v, wt, S, d0, Work{sv, si, cum}, res);
}

// all-NaN record; flags: the free bits alone (mappsis::invalid_row's)
MDFIT_NS_FN void invalid_row(double* rec, unsigned free_mask) {
  for (int k = 0; k < kFlags; ++k) rec[k] = ns_nan();
  rec[kFlags] = (double)((free_mask & 15u) << 2);
}

// the value of series `ser` (D_max, q, A, c, phi) from a draw's f[4] = (q, A, c, phi)
MDFIT_NS_FN double series_value(int ser, const double f[4]) {
  return ser == 0 ? f[1] + f[2] : (ser == 1 ? f[0] : (ser == 2 ? f[1] : (ser == 3 ? f[2] : f[3])));
}

// the kernel's dynamic LDS in doubles: psis_weights' work buffer, whose part
// behind the S weights the sort overlays afterwards, and the prefix sums
MDFIT_NS_FN int work_len(int S) { return mappsis::work_len(S) + S; }

// the sort's buffers in psis_weights' work buffer buf (work_len(S) doubles):
// the values where its sorted values were, the indices where its were
MDFIT_NS_FN Work work_of(double* buf, int S) {
  Work wk;
  wk.sv = buf + S;
  wk.si = reinterpret_cast<int*>(wk.sv + sort_len(S) + mappsis::kMaxTail + 2 * mappsis::kMaxGrid);
  wk.cum = reinterpret_cast<uint64_t*>(buf + mappsis::work_len(S));
  return wk;
}

// One sub-fit's record from the normalised weights wt = buf[0..S) and the
// draws: draw(t, f) gives f[4] = (q, A, c, phi) of draw t, the same values at
// every call (psis_estimates' draws).  Every lane calls it; lane 0 writes rec.
// flags: the psis record's.  tap: [S][6] = D_max, q, A, c, phi, weight; or null.
template <class L, class G>
MDFIT_NS_FN void quant_row(const L& w, double* buf, int S, const G& draw, double d0, double khat, double flags,
                           double* rec, double* tap) {
  const int lane = w.lane(), nl = w.nlanes();
  const Work wk = work_of(buf, S);
  const double ess = mapadapt::weights_ess(w, buf, S);
#pragma unroll 1
  for (int ser = 0; ser < kNSeries; ++ser) {
    const Stats st = order_stats(
        w, buf, S,
        [&](int t) {
          double f[4];
          draw(t, f);
          return series_value(ser, f);
        },
        d0, ser < 2, wk);
    if (lane == 0) {
      if (ser == 0) {
        rec[kDMedian] = st.median;
        rec[kDLo] = st.lo;
        rec[kDHi] = st.hi;
        rec[kDQ05] = st.q05;
        rec[kDQ95] = st.q95;
        rec[kDPAbove] = st.p_above;
        rec[kNWindow] = st.n_window;
      } else if (ser == 1) {
        rec[kQMedian] = st.median;
        rec[kQLo] = st.lo;
        rec[kQHi] = st.hi;
      } else {
        rec[kAMedian + (ser - 2)] = st.median;
      }
    }
  }
  if (tap != nullptr) {
    for (int t = lane; t < S; t += nl) {
      double f[4];
      draw(t, f);
      tap[t * 6 + 0] = f[1] + f[2];
      tap[t * 6 + 1] = f[0];
      tap[t * 6 + 2] = f[1];
      tap[t * 6 + 3] = f[2];
      tap[t * 6 + 4] = f[3];
      tap[t * 6 + 5] = buf[t];
    }
  }
  if (lane == 0) {
    rec[kKhat] = khat;
    rec[kEss] = ess;
    rec[kFlags] = flags;
  }
}

}  // namespace mdfit::mapquant

#if defined(__HIPCC__)
namespace mdfit::mapquant {

using namespace mapis;

// the 64 lanes of a wave: PsisWave with the integer sum and scan and the window's argmin
struct QuantWave : PsisWave {
  __device__ __forceinline__ uint64_t usum(uint64_t v) const {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
  }
  __device__ __forceinline__ uint64_t uscan(uint64_t v, uint64_t& carry) const {
    const int lane = (int)threadIdx.x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t up = (uint64_t)__shfl_up((unsigned long long)v, o, 64);
      if (lane >= o) v += up;
    }
    const uint64_t got = carry + v;
    carry += (uint64_t)__shfl((unsigned long long)v, 63, 64);
    return got;
  }
  __device__ __forceinline__ void argmin(double& wd, int& i) const {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double ow = __shfl_xor(wd, o, 64);
      const int oi = __shfl_xor(i, o, 64);
      if (oi != kNoIndex && (i == kNoIndex || window_before(ow, oi, wd, i))) {
        wd = ow;
        i = oi;
      }
    }
  }
};

// One wave per taxon, its three PMD sub-fits one after another.  Phases 1-3
// are the core's, as map_psis_kernel runs them (proposals<true>,
// subfit_weights<kAdapt, false>): khat, ess, the flags and the weights are
// that kernel's bits.  Phase 4 is quant_row with the draws regenerated from
// the stream (mappsis::StreamDraws).  Dynamic LDS: work_len(S) doubles (30,208 B
// at S = 1024, 8,704 B at S = 256); static: 1,536 B.  Reads y, N, out and
// status only.  adapt: [T][3][4], optional; values: [T][3][S][6], optional.
template <bool kAdapt>
__global__ __launch_bounds__(64) void map_quant_kernel(const uint32_t* __restrict__ gy,
                                                       const uint32_t* __restrict__ gN,
                                                       const double* __restrict__ out,
                                                       const int32_t* __restrict__ status, int64_t n_taxa, int S,
                                                       uint64_t seed, int64_t index_base, double tau, double d0,
                                                       double* __restrict__ quant, double* __restrict__ values,
                                                       int adapt_rounds, double* __restrict__ adapt) {
  extern __shared__ double s_w[];
  __shared__ double s_y[kLD], s_N[kLD];
  __shared__ double s_par[4][kNPar];  // by diagnostic slot: 0, 2, 3 (1, the null fit's, unused)
  const int lane = threadIdx.x;
  const int64_t t = blockIdx.x;
  if (t >= n_taxa) return;
  double* va0 = values != nullptr ? values + t * 3 * (int64_t)S * 6 : nullptr;

  if (status[t] != MDFIT_OK) {  // wave-uniform: NaN statistics, flags 0
    if (lane < 3) invalid_row(quant + (t * 3 + lane) * MDFIT_NMAPQUANT, 0u);
    bad_status_fills<kAdapt>(va0, (int64_t)3 * S * 6, adapt, t);
    return;
  }
  load_counts(gy, gN, t, s_y, s_N);

  // ---- phase 1: the modes, g and H there, the held sets ----
  proposals<true>(gy, gN, out, t, s_par);
  __syncthreads();

  const QuantWave w;
  const uint64_t gtaxon = (uint64_t)(index_base + t);
  for (int s = 0; s < 3; ++s) {
    const int slot = s == 0 ? 0 : s + 1;  // the chain's sub-fit index: 0, 2, 3
    const double* P = s_par[slot];
    const unsigned mask = (unsigned)P[kPMask];
    double* rec = quant + (t * 3 + s) * MDFIT_NMAPQUANT;
    double* va = va0 != nullptr ? va0 + (int64_t)s * S * 6 : nullptr;
    if (P[kPValid] == 0.0) {  // (wave-uniform)
      if (lane == 0) invalid_row(rec, mask);
      if (va != nullptr) nan_fill(va, (int64_t)S * 6);
      if constexpr (kAdapt) adapt_row_nan(adapt, t, s);
      continue;
    }
    const Stream st = subfit_stream(seed, gtaxon, slot);
    const int lo = s == 2 ? kNHalf : 0, hi = s == 1 ? kNHalf : kNPos;
    // ---- phases 2-3: the draws, the smoothed weights, the rounds ----
    const SubfitWeights sw = subfit_weights<kAdapt, false>(w, true, lo, hi, s_par[slot], st, S, tau, adapt_rounds, s_y,
                                                           s_N, s_w, nullptr, nullptr);
    // ---- phase 4: the order statistics ----
    if (sw.ok) {
      unsigned fl = mappsis::kValidBit | (sw.khat <= tau ? mappsis::kReliableBit : 0u) | ((mask & 15u) << 2);
      if constexpr (kAdapt)
        if (sw.best > 0) fl |= mapadapt::kAdaptedBit;
      quant_row(w, s_w, S, mappsis::StreamDraws{P, st}, d0, sw.khat, (double)fl, rec, va);
    } else {
      if (lane == 0) invalid_row(rec, mask);
      if (va != nullptr) nan_fill(va, (int64_t)S * 6);
    }
    if constexpr (kAdapt) adapt_row(adapt, t, s, sw);
    __syncthreads();  // (the next sub-fit overwrites s_w)
  }
}

// mdfit_weighted_order_stats: one wave per series v[row][0..S), w[row][0..S)
__global__ __launch_bounds__(64) void weighted_order_stats_kernel(const double* __restrict__ v,
                                                                  const double* __restrict__ wt, int64_t n_series,
                                                                  int S, double d0, double* __restrict__ res) {
  extern __shared__ double s_w[];
  const int64_t row = blockIdx.x;
  if (row >= n_series) return;
  for (int x = threadIdx.x; x < S; x += 64) s_w[x] = wt[row * (int64_t)S + x];
  __syncthreads();
  series_stats(QuantWave{}, v + row * (int64_t)S, s_w, S, d0, work_of(s_w, S), res + row * kNRes);
}

}  // namespace mdfit::mapquant
#endif  // __HIPCC__
