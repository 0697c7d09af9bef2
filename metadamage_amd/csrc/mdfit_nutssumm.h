// mdfit_nutssumm.h — MDFIT-SUMM v1: posterior summary of one
// chain's draws: the standard deviations of q, A, c, phi and D_max, the median
// and 68 % highest-posterior-density interval of D_max, q and phi (numpyro's
// hpdi: the narrowest window of int(0.68 S) + 1 sorted draws, the lowest index
// among equals), the A-c correlation and mean(D_max) / std(D_max).
//
// The arithmetic is written once over a `lanes` policy, as mdfit_nutsdiag.h:
// the summary kernel (mdfit_nuts.hip) runs it with the 64 lanes of a wave over
// the sample index t and the series being sorted in LDS; a plain C++ program
// (g++, no HIP) runs it with the one-lane policy below
// (tests/nutssumm_host_main.cpp).  Every sum is a per-lane strided partial sum
// in ascending t followed by the policy's cross-lane reduction, so a record
// depends on the policy alone, not on the grid.  The order statistics are
// selections and single subtractions of draws: they do not depend on the
// policy, whose sort() may be the network below or any other (the kernel sorts
// 513..1024 draws in registers).
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>

#include "../../include/mdfit.h"

#if defined(__HIPCC__)
#define MDFIT_NS_FN __host__ __device__ __forceinline__
#else
#define MDFIT_NS_FN inline
#endif

namespace mdfit::nutssumm {

constexpr int kNSeries = 5;  // q, A, c, phi, D_max
// record layout (MDFIT_NNUTSSUMM = 16 doubles per sub-fit)
constexpr int kStd = 0, kDmaxMean = 5, kDmaxMedian = 6, kDmaxLo = 7, kDmaxHi = 8, kQMedian = 9, kQLo = 10, kQHi = 11,
              kPhiMedian = 12, kRhoAc = 13, kSignificance = 14, kFlags = 15;
constexpr double kValid = 1.0;  // flags bit 0
constexpr int kNoIndex = 0x7fffffff;

template <class L>
MDFIT_NS_FN void sort_series(const L& w, double* v, int S);

// the one-lane policy: sequential sums in index order
struct OneLane {
  MDFIT_NS_FN int lane() const { return 0; }
  MDFIT_NS_FN int nlanes() const { return 1; }
  MDFIT_NS_FN double sum(double v) const { return v; }
  MDFIT_NS_FN void argmin(double& w, int& i) const { (void)w, (void)i; }
  MDFIT_NS_FN void sort(double* v, int S) const { sort_series(*this, v, S); }
  MDFIT_NS_FN void sync() const {}
};

MDFIT_NS_FN double ns_nan() { return std::nan(""); }
MDFIT_NS_FN double ns_inf() { return std::numeric_limits<double>::infinity(); }

// the rule that combines two (width, index) candidates of the narrowest window:
// the smaller width, else the smaller index (np.argmin's first minimum)
MDFIT_NS_FN bool window_before(double wa, int ia, double wb, int ib) { return wa < wb || (wa == wb && ia < ib); }

// the sort buffer's length for S draws: S rounded up to a power of two
MDFIT_NS_FN int sort_len(int S) {
  int m = 2;
  while (m < S) m <<= 1;
  return m;
}

// Ascending bitonic sort of v[0..S) (finite), v holding sort_len(S) doubles:
// the network of the post kernel's lds_sort_u32, over compare-exchange pairs;
// the padding is +inf and ends beyond index S - 1.  The caller's writes of
// v[0..S) need no barrier of their own before the call.  A policy's sort() is
// this or anything that leaves the same ascending v[0..S) (a sort's result is
// unique up to the order of equal values).
template <class L>
MDFIT_NS_FN void sort_series(const L& w, double* v, int S) {
  const int lane = w.lane(), nl = w.nlanes();
  const int m = sort_len(S);
  for (int j = S + lane; j < m; j += nl) v[j] = ns_inf();
  w.sync();
  for (int k = 2; k <= m; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = lane; p < (m >> 1); p += nl) {
        const int x = ((p & ~(j - 1)) << 1) | (p & (j - 1)), y = x | j;  // the p-th pair of stride j
        const double a = v[x], b = v[y];
        const bool up = (x & k) == 0;
        if ((a > b) == up) {
          v[x] = b;
          v[y] = a;
        }
      }
      w.sync();
    }
  }
}

struct OrderStats {
  double median, lo, hi;
};

// median and 68 % HPDI of the sorted v[0..S); every lane gets the same result
template <class L>
MDFIT_NS_FN OrderStats order_stats(const L& w, const double* v, int S) {
  const int lane = w.lane(), nl = w.nlanes();
  OrderStats r;
  r.median = 0.5 * (v[(S - 1) / 2] + v[S / 2]);
  const int len = (int)(0.68 * (double)S);  // Python's int(0.68 * S)
  const int n = S - len;                    // windows [i, i + len], n >= 1
  double bw = ns_inf();
  int bi = kNoIndex;  // (a lane without a window: loses to every window)
  if (lane < n) {
    bw = v[lane + len] - v[lane];
    bi = lane;
  }
  for (int i = lane + nl; i < n; i += nl) {  // ascending i: only a strictly smaller width replaces
    const double wd = v[i + len] - v[i];
    if (wd < bw) {
      bw = wd;
      bi = i;
    }
  }
  w.argmin(bw, bi);
  r.lo = v[bi];
  r.hi = v[bi + len];
  return r;
}

// all-NaN record with flags 0
MDFIT_NS_FN void invalid_row(double* rec) {
  for (int k = 0; k < kFlags; ++k) rec[k] = ns_nan();
  rec[kFlags] = 0.0;
}

// One sub-fit's record from its draws x[S][4] = (q, A, c, phi), 32-byte
// aligned; S in [2, 4096]; pmd selects D_max = A + c (else q); buf holds
// sort_len(S) doubles shared by the policy's lanes.  Every lane of the policy
// calls it with the same arguments; lane 0 writes rec.
template <class L>
MDFIT_NS_FN void summary_row(const L& w, const double* x_, int S, bool pmd, double chain_status, double* buf,
                             double* rec) {
  const int lane = w.lane(), nl = w.nlanes();
  if (!(chain_status == 0.0)) {
    if (lane == 0) invalid_row(rec);
    return;
  }
  const double* x = (const double*)__builtin_assume_aligned(x_, 32);
  // one pass over whole draws: the moments of the five series shifted by the
  // first draw (a constant series gives exactly 0, a large common offset
  // cancels before anything is rounded to its magnitude), the finiteness of
  // every draw, and the D_max series into the sort buffer
  const double q0 = x[0], A0 = x[1], c0 = x[2], p0 = x[3];
  const double D0 = pmd ? A0 + c0 : q0;
  double s1[kNSeries] = {0.0, 0.0, 0.0, 0.0, 0.0}, s2[kNSeries] = {0.0, 0.0, 0.0, 0.0, 0.0};
  double sAc = 0.0, bad = 0.0;
  for (int t = lane; t < S; t += nl) {
    const double q = x[4 * t], A = x[4 * t + 1], c = x[4 * t + 2], p = x[4 * t + 3];
    if (!(std::isfinite(q) && std::isfinite(A) && std::isfinite(c) && std::isfinite(p))) bad = 1.0;
    const double D = pmd ? A + c : q;
    if (pmd) buf[t] = D;
    const double d[kNSeries] = {q - q0, A - A0, c - c0, p - p0, D - D0};
    for (int s = 0; s < kNSeries; ++s) {
      s1[s] += d[s];
      s2[s] = std::fma(d[s], d[s], s2[s]);
    }
    sAc = std::fma(d[1], d[2], sAc);
  }
  if (w.sum(bad) > 0.0) {  // (before any sort: the network orders finite values)
    if (lane == 0) invalid_row(rec);
    return;
  }
  double css[kNSeries], sd[kNSeries];
  for (int s = 0; s < kNSeries; ++s) {
    s1[s] = w.sum(s1[s]);
    s2[s] = w.sum(s2[s]);
    css[s] = s2[s] - s1[s] * s1[s] / S;
    sd[s] = std::sqrt((css[s] > 0.0 ? css[s] : 0.0) / (S - 1));
  }
  sAc = w.sum(sAc);
  const double D_mean = D0 + s1[4] / S;
  double rho = ns_nan();
  if (css[1] > 0.0 && css[2] > 0.0) rho = (sAc - s1[1] * s1[2] / S) / std::sqrt(css[1] * css[2]);
  // the order statistics: D_max (a PMD sub-fit's; a null one's are its q's),
  // then q, then phi, each sorted in the one buffer
  OrderStats oD{}, oq{}, op{};
  if (pmd) {
    w.sort(buf, S);
    oD = order_stats(w, buf, S);
    w.sync();  // (every lane has read its windows; the next series overwrites buf)
  }
  for (int t = lane; t < S; t += nl) buf[t] = x[4 * t];
  w.sort(buf, S);
  oq = order_stats(w, buf, S);
  w.sync();
  if (!pmd) oD = oq;
  for (int t = lane; t < S; t += nl) buf[t] = x[4 * t + 3];
  w.sort(buf, S);
  op = order_stats(w, buf, S);
  if (lane == 0) {
    for (int s = 0; s < kNSeries; ++s) rec[kStd + s] = sd[s];
    rec[kDmaxMean] = D_mean;
    rec[kDmaxMedian] = oD.median;
    rec[kDmaxLo] = oD.lo;
    rec[kDmaxHi] = oD.hi;
    rec[kQMedian] = oq.median;
    rec[kQLo] = oq.lo;
    rec[kQHi] = oq.hi;
    rec[kPhiMedian] = op.median;
    rec[kRhoAc] = rho;
    rec[kSignificance] = sd[4] > 0.0 ? D_mean / sd[4] : ns_nan();
    rec[kFlags] = kValid;
  }
}

// Host form: work holds sort_len(S) doubles.
inline void summary_row_host(const double* x, int S, bool pmd, double chain_status, double* work, double* rec) {
  summary_row(OneLane{}, x, S, pmd, chain_status, work, rec);
}

}  // namespace mdfit::nutssumm
