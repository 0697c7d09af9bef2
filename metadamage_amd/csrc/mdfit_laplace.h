// mdfit_laplace.h — Laplace standard errors of the MAP modes (mdfit_map_laplace,
// DESIGN.md §3.7): one Hessian evaluation at the mode of each PMD sub-fit by
// the fit kernel's own objective code, the covariance of the coordinates that
// are not held on a box bound, and the delta method to (q, A, c, phi, D_max).
//
// The 4x4 linear algebra (laplace4) is plain C++ without lane intrinsics and
// also compiles for the host (tests/test_laplace.py builds it with g++ under
// the address and undefined-behaviour sanitizers); the kernel follows it under
// __HIPCC__.
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/mdfit.h"

#if defined(__HIPCC__)
#include "mdfit_model.h"
#define MDFIT_LAP_FN __host__ __device__ __forceinline__
#else
#define MDFIT_LAP_FN inline
#endif

namespace mdfit::laplace {

// fields of one Laplace record (MDFIT_NLAPLACE doubles)
enum { kQStd = 0, kAStd, kCStd, kPhiStd, kDmaxStd, kRhoAc, kSignif, kFlags };
constexpr int kValidBit = 16;  // flags: bits 0..3 coordinate j free, bit 4 valid

// The smallest pivot (Schur-complement diagonal L_jj^2) of the Jacobi-scaled
// Cholesky that still counts as information: the Hessian itself is only pinned
// to 1e-8 of its largest entry (test_objective_vs_oracle).
constexpr double kLaplacePivMin = 1e-8;

MDFIT_LAP_FN int lidx(int j, int m) {  // packed upper triangle, j <= m (mdfit::hidx)
  return j == 0 ? m : (j == 1 ? 3 + m : (j == 2 ? 5 + m : 9));
}

MDFIT_LAP_FN double rsqrt_pos(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return mdfit::rsqrt_nr(x);
#else
  return 1.0 / std::sqrt(x);
#endif
}

// sqrt(x), x >= 0 (device: x * rsqrt_nr(x), no IEEE sqrt sequence)
MDFIT_LAP_FN double sqrt_nonneg(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return x > 0.0 ? x * mdfit::rsqrt_nr(x) : 0.0;
#else
  return std::sqrt(x);
#endif
}

// Covariance C_u = D^-1/2 R^-1 D^-1/2 of the free coordinates, R = D^-1/2 H_ff
// D^-1/2 with D = diag(H_ff) (Jacobi scaling: the entries of H span 1e-12 to
// 1e7 in u), by the Cholesky R = L L', then C = L^-T L^-1.  H is the packed
// upper triangle (lidx), free_mask bit j set when coordinate j is free.  C is
// the full symmetric 4x4 (rows and columns of held coordinates 0).  Returns
// false -- C then unspecified -- when no coordinate is free, a free H_jj is not
// positive, or a pivot does not exceed kLaplacePivMin.
MDFIT_LAP_FN bool free_covariance(const double H[10], unsigned free_mask, double C[4][4]) {
  bool fr[4];
  double d[4];
  bool ok = (free_mask & 15u) != 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    fr[j] = (free_mask >> j) & 1u;
    const double hjj = H[lidx(j, j)];
    const bool pos = hjj > 0.0;
    ok = ok && (!fr[j] || pos);
    d[j] = (fr[j] && pos) ? rsqrt_pos(hjj) : 1.0;
  }
  // L: lower triangle of the scaled free block (held rows: identity)
  double L[4][4], iL[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int m = 0; m <= j; ++m) {
      double s;
      if (!fr[j] || !fr[m]) s = (j == m) ? 1.0 : 0.0;
      else s = H[lidx(m, j)] * d[j] * d[m];
#pragma unroll
      for (int p = 0; p < m; ++p) s -= L[j][p] * L[m][p];
      if (j == m) {
        const bool piv = s > kLaplacePivMin;  // (false for NaN)
        ok = ok && piv;
        const double sp = piv ? s : 1.0;
        iL[j] = rsqrt_pos(sp);
        L[j][j] = sp * iL[j];
      } else {
        L[j][m] = s * iL[m];
      }
    }
  }
  // M = L^-1 (lower triangular), column by column
  double M[4][4];
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
  // R^-1 = M' M, then the scaling back
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int m = j; m < 4; ++m) {
      double s = 0.0;
#pragma unroll
      for (int p = m; p < 4; ++p) s += M[p][j] * M[p][m];
      const double c = (fr[j] && fr[m]) ? s * d[j] * d[m] : 0.0;
      C[j][m] = c;
      C[m][j] = c;
    }
  }
  return ok;
}

// One sub-fit's Laplace record from its Hessian at the mode (packed upper
// triangle, d/du), the free mask, the Jacobian J = dtheta/du = (q(1-q),
// A(1-A), 1, delta) and D_max = A + c.  Held coordinates get std 0; an invalid
// sub-fit (free_covariance false) NaN statistics and a clear valid bit.
MDFIT_LAP_FN void laplace4(const double H[10], unsigned free_mask, const double J[4], double dmax,
                           double rec[MDFIT_NLAPLACE]) {
  double C[4][4];
  const bool ok = free_covariance(H, free_mask, C);
  const double nan = (double)NAN;
  if (!ok) {
#pragma unroll
    for (int i = 0; i < kFlags; ++i) rec[i] = nan;
    rec[kFlags] = (double)(free_mask & 15u);
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) rec[kQStd + j] = J[j] * sqrt_nonneg(C[j][j]);
  const double cAA = C[1][1], ccc = C[2][2], cAc = C[1][2];
  const double var = J[1] * J[1] * cAA + ccc + 2.0 * J[1] * cAc;
  const double sd = sqrt_nonneg(var > 0.0 ? var : 0.0);
  rec[kDmaxStd] = sd;
  const bool both = (free_mask & 2u) && (free_mask & 4u);
  rec[kRhoAc] = both ? cAc * rsqrt_pos(cAA * ccc) : nan;
  rec[kSignif] = sd > 0.0 ? dmax / sd : nan;
  rec[kFlags] = (double)((free_mask & 15u) | (unsigned)kValidBit);
}

}  // namespace mdfit::laplace

#if defined(__HIPCC__)
namespace mdfit {

// The mode of one sub-fit and the objective's g and H there, in the row layout
// of laplace_kernel below (lane = 16 row + k; rows 0-1 one all-position fit,
// row 2 a forward, row 3 a reverse one): the one evaluation behind
// mdfit_map_laplace and the proposals of the importance-sampled entries
// (mdfit_mapis.h), so the mode, g, H and the free set are the same bits in all
// of them.
struct ModeEval {
  double u[4];    // the mode in the unconstrained coordinates (logit q, logit A, c, log(phi - 2)), clamped
  Theta th;       // the constrained parameters there
  Eval e;         // g and H (the value and its rounding scale are not formed)
  unsigned mask;  // bit j: coordinate j is free by the optimiser's own binding rule (eps = kEpsBind[j])
};

// dg: the sub-fit's diagnostic slot of the record, (q, A, c, phi).  kPmd: the
// PMD objective; otherwise the null one, with A and c held (A = 0.5, c = 0).
// Lane 0 of a row resolves logit q, lane 1 logit A, lane 2 log(phi - 2) (two
// logarithms per lane instead of five), then the row shares them.
template <bool kPmd>
__device__ __forceinline__ void mode_eval(const uint32_t* __restrict__ gy, const uint32_t* __restrict__ gN,
                                          const double* __restrict__ dg, int64_t t, ModeEval& m) {
  const int row = (int)threadIdx.x >> 4, k = (int)threadIdx.x & 15;
  const double q = dg[0], A = kPmd ? dg[1] : 0.5, c = kPmd ? dg[2] : 0.0, phi = dg[3];
  const double x = k == 0 ? q : (k == 1 ? A : phi - 2.0);
  const double lx = flog(x), l1mx = flog1p(k < 2 ? -x : 0.0);
  const double v = lx - l1mx;  // logit(x) on lanes 0, 1; log(x) on lane 2
  m.u[0] = rowb<0>(v);
  m.u[1] = rowb<1>(v);
  m.u[2] = c;
  m.u[3] = rowb<2>(v);
#pragma unroll
  for (int j = 0; j < 4; ++j) m.u[j] = clampd(m.u[j], kULo[j], kUHi[j]);

  PointData pd;
  pd.pmd = kPmd ? 1 : 0;
  pd.valid = k < kNHalf;
  pd.k = pd.valid ? k : 0;
  const int col = pd.valid ? (row & 1) * kNHalf + k : 0;
  pd.y = pd.valid ? (double)gy[t * kLD + col] : 0.0;
  pd.N = pd.valid ? (double)gN[t * kLD + col] : 0.0;
  m.th = make_theta<16>(kPmd, m.u);
  double acc[kNAcc];
#pragma unroll
  for (int j = 0; j < kNAcc; ++j) acc[j] = 0.0;
  point_accum<true>(pd, m.th, acc);
#pragma unroll
  for (int j = 2; j < kNAcc; ++j) {  // (not the value and its rounding scale: only g and H are used)
    const double s16 = gsum<16>(acc[j]);
    const double s32 = s16 + xrow(s16);  // the all-position fit: both halves
    acc[j] = row < 2 ? s32 : s16;
  }
  acc[0] = acc[1] = 0.0;
  finish_eval(kPmd, m.th, acc, m.e);
  // held coordinates leave the system
  bool fr[4];
  double dbind[4];
  free_set(kPmd, m.u, m.e.g, m.e.H, INFINITY, fr, dbind);
  m.mask = (fr[0] ? 1u : 0u) | (fr[1] ? 2u : 0u) | (fr[2] ? 4u : 0u) | (fr[3] ? 8u : 0u);
}

// One wave per taxon; the three PMD sub-fits share it: rows 0-1 (lanes 0-31)
// the all-position fit (diag sub-fit 0; row 0 z > 0, row 1 z < 0, summed as
// objective_group<kAll> does), row 2 the forward fit (diag sub-fit 2), row 3
// the reverse fit (diag sub-fit 3); lane 15 of every row is the pad that holds
// lg3(phi) (point_accum<true>).  60 of the 64 lanes hold a point.
#ifndef MDFIT_NO_HELPER_KERNELS  // (a second unit of libmdfit.so includes this header for the templates alone)
__global__ __launch_bounds__(64) void laplace_kernel(const uint32_t* __restrict__ gy,
                                                     const uint32_t* __restrict__ gN,
                                                     const double* __restrict__ out,
                                                     const int32_t* __restrict__ status, int64_t n_taxa,
                                                     double* __restrict__ lap, double* __restrict__ gh,
                                                     double* __restrict__ uo) {
  const int lane = threadIdx.x;
  const int64_t t = blockIdx.x;
  if (t >= n_taxa) return;
  const int row = lane >> 4, k = lane & 15;
  const int sub = row < 2 ? 0 : row - 1;  // index in lap / gh: all, forward, reverse
  const bool writer = k == 0 && row != 1;

  if (status[t] != MDFIT_OK) {  // wave-uniform: NaN statistics, flags 0
    if (writer) {
      double* r = lap + (t * 3 + sub) * MDFIT_NLAPLACE;
      for (int i = 0; i < laplace::kFlags; ++i) r[i] = NAN;
      r[laplace::kFlags] = 0.0;
      if (gh != nullptr)
        for (int i = 0; i < 20; ++i) gh[(t * 3 + sub) * 20 + i] = NAN;
      if (uo != nullptr)
        for (int i = 0; i < 4; ++i) uo[(t * 3 + sub) * 4 + i] = NAN;
    }
    return;
  }

  ModeEval me;
  mode_eval<true>(gy, gN, out + t * MDFIT_NOUT + MDFIT_F_DIAG + MDFIT_DIAG_STRIDE * (row < 2 ? 0 : row), t, me);
  const Theta& th = me.th;
  const Eval& e = me.e;
  const double J[4] = {th.q * th.omq, th.JA, 1.0, th.delta};
  double rec[MDFIT_NLAPLACE];
  laplace::laplace4(e.H, me.mask, J, th.A + th.c, rec);

  if (writer) {
    double* r = lap + (t * 3 + sub) * MDFIT_NLAPLACE;
#pragma unroll
    for (int i = 0; i < MDFIT_NLAPLACE; ++i) r[i] = rec[i];
    if (uo != nullptr) {
#pragma unroll
      for (int j = 0; j < 4; ++j) uo[(t * 3 + sub) * 4 + j] = me.u[j];
    }
    if (gh != nullptr) {
      double* o = gh + (t * 3 + sub) * 20;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[j] = e.g[j];
#pragma unroll
        for (int m = 0; m < 4; ++m) o[4 + 4 * j + m] = e.H[j <= m ? hidx(j, m) : hidx(m, j)];
      }
    }
  }
}
#endif  // MDFIT_NO_HELPER_KERNELS

}  // namespace mdfit
#endif  // __HIPCC__
