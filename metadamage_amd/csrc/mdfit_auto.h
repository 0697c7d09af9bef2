// mdfit_auto.h — MDFIT-AUTO v1 (mdfit_auto_route): which taxa
// of a finished MAP call the importance sampling of mdfit_map_psis /
// mdfit_map_waic settles and which need the sampler, and the record of a
// settled taxon.  The rule reads three things per taxon -- status[t], the flags
// of the three rows of its psis record and the flags of row 6 of its waic
// record -- and the composition copies nine fields; neither does any
// arithmetic, so the device kernel (mdfit.hip: one thread per taxon) and a plain
// C++ program (tests/auto_host_main.cpp, g++) give the same bits.
// MDFIT-AUTO v1.1 (mdfit_auto_route_pred) below them: the rule
// with the pred record's bit and the composition with the predictive columns
// and prediction floats (tests/auto_pred_host_main.cpp).
#pragma once

#include <cstdint>

#include "../../include/mdfit.h"

#if defined(__HIPCC__)
#define MDFIT_AUTO_FN __host__ __device__ __forceinline__
#else
#define MDFIT_AUTO_FN inline
#endif

namespace mdfit::autoroute {

// route bits
constexpr int kWaicUnreliable = 1;  // row 6 of the waic record lacks bit 1
constexpr int kPsisUnreliable = 2;  // some psis row 0..2 lacks bit 0 or bit 1
constexpr int kFitFailed = 4;       // status MDFIT_MAXITER or MDFIT_NONFINITE
constexpr int kInvalid = 8;         // status MDFIT_INVALID: not sampled, the NaN record left alone
constexpr int kSampleMask = kWaicUnreliable | kPsisUnreliable | kFitFailed;

constexpr int kPsisFlags = MDFIT_NMAPPSIS - 1, kWaicFlags = MDFIT_NMAPWAIC - 1, kWaicCompareRow = 6;
constexpr int kPsisQMean = 0, kPsisPhiMean = 3, kPsisDmaxMean = 4;

// a record's flags field (an integer stored as double); anything that is no
// such integer -- NaN, negative, 2^32 or more -- has no bit set
MDFIT_AUTO_FN unsigned flag_bits(double f) { return f >= 0.0 && f < 4294967296.0 ? (unsigned)f : 0u; }

// route of one taxon: psis its [3][MDFIT_NMAPPSIS], waic its [7][MDFIT_NMAPWAIC]
MDFIT_AUTO_FN int route_of(int32_t status, const double* psis, const double* waic) {
  if (status == MDFIT_INVALID) return kInvalid;
  int r = 0;
  if ((flag_bits(waic[kWaicCompareRow * MDFIT_NMAPWAIC + kWaicFlags]) & 2u) == 0u) r |= kWaicUnreliable;
  for (int row = 0; row < 3; ++row)
    if ((flag_bits(psis[row * MDFIT_NMAPPSIS + kPsisFlags]) & 3u) != 3u) r |= kPsisUnreliable;
  if (status == MDFIT_MAXITER || status == MDFIT_NONFINITE) r |= kFitFailed;
  return r;
}

// the record of a taxon with route 0: the nine columns that are posterior
// statistics in the reference's record take the importance-sampled values; the
// predictive columns (D_max, its HPDI, D_max_forward / _reverse), the sums, the
// noise and the diagnostic slots stay the MAP call's
MDFIT_AUTO_FN void compose(double* rec, const double* psis, const double* waic) {
  rec[MDFIT_F_Q_MEAN] = psis[0 * MDFIT_NMAPPSIS + kPsisQMean];
  rec[MDFIT_F_CONCENTRATION_MEAN] = psis[0 * MDFIT_NMAPPSIS + kPsisPhiMean];
  rec[MDFIT_F_D_MAX_MARGINALIZED_MEAN] = psis[0 * MDFIT_NMAPPSIS + kPsisDmaxMean];
  rec[MDFIT_F_Q_MEAN_FORWARD] = psis[1 * MDFIT_NMAPPSIS + kPsisQMean];
  rec[MDFIT_F_Q_MEAN_REVERSE] = psis[2 * MDFIT_NMAPPSIS + kPsisQMean];
  const double* cmp = waic + kWaicCompareRow * MDFIT_NMAPWAIC;
  rec[MDFIT_F_N_SIGMA] = cmp[0];
  rec[MDFIT_F_N_SIGMA_FORWARD] = cmp[1];
  rec[MDFIT_F_N_SIGMA_REVERSE] = cmp[2];
  rec[MDFIT_F_ASYMMETRY] = cmp[3];
}

// one taxon of mdfit_auto_route: writes route[t], composes out's row t when it is 0
MDFIT_AUTO_FN void route_one(int64_t t, const int32_t* status, const double* psis, const double* waic, double* out,
                             int32_t* route) {
  const double* p = psis + t * (3 * MDFIT_NMAPPSIS);
  const double* w = waic + t * (7 * MDFIT_NMAPWAIC);
  const int r = route_of(status[t], p, w);
  route[t] = r;
  if (r == 0) compose(out + t * MDFIT_NOUT, p, w);
}

// ---- MDFIT-AUTO v1.1 (mdfit_auto_route_pred): the rule also
// reads the flags and n_noncount of the taxon's mdfit_map_pred_adapt record, and
// a settled taxon's five predictive columns and 90 prediction floats take the
// importance-weighted posterior predictive.  Still no arithmetic.
constexpr int kPredUnreliable = 16;  // the pred record lacks bit 1, or counts a job made NaN by a draw that is no count
constexpr int kSamplePredMask = kSampleMask | kPredUnreliable;
constexpr int kPredFlags = MDFIT_NMAPPRED - 1, kPredNNonCount = MDFIT_NMAPPRED - 2;
constexpr int kNPredFloats = MDFIT_NPRED * 30;

// route of one taxon: route_of and the pred record's bit (prec its [MDFIT_NMAPPRED])
MDFIT_AUTO_FN int route_pred_of(int32_t status, const double* psis, const double* waic, const double* prec) {
  if (status == MDFIT_INVALID) return kInvalid;
  int r = route_of(status, psis, waic);
  if ((flag_bits(prec[kPredFlags]) & 2u) == 0u || prec[kPredNNonCount] != 0.0) r |= kPredUnreliable;
  return r;
}

// the record of a taxon with route 0: compose()'s nine columns, the five
// predictive columns <- prec[0..4] and, with pred non-NULL, its 90 floats <- ppred's
MDFIT_AUTO_FN void compose_pred(double* rec, float* pred, const double* psis, const double* waic, const double* prec,
                                const float* ppred) {
  compose(rec, psis, waic);
  rec[MDFIT_F_D_MAX] = prec[0];
  rec[MDFIT_F_D_MAX_LOWER_HPDI] = prec[1];
  rec[MDFIT_F_D_MAX_UPPER_HPDI] = prec[2];
  rec[MDFIT_F_D_MAX_FORWARD] = prec[3];
  rec[MDFIT_F_D_MAX_REVERSE] = prec[4];
  if (pred != nullptr)
    for (int x = 0; x < kNPredFloats; ++x) pred[x] = ppred[x];
}

// one taxon of mdfit_auto_route_pred
MDFIT_AUTO_FN void route_pred_one(int64_t t, const int32_t* status, const double* psis, const double* waic,
                                  const double* prec, const float* ppred, double* out, float* pred, int32_t* route) {
  const double* p = psis + t * (3 * MDFIT_NMAPPSIS);
  const double* w = waic + t * (7 * MDFIT_NMAPWAIC);
  const double* q = prec + t * MDFIT_NMAPPRED;
  const int r = route_pred_of(status[t], p, w, q);
  route[t] = r;
  if (r == 0)
    compose_pred(out + t * MDFIT_NOUT, pred != nullptr ? pred + t * kNPredFloats : nullptr, p, w, q,
                 ppred + t * kNPredFloats);
}

}  // namespace mdfit::autoroute
