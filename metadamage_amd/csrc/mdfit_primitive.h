// mdfit_primitive.h -- one primitive of mdfit_special.h by its selector (enum
// mdfit_primitive_id, include/mdfit.h): the body of mdfit_primitive's kernel
// and of the host build tests/special_host_main.cpp, so that both evaluate the
// same expressions.
#pragma once

#include "../../include/mdfit.h"
#include "mdfit_special.h"

namespace mdfit {

__device__ __forceinline__ double primitive_eval(int which, double x, double x2) {
  switch (which) {
    case MDFIT_P_RCP: return rcp(x);
    case MDFIT_P_RCP1: return rcp1(x);
    case MDFIT_P_FLOG: return flog(x);
    case MDFIT_P_FLOG_T: return flog_t<false>(x);
    case MDFIT_P_FLOG_T_ZERO: return flog_t<true>(x);
    case MDFIT_P_FLOG1P: return flog1p(x);
    case MDFIT_P_FEXP: return fexp(x);
    case MDFIT_P_FEXP_T: return fexp_t(x);
    case MDFIT_P_LG3_L: return lg3<true, false>(x).l;
    case MDFIT_P_LG3_P: return lg3<true, false>(x).p;
    case MDFIT_P_LG3_Q: return lg3<true, false>(x).q;
    case MDFIT_P_LG3_FAST_L: return lg3<false, true>(x).l;
    case MDFIT_P_LG3_FAST_P: return lg3<false, true>(x).p;
    case MDFIT_P_STIRLING_REM: return stirling_rem(x);
    case MDFIT_P_LGDIFF: return lgdiff(x, x2);
    case MDFIT_P_LRISE: return lrise(x, x2);
    default: return NAN;
  }
}

}  // namespace mdfit
