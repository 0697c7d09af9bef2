// Stand-in for <hip/hip_runtime.h> on the include path of the host build of
// csrc/mdfit_special.h (tests/special_host_main.cpp): plain C++ for the few
// device names that header uses, so that the unmodified header compiles with
// g++ -ffp-contract=off and computes with the device's arithmetic wherever the
// device's is IEEE (every fusion in the header is an explicit fma).  The one
// difference is the reciprocal seed: 1.0 / x here, v_rcp_f64 (~2^-25) there.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#define __device__
#define __host__
#define __constant__
#define __global__
#define __forceinline__ inline

using std::fma;
using std::fmax;
using std::fmin;
using std::rint;

struct double2 {
  double x, y;
};

inline int __double2hiint(double x) {
  uint64_t b;
  std::memcpy(&b, &x, 8);
  return (int)(uint32_t)(b >> 32);
}
inline int __double2loint(double x) {
  uint64_t b;
  std::memcpy(&b, &x, 8);
  return (int)(uint32_t)b;
}
inline double __hiloint2double(int hi, int lo) {
  const uint64_t b = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
  double x;
  std::memcpy(&x, &b, 8);
  return x;
}

namespace mdfit_shim {
// v_frexp_mant_f64 / v_frexp_exp_i32_f64: mantissa in [0.5, 1) (subnormals
// normalised); 0, inf and NaN pass through with exponent 0
inline double frexp_mant(double x) {
  int e;
  return std::isfinite(x) ? std::frexp(x, &e) : x;
}
inline int frexp_exp(double x) {
  int e = 0;
  if (std::isfinite(x) && x != 0.0) (void)std::frexp(x, &e);
  return e;
}
}  // namespace mdfit_shim
#define __builtin_amdgcn_frexp_mant(x) mdfit_shim::frexp_mant(x)
#define __builtin_amdgcn_frexp_exp(x) mdfit_shim::frexp_exp(x)
// v_ldexp_f64: one rounding (to nearest even) into the subnormal range
#define __builtin_amdgcn_ldexp(x, e) std::ldexp((x), (e))
#define __builtin_amdgcn_rcp(x) (1.0 / (x))
