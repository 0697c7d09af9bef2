// Stand-in for <hip/hip_runtime.h> on the include path of the host build of
// csrc/mdfit_model.h (tests/pad_neutral_host_main.cpp): tests/host_shim's
// plain-C++ names for csrc/mdfit_special.h, and a replay of the cross-lane
// moves that the point evaluation uses, so that the unmodified header runs its
// row-collective code lane by lane.
//
// The program evaluates the 32 lanes of a slot twice.  In the first pass a
// cross-lane move records the value its lane passes in (per lane, in call
// order) and returns it unchanged; in the second it returns the value that the
// source lane recorded at the same call.  That is the device's result as long
// as every lane makes the same sequence of calls (the callers' conditions are
// wave-uniform) and no recorded value depends on an earlier move's result --
// true of point_accum: it broadcasts and exchanges lg3 triples of per-lane
// arguments.
#pragma once

#include "../../host_shim/hip/hip_runtime.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using std::exp;
using std::fabs;
using std::isfinite;
using std::isnan;
using std::sqrt;

namespace mdfit_shim {
struct Idx {
  unsigned x;
};
struct Lanes {
  int pass = 0;
  int seq[64] = {};
  std::vector<int> rec[64];
};
inline Lanes& lanes() {
  static Lanes l;
  return l;
}
inline Idx& thread_idx() {
  static Idx i{0};
  return i;
}
// one move of a 32-bit value: record (pass 0) or fetch the source lane's (pass 1)
inline int move(int v, int src_lane) {
  Lanes& l = lanes();
  const int lane = (int)thread_idx().x;
  const int k = l.seq[lane]++;
  if (l.pass == 0) {
    if ((int)l.rec[lane].size() <= k) l.rec[lane].resize((size_t)k + 1);
    l.rec[lane][(size_t)k] = v;
    return v;
  }
  if ((int)l.rec[src_lane].size() <= k) {
    std::fprintf(stderr, "lane %d read call %d of lane %d, which made fewer calls\n", lane, k, src_lane);
    std::abort();
  }
  return l.rec[src_lane][(size_t)k];
}
inline int mov_dpp(int v, int ctrl) {
  const int lane = (int)thread_idx().x;
  if (ctrl < 0x150 || ctrl > 0x15F) {  // row_newbcast only: what point_accum uses
    std::fprintf(stderr, "DPP control 0x%x is not replayed\n", ctrl);
    std::abort();
  }
  return move(v, (lane & ~15) + (ctrl - 0x150));
}
struct Pair {
  unsigned v[2];
  unsigned operator[](int i) const { return v[i]; }
};
// v_permlane16_swap with one register as both operands: the odd rows of the
// first result and the even rows of the second hold the value 16 lanes away
inline Pair permlane16_swap(unsigned v) {
  const int lane = (int)thread_idx().x;
  const unsigned o = (unsigned)move((int)v, lane ^ 16);
  const bool odd = (lane & 16) != 0;
  return odd ? Pair{{o, v}} : Pair{{v, o}};
}
[[noreturn]] inline void not_replayed(const char* what) {
  std::fprintf(stderr, "%s is not replayed by this host build\n", what);
  std::abort();
}
inline double rsq(double x) { return 1.0 / std::sqrt(x); }
}  // namespace mdfit_shim

#define threadIdx (mdfit_shim::thread_idx())
#define __builtin_amdgcn_mov_dpp(v, ctrl, rm, bm, bc) mdfit_shim::mov_dpp((v), (ctrl))
#define __builtin_amdgcn_permlane16_swap(a, b, fi, bc) mdfit_shim::permlane16_swap((a))
#define __builtin_amdgcn_rsq(x) mdfit_shim::rsq(x)

// wave-collective operations outside the point evaluation: declared so that
// the header compiles; calling one ends the program
template <class T>
inline T __shfl_xor(T, int, int) {
  mdfit_shim::not_replayed("__shfl_xor");
}
template <class T>
inline T __shfl(T, int, int) {
  mdfit_shim::not_replayed("__shfl");
}
inline bool __any(bool) { mdfit_shim::not_replayed("__any"); }
inline unsigned long long __ballot(bool) { mdfit_shim::not_replayed("__ballot"); }
inline int __ffsll(unsigned long long) { mdfit_shim::not_replayed("__ffsll"); }
inline void __syncthreads() { mdfit_shim::not_replayed("__syncthreads"); }
