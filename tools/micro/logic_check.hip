// Development check: the Newton logic with its arithmetic pinned (contraction
// off, explicit fma) and free_set's binding test without short-circuit behind a
// wave-uniform guard -- finish_eval, free_set, chol4, newton_dir<8> /
// newton_dir<16> -- against the forms they replaced
// (old_logic.h), bit for bit, on random systems replicated over G-lane groups:
// mostly indefinite H, both models, want_nc on and off, u near both bounds.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/micro/logic_check.hip -o tools/micro/logic_check
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include "../../metadamage_amd/csrc/mdfit_model.h"
namespace mdfit {
#include "old_logic.h"
}
using namespace mdfit;

__device__ double rnd(uint64_t& s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(s >> 11) * 0x1.0p-53 * 2.0 - 1.0;
}

__device__ bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b); }

// bad[0]: lanes with any difference; bad[1..4]: by piece (finish_eval, free_set, chol4, newton_dir)
template <int G>
__global__ void k(int n, unsigned long long* bad, unsigned long long* tot) {
  const int grp = (blockIdx.x * 64 + threadIdx.x) / G;
  if (grp >= n) return;  // (never: the grid is exactly n groups)
  uint64_t s = 0x9E3779B97F4A7C15ull * (grp + 1);
  double H[10], g[4], u[4];
  for (int j = 0; j < 10; ++j) H[j] = rnd(s) * pow(10.0, 4.0 * rnd(s));
  for (int j = 0; j < 4; ++j) {
    g[j] = rnd(s) * (rnd(s) > 0.5 ? 1e-8 : 10.0);
    const double where = rnd(s);
    // a third at / next to the lower bound, a third at the upper, a third inside
    const double off = fabs(rnd(s)) * (rnd(s) > 0.0 ? 2e-3 : 1e-5);
    u[j] = where < -0.33 ? kULo[j] + (rnd(s) > 0.5 ? 0.0 : off)
                         : (where > 0.33 ? kUHi[j] - (rnd(s) > 0.5 ? 0.0 : off) : clampd(rnd(s) * 3.0, kULo[j], kUHi[j]));
  }
  if (rnd(s) > 0.6) {  // a positive definite H now and then (the common case of the kernel)
    for (int j = 0; j < 10; ++j) H[j] *= 1e-3;
    for (int j = 0; j < 4; ++j) H[hidx(j, j)] = 1.0 + fabs(rnd(s)) * 10.0;
  }
  const bool pmd = rnd(s) > -0.2;
  const bool nc = rnd(s) > 0.5;
  const double w = rnd(s) > 0.0 ? 1.0 : 1e-4 * fabs(rnd(s));
  bool ok_fe = true, ok_fs = true, ok_ch = true, ok_nd = true;
  {  // finish_eval on random sums at theta(u)
    double us[4], acc[kNAcc];
    for (int j = 0; j < 4; ++j) us[j] = clampd(rnd(s) * 4.0, kULo[j], kUHi[j]);
    for (int j = 0; j < kNAcc; ++j) acc[j] = rnd(s) * pow(10.0, 3.0 * rnd(s));
    const Theta th = make_theta<G>(pmd, us);
    Eval a, b;
    finish_eval(pmd, th, acc, a);
    finish_eval_old(pmd, th, acc, b);
    ok_fe = same_bits(a.F, b.F) && same_bits(a.mag, b.mag);
    for (int j = 0; j < 4; ++j) ok_fe = ok_fe && same_bits(a.g[j], b.g[j]);
    for (int j = 0; j < 10; ++j) ok_fe = ok_fe && same_bits(a.H[j], b.H[j]);
  }
  bool fr1[4], fr2[4];
  {
    double b1[4], b2[4];
    free_set(pmd, u, g, H, w, fr1, b1);
    free_set_old(pmd, u, g, H, w, fr2, b2);
    for (int j = 0; j < 4; ++j) ok_fs = ok_fs && fr1[j] == fr2[j] && same_bits(b1[j], b2[j]);
  }
  for (int pass = 0; pass < 2; ++pass) {
    const double mu = pass ? opaque(1e-10 * pow(10.0, 6.0 * (rnd(s) + 1.0))) : 0.0;
    double L1[10], L2[10], i1[4], i2[4];
    const int j1 = chol4(fr2, H, mu, L1, i1), j2 = chol4_old(fr2, H, mu, L2, i2);
    ok_ch = ok_ch && j1 == j2;
    for (int j = 0; j < 10; ++j) ok_ch = ok_ch && same_bits(L1[j], L2[j]);
    for (int j = 0; j < 4; ++j) ok_ch = ok_ch && same_bits(i1[j], i2[j]);
  }
  {
    double d1[4] = {0, 0, 0, 0}, d2[4] = {0, 0, 0, 0};
    const bool r1 = newton_dir<G>(pmd, u, g, H, w, d1, nc);
    const bool r2 = newton_dir_old2<G>(pmd, u, g, H, w, d2, nc);
    ok_nd = r1 == r2;
    for (int j = 0; j < 4; ++j) ok_nd = ok_nd && same_bits(d1[j], d2[j]);
  }
  if (!ok_fe) atomicAdd(&bad[1], 1ull);
  if (!ok_fs) atomicAdd(&bad[2], 1ull);
  if (!ok_ch) atomicAdd(&bad[3], 1ull);
  if (!ok_nd) atomicAdd(&bad[4], 1ull);
  if (!(ok_fe && ok_fs && ok_ch && ok_nd)) atomicAdd(&bad[0], 1ull);
  atomicAdd(tot, 1ull);
}

int main() {
  unsigned long long *b, *t;
  if (hipMalloc(&b, 8 * 8) != hipSuccess || hipMalloc(&t, 8) != hipSuccess) {
    printf("no device memory\n");
    return 2;
  }
  unsigned long long worst = 0;
  for (int G : {8, 16}) {
    (void)hipMemset(b, 0, 8 * 8);
    (void)hipMemset(t, 0, 8);
    const int n = 1 << 16;
    if (G == 8) k<8><<<n * 8 / 64, 64>>>(n, b, t);
    else k<16><<<n * 16 / 64, 64>>>(n, b, t);
    unsigned long long hb[8], ht;
    if (hipMemcpy(hb, b, 8 * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&ht, t, 8, hipMemcpyDeviceToHost) != hipSuccess) {
      printf("G=%d: the kernel failed: %s\n", G, hipGetErrorString(hipGetLastError()));
      return 2;
    }
    printf("G=%d: %llu of %llu lanes differ (finish_eval %llu, free_set %llu, chol4 %llu, newton_dir %llu)\n", G,
           hb[0], ht, hb[1], hb[2], hb[3], hb[4]);
    worst += hb[0];
  }
  return worst ? 1 : 0;
}
