// The forms of finish_eval, chol4, free_set and newton_dir before the Newton
// logic's arithmetic was pinned and free_set's binding test rewritten
// (compiler-chosen contraction, short-circuit predicates), kept for
// tools/micro/logic_check.hip.  Included inside namespace mdfit, after
// mdfit_model.h.
__device__ __forceinline__ void finish_eval_old(bool pmd, const Theta& th, const double s[kNAcc],
                                            Eval& e) {
  const double q = th.q, A = th.A, c = th.c, delta = th.delta;
  const double J[4] = {q * th.omq, th.JA, 1.0, delta};
  const double J2[4] = {J[0] * (1.0 - 2.0 * q), th.JA * (1.0 - 2.0 * A), 0.0, delta};
  const double gp[4] = {1.0 - 3.0 * q, pmd ? 1.0 - 3.0 * A : 0.0, pmd ? -8.0 * th.iomc : 0.0,
                        -delta / 1000.0};
  const double hp[4] = {-3.0 * J[0], pmd ? -3.0 * th.JA : 0.0,
                        pmd ? -8.0 * th.iomc * th.iomc : 0.0, -delta / 1000.0};
  const bool infeasible = pmd && (A + c >= 1.0);
  e.F = infeasible ? INFINITY : -(s[0] + th.lprior);
  e.mag = s[1];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool fixed = !pmd && (j == 1 || j == 2);
    e.g[j] = fixed ? 0.0 : -(J[j] * s[2 + j] + gp[j]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int m = j; m < 4; ++m) {
      const int k = hidx(j, m);
      double h = J[j] * s[6 + k] * J[m];
      if (j == m) h += J2[j] * s[2 + j] + hp[j];
      const bool fixed = !pmd && (j == 1 || j == 2 || m == 1 || m == 2);
      e.H[k] = fixed ? 0.0 : -h;
    }
  }
}

// Cholesky of the free block of H + mu*I (fixed / bound rows -> identity);
// returns the first non-positive pivot's index (-1: positive definite).
// Packed lower triangle L (same index as H), iL = 1 / diag(L).
__device__ __forceinline__ int chol4_old(const bool fr[4], const double H[10], double mu, double L[10],
                                     double iL[4]) {
  int jf = -1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int m = 0; m <= j; ++m) {
      double s;
      if (!fr[j] || !fr[m]) s = (j == m) ? 1.0 : 0.0;
      else s = H[hidx(m, j)] + ((j == m) ? mu : 0.0);
#pragma unroll
      for (int p = 0; p < m; ++p) s = fma(-L[hidx(p, j)], L[hidx(p, m)], s);  // explicit: the same rounding in every instance
      if (j == m) {
        if (!(s > 0.0) && jf < 0) jf = j;
        const double sp = fmax(s, 1e-300);
        const double il = rsqrt_nr(sp);  // 1/L_jj, then L_jj = s/L_jj
        L[hidx(j, j)] = sp * il;
        iL[j] = il;
      } else {
        L[hidx(m, j)] = s * iL[m];  // L(j,m) stored at packed (m,j)
      }
    }
  }
  return jf;
}

__device__ __forceinline__ void free_set_old(bool pmd, const double u[4], const double g[4], const double H[10],
                                         double w, bool fr[4], double dbind[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool fixed = !pmd && (j == 1 || j == 2);
    const double eps = fmin(kEpsBind[j], w);
    const double dlo = u[j] - kULo[j], dhi = kUHi[j] - u[j];
    const bool atlo = dlo <= eps, athi = dhi <= eps;
    // on / next to a box bound and not pulled inward by more than kEpsAct --
    // unless, with positive curvature, its own Newton step g/H stops short of
    // the bound (an interior optimum just inside it)
    const double hjj = H[hidx(j, j)];
    const bool bind = (atlo && g[j] > -kEpsAct && (hjj <= 0.0 || g[j] + kEpsAct > hjj * dlo)) ||
                      (athi && g[j] < kEpsAct && (hjj <= 0.0 || -g[j] + kEpsAct > hjj * dhi));
    dbind[j] = (bind && !fixed) ? (atlo ? kULo[j] : kUHi[j]) - u[j] : 0.0;
    fr[j] = !(fixed || bind);
  }
}

template <int G>
__device__ __forceinline__ bool newton_dir_old2(bool pmd, const double u[4], const double g[4],
                                           const double H[10], double w, double d[4], bool want_nc = false) {
  bool fr[4];
  double dbind[4];
  free_set_old(pmd, u, g, H, w, fr, dbind);
  double L[10], iL[4];
  const int jf = chol4_old(fr, H, 0.0, L, iL);  // plain Newton: the common case
  const bool indef = jf >= 0;
  if (want_nc && indef) {
    double z[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = j == jf ? 1.0 : 0.0;
#pragma unroll
    for (int p = 2; p >= 0; --p) {
      if (p < jf) {
        double s = 0.0;
#pragma unroll
        for (int k = p + 1; k < 4; ++k) s += k <= jf ? L[hidx(p, k)] * z[k] : 0.0;  // L(k,p)
        z[p] = -s * iL[p];
      }
    }
    const double mx = maxabs4(z);
    const double gz = g[0] * z[0] + g[1] * z[1] + g[2] * z[2] + g[3] * z[3];
    const double sg = gz > 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = sg * z[j] / mx;
    return true;
  }
  bool ok = !indef;
  // the solve with the accepted factor: every lane of a group that needed a
  // shift solves with its own attempt's factor, then takes the winner's step
  int src = -1;  // >= 0: the lane (absolute) whose step this lane takes
  if (__any(!ok)) {
    double sc = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (fr[j]) sc = fmax(sc, fabs(H[hidx(j, j)]));
    if (sc == 0.0) sc = 1.0;
    const int kl = (int)(threadIdx.x & (G - 1));
    const int gbase = (int)(threadIdx.x & ~(G - 1));
    double mu = 1e-10 * sc;
#pragma unroll
    for (int i = 1; i < G; ++i) mu = i <= kl ? mu * 10.0 : mu;  // attempt kl + 1
    double L2[10], iL2[4];
    // (mu opaque: a product the compiler may not fuse into the Cholesky's
    // diagonal add -- it would round differently in the parallel and the
    // sequential instance, and the two layouts reach them at different attempts)
    const bool ok2 = !ok && chol4_old(fr, H, opaque(mu), L2, iL2) < 0;
    const unsigned long long gm = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << gbase;
    const unsigned long long okm = __ballot(ok2) & gm;
    if (!ok) {
      if (okm != 0ull) {
        ok = true;
        src = __ffsll(okm) - 1;
#pragma unroll
        for (int j = 0; j < 10; ++j) L[j] = L2[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) iL[j] = iL2[j];
      } else {  // attempts G+1 .. 39, replicated on the group's lanes
        mu = 1e-10 * sc;
#pragma unroll 1
        for (int i = 1; i < G; ++i) mu *= 10.0;  // attempt G
        mu *= 10.0;
        for (int attempt = G + 1; attempt < 40 && !ok; ++attempt, mu *= 10.0) ok = chol4_old(fr, H, opaque(mu), L, iL) < 0;
      }
    }
  }
  if (!ok) {
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = (fr[j] && isfinite(g[j])) ? -g[j] : 0.0;
  } else {
    double z[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // L z = -g (free rows)
      double s = fr[j] ? -g[j] : 0.0;
#pragma unroll
      for (int p = 0; p < j; ++p) s = fma(-L[hidx(p, j)], z[p], s);
      z[j] = s * iL[j];
    }
#pragma unroll
    for (int j = 3; j >= 0; --j) {  // L^T d = z
      double s = z[j];
#pragma unroll
      for (int p = j + 1; p < 4; ++p) s = fma(-L[hidx(j, p)], d[p], s);
      d[j] = s * iL[j];
    }
  }
  if (__any(src >= 0)) {
    const int from = src >= 0 ? src : (int)threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = __shfl(d[j], from, 64);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (!fr[j]) d[j] = dbind[j];
  const double mx = maxabs4(d);
  if (mx > 4.0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] *= 4.0 / mx;
  }
  return indef;
}
