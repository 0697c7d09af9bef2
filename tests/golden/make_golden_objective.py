#!/usr/bin/env python
"""Regenerates tests/golden/objective_golden.npz: the MAP objective F, its
gradient g[4] and Hessian H[4][4] in u = (logit q, logit A, c, log delta) and
the pointwise ell[30] of DESIGN.md §3.1-3.2, from the analytic formulas in
mpmath at 300 bits (90 digits), with the error bars' ingredients (DESIGN.md
§3.4.2; constants in tests/objective_cases.py).  Seeded: a rerun writes the
same bytes.  Nothing here reads the kernel's or the oracle's output.

Per item (n items; an item's entries X are flat: F, g[4], H[16], ell[30]):
  model, subset, row, u, group   the case (objective_cases.items)
  rows_y, rows_N                 the nine data rows the items index by `row`
  ref, res                       X rounded to the nearest double and the signed
                                 residual; an infeasible item has F = +inf, 0 else
  mag                            the same analytic sum with every term's absolute
                                 value taken (objective_cases: "mag(X)")
  cond                           sum over the intermediates of |dX / d ln p| eps_p
                                 (objective_cases.EPS), one perturbed at a time
  null_omd                       which 1 - D conditioning term `cond` carries for
                                 model_null items (PMD items always "omD_sub")
  min_D, gap                     min D_i over the subset and 1 - A - c
  accf_ref, accf_res             [n][31]: the polish form's F and ell[30], the full
                                 log-pmf objective: ell_i + ln C(N_i, y_i) and
                                 F - sum ln C(N_i, y_i); split like ref, res
  accf_F, accf_ell               the bar of the polish form's F and ell without
                                 cond and the absolute floor: lrise's bar summed
                                 over the three terms per point and the sums' roundings
  planted                        [n_pmd_interior][3][16] wrong Hessians (no J2 G
                                 term; no lD Dqq term; the prior's -8/(1-c)^2 as
                                 -8/(1-c)) and planted_item, their items
  digest                         objective_cases.digest() at the time of writing

u is taken as the exact double; 1 - q, 1 - A and 1 - D are formed without
cancellation (sigmoid(-u); PMD 1 - D = sigmoid(-u1) + A (1 - w) - c).  g and H
of every tenth item are cross-checked here against mp.diff of an mpmath F that
shares no derivation with them.

Usage: python tests/golden/make_golden_objective.py [out.npz]
"""

from __future__ import annotations

import io
import sys
import zipfile
from pathlib import Path

import numpy as np
from mpmath import mp, mpf

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from tests import objective_cases as oc  # noqa: E402
from tests import special_cases as sc  # noqa: E402
import make_golden_primitives as mgp  # noqa: E402  (lrise_ref_mag, _lg_mag; sets mp.prec = 300)

assert mp.prec >= 200
H_REL = mpf(2) ** -80  # the relative step of the conditioning terms' one-sided differences
ZERO, ONE = mpf(0), mpf(1)


def sig(t):
    return 1 / (1 + mp.exp(-t))


def lsig(t):
    return -mp.log1p(mp.exp(-t))


class Globals:
    """The trial point's intermediates; `pert` = (name, h) scales one by 1 + h."""

    def __init__(self, model, u, pert=None):
        u = [mpf(float(t)) for t in u]
        self.pmd = model == oc.PMD
        self.u = u
        self.q, self.omq = sig(u[0]), sig(-u[0])
        self.A, self.omA, self.c = (sig(u[1]), sig(-u[1]), u[2]) if self.pmd else (ZERO, ONE, ZERO)
        self.delta = mp.exp(u[3])
        if pert is not None and pert[0] in ("q", "omq", "A", "omA", "delta"):
            setattr(self, pert[0], getattr(self, pert[0]) * (1 + pert[1]))
        self.phi = self.delta + 2
        if pert is not None and pert[0] == "phi":
            self.phi *= 1 + pert[1]

    def D_parts(self, k):
        """D and its derivatives at |z| - 1 = k from the (possibly perturbed) intermediates."""
        if not self.pmd:
            return self.q, ONE, ZERO, ZERO, ZERO, ZERO
        w = self.omq ** k
        D = self.A * w + self.c
        Dq = -self.A * k * self.omq ** (k - 1) if k >= 1 else ZERO
        DqA = -k * self.omq ** (k - 1) if k >= 1 else ZERO
        Dqq = self.A * k * (k - 1) * self.omq ** (k - 2) if k >= 2 else ZERO
        return D, Dq, w, ONE, Dqq, DqA

    def omD_exact(self, k):
        if not self.pmd:
            return self.omq
        return self.omA + self.A * (1 - self.omq ** k) - self.c


def pm(x, f):
    """A psi / psi1 value's magnitude: lg3's bar is on max(1, |f|) below 10."""
    return max(ONE, abs(f)) if x < 10 else abs(f)


def point(y, N, D, omD, a, b, phi, dD, Dqq, DqA, sp_phi, want_mag=False):
    """One point's theta-space contribution: (ell, G[4], Hh[4][4] upper, T_qq)
    and, with want_mag, the same with absolute values."""
    args = (y + a, N - y + b, N + phi, a, b)
    lg = [mp.loggamma(t) for t in args] + [sp_phi[0]]
    ps = [mp.psi(0, t) for t in args] + [sp_phi[1]]
    tg = [mp.psi(1, t) for t in args] + [sp_phi[2]]
    ell = (lg[0] - lg[3]) + (lg[1] - lg[4]) - (lg[2] - lg[5])
    Pa, Pb, S = ps[0] - ps[3], ps[1] - ps[4], ps[5] - ps[2]
    Qa, Qb, S1 = tg[0] - tg[3], tg[1] - tg[4], tg[5] - tg[2]
    lD = phi * (Pa - Pb)
    lF = D * Pa + omD * Pb + S
    lDD = phi * phi * (Qa + Qb)
    lDF = (Pa - Pb) + phi * (D * Qa - omD * Qb)
    lFF = D * D * Qa + omD * omD * Qb + S1
    G = [lD * dD[0], lD * dD[1], lD * dD[2], lF]
    Hh = [[ZERO] * 4 for _ in range(4)]
    for j in range(3):
        for m in range(j, 3):
            Hh[j][m] = lDD * dD[j] * dD[m]
        Hh[j][3] = lDF * dD[j]
    Hh[0][0] += lD * Dqq
    Hh[0][1] += lD * DqA
    Hh[3][3] = lFF
    if not want_mag:
        return (ell, G, Hh, lD * Dqq), None
    xs = args + (phi,)
    ell_m = sum(mgp._lg_mag(t) for t in xs)
    pP = [pm(x, f) for x, f in zip(xs, ps)]
    pQ = [pm(x, f) for x, f in zip(xs, tg)]
    Pa_m, Pb_m, S_m = pP[0] + pP[3], pP[1] + pP[4], pP[5] + pP[2]
    Qa_m, Qb_m, S1_m = pQ[0] + pQ[3], pQ[1] + pQ[4], pQ[5] + pQ[2]
    lD_m = phi * (Pa_m + Pb_m)
    lF_m = D * Pa_m + omD * Pb_m + S_m
    lDD_m = phi * phi * (Qa_m + Qb_m)
    lDF_m = Pa_m + Pb_m + phi * (D * Qa_m + omD * Qb_m)
    lFF_m = D * D * Qa_m + omD * omD * Qb_m + S1_m
    aD = [abs(t) for t in dD]
    G_m = [lD_m * aD[0], lD_m * aD[1], lD_m * aD[2], lF_m]
    Hm = [[ZERO] * 4 for _ in range(4)]
    for j in range(3):
        for m in range(j, 3):
            Hm[j][m] = lDD_m * aD[j] * aD[m]
        Hm[j][3] = lDF_m * aD[j]
    Hm[0][0] += lD_m * abs(Dqq)
    Hm[0][1] += lD_m * abs(DqA)
    Hm[3][3] = lFF_m
    return (ell, G, Hh, lD * Dqq), (ell_m, G_m, Hm)


def add_into(tot, c, sign=1):
    tot[0] += sign * c[0]
    for j in range(4):
        tot[1][j] += sign * c[1][j]
        for m in range(j, 4):
            tot[2][j][m] += sign * c[2][j][m]


def finish(gl, tot, ells, lo, hi, absolute=False):
    """The chain rule to u-space and the prior: the flat X (F, g, H, ell[30]);
    `absolute`: the magnitudes instead (tot, ells hold the absolute sums)."""
    q, omq, A, omA, c, delta = gl.q, gl.omq, gl.A, gl.omA, gl.c, gl.delta
    u = gl.u
    J = [q * omq, A * omA, ONE, delta]
    J2 = [q * omq * (omq - q), A * omA * (omA - A), ZERO, delta]
    pmd = gl.pmd
    omc = 1 - c
    if not absolute:
        lp = lsig(u[0]) + 2 * lsig(-u[0]) - delta / 1000
        gp = [1 - 3 * q, ZERO, ZERO, -delta / 1000]
        hp = [-3 * q * omq, ZERO, ZERO, -delta / 1000]
        if pmd:
            lp += lsig(u[1]) + 2 * lsig(-u[1]) + 8 * mp.log1p(-c)
            gp[1], hp[1] = 1 - 3 * A, -3 * A * omA
            gp[2], hp[2] = -8 / omc, -8 / (omc * omc)
    else:
        lp = abs(lsig(u[0])) + 2 * abs(lsig(-u[0])) + delta / 1000
        gp = [1 + 3 * q, ZERO, ZERO, delta / 1000]
        hp = [3 * q * omq, ZERO, ZERO, delta / 1000]
        if pmd:
            lp += abs(lsig(u[1])) + 2 * abs(lsig(-u[1])) + 8 * abs(mp.log1p(-c))
            gp[1], hp[1] = 1 + 3 * A, 3 * A * omA
            gp[2], hp[2] = 8 / omc, 8 / (omc * omc)
        J2 = [abs(t) for t in J2]
    sgn = 1 if absolute else -1
    X = [sgn * (tot[0] + lp)]
    g = [sgn * (J[j] * tot[1][j] + gp[j]) for j in range(4)]
    Hm = [[ZERO] * 4 for _ in range(4)]
    for j in range(4):
        for m in range(j, 4):
            h = J[j] * tot[2][j][m] * J[m]
            if j == m:
                h += J2[j] * tot[1][j] + hp[j]
            Hm[j][m] = Hm[m][j] = sgn * h
    if not pmd:
        for j in (1, 2):
            g[j] = ZERO
            for m in range(4):
                Hm[j][m] = Hm[m][j] = ZERO
    X += g + [Hm[j][m] for j in range(4) for m in range(4)]
    X += [ells[i] if lo <= i < hi else ZERO for i in range(30)]
    return X


def kpos(i):
    return i if i < 15 else i - 15


def reference(model, subset, y, N, u, null_omd):
    """X, mag, cond (lists of mpf, length NX), the extras, or None for an infeasible item."""
    gl = Globals(model, u)
    pmd = gl.pmd
    if pmd and float(gl.A) + float(gl.c) >= 1.0:
        return None
    lo, hi = (15 if subset == 2 else 0), (15 if subset == 1 else 30)
    pts = [i for i in range(lo, hi) if int(N[i]) > 0]  # N = 0: every difference is exactly 0
    sp = lambda phi: (mp.loggamma(phi), mp.psi(0, phi), mp.psi(1, phi))  # noqa: E731
    sp0 = sp(gl.phi)
    zero_tot = lambda: [ZERO, [ZERO] * 4, [[ZERO] * 4 for _ in range(4)]]  # noqa: E731

    base, base_D = {}, {}
    tot, tot_m = zero_tot(), zero_tot()
    ells, ells_m = [ZERO] * 30, [ZERO] * 30
    Tqq = ZERO
    for i in pts:
        k = kpos(i)
        D, Dq, DA, Dc, Dqq, DqA = gl.D_parts(k)
        omD = gl.omD_exact(k)
        base_D[i] = (D, omD)
        yy, nn = mpf(int(y[i])), mpf(int(N[i]))
        c, cm = point(yy, nn, D, omD, D * gl.phi, omD * gl.phi, gl.phi, (Dq, DA, Dc), Dqq, DqA, sp0, True)
        base[i] = c
        add_into(tot, c)
        add_into(tot_m, cm)
        ells[i], ells_m[i] = c[0], cm[0]
        Tqq += c[3]
    X = finish(gl, tot, ells, lo, hi)
    mag = finish(gl, tot_m, ells_m, lo, hi, absolute=True)

    def contrib(g2, i, D=None, omD=None, a=None, b=None, sp_phi=None):
        k = kpos(i)
        D2, Dq, DA, Dc, Dqq, DqA = g2.D_parts(k)
        D0, omD0 = base_D[i]
        if omD is None:
            # 1 - fl(D): D's change passes on unreduced; the complementary-sigmoid form of model_null at
            # u0 > 0 follows omq instead
            if not pmd and null_omd == "omD_omq" and float(u[0]) > 0:
                omD = g2.omq
            else:
                omD = omD0 - (D2 - D0)
        D = D2 if D is None else D
        a = D * g2.phi if a is None else a
        b = omD * g2.phi if b is None else b
        yy, nn = mpf(int(y[i])), mpf(int(N[i]))
        return point(yy, nn, D, omD, a, b, g2.phi, (Dq, DA, Dc), Dqq, DqA, sp_phi)[0]

    cond = [ZERO] * oc.NX

    def account(X2, eps):
        for j in range(oc.NX):
            cond[j] += abs(X2[j] - X[j]) / H_REL * eps

    # the global intermediates, one at a time: the whole sum again
    for name in ("q", "omq", "A", "omA", "delta", "phi"):
        if not pmd and name in ("A", "omA"):
            continue
        g2 = Globals(model, u, (name, H_REL))
        sp2 = sp(g2.phi) if name in ("delta", "phi") else sp0
        t2, e2 = zero_tot(), [ZERO] * 30
        for i in pts:
            c = contrib(g2, i, sp_phi=sp2)
            add_into(t2, c)
            e2[i] = c[0]
        account(finish(g2, t2, e2, lo, hi), oc.EPS[name])
    # the per-point intermediates: only that point's contribution changes
    eD = mpf(oc.EPS["D"])
    for i in pts:
        D0, omD0 = base_D[i]
        if pmd or null_omd == "omD_sub":
            e_omD = eD * D0 / omD0 + mpf(oc.EPS["omD"])
        elif float(u[0]) > 0:
            e_omD = ZERO  # omD is omq itself: the omq perturbation above carries it
        else:
            e_omD = mpf(oc.EPS["q"]) * D0 / omD0 + mpf(oc.EPS["omD"])
        for name, eps, kw in (("D", eD if pmd else ZERO, dict(D=D0 * (1 + H_REL), omD=omD0)),
                              ("omD", e_omD, dict(omD=omD0 * (1 + H_REL))),
                              ("a", mpf(oc.EPS["a"]), dict(a=D0 * gl.phi * (1 + H_REL))),
                              ("b", mpf(oc.EPS["b"]), dict(b=omD0 * gl.phi * (1 + H_REL)))):
            if eps == 0:
                continue
            if "omD" not in kw:
                kw["omD"] = omD0
            c = contrib(gl, i, sp_phi=sp0, **kw)
            t2 = [tot[0], list(tot[1]), [list(r) for r in tot[2]]]
            add_into(t2, base[i], -1)
            add_into(t2, c)
            e2 = list(ells)
            e2[i] = c[0]
            account(finish(gl, t2, e2, lo, hi), eps)

    # planted wrong Hessians (flat [16], as doubles)
    Hx = X[5:21]
    J = [gl.q * gl.omq, gl.A * gl.omA, ONE, gl.delta]
    J2 = [gl.q * gl.omq * (gl.omq - gl.q), gl.A * gl.omA * (gl.omA - gl.A), ZERO, gl.delta]
    p1 = list(Hx)
    for j in range(4):
        p1[5 * j] += J2[j] * tot[1][j]
    p2 = list(Hx)
    p2[0] += J[0] * J[0] * Tqq
    p3 = list(Hx)
    omc = 1 - gl.c
    p3[10] += -8 / (omc * omc) + 8 / omc
    planted = [[float(t) for t in p] for p in (p1, p2, p3)]

    # ln C(N, y) and the polish form's bar (lrise's, special_cases.py)
    logC = [ZERO] * 30
    accf_ell = [0.0] * 30
    sumR = ZERO
    for i in pts:
        yy, nn = int(y[i]), int(N[i])
        logC[i] = mp.loggamma(nn + 1) - mp.loggamma(yy + 1) - mp.loggamma(nn - yy + 1)
        D0, omD0 = base_D[i]
        a, b = float(D0 * gl.phi), float(omD0 * gl.phi)
        bar_i, absR = 0.0, ZERO
        for n_, s_ in ((yy, a), (nn - yy, b), (nn, float(gl.phi))):
            r, m = mgp.lrise_ref_mag(float(n_), s_)
            bar_i += sc.ULP1 * m + sc.BINARY_ABS
            absR += abs(r)
        accf_ell[i] = bar_i + 3 * oc.U * float(absR)
        sumR += absR
    lp_m = abs(lsig(gl.u[0])) + 2 * abs(lsig(-gl.u[0])) + gl.delta / 1000
    if pmd:
        lp_m += abs(lsig(gl.u[1])) + 2 * abs(lsig(-gl.u[1])) + 8 * abs(mp.log1p(-gl.c))
    accf_F = sum(accf_ell) + oc.C_ACCF_SUM * float(sumR) + oc.C_F * float(lp_m)
    full = [X[0] - sum(logC)] + [X[21 + i] + logC[i] for i in range(30)]
    extras = dict(planted=planted, full=full, accf_ell=accf_ell, accf_F=accf_F,
                  min_D=float(min(gl.D_parts(kpos(i))[0] for i in range(lo, hi))),
                  gap=float(gl.omA - gl.c) if pmd else 1.0)
    return X, mag, cond, extras


# --------------------------------------------------------------------------
# the independent cross-check: mp.diff of an F written from DESIGN §3.1 alone
# --------------------------------------------------------------------------
def F_only(model, subset, y, N, u):
    lo, hi = (15 if subset == 2 else 0), (15 if subset == 1 else 30)
    q = 1 / (1 + mp.exp(-u[0]))
    delta = mp.exp(u[3])
    phi = delta + 2
    lp = mp.log(q) + 2 * mp.log(1 / (1 + mp.exp(u[0]))) - delta / 1000
    if model == oc.PMD:
        A, c = 1 / (1 + mp.exp(-u[1])), u[2]
        lp += mp.log(A) + 2 * mp.log(1 / (1 + mp.exp(u[1]))) + 8 * mp.log(1 - c)
    s = ZERO
    for i in range(lo, hi):
        if int(N[i]) == 0:
            continue
        k = kpos(i)
        if model == oc.PMD:
            D = A * (1 / (1 + mp.exp(u[0]))) ** k + c
            omD = 1 / (1 + mp.exp(u[1])) + A * (1 - (1 / (1 + mp.exp(u[0]))) ** k) - c
        else:
            D, omD = q, 1 / (1 + mp.exp(u[0]))
        yy, nn = int(y[i]), int(N[i])
        a, b = D * phi, omD * phi
        s += (mp.loggamma(yy + a) - mp.loggamma(a) + mp.loggamma(nn - yy + b) - mp.loggamma(b)
              - mp.loggamma(nn + phi) + mp.loggamma(phi))
    return -(s + lp)


def cross_check(model, subset, y, N, u, X, mag):
    """g and H against one- or two-sided mp.diff of F_only; returns the worst
    error as a fraction of 1e-6 of the double-precision bar's leading term."""
    free = (0, 1, 2, 3) if model == oc.PMD else (0, 3)
    x0 = [mpf(float(t)) for t in u]
    kw = dict(direction=1) if (model == oc.PMD and float(u[2]) == 0.0) else {}

    def f(*v):
        w = list(x0)
        for j, t in zip(free, v):
            w[j] = t
        return F_only(model, subset, y, N, w)

    pt = tuple(x0[j] for j in free)
    worst = 0.0
    for a_, j in enumerate(free):
        order = [0] * len(free)
        order[a_] = 1
        d = mp.diff(f, pt, tuple(order), **kw)
        worst = max(worst, float(abs(d - X[1 + j]) / (mpf(oc.C_G) * 1e-6 * mag[1 + j] + mpf(10) ** -30)))
        for b_, m in enumerate(free):
            if b_ < a_:
                continue
            order = [0] * len(free)
            order[a_] += 1
            order[b_] += 1
            d = mp.diff(f, pt, tuple(order), **kw)
            worst = max(worst, float(abs(d - X[5 + 4 * j + m]) /
                                     (mpf(oc.C_H) * 1e-6 * mag[5 + 4 * j + m] + mpf(10) ** -30)))
    return worst


def build(out_path: Path) -> dict:
    rows_y, rows_N = oc.data_rows()
    model, subset, row, u, group = oc.items()
    n = len(model)
    null_omd = oc.NULL_OMD
    ref = np.zeros((n, oc.NX))
    res = np.zeros((n, oc.NX))
    mag = np.zeros((n, oc.NX))
    cond = np.zeros((n, oc.NX))
    accf_ref = np.zeros((n, 31))
    accf_res = np.zeros((n, 31))
    accf_ell = np.zeros((n, 30))
    accf_F = np.zeros(n)
    min_D = np.zeros(n)
    gap = np.zeros(n)
    planted, planted_item = [], []
    worst_cc = 0.0
    for i in range(n):
        y, N = rows_y[row[i]], rows_N[row[i]]
        r = reference(int(model[i]), int(subset[i]), y, N, u[i], null_omd)
        if r is None:
            assert group[i] == oc.INFEASIBLE, i
            ref[i, 0] = np.inf
            continue
        X, m, c, ex = r
        ref[i], res[i] = mgp._split(X)
        mag[i] = [float(t) for t in m]
        cond[i] = [float(t) for t in c]
        accf_ref[i], accf_res[i] = mgp._split(ex["full"])
        accf_ell[i], accf_F[i] = ex["accf_ell"], ex["accf_F"]
        min_D[i], gap[i] = ex["min_D"], ex["gap"]
        assert group[i] != oc.INFEASIBLE, i
        if group[i] == oc.OVERFLOW:
            assert min_D[i] < oc.D_FLOOR, (i, min_D[i])
        else:
            assert min_D[i] >= oc.D_FLOOR and gap[i] >= oc.GAP_FLOOR, (i, min_D[i], gap[i])
        if group[i] == oc.INTERIOR and model[i] == oc.PMD:
            planted.append(ex["planted"])
            planted_item.append(i)
        # (not in the overflow corner: at c = 0 with D ~ 1e-153 the one-sided difference's step would have to
        # be far below D itself)
        if i % 10 == 0 and group[i] != oc.OVERFLOW:
            w = cross_check(int(model[i]), int(subset[i]), y, N, u[i], X, m)
            worst_cc = max(worst_cc, w)
            assert w < 1.0, ("mp.diff disagrees with the analytic g / H", i, w)
        if i % 20 == 0:
            print(f"item {i} / {n}", flush=True)
    print(f"mp.diff cross-check: worst difference {worst_cc:.2e} of a millionth of the double-precision bar")
    out = {"model": model, "subset": subset, "row": row, "u": u, "group": group, "rows_y": rows_y,
           "rows_N": rows_N, "ref": ref, "res": res, "mag": mag, "cond": cond, "accf_ref": accf_ref, "accf_res": accf_res,
           "accf_ell": accf_ell, "accf_F": accf_F, "min_D": min_D, "gap": gap,
           "planted": np.array(planted), "planted_item": np.array(planted_item, np.int32),
           "null_omd": np.array(null_omd), "digest": np.array(oc.digest())}
    write_npz(out_path, out)
    return out


def write_npz(path: Path, arrays: dict):
    """np.savez_compressed with fixed member dates: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(__file__).with_name("objective_golden.npz")
    r = build(out)
    print(f"wrote {out}: {len(r['model'])} items, {out.stat().st_size} bytes on disk")
