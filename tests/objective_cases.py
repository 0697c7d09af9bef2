"""Shared by the tests that pin the MAP objective, gradient and Hessian to
mpmath (test_map_objective.py, test_gpu_map_objective.py) and the fixture's
script (golden/make_golden_objective.py): the items, the constants of the error
bars with their derivation (DESIGN.md §3.4.2 -- none is measured from the kernel
or the oracle), the digest that ties the fixture to the items, and the error
measure.  Needs numpy alone."""

from __future__ import annotations

import hashlib
from pathlib import Path

import numpy as np

from tests import special_cases as sc

ROOT = Path(__file__).resolve().parents[1]
FIXTURE = ROOT / "tests" / "golden" / "objective_golden.npz"
SEED = 20261021

PMD, NULL = 0, 1
U_LO = np.array([-25.0, -25.0, 0.0, -25.0])
U_HI = np.array([25.0, 25.0, 0.999, 20.0])
D_FLOOR = 1e-150     # every group but the overflow corner keeps min D_i at or above it
GAP_FLOOR = 1e-6     # ... and 1 - A - c at or above it
GROUPS = ("interior", "edge", "infeasible", "overflow")
INTERIOR, EDGE, INFEASIBLE, OVERFLOW = range(4)

# --------------------------------------------------------------------------
# the bars: bar(X) = C_X mag(X) + cond(X) + ABS, X an entry of F, g, H or ell
# --------------------------------------------------------------------------
U = sc.U  # one rounding, 2^-53
ABS = 1e-12
# mag(X): the analytic sum of X with every term's absolute value taken.  A psi or psi1 of an argument below 10
# counts as max(1, |.|), the form of lg3's bar there; a lnGamma of an argument below 10 as |lnGamma(x + 10)| +
# |ln P(x)|, the two terms lg3 sums (at least lnGamma(10) = 12.8).
#
# C_F: lg3.l's bar as a relative figure: from 10, 1e-15; below 10 (2.5e-14 + 4.5e-16 |f|) against a magnitude of
# at least 12.8: 2.0e-15 + 4.5e-16 = 2.5e-15.  The rounded argument (y + a, N - y + b, N + phi): one rounding
# through x psi(x) against x ln x - x, a factor ln x / (ln x - 1) <= 1.8 from 10 (2 U); below 10, x |psi| U <= 22.5 U
# against 12.8 (2 U).  The sum: one rounding per term, 30 points of six: 180 U.
C_F = 2.5e-15 + 2 * U + 180 * U
# C_g: lg3.p's bar 1.4e-14 max(1, |psi|) below 10 (2.5 ulp = 5 U from 10); the rounded argument through
# x psi1(x) <= 1.65 for x >= 1 (an argument below 1 has y = 0 and is a or b itself: no rounding): 2 U; the
# products of a term (phi, D or its derivative, J: 10 roundings with those of the derivatives of D): 10 U; the sum: 180 U.
C_G = sc.LG3_P_C + 2 * U + 10 * U + 180 * U
# C_H: lg3.q's bar 6.1e-14 max(1, psi1) below 10; from 10 2.5 ulp + B16 / x^17, at most 6.7e-16 psi1 (at x = 10):
# 5 U + 7e-16; the rounded argument through x |psi2| / psi1 <= 2: 2 U; products (phi^2, two derivatives of D, two
# J: 14 roundings): 14 U; the sum: 180 U.  The psi terms of H (lD Dqq, lD DqA, lDF, J2 G) have the smaller C_g.
C_H = sc.LG3_Q_C + 7e-16 + 2 * U + 14 * U + 180 * U

# cond(X): the first-order effect on X of the roundings that the formulas of DESIGN.md §3.1-3.2 are entitled to:
# sum over the intermediates p of |dX / d ln p| eps_p, one at a time, in the mpmath evaluation.  Relative eps:
EPS = {
    # q = sigmoid(u0) as e r or r, e = exp(-|u0|) (1 ulp = 2 U), 1 + e (U), r = rcp (1 ulp = 2 U), the product (U)
    "q": 6 * U,
    "omq": 6 * U,     # the complementary sigmoid, the same four operations
    "A": 6 * U,       # sigmoid(u1), as q
    "omA": 6 * U,
    "delta": 2 * U,   # exp(u3): 1 ulp
    "phi": U,         # delta + 2: one rounding (delta's own error reaches phi through the delta perturbation)
    # D_i = fma(A, w, c), w = (1-q)^k by powk: three squarings and three products (6 U; the k eps_omq of the base
    # arrive through the omq perturbation), the fma (U)
    "D": 7 * U,
    # omD_i = 1 - fl(D_i): the subtraction's rounding, relative U, plus ABSOLUTE eps_D D_i, the error of fl(D_i)
    # that the subtraction passes on unreduced -- relative eps_D D_i / (1 - D_i), the term that lets 1 - D pass
    # as D -> 1.  (PMD, and model_null without the complementary-sigmoid form: "omD_sub" in the fixture.)
    "omD": U,
    "a": U,           # D_i phi: one rounding
    "b": U,           # omD_i phi: one rounding
}
# model_null with 1 - D taken from the complementary sigmoid where u0 > 0 ("omD_omq" in the fixture): omD is omq
# there, eps_omq relative, and 1 - q at u0 <= 0, where q <= 1/2 and the subtraction passes on eps_q q / omq <= eps_q
NULL_OMD = "omD_omq"   # the one that applies to model_null (PMD: always "omD_sub")
NULL_OMD_BAR = {"omD_sub": "1 - fl(D): eps_D D / (1 - D) + U", "omD_omq": "u0 > 0 ? eps_omq : eps_q q / (1 - q) + U"}

# accf (the polish form): F and ell are the full log-pmf R(y, a) + R(N - y, b) - R(N, phi); each R = lrise holds
# 2^-52 mag_R + 1e-15 (special_cases.py), mag_R from mpmath in the fixture; summed over the three terms per
# point, plus one rounding per summed term (C_ACCF_SUM |R|) and cond(F)
C_ACCF_SUM = 90 * U

# form bits of mdfit_objective_form (include/mdfit.h)
FORM_ACCF, FORM_NULL_ROW, FORM_WHOLE_PAIR = 1, 2, 4


# --------------------------------------------------------------------------
# the items
# --------------------------------------------------------------------------
def data_rows():
    """(y, N)[9][32], uint32: three typical synthetic taxa, N = 4e9 with y = 1 %,
    0 and N, N = 1 with alternating y, a ragged row, a row of mixed N."""
    from metadamage_amd.synthetic import generate

    b = generate(3, seed=SEED % 1000)
    y = np.zeros((9, 32), np.uint32)
    N = np.zeros((9, 32), np.uint32)
    y[:3, :30], N[:3, :30] = b.y[:, :30], b.N[:, :30]
    N[3:6, :30] = 4_000_000_000
    y[3, :30] = 40_000_000
    y[5, :30] = 4_000_000_000
    N[6, :30] = 1
    y[6, :30] = np.arange(30) % 2
    base = (1000 + 37 * np.arange(30)).astype(np.uint32)
    N[7, :30], y[7, :30] = base, base // 7
    N[7, 5:12] = y[7, 5:12] = 0        # ragged: no coverage at positions 5..11 ...
    N[7, 17] = y[7, 17] = 0            # ... and 17
    rng = np.random.default_rng([SEED, 1])
    mixed = np.floor(10.0 ** np.linspace(0.0, 9.0, 30)).astype(np.uint32)
    N[8, :30] = rng.permutation(mixed)
    y[8, :30] = np.floor(N[8, :30] * rng.uniform(0.0, 0.4, 30)).astype(np.uint32)
    assert (y <= N).all()
    return y, N


ROW_NAMES = ("synthetic0", "synthetic1", "synthetic2", "N4e9_y1pct", "N4e9_y0", "N4e9_yN", "N1_alt", "ragged",
             "mixedN")


def _logit(p):
    return float(np.log(p) - np.log1p(-p))


def items():
    """(model, subset, row, u[4], group) per item, int32 / float64 arrays."""
    rng = np.random.default_rng([SEED, 2])
    out = []

    def add(model, subset, row, u, group):
        u = np.array(u, np.float64)
        if model == NULL:
            u[1] = u[2] = 0.0
        out.append((model, subset, row, u, group))

    # interior: six seeded points per data row, both models, the subset cycling
    n = 0
    for row in range(9):
        for j in range(6):
            u = [rng.uniform(-6, 6), rng.uniform(-6, 6), 0.0 if j % 2 == 0 else rng.uniform(0.0, 0.3),
                 rng.uniform(-3, 9)]
            if 1.0 / (1.0 + np.exp(-u[1])) + u[2] > 0.95:
                u[1] = -u[1]
            for model in (PMD, NULL):
                add(model, n % 3, row, u, INTERIOR)
                n += 1
    # edges: each coordinate on each bound with the others interior (c > 0 at u0 = 25: with c = 0 the far
    # positions' D falls below D_FLOOR, the overflow corner's business), pairs of bounds, c's corners
    mid = lambda: [rng.uniform(-3, 3), rng.uniform(-3, 0.5), rng.uniform(0.01, 0.2), rng.uniform(0, 7)]  # noqa: E731
    edges = []
    for j in (0, 1, 3):
        for bound in (U_LO[j], U_HI[j]):
            u = mid()
            u[j] = bound
            if j == 1 and bound > 0:
                u[2] = 0.0           # A = 1 - 1.4e-11, c = 0: the gap 1 - A - c is 1.4e-11 < GAP_FLOOR ...
                u[1] = _logit(1.0 - 2e-6)  # ... so A's upper edge is taken at the gap floor instead
            edges.append(u)
    for u0 in (12.0, -12.0):
        u = mid()
        u[0] = u0
        edges.append(u)
    u = mid(); u[2] = 0.0; edges.append(u)                       # c on its lower bound
    u = mid(); u[2] = 0.999; u[1] = _logit(5e-4); edges.append(u)  # c on its upper bound, A small
    u = mid(); u[2] = 0.3; u[1] = _logit(0.7 - 1e-6); edges.append(u)  # A + c = 1 - 1e-6
    for (j, bj), (m, bm) in (((0, 25.0), (3, 20.0)), ((0, 25.0), (3, -25.0)), ((0, -25.0), (1, -25.0)),
                             ((0, -25.0), (3, 20.0)), ((1, -25.0), (3, -25.0)), ((0, 25.0), (1, -25.0)),
                             ((0, -25.0), (3, -25.0)), ((1, -25.0), (3, 20.0))):
        u = mid()
        u[j], u[m] = bj, bm
        edges.append(u)
    u = mid(); u[0], u[2], u[3] = -25.0, 0.0, 20.0; edges.append(u)
    u = mid(); u[0], u[2], u[3] = 12.0, 0.0, -25.0; edges.append(u)
    for e, u in enumerate(edges):
        for t in range(3):
            row = (e + 3 * t) % 9
            for model in (PMD, NULL):
                add(model, n % 3, row, u, EDGE)
                n += 1
    # infeasible: A + c >= 1
    add(PMD, 0, 0, [0.0, 3.0, 0.3, 5.0], INFEASIBLE)
    add(PMD, 1, 7, [-2.0, 25.0, 0.001, 2.0], INFEASIBLE)
    add(PMD, 2, 3, [1.0, 0.0, 0.5, 0.0], INFEASIBLE)
    # the overflow corner: c = 0, q -> 1 (A -> 0): D_i = A (1-q)^k below D_FLOOR at the far positions
    for u in ([25.0, -25.0, 0.0, 20.0], [25.0, 0.0, 0.0, 5.0], [25.0, -25.0, 0.0, -25.0]):
        for row in (0, 6):
            add(PMD, n % 3, row, u, OVERFLOW)
            n += 1
    return (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.int32),
            np.array([o[2] for o in out], np.int32), np.array([o[3] for o in out], np.float64),
            np.array([o[4] for o in out], np.int32))


def digest() -> str:
    """sha256 over the case arrays: the fixture stores it, the tests recompute it."""
    h = hashlib.sha256()
    for a in (*data_rows(), *items()):
        h.update(np.ascontiguousarray(a).tobytes())
    for c in (C_F, C_G, C_H, ABS, C_ACCF_SUM, *EPS.values()):
        h.update(np.float64(c).tobytes())
    h.update(NULL_OMD.encode())
    return h.hexdigest()


# --------------------------------------------------------------------------
# the fixture and the error measure
# --------------------------------------------------------------------------
NX = 1 + 4 + 16 + 30   # an item's entries, flat: F, g[4], H[4][4], ell[30]
SL_F, SL_G, SL_H, SL_ELL = slice(0, 1), slice(1, 5), slice(5, 21), slice(21, 51)
QUANTITIES = (("F", SL_F), ("g", SL_G), ("H", SL_H), ("ell", SL_ELL))


def load():
    """The fixture as a dict, with the items' y and N rows expanded and `bar`
    [n][NX] assembled from the stored magnitudes and conditioning terms; `bar`
    holds the bar that applies to each model (`null_omd` names model_null's)."""
    g = dict(np.load(FIXTURE))
    g["y"], g["N"] = g["rows_y"][g["row"]], g["rows_N"][g["row"]]
    c = np.empty(NX)
    c[SL_F], c[SL_G], c[SL_H], c[SL_ELL] = C_F, C_G, C_H, C_F
    g["bar"] = c * g["mag"] + g["cond"] + ABS
    # the polish form's F and ell[30]: lrise's bars and the sums' roundings (from the generator) + cond + ABS
    g["accf_bar"] = (np.concatenate([g["accf_F"][:, None], g["accf_ell"]], 1)
                     + np.concatenate([g["cond"][:, SL_F], g["cond"][:, SL_ELL]], 1) + ABS)
    return g


def flat(F, g, H, ell):
    n = len(F)
    return np.concatenate([np.asarray(F, np.float64).reshape(n, 1), np.asarray(g, np.float64).reshape(n, 4),
                           np.asarray(H, np.float64).reshape(n, 16), np.asarray(ell, np.float64).reshape(n, 30)], 1)


def fractions(got, ref, res, bar):
    """|got - (ref + res)| / bar, elementwise (res: the reference's residual
    beyond its nearest double); a non-finite `got` gives inf."""
    with np.errstate(all="ignore"):
        err = np.abs((got - ref) - res)
        r = np.where(err == 0.0, 0.0, err / bar)
    return np.where(np.isfinite(got) & ~np.isnan(r), r, np.inf)


def worst(frac, sel):
    """{quantity: (worst fraction, item)} over the items `sel` (indices)."""
    out = {}
    for name, sl in QUANTITIES:
        f = frac[sel][:, sl]
        i = int(np.argmax(f.max(1)))
        out[name] = (float(f[i].max()), int(sel[i]))
    return out


def null_corner(fx):
    """The model_null items at logit q in {12, 25}: where 1.0 - q lost b = (1 - q) phi
    (relative 2^-53 / (1 - q)); they pass at the bar without the omD_i term (NULL_OMD)."""
    s = np.flatnonzero((fx["model"] == NULL) & np.isin(fx["u"][:, 0], (12.0, 25.0)) & (fx["group"] == EDGE))
    assert len(s) >= 12 and (fx["u"][s, 0] == 25.0).sum() >= 6
    return s


def report(tag, w):
    print(f"{tag}: worst error as a fraction of the bar: " +
          ", ".join(f"{k} {v[0]:.3f} (item {v[1]})" for k, v in w.items()))
