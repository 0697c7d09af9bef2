"""Crafted series for the pointwise accumulation of MDFIT-WAIC v1 (DESIGN.md
§3.9; a helper, no test): normalised weights w[S], log-pmf values l[S, n] and
shifts l0[n] per kind, and the reference's lppd_i and p_i for them."""

from __future__ import annotations

import numpy as np

from tests import map_waic_ref as ref

S_VALUES = (25, 64, 65, 100, 256, 1024)
KINDS = ("random", "random15", "const", "zeros", "one", "span", "deep", "deep15")


def _weights(rng, S, heavy):
    lw = rng.standard_normal(S) * (3.0 if heavy else 1.0)
    w = np.exp(lw - lw.max())
    return w / w.sum()


def series(S: int, kind: str, seed: int = 0):
    """(w[S], l[S, n], l0[n], khat) float64 of one crafted series."""
    rng = np.random.default_rng([S, KINDS.index(kind), seed])
    n = 15 if kind.endswith("15") else 30
    w = _weights(rng, S, heavy=seed % 2 == 1)
    centre = -rng.uniform(1.0, 12.0, n)
    l = centre[None, :] + rng.standard_normal((S, n)) * rng.uniform(0.01, 1.5, n)[None, :]
    if kind == "const":  # one column the same in every draw, one column of exact zeros (N = 0)
        l[:, 3] = -7.25
        l[:, 11] = 0.0
    elif kind == "zeros":  # a third of the draws infeasible: weight 0, their values never read
        dead = rng.random(S) < 0.33
        dead[int(np.argmax(w))] = False
        w = np.where(dead, 0.0, w)
        w = w / w.sum()
        l[dead] = np.nan
    elif kind == "one":  # one draw holds all the weight
        k = int(rng.integers(S))
        w = np.zeros(S)
        w[k] = 1.0
    elif kind == "span":  # -1e4 ... 0 in one column
        l[:, 5] = -np.linspace(0.0, 1e4, S)[rng.permutation(S)]
    elif kind.startswith("deep"):  # below exp's underflow in every draw of a column
        l[:, 2] = -800.0 - np.abs(rng.standard_normal(S)) * 20.0
        l[:, 7] = -5000.0 + rng.standard_normal(S) * 0.3
    top = int(np.argmax(w))
    l0 = l[top].copy()  # the shift: the values at the heaviest draw, as the mode's
    return w, l, l0, float(rng.uniform(-0.2, 1.0))


def all_series(S: int, reps: int = 3):
    return [(kind, seed, *series(S, kind, seed)) for kind in KINDS for seed in range(reps)]


def reference(w, l):
    """(lppd_i, p_i) longdouble of one series."""
    return ref.points(w, l)


def errors(lppd, p, want_lppd, want_p):
    """Worst deviations of one series: lppd absolute over max(1, |lppd|), p
    relative (a p of exactly 0 is checked on its own)."""
    wl, wp = np.asarray(want_lppd, np.longdouble), np.asarray(want_p, np.longdouble)
    e_l = float((np.abs(lppd - wl) / np.maximum(1, np.abs(wl))).max())
    nz = wp != 0
    e_p = float((np.abs(p[nz] - wp[nz]) / np.abs(wp[nz])).max()) if nz.any() else 0.0
    return {"lppd": e_l, "p": e_p}
