"""Crafted raw log-weight series for the smoothing of MDFIT-PSIS v1
(tests/test_map_psis.py on the host program, tests/test_gpu_map_psis.py on
mdfit_psis_weights), with their reference weights computed once."""

from __future__ import annotations

import functools

import numpy as np

from tests import map_psis_ref as ref

# 25: the smallest S (a five-draw tail); 26; 64 / 65: the lanes; 100: no power
# of two; 256: the default; 1024: the bound
S_VALUES = (25, 26, 64, 65, 100, 256, 1024)
KINDS = ("pareto0.2", "pareto0.5", "pareto0.9", "gauss1", "gauss30", "const", "const_tail", "ties", "xstar0",
         "one_inf", "many_inf", "cut_edge", "cut_inf", "all_inf", "nan", "posinf")
SEED = 31


def series(kind: str, S: int, rng) -> np.ndarray:
    """One raw log-weight series lw[S] float64; -inf is an infeasible draw."""
    M = ref.tail_len(S)
    if kind.startswith("pareto"):  # importance ratios (1 - u)^(-k)
        return 3.0 - float(kind[6:]) * np.log1p(-rng.uniform(size=S))
    if kind == "gauss1":
        return 2.0e4 + rng.standard_normal(S)
    if kind == "gauss30":  # a few draws carry everything
        return -50.0 + 30.0 * rng.standard_normal(S)
    if kind == "const":  # uniform weights, khat 0
        return np.full(S, 1.25)
    if kind == "const_tail":  # the tail and its cut-off equal: khat 0, nothing smoothed
        r = np.sort(rng.standard_normal(S))
        r[S - M - 1:] = r[S - M - 1]
        return rng.permutation(r)
    if kind == "ties":  # a coarse grid: equal values across the cut-off rank
        return 7.0 + np.rint(3.0 * rng.standard_normal(S)) / 3.0
    if kind == "xstar0":  # the tail's lowest quarter equals the cut-off, its top does not
        r = np.sort(rng.standard_normal(S))
        r[S - M - 1:S - M + (M + 2) // 4] = r[S - M - 1]
        return rng.permutation(r)
    lw = 5.0 + 1.5 * rng.standard_normal(S)
    if kind == "one_inf":
        lw[rng.integers(S)] = -np.inf
    elif kind == "many_inf":
        lw[rng.permutation(S)[: S // 3]] = -np.inf
    elif kind == "cut_edge":  # one fewer than reaches the cut-off rank: valid
        lw[rng.permutation(S)[: S - M - 1]] = -np.inf
    elif kind == "cut_inf":  # the cut-off draw is infeasible: invalid
        lw[rng.permutation(S)[: S - M]] = -np.inf
    elif kind == "all_inf":
        lw[:] = -np.inf
    elif kind == "nan":
        lw[rng.integers(S)] = np.nan
    elif kind == "posinf":
        lw[rng.integers(S)] = np.inf
    else:
        raise ValueError(kind)
    return lw


@functools.lru_cache(maxsize=None)
def weights_case(S: int, n: int | None = None):
    """(lw[n, S] float64, kinds): every kind once, or n series cycling through them."""
    kinds = KINDS if n is None else tuple(KINDS[i % len(KINDS)] for i in range(n))
    rng = np.random.default_rng([SEED, S, len(kinds)])
    lw = np.stack([series(k, S, rng) for k in kinds])
    lw.setflags(write=False)
    return lw, kinds


@functools.lru_cache(maxsize=None)
def weights_reference(S: int, n: int | None = None):
    """(w[n, S], khat[n], valid[n]) longdouble of weights_case(S, n); computed once."""
    lw, _ = weights_case(S, n)
    got = [ref.psis_weights(l) for l in lw]
    w = np.stack([g[0] for g in got])
    k = np.array([g[1] for g in got], dtype=ref.LD)
    v = np.array([g[3] for g in got])
    for a in (w, k, v):
        a.setflags(write=False)
    return w, k, v


@functools.lru_cache(maxsize=None)
def draws_case(S: int, n: int):
    """f[n, S, 4] = (q, A, c, phi) float64 for the estimates of the host program."""
    rng = np.random.default_rng([SEED, S, n, 5])
    f = np.stack([rng.uniform(0.05, 0.9, (n, S)), rng.uniform(0.01, 0.6, (n, S)), rng.uniform(0.0, 0.3, (n, S)),
                  2.0 + 10.0 ** rng.uniform(0.0, 4.0, (n, S))], axis=-1)
    f.setflags(write=False)
    return f


def weight_errors(w, khat, want_w, want_k, want_valid):
    """NaN exactly where the reference has it, khat's special values (+inf,
    exactly 0) by value; returns the worst errors {"w": of a weight relative to
    the series' largest, "khat": absolute}."""
    w, khat = np.asarray(w, np.float64), np.asarray(khat, np.float64)
    want_valid = np.asarray(want_valid, bool)
    assert np.array_equal(np.isnan(khat), ~want_valid), (np.isnan(khat), want_valid)
    assert np.array_equal(np.isnan(w), np.isnan(want_w.astype(np.float64)))
    wk64 = want_k.astype(np.float64)
    special = want_valid & (np.isinf(wk64) | (wk64 == 0))
    assert np.array_equal(khat[special], wk64[special]), (khat[special], wk64[special])
    ok = want_valid
    err_w = np.abs(w[ok].astype(ref.LD) - want_w[ok]) / want_w[ok].max(axis=1, keepdims=True)
    okk = want_valid & ~special
    err_k = np.abs(khat[okk].astype(ref.LD) - want_k[okk])
    return {"w": float(err_w.max()) if err_w.size else 0.0, "khat": float(err_k.max()) if err_k.size else 0.0}
