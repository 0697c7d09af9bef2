"""Crafted draws for the sampling-diagnostics tests (tests/test_nuts_diag.py on
the host program, tests/test_gpu_nuts_diag.py on the kernel): the series kinds
and shapes at which the statistic's code paths differ, and the condition under
which its one discrete decision -- where the lag sum stops -- is not a matter
of rounding."""

from __future__ import annotations

import functools

import numpy as np

from tests import nuts_diag_ref as ref

KINDS = ("iid", "ar09", "ar0999", "arneg05", "alt", "const", "offset", "trend")
S_VALUES = (2, 3, 4, 5, 63, 64, 65, 127, 129, 1000, 1001, 4096)
# (S, T): every S at T = 3; T = 1 and T = 67 (more rows than one block) at small S
SHAPES = tuple((S, 3) for S in S_VALUES) + ((5, 1), (1000, 1), (65, 67))
SEED = 11  # chosen so that decision_margin_ok holds for every shape (checked by the CPU test)
P_MARGIN = 1e-6


def _ar1(rng, S, phi):
    z = rng.standard_normal(S)
    x = np.empty(S)
    x[0] = z[0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, S):
        x[t] = phi * x[t - 1] + z[t]
    return x


def series(kind: str, S: int, rng) -> np.ndarray:
    if kind == "iid":
        return rng.standard_normal(S)
    if kind == "ar09":
        return _ar1(rng, S, 0.9)
    if kind == "ar0999":  # the truncation runs to far lags: the S^2 path
        return _ar1(rng, S, 0.999)
    if kind == "arneg05":  # antithetic: ess > S
        return _ar1(rng, S, -0.5)
    if kind == "alt":  # strictly alternating: reaches the S log10 S cap
        return np.where(np.arange(S) % 2 == 0, 1.0, -1.0)
    if kind == "const":  # gamma_0 == 0: NaN
        return np.full(S, 0.3)
    if kind == "offset":  # fails without centring
        return 1e8 + 1e-3 * rng.standard_normal(S)
    if kind == "trend":  # rhat far above 1
        return np.arange(S, dtype=np.float64) / S + 1e-3 * rng.standard_normal(S)
    raise ValueError(kind)


def kind_of(t: int, k: int, j: int) -> str:
    return KINDS[(5 * t + 3 * k + j) % len(KINDS)]


def faults(T: int):
    """((t, k) of the row with one NaN draw, (t, k) of the row whose chain status is non-zero)."""
    return ((1, 2), (2, 4)) if T >= 3 else ((0, 3), (0, 5))


@functools.lru_cache(maxsize=None)
def case(S: int, T: int):
    """(samples[T, 6, S, 4] float64, chain_status[T, 6] float64) of one shape."""
    rng = np.random.default_rng([SEED, S, T])
    x = np.empty((T, 6, S, 4))
    for t in range(T):
        for k in range(6):
            for j in range(4):
                x[t, k, :, j] = series(kind_of(t, k, j), S, rng)
    status = np.zeros((T, 6))
    (tn, kn), (ts, ks) = faults(T)
    x[tn, kn, S // 2, 1] = np.nan
    status[ts, ks] = 2.0
    x.setflags(write=False)
    status.setflags(write=False)
    return x, status


@functools.lru_cache(maxsize=None)
def reference(S: int, T: int):
    """(diag[T, 6, 12] longdouble, trace) of the shape's case; computed once."""
    x, status = case(S, T)
    want, tr = ref.diag_rows(x, status, trace=True)
    want.setflags(write=False)
    return want, tr


def decision_margin_ok(tr) -> list:
    """The series of a trace whose stopping decision could hinge on rounding
    (empty: none).  The sum stops at the first raw P_j <= 0, so every decision
    taken is the sign of a raw P_j; it is safe when |P_j| > P_MARGIN at every
    pair evaluated -- the stopping pair and the one before it among them.  One
    exception needs no margin: when P_0 < P_MARGIN, every later term is at most
    P_0 (the running minimum), the whole sum is below S/2 * 1e-6 < 0.01, tau is
    below -0.98 and the ESS sits at the S log10 S cap whichever way any
    decision goes (the alternating series, whose P_0 is -1/(S(S-1)))."""
    bad = []
    for t, k, s, raws, _stopped in tr:
        if not raws or raws[0] < P_MARGIN:
            continue
        if min(abs(r) for r in raws) <= P_MARGIN:
            bad.append((t, k, s))
    return bad
