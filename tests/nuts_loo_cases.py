"""Crafted inputs for the PSIS-LOO tests (tests/test_nuts_loo.py on the host
program, tests/test_gpu_nuts_loo.py on the kernels): pointwise log-likelihood
series at the lane, sort-path and M < 5 edges, and small crafted draws, y and N
for mdfit_nuts_loo with the CPU-side precondition on near-ties at the cutoff
rank."""

from __future__ import annotations

import functools

import numpy as np

from tests import nuts_loo_ref as ref

# 24 / 25: M < 5 and the first fit; 63 .. 65 and 129: the lanes; 1000: the
# default (the register sort); 1024 / 1025: the sort's padding; 4096: the bound
S_VALUES = (2, 24, 25, 63, 64, 65, 129, 1000, 1024, 1025, 4096)
KINDS = ("pareto0.2", "pareto0.5", "pareto0.9", "gauss0.1", "gauss2", "const", "ties", "xstar0", "offset")
BATCH = (65, 67)  # one batch with more series than a few: 67 at S = 65
SEED = 29


def series(kind: str, S: int, rng) -> np.ndarray:
    """One pointwise log-likelihood series l[S] float64."""
    if kind.startswith("pareto"):  # importance ratios (1 - u)^(-k): l = -log ratio
        return float(kind[6:]) * np.log1p(-rng.uniform(size=S))
    if kind == "gauss0.1":
        return -3.0 + 0.1 * rng.standard_normal(S)
    if kind == "gauss2":
        return -40.0 + 2.0 * rng.standard_normal(S)
    if kind == "const":
        return np.full(S, -2.75)
    if kind == "ties":  # a coarse grid: equal values across the cutoff rank
        return -5.0 + np.rint(4.0 * rng.standard_normal(S)) / 4.0
    if kind == "offset":  # N ~ 1e6 and a poor fit: large, widely spread
        return -1.0e4 + 30.0 * rng.standard_normal(S)
    if kind == "xstar0":  # the tail's lowest quarter equals the cutoff, its top does not
        l = -3.0 + rng.standard_normal(S)
        M = ref.tail_len(S)
        if M >= 5:
            r = np.sort(-l)
            r[S - M - 1:S - M + (M + 2) // 4] = r[S - M - 1]
            l = -rng.permutation(r)
        return l
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def psis_case(S: int, n: int | None = None):
    """(ll[n, S] float64, kinds): every kind once, or n series cycling through them."""
    kinds = KINDS if n is None else tuple(KINDS[i % len(KINDS)] for i in range(n))
    rng = np.random.default_rng([SEED, S, len(kinds)])
    ll = np.stack([series(k, S, rng) for k in kinds])
    ll.setflags(write=False)
    return ll, kinds


PSIS_SHAPES = tuple((S, None) for S in S_VALUES) + (BATCH,)


@functools.lru_cache(maxsize=None)
def psis_reference(S: int, n: int | None = None):
    """(elpd[n], khat[n]) longdouble of psis_case(S, n); computed once."""
    ll, _ = psis_case(S, n)
    got = np.array([ref.psis(l) for l in ll], dtype=ref.LD)
    got.setflags(write=False)
    return got[:, 0], got[:, 1]


def special_series():
    """Series whose result is a special value: (name, l)."""
    rng = np.random.default_rng([SEED, 7])
    base = -3.0 + rng.standard_normal(200)
    nan, ninf, pinf = base.copy(), base.copy(), base.copy()
    nan[17] = np.nan
    ninf[3] = -np.inf
    pinf[150] = np.inf
    flat_tail = base.copy()  # the whole tail and its cutoff equal: khat 0 although the series is not constant
    M = ref.tail_len(200)
    r = np.sort(-flat_tail)
    r[200 - M - 1:] = r[200 - M - 1]
    flat_tail = -rng.permutation(r)
    return [("nan", nan), ("-inf", ninf), ("+inf", pinf), ("const", np.full(200, -1.5)), ("flat_tail", flat_tail),
            ("xstar0", series("xstar0", 200, rng)), ("ties", series("ties", 200, rng)),
            ("S24", base[:24]), ("S2", base[:2])]


# --------------------------------------------------------------------------
# crafted draws for mdfit_nuts_loo
# --------------------------------------------------------------------------
LOO_SHAPES = ((65, 3), (1000, 2))  # (S, T)
# the device's log-likelihood against the reference's (scipy gammaln on float64
# arguments combined in longdouble): the worst absolute difference relative to
# max(1, |l|) measured on the MI355X over these cases; two
# distinct values of a series closer than this at the cutoff rank may change
# rank between the two
LL_ERROR = 6.0e-10
MAX_EXEMPT = 0.01


@functools.lru_cache(maxsize=None)
def loo_case(S: int, T: int):
    """(samples[T, 6, S, 4], chain_status[T, 6], y[T, 32] uint32, N[T, 32]
    uint32).  Taxon 0 has a position with N = 0, one with y = N and one with N
    ~ 1e6; the last taxon has one failed chain and one NaN draw."""
    rng = np.random.default_rng([SEED, S, T, 3])
    x = np.zeros((T, 6, S, 4))
    for t in range(T):
        q0, A0, c0, p0 = rng.uniform(0.2, 0.6), rng.uniform(0.05, 0.3), rng.uniform(0.005, 0.02), 10 ** rng.uniform(1.5, 3)
        for k in range(6):
            x[t, k, :, 0] = np.clip(q0 + 0.05 * rng.standard_normal(S), 0.01, 0.99)
            x[t, k, :, 3] = p0 * np.exp(0.2 * rng.standard_normal(S))
            if k in ref.PMD_SUBFITS:
                x[t, k, :, 1] = np.clip(A0 + 0.02 * rng.standard_normal(S), 0.001, 0.9)
                x[t, k, :, 2] = np.clip(c0 + 0.002 * rng.standard_normal(S), 0.0005, 0.09)
            else:  # a null sub-fit: D = q, small
                x[t, k, :, 0] = np.clip(0.03 + 0.004 * rng.standard_normal(S), 0.001, 0.99)
    N = np.zeros((T, 32), np.uint32)
    y = np.zeros((T, 32), np.uint32)
    N[:, :30] = rng.integers(50, 5000, (T, 30))
    N[0, 4] = 0
    N[0, 9] = 1_000_003
    N[0, 20] = 7
    z = np.tile(np.arange(15), 2)
    D = x[:, 0, 0, 1:2] * (1 - x[:, 0, 0, 0:1]) ** z[None, :] + x[:, 0, 0, 2:3]
    y[:, :30] = rng.binomial(N[:, :30], D)
    y[0, 20] = 7  # y = N
    status = np.zeros((T, 6))
    status[T - 1, 4] = 2.0
    x[T - 1, 3, S // 2, 3] = np.nan
    for a in (x, status, y, N):
        a.setflags(write=False)
    return x, status, y, N


@functools.lru_cache(maxsize=None)
def loo_reference(S: int, T: int):
    """(loo[T, 7, 8], pointwise[T, 6, 30, 2], exempt[T, 6, 30]) of loo_case:
    exempt marks the series with two distinct log-likelihoods within LL_ERROR of
    each other at the cutoff rank."""
    x, status, y, N = loo_case(S, T)
    loo, pw, ll = ref.loo_rows(x, status, y, N)
    M = ref.tail_len(S)
    exempt = np.zeros((T, 6, ref.NPOS), bool)
    if M >= 5:
        r = np.sort(-ll, axis=-1)
        u, above = r[..., S - M - 1], r[..., S - M]
        gap = above - u
        with np.errstate(invalid="ignore"):
            exempt = (gap != 0) & (gap <= LL_ERROR * np.maximum(1, np.abs(u)))
    for a in (loo, pw, exempt):
        a.setflags(write=False)
    return loo, pw, exempt
