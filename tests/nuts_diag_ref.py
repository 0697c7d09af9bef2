"""Reference of MDFIT-DIAG v1 in numpy on np.longdouble: the
single-chain effective sample size (Geyer's initial monotone sequence, capped
at S log10 S), split R-hat and Monte Carlo standard error, with direct lag sums
(no FFT).  Written from the specification, not from the kernel's code."""

from __future__ import annotations

import numpy as np

LD = np.longdouble
NFIELD = 12
ESS, RHAT, MCSE, FLAGS = 0, 5, 10, 11
PMD_SUBFITS = (0, 2, 3)  # sub-fit k: 0 PMD-all, 1 null-all, 2 PMD-fwd, 3 PMD-rev, 4 null-fwd, 5 null-rev


def series_stats(x, trace: bool = False):
    """(ess, rhat, mcse) of one series, longdouble.  trace: also the raw
    (unclipped) P_j of every pair evaluated, in order, and whether the last of
    them stopped the sum (False: the sum ran to the last pair)."""
    x = np.asarray(x, dtype=LD)
    S = x.size
    nan = LD("nan")
    # mean(x) taken about the first draw: the same number, and d == 0 exactly for a constant series
    e = x - x[0]
    d = e - e.sum() / S
    g0 = (d * d).sum() / S
    if not g0 > 0:
        return (nan, nan, nan, [], False) if trace else (nan, nan, nan)
    h = S // 2
    rhat = nan
    if h >= 2:
        a, b = d[:h], d[S - h:]
        ma, mb = a.sum() / h, b.sum() / h
        va, vb = ((a - ma) ** 2).sum() / (h - 1), ((b - mb) ** 2).sum() / (h - 1)
        W = (va + vb) / 2
        mm = (ma + mb) / 2
        B = ((ma - mm) ** 2 + (mb - mm) ** 2) / (2 - 1)
        if W > 0:
            rhat = np.sqrt((W * LD(h - 1) / LD(h) + B) / W)

    def rho(k):
        if k == 0:
            return LD(1)
        return (d[: S - k] * d[k:]).sum() / S / g0 - LD(1) / LD(S - 1)

    total = LD(0)
    prev = None
    raws = []
    stopped = False
    for j in range(h):
        raw = rho(2 * j) + rho(2 * j + 1)
        raws.append(raw)
        P = raw
        if j > 0:
            P = min(max(P, LD(0)), prev)
        if not P > 0:
            if j == 0:
                total = P
            stopped = True
            break
        total += P
        prev = P
    tau = -1 + 2 * total
    ess = S / max(tau, 1 / np.log10(LD(S)))
    mcse = np.sqrt(g0 * LD(S) / LD(S - 1) / ess)
    if trace:
        return ess, rhat, mcse, raws, stopped
    return ess, rhat, mcse


def series_of(draws, sub: int):
    """The five series (q, A, c, phi, D_max) of one sub-fit's draws [S, 4], longdouble."""
    x = np.asarray(draws, dtype=np.float64)
    dmax = x[:, 1] + x[:, 2] if sub in PMD_SUBFITS else x[:, 0]  # (the FP64 sum is the series)
    return [x[:, 0], x[:, 1], x[:, 2], x[:, 3], dmax]


def diag_rows(samples, chain_status, trace: bool = False):
    """samples[T, 6, S, 4] float64, chain_status[T, 6] -> diag[T, 6, 12]
    longdouble (flags: 1 valid, 0 not).  trace: also a list of (t, k, series,
    raw P_j of the evaluated pairs, stopped) per evaluated series."""
    samples = np.asarray(samples, dtype=np.float64)
    T, K, S, _ = samples.shape
    out = np.full((T, K, NFIELD), np.nan, dtype=LD)
    tr = []
    for t in range(T):
        for k in range(K):
            x = samples[t, k]
            if not (chain_status[t][k] == 0 and np.isfinite(x).all()):
                out[t, k, FLAGS] = 0
                continue
            for s, ser in enumerate(series_of(x, k)):
                ess, rhat, mcse, raws, stopped = series_stats(ser, trace=True)
                out[t, k, ESS + s] = ess
                out[t, k, RHAT + s] = rhat
                if s == 4:
                    out[t, k, MCSE] = mcse
                tr.append((t, k, s, raws, stopped))
            out[t, k, FLAGS] = 1
    return (out, tr) if trace else out
