"""Reference of MDFIT-SUMM v1: the moments in numpy on
np.longdouble straight from their definitions (mean, ddof-1 variance, Pearson
correlation), the order statistics in float64 with np.sort, np.median and the
oracle's restatement of numpyro's hpdi.  Written from the specification, not
from the kernel's code."""

from __future__ import annotations

import numpy as np

from oracle.oracle import hpdi
from tests.nuts_diag_ref import PMD_SUBFITS, series_of

LD = np.longdouble
NFIELD = 16
STD, D_MEAN, D_MEDIAN, D_LO, D_HI, Q_MEDIAN, Q_LO, Q_HI, PHI_MEDIAN, RHO, SIGNIFICANCE, FLAGS = (
    0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
# fields compared within a tolerance (relative; rho absolute) and by value
MOMENT_FIELDS = (0, 1, 2, 3, 4, D_MEAN, RHO, SIGNIFICANCE)
ORDER_FIELDS = (D_MEDIAN, D_LO, D_HI, Q_MEDIAN, Q_LO, Q_HI, PHI_MEDIAN)


def mean_std(x):
    """(mean, std with ddof 1) of one series, longdouble; the spread of a
    constant series is 0, exactly."""
    x = np.asarray(x, dtype=LD)
    S = x.size
    mean = x.sum() / S
    if (x == x[0]).all():
        return mean, LD(0)
    return mean, np.sqrt(((x - mean) ** 2).sum() / (S - 1))


def pearson(a, b):
    """Pearson correlation, longdouble; NaN when either series is constant."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    if (a == a[0]).all() or (b == b[0]).all():
        return LD("nan")
    da, db = a - a.sum() / a.size, b - b.sum() / b.size
    return (da * db).sum() / np.sqrt((da * da).sum() * (db * db).sum())


def order_stats(x):
    """(median, lo, hi) of one float64 series: np.median and the 68 % HPDI."""
    x = np.asarray(x, dtype=np.float64)
    lo, hi = hpdi(x, 0.68)
    return float(np.median(x)), float(lo), float(hi)


def summary_rows(samples, chain_status):
    """samples[T, 6, S, 4] float64, chain_status[T, 6] -> summ[T, 6, 16]
    longdouble (flags: 1 valid, 0 not)."""
    samples = np.asarray(samples, dtype=np.float64)
    T, K, S, _ = samples.shape
    out = np.full((T, K, NFIELD), np.nan, dtype=LD)
    for t in range(T):
        for k in range(K):
            x = samples[t, k]
            if not (chain_status[t][k] == 0 and np.isfinite(x).all()):
                out[t, k, FLAGS] = 0
                continue
            q, A, c, phi, dmax = series_of(x, k)
            for s, ser in enumerate((q, A, c, phi, dmax)):
                mean, std = mean_std(ser)
                out[t, k, STD + s] = std
            out[t, k, D_MEAN] = mean
            out[t, k, SIGNIFICANCE] = mean / std if std > 0 else LD("nan")
            out[t, k, D_MEDIAN:D_HI + 1] = order_stats(dmax)
            out[t, k, Q_MEDIAN:Q_HI + 1] = order_stats(q)
            out[t, k, PHI_MEDIAN] = order_stats(phi)[0]
            out[t, k, RHO] = pearson(A, c)
            out[t, k, FLAGS] = 1
    return out


__all__ = ["PMD_SUBFITS", "summary_rows", "mean_std", "pearson", "order_stats"]
