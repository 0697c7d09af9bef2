"""Reference of MDFIT-LOO v1 in numpy on np.longdouble, written
from the specification's six steps, not from the kernel's code: np.sort, the
generalised Pareto fit of Zhang & Stephens (2009) with loo's priors as whole-array
expressions, np.logaddexp-free log-sum-exps.  Also the pointwise beta-binomial
log-pmf with scipy.special.gammaln, the record rows and the n_sigma comparisons
of fits.py:194-227."""

from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
NFIELD = 8
ELPD, P_LOO, ELPD_SE, KHAT_MAX, KHAT_ARGMAX, N_BAD, LPPD, FLAGS = range(8)
N_SIGMA, N_SIGMA_FORWARD, N_SIGMA_REVERSE, ASYMMETRY, ALL_KHAT_MAX, ALL_N_BAD = range(6)
PMD_SUBFITS = (0, 2, 3)
NPOS, NHALF = 30, 15


def points_of(k: int) -> range:
    """The columns of sub-fit k: all 30, the forward 15 or the reverse 15."""
    if k < 2:
        return range(0, NPOS)
    return range(NHALF, NPOS) if k in (3, 5) else range(0, NHALF)


def tail_len(S: int) -> int:
    return min(S // 5, math.isqrt(9 * S - 1) + 1)  # min(floor(S / 5), ceil(3 sqrt S))


def khat_threshold(S: int) -> float:
    return min(1.0 - 1.0 / math.log10(S), 0.7)


def gpd_fit(x):
    """(khat, sigma) of the ascending excesses x (longdouble, x[-1] > 0 and the
    first-quartile excess > 0): step 4."""
    M = x.size
    m = 30 + math.isqrt(M)
    xstar = x[(M + 2) // 4 - 1]
    j = np.arange(1, m + 1, dtype=LD)
    theta = 1 / x[-1] + (1 - np.sqrt(m / (j - LD(0.5)))) / (3 * xstar)
    kappa = np.log1p(-theta[:, None] * x[None, :]).mean(axis=1)
    L = M * (np.log(-theta / kappa) - kappa - 1)
    w = 1 / np.exp(L[None, :] - L[:, None]).sum(axis=1)
    theta_hat = (w * theta).sum()
    kappa_hat = np.log1p(-theta_hat * x).mean()
    return (M * kappa_hat + 5) / (M + 10), -kappa_hat / theta_hat


def _lse(v):
    mx = v.max()
    return mx + np.log(np.exp(v - mx).sum())


def psis(ll):
    """(elpd, khat) of one pointwise log-likelihood series (float64 in,
    longdouble out): steps 1-6.  A series with a value that is not finite: NaN."""
    ll = np.asarray(ll, dtype=np.float64)
    S = ll.size
    if not np.isfinite(ll).all():
        return LD("nan"), LD("nan")
    r = -ll.astype(LD)
    c = r.max()
    rt = np.sort(r - c)
    M = tail_len(S)
    wt = rt.copy()
    khat = LD("inf")
    if M >= 5:
        eu = np.exp(rt[S - M - 1])
        x = np.maximum(np.exp(rt[S - M:]) - eu, 0)
        if x[-1] == 0:
            khat = LD(0)
        elif x[(M + 2) // 4 - 1] > 0:
            khat, sigma = gpd_fit(x)
            if np.isfinite(khat):
                l1 = np.log1p(-(np.arange(M, dtype=LD) + LD(0.5)) / M)
                if abs(khat) < 30 * np.finfo(np.float64).eps:
                    q = -sigma * l1
                else:
                    q = sigma * np.expm1(-khat * l1) / khat
                wt[S - M:] = np.minimum(np.log(q + eu), 0)
    return _lse(wt - rt) - _lse(wt) - c, khat


def lppd(ll):
    ll = np.asarray(ll, dtype=np.float64).astype(LD)
    return _lse(ll) - np.log(LD(ll.size))


def d_at(theta, pmd: bool, k: int):
    """The model's damage at |z| - 1 = k from draws theta[S, 4] (longdouble),
    clipped to [0, 1] as the kernel's d_at."""
    q, A, c = theta[:, 0], theta[:, 1], theta[:, 2]
    D = A * (1 - q) ** k + c if pmd else q
    return np.clip(D, 0, 1)


def log_likelihood(theta, pmd: bool, k: int, y, N):
    """The full beta-binomial log-pmf of every draw at one point, log C(N, y)
    included: scipy's gammaln on float64 arguments, combined in longdouble."""
    from scipy.special import gammaln

    th = np.asarray(theta, dtype=np.float64).astype(LD)
    D, phi = d_at(th, pmd, k), th[:, 3]
    a, b = D * phi, (1 - D) * phi
    g = lambda v: gammaln(np.asarray(v, dtype=np.float64)).astype(LD)  # noqa: E731
    y, N = LD(y), LD(N)
    return (g(N + 1) - g(y + 1) - g(N - y + 1) + (g(y + a) - g(a)) + (g(N - y + b) - g(b))
            - (g(N + phi) - g(a + b)))


def n_sigma(a, b):
    """fits.py:194-227 on two pointwise columns: a the PMD model's, b the null's."""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    d = a - b
    n = d.size
    return (b.sum() - a.sum()) / np.sqrt(n * ((d - d.mean()) ** 2).mean())


def rows_from_pointwise(pw, lp, valid, S: int):
    """loo[7, 8] longdouble of one taxon from pw[6, 30, 2] = (elpd_i, khat_i),
    lp[6, 30] = lppd_i (NaN outside a sub-fit's points) and valid[6]."""
    out = np.full((7, NFIELD), np.nan, dtype=LD)
    tau = khat_threshold(S)
    looic = np.full((7, NPOS), np.nan, dtype=LD)
    for k in range(6):
        cols = list(points_of(k))
        if not valid[k]:
            out[k, FLAGS] = 0
            continue
        e, kh, l = pw[k, cols, 0].astype(LD), pw[k, cols, 1].astype(LD), lp[k, cols].astype(LD)
        n = len(cols)
        out[k, ELPD] = e.sum()
        out[k, P_LOO] = (l - e).sum()
        out[k, ELPD_SE] = np.sqrt(n * ((e - e.mean()) ** 2).mean())
        out[k, KHAT_MAX] = kh.max()
        out[k, KHAT_ARGMAX] = cols[int(np.argmax(kh))]
        out[k, N_BAD] = (kh > tau).sum()
        out[k, LPPD] = l.sum()
        out[k, FLAGS] = 1
        looic[k, cols] = -2 * e
    looic[6, :NHALF], looic[6, NHALF:] = looic[2, :NHALF], looic[3, NHALF:]
    with np.errstate(invalid="ignore"):
        out[6, N_SIGMA] = n_sigma(looic[0], looic[1])
        out[6, N_SIGMA_FORWARD] = n_sigma(looic[2, :NHALF], looic[4, :NHALF])
        out[6, N_SIGMA_REVERSE] = n_sigma(looic[3, NHALF:], looic[5, NHALF:])
        out[6, ASYMMETRY] = n_sigma(looic[0], looic[6])
    ok = np.asarray(valid, dtype=bool)
    if ok.any():
        out[6, ALL_KHAT_MAX] = out[:6, KHAT_MAX][ok].max()
    out[6, ALL_N_BAD] = out[:6, N_BAD][ok].sum()
    out[6, 6] = 0
    out[6, FLAGS] = 1 if ok.all() else 0
    return out


def loo_rows(samples, chain_status, y, N):
    """samples[T, 6, S, 4] float64, chain_status[T, 6], y, N[T, >= 30] ->
    (loo[T, 7, 8], pointwise[T, 6, 30, 2], ll[T, 6, 30, S]) longdouble, fed the
    reference's own log-likelihoods."""
    samples = np.asarray(samples, dtype=np.float64)
    T, K, S, _ = samples.shape
    loo = np.full((T, 7, NFIELD), np.nan, dtype=LD)
    pw = np.full((T, K, NPOS, 2), np.nan, dtype=LD)
    ll = np.full((T, K, NPOS, S), np.nan, dtype=LD)
    for t in range(T):
        if (np.asarray(y[t][:NPOS]) > np.asarray(N[t][:NPOS])).any():
            loo[t, :, FLAGS] = 0
            continue
        lp = np.full((K, NPOS), np.nan, dtype=LD)
        valid = np.zeros(K, bool)
        for k in range(K):
            ok = chain_status[t][k] == 0
            for col in points_of(k):
                ll[t, k, col] = log_likelihood(samples[t, k], k in PMD_SUBFITS, col % NHALF, y[t][col], N[t][col])
                ok = ok and bool(np.isfinite(ll[t, k, col]).all())
            valid[k] = ok
            if not ok:
                continue
            for col in points_of(k):
                l64 = ll[t, k, col].astype(np.float64)
                pw[t, k, col] = psis(l64)
                lp[k, col] = lppd(l64)
        loo[t] = rows_from_pointwise(pw[t], lp, valid, S)
    return loo, pw, ll
