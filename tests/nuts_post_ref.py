"""Reference of the NUTS record assembly (the post kernel),
written from the specification and not from the kernel's or the oracle's code:

  * np.median and numpyro's hpdi(prob = 0.68) on the fractions count / N of the
    predictive draws, as oracle.hpdi states it (np.sort, np.argmin: the first of
    the shortest windows);
  * waic_i by the two passes of fits.py:126-172 (scipy logsumexp-style and
    np.var) -- in float64 with scipy's gammaln for the value class, and from
    mpmath at 60 digits for the values (tests/golden/make_golden_nuts_post.py);
  * n_sigma and asymmetry of fits.py:194-227 in longdouble, with the condition
    number of their sums;
  * the posterior means in longdouble;
  * the exact moments of the Beta-Binomial for the distribution check.
"""

from __future__ import annotations

import math

import numpy as np

LDBL = np.longdouble
NPOS, NHALF = 30, 15
K = np.tile(np.arange(NHALF), 2)
PMD_SUBFITS = (0, 2, 3)
EPS = 2.0 ** -53
NO_COUNT = 0xFFFFFFFF

# record fields (include/mdfit.h)
F_D_MAX, F_D_MAX_LO, F_D_MAX_HI = 0, 1, 2


def points_of(k: int) -> range:
    """The columns of sub-fit k: all 30, the forward 15 or the reverse 15."""
    if k < 2:
        return range(0, NPOS)
    return range(NHALF, NPOS) if k in (3, 5) else range(0, NHALF)


# ---------------------------------------------------------------------------
# median and HPDI
# ---------------------------------------------------------------------------
def median_hpdi(counts, N, valid=True):
    """(median, lo, hi) float64 of the fractions counts / N (counts uint32[S]):
    np.median and numpyro.diagnostics.hpdi(x, 0.68).  NaN when the job was
    skipped (N = 0) or a draw was no count."""
    if N == 0 or not valid:
        return np.full(3, np.nan)
    x = np.sort(np.asarray(counts, np.float64) / np.float64(N))
    n = x.size
    length = int(0.68 * n)
    widths = x[length:] - x[: n - length]
    i = int(np.argmin(widths))
    return np.array([np.median(x), x[i], x[i + length]])


# ---------------------------------------------------------------------------
# pointwise log-likelihood and WAIC
# ---------------------------------------------------------------------------
def d_of(theta, pmd: bool, col: int):
    """D of the draws theta[S, 4] at column col, float64, as the model forms it."""
    if not pmd:
        D = theta[:, 0].copy()
    else:
        D = theta[:, 1] * (1.0 - theta[:, 0]) ** K[col] + theta[:, 2]
    return np.clip(D, 0.0, 1.0)


def loglik64(y, N, D, phi, with_e=False):
    """The full beta-binomial log-pmf in float64 (scipy gammaln): the value
    class.  with_e: also e_lp, the sum over the nine lnGamma values f of the fast
    form's contract 2.5e-14 + 4.5e-16 |f|."""
    from scipy.special import gammaln

    y, N = float(y), float(N)
    a, b = D * phi, (1.0 - D) * phi
    with np.errstate(all="ignore"):
        t = [gammaln(N + 1) + 0 * a, gammaln(y + 1) + 0 * a, gammaln(N - y + 1) + 0 * a, gammaln(y + a), gammaln(a),
             gammaln(N - y + b), gammaln(b), gammaln(N + phi), gammaln(a + b)]
        lp = t[0] - t[1] - t[2] + t[3] - t[4] + t[5] - t[6] - t[7] + t[8]
        if not with_e:
            return lp
        return lp, sum(2.5e-14 + 4.5e-16 * np.abs(f) for f in t)


def waic_two_pass(lp):
    """waic_i of one series lp[S] (any float type) by the two passes of
    fits.py:147-172: logsumexp - log S and the population variance."""
    lp = np.asarray(lp)
    S = lp.size
    with np.errstate(all="ignore"):
        mx = lp.max()
        lppd = mx + np.log(np.exp(lp - mx).sum()) - np.log(lp.dtype.type(S))
        var = ((lp - lp.mean()) ** 2).mean()
        return -2 * (lppd - var)


def waic_class(x, y, N, with_mag=False):
    """waic64[T, 6, 30] by float64 gammaln: finite values where the reference is
    finite, NaN / inf where it is not (and NaN at the columns a sub-fit has not).
    with_mag: also mag[T, 6, 30, 5], the magnitudes of waic_bar from the float64
    log-likelihoods (a bar needs its magnitudes to a few per cent only)."""
    T = x.shape[0]
    w = np.full((T, 6, NPOS), np.nan)
    mag = np.full((T, 6, NPOS, 5), np.nan)
    for t in range(T):
        for k in range(6):
            for col in points_of(k):
                D = d_of(x[t, k], k in PMD_SUBFITS, col)
                lp, e = loglik64(y[t, col], N[t, col], D, x[t, k, :, 3], with_e=True)
                w[t, k, col] = waic_two_pass(lp)
                if with_mag and np.isfinite(w[t, k, col]):
                    mx = lp.max()
                    lppd = mx + np.log(np.exp(lp - mx).sum()) - np.log(lp.size)
                    mag[t, k, col] = (e.max(), lp.std(), abs(lppd), lp.var(), np.abs(lp).mean())
    return (w, mag) if with_mag else w


def waic_bar(S, e_lp, sd, lppd, var, mean_abs):
    """The bar on waic_i: the fast lnGamma's contract through
    lppd and the variance, plus the one-pass summation."""
    return 2.0 * (1.0 + 2.0 * sd) * e_lp + (math.ceil(S / 64) + 8) * EPS * (abs(lppd) + var + mean_abs)


# ---------------------------------------------------------------------------
# n_sigma, asymmetry
# ---------------------------------------------------------------------------
def _nsig(wp, wn):
    """(value, bar) of (sum wn - sum wp) / sqrt(n var(wp - wn)) in longdouble;
    bar = 64 eps kappa |value| with kappa the condition numbers of the sums."""
    wp, wn = np.asarray(wp, LDBL), np.asarray(wn, LDBL)
    n = wp.size
    with np.errstate(all="ignore"):
        d = wp - wn
        num = wn.sum() - wp.sum()
        md = d.mean()
        dev = d - md
        var = (dev * dev).mean()
        val = num / np.sqrt(n * var)
        # condition: the numerator's sum, the mean inside the deviations, and
        # the subtraction of each pair
        k_num = (np.abs(wn).sum() + np.abs(wp).sum()) / abs(num)
        k_dev = ((np.abs(wp) + np.abs(wn) + abs(md)) * np.abs(dev)).sum() / (dev * dev).sum()
        kappa = 1.0 + k_num + k_dev
        bar = 64 * EPS * kappa * abs(val)
    return val, bar


def n_sigma_block(waic):
    """[(value, bar)] x 4 of n_sigma, n_sigma_forward, n_sigma_reverse and
    asymmetry from waic[6, 30] (fits.py:194-227)."""
    f, r = slice(0, NHALF), slice(NHALF, NPOS)
    fr = np.concatenate([waic[2, f], waic[3, r]])
    return [_nsig(waic[0], waic[1]), _nsig(waic[2, f], waic[4, f]), _nsig(waic[3, r], waic[5, r]),
            _nsig(waic[0], fr)]


# ---------------------------------------------------------------------------
# posterior means
# ---------------------------------------------------------------------------
def means(x):
    """(diag[T, 6, 4], mean_abs[T, 6, 4], dmm[T], dmm_abs[T]) longdouble: the
    means of q, A, c, phi per chain and of A + c of the PMD-all chain."""
    xl = x.astype(LDBL)
    dm = xl[:, 0, :, 1] + xl[:, 0, :, 2]
    return xl.mean(axis=2), np.abs(xl).mean(axis=2), dm.mean(axis=1), np.abs(dm).mean(axis=1)


def mean_bar(S, mean_abs, serial=False):
    """The bar on a mean of S terms: the kernel adds ceil(S / 64) terms per lane,
    six levels of the wave's tree and one division; a serial sum (the oracle's)
    S - 1 additions (+ the term's own A + c, the division)."""
    return ((S + 2) if serial else (math.ceil(S / 64) + 6)) * EPS * mean_abs


# ---------------------------------------------------------------------------
# Beta-Binomial moments (the independent check of the draws)
# ---------------------------------------------------------------------------
def betabinom_central_moments(n, a, b):
    """(mean, mu2, mu4) of BetaBinomial(n, a, b), exactly: from the factorial
    moments E[X^(r falling)] = n^(r falling) a^(r rising) / (a + b)^(r rising) in
    rational arithmetic on the doubles a and b (the central moments cancel
    heavily at large n), rounded once at the end."""
    from fractions import Fraction

    n, a, b = Fraction(int(n)), Fraction(float(a)), Fraction(float(b))
    fm = []
    for r in range(1, 5):
        num, den, nf = Fraction(1), Fraction(1), Fraction(1)
        for i in range(r):
            num *= a + i
            den *= a + b + i
            nf *= n - i
        fm.append(nf * num / den)
    f1, f2, f3, f4 = fm
    m1 = f1
    m2 = f2 + f1
    m3 = f3 + 3 * f2 + f1
    m4 = f4 + 6 * f3 + 7 * f2 + f1
    mu2 = m2 - m1 ** 2
    mu4 = m4 - 4 * m1 * m3 + 6 * m1 ** 2 * m2 - 3 * m1 ** 4
    return float(m1), float(mu2), float(mu4)


def moment_z(counts, n, a, b):
    """(z_mean, z_var) of S iid counts against BetaBinomial(n, a, b): the sample
    mean and the sample variance (about the exact mean) against their exact
    expectations, standard errors from the exact second and fourth central
    moments."""
    c = np.asarray(counts, np.float64)
    S = c.size
    m1, mu2, mu4 = betabinom_central_moments(n, a, b)
    z_mean = (c.mean() - m1) / math.sqrt(mu2 / S)
    s2 = ((c - m1) ** 2).mean()  # about the known mean: E = mu2, Var = (mu4 - mu2^2) / S
    z_var = (s2 - mu2) / math.sqrt((mu4 - mu2 * mu2) / S)
    return z_mean, z_var


def chi_square_tail(counts, n, a, b):
    """Tail probability of Pearson's chi-square of S iid counts against
    scipy.stats.betabinom.pmf(., n, a, b), neighbouring bins merged from the
    left until each expects at least 5 (the rest joins the last bin)."""
    from scipy import stats

    c = np.asarray(counts, np.int64)
    S = c.size
    pmf = stats.betabinom.pmf(np.arange(n + 1), n, a, b)
    obs = np.bincount(c, minlength=n + 1).astype(float)
    eb, ob, e_acc, o_acc = [], [], 0.0, 0.0
    for i in range(n + 1):
        e_acc += S * pmf[i]
        o_acc += obs[i]
        if e_acc >= 5.0:
            eb.append(e_acc), ob.append(o_acc)
            e_acc = o_acc = 0.0
    if eb:
        eb[-1] += e_acc
        ob[-1] += o_acc
    if len(eb) < 2:
        return 1.0, len(eb)
    eb, ob = np.array(eb), np.array(ob)
    chi2 = ((ob - eb) ** 2 / eb).sum()
    return float(stats.chi2.sf(chi2, len(eb) - 1)), len(eb)
