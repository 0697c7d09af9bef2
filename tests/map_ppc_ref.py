"""Reference of MDFIT-PPC v1 in numpy (a helper, no test),
written from the specification, not from the kernel's code: the weights of
tests/map_psis_ref.psis_taxon, the resampling and the predictive counts of
tests/map_pred_ref (the CPU oracle's nuts_predictive), then the standardised
residuals, the two discrepancies and the mid-p values in plain numpy."""

from __future__ import annotations

import numpy as np

from tests import map_pred_ref as qref
from tests import map_psis_ref as pref

NFIELD = 12
FIELDS = ["p_outlier", "p_strand", "t_outlier", "t_strand", "worst_pos", "p_worst", "n_low", "n_points", "khat", "ess",
          "n_distinct", "flags"]
P_OUT, P_STR, T_OUT, T_STR, WORST, P_WORST, N_LOW, N_POINTS, KHAT, ESS, NDISTINCT, FLAGS = range(12)
VALID, RELIABLE, NONCOUNT, ADAPTED = 1, 2, 8, 64
NCOL = 30
NO_COUNT = qref.NO_COUNT
LOW_P = 0.05


def residual_parts(theta, N30):
    """(mu[R, 30], sd[R, 30], use[R, 30]) of the draws theta[R, 4] = (q, A, c,
    phi): D = clamp(A (1 - q)^k + c, 0, 1), mu = N D, v = N D (1 - D)(phi + N) /
    (phi + 1) in that order of operations; use: N > 0 and v > 0."""
    th = np.asarray(theta, np.float64)
    q, A, c, phi = (th[:, j, None] for j in range(4))
    k = (np.arange(NCOL) % 15).astype(np.float64)[None, :]
    Nn = np.asarray(N30, np.float64)[None, :]
    with np.errstate(all="ignore"):
        D = np.clip(A * np.power(1.0 - q, k) + c, 0.0, 1.0)
        mu = Nn * D
        v = Nn * D * (1.0 - D) * (phi + Nn) / (phi + 1.0)
        use = (Nn > 0) & (v > 0)
        sd = np.sqrt(np.where(use, v, 1.0))
    return mu, sd, use


def discrepancies(theta, y30, N30, counts):
    """disc[R, 4] = T_out(obs), T_out(rep), T_str(obs), T_str(rep) and
    abs_sum[R] = sum |r_i| over both sides' terms (the scale of T_str's
    rounding) of the draws theta[R, 4] and the replicated counts[30, R] (uint32;
    a column with N = 0 is not read).  A replicated draw that is no count is
    skipped with its column."""
    mu, sd, use = residual_parts(theta, N30)
    y = np.asarray(y30, np.float64)[None, :]
    rep = np.asarray(counts, np.uint32).astype(np.float64).T
    Nn = np.asarray(N30, np.float64)[None, :]
    use = use & (rep <= Nn)
    ro = np.where(use, (y - mu) / sd, 0.0)
    rr = np.where(use, (rep - mu) / sd, 0.0)
    disc = np.empty((len(mu), 4))
    disc[:, 0] = (ro * ro).max(axis=1, initial=0.0)
    disc[:, 1] = (rr * rr).max(axis=1, initial=0.0)
    # summed in ascending column order per strand, as the specification's sums read
    for j, r in ((2, ro), (3, rr)):
        f = np.zeros(len(mu))
        b = np.zeros(len(mu))
        for i in range(15):
            f = f + r[:, i]
            b = b + r[:, 15 + i]
        disc[:, j] = f - b
    abs_sum = np.maximum(np.abs(ro).sum(axis=1), np.abs(rr).sum(axis=1))
    return disc, abs_sum


def column_counts(y30, N30, counts):
    """(gt[30], eq[30], live[30], some draw is no count): #{rep > y}, #{rep = y}
    over the draws of each column with N > 0."""
    y = np.asarray(y30, np.int64)
    Nn = np.asarray(N30, np.int64)
    c = np.asarray(counts, np.uint32).astype(np.int64)
    live = Nn > 0
    isc = c <= Nn[:, None]
    gt = ((c > y[:, None]) & isc).sum(axis=1) * live
    eq = ((c == y[:, None]) & isc).sum(axis=1) * live
    return gt, eq, live, bool((~isc[live]).any())


def record_from(disc, gt, eq, live, noncount: bool, R: int, khat, ess, nd, tau: float, adapted: bool = False):
    """(rec[12], ppos[30]) from the per-draw discrepancies and the per-column
    integer counts: every p-value is a count over R."""
    rec = np.full(NFIELD, np.nan)
    ppos = np.full(NCOL, np.nan)
    ok = not noncount
    rec[T_OUT], rec[T_STR] = disc[:, 0].mean(), disc[:, 2].mean()
    rec[N_POINTS] = int(live.sum())
    rec[KHAT], rec[ESS], rec[NDISTINCT] = khat, ess, nd
    if ok:
        rec[P_OUT] = int((disc[:, 1] >= disc[:, 0]).sum()) / R
        if live[:15].any() and live[15:].any():
            rec[P_STR] = int((np.abs(disc[:, 3]) >= np.abs(disc[:, 2])).sum()) / R
        p = (2.0 * gt + eq) / (2.0 * R)
        ppos[live] = p[live]
        p2 = 2.0 * np.minimum(p, 1.0 - p)
        rec[N_LOW] = int((p2[live] < LOW_P).sum())
        if live.any():
            cols = np.flatnonzero(live)
            w = cols[np.argmin(p2[cols])]  # (argmin: the first among equals)
            rec[WORST], rec[P_WORST] = w, p2[w]
    rec[FLAGS] = (VALID if ok else 0) | (RELIABLE if khat <= tau else 0) | (NONCOUNT if noncount else 0) | \
        (ADAPTED if adapted else 0)
    return rec, ppos.astype(np.float32)


def invalid_taxon(R: int):
    rec = np.full(NFIELD, np.nan)
    rec[FLAGS] = 0
    return {"rec": rec, "ppos": np.full(NCOL, np.nan, np.float32), "index": np.full(R, -1, np.int64),
            "counts": np.full((NCOL, R), NO_COUNT, np.uint32), "disc": np.full((R, 4), np.nan)}


def assemble(row, S: int, R: int, y30, N30, oracle_lib, seed: int, g: int, index=None, counts=None,
             adapted: bool = False):
    """The check from row = (valid, khat, ess, w[S], theta[S, 4]) of the PMD-all
    sub-fit.  index, counts: a kernel's taps in place of the reference's own
    resampling and predictive draws."""
    valid, khat, ess, w, theta = row
    if not valid:
        return invalid_taxon(R)
    idx, nd = qref.resample(w, R)
    if index is not None:
        idx = np.asarray(index, np.int64)
        nd = int(np.unique(idx).size)
    th = np.asarray(theta, np.float64)[idx]
    if counts is None:
        counts = np.stack([qref.job_draws(oracle_lib, th, j, N30, seed, g)[0] for j in range(NCOL)])
    counts = np.asarray(counts, np.uint32)
    disc, abs_sum = discrepancies(th, y30, N30, counts)
    gt, eq, live, noncount = column_counts(y30, N30, counts)
    rec, ppos = record_from(disc, gt, eq, live, noncount, R, khat, ess, nd, pref.khat_threshold(S), adapted)
    return {"rec": rec, "ppos": ppos, "index": idx, "counts": counts, "disc": disc, "abs_sum": abs_sum}


def ppc_taxon(oracle_lib, y30, N30, out_rec, status: int, S: int, R: int, seed: int = 0, g: int = 0):
    """One taxon end to end on the reference's own draws and weights."""
    if status != 0:
        return invalid_taxon(R)
    r = pref.psis_taxon(oracle_lib, y30, N30, out_rec, 0, S, seed=seed, g=g, rows=(0,))[0]
    rec = r["rec"]
    if not int(rec[pref.FLAGS]) & pref.VALID:
        return invalid_taxon(R)
    row = (True, float(rec[pref.KHAT]), float(rec[pref.ESS]), np.asarray(r["w"], np.float64),
           pref.constrained(np.asarray(r["u"], np.float64)).astype(np.float64))
    return assemble(row, S, R, y30, N30, oracle_lib, seed, g)


def ppc_given(oracle_lib, y30, N30, psis_rec, draws, S: int, R: int, seed: int = 0, g: int = 0, index=None,
              counts=None):
    """The check from a taxon's mdfit_map_psis output: psis_rec[3, 16] and its
    draws tap draws[3, S, 6] = u[4], lw, w (the kernel's own weights and u),
    and, when given, a kernel's index[R] and counts[30, R] taps."""
    if not int(psis_rec[0, pref.FLAGS]) & pref.VALID:
        return invalid_taxon(R)
    theta = pref.constrained(np.asarray(draws[0, :, :4], np.float64)).astype(np.float64)
    row = (True, float(psis_rec[0, pref.KHAT]), float(psis_rec[0, pref.ESS]), np.asarray(draws[0, :, 5], np.float64),
           theta)
    adapted = bool(int(psis_rec[0, pref.FLAGS]) & ADAPTED)
    return assemble(row, S, R, y30, N30, oracle_lib, seed, g, index=index, counts=counts, adapted=adapted)
