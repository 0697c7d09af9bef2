"""Reference of MDFIT-PPRED v1 in numpy (a helper, no test),
written from the specification, not from the kernel's code: the weights of
tests/map_psis_ref.psis_taxon, the midpoint systematic resampling with
np.cumsum and np.searchsorted, the predictive draws, the median and the 68 %
interval through the CPU oracle's nuts_predictive."""

from __future__ import annotations

import numpy as np

from tests import map_psis_ref as pref

NFIELD = 16
FIELDS = ["D_max", "D_max_lower_hpdi", "D_max_upper_hpdi", "D_max_forward", "D_max_reverse", "khat_all",
          "khat_forward", "khat_reverse", "ess_all", "ess_forward", "ess_reverse", "n_distinct_all",
          "n_distinct_forward", "n_distinct_reverse", "n_noncount_jobs", "flags"]
KHAT, ESS, NDISTINCT, NNONCOUNT, FLAGS = 5, 8, 11, 14, 15
VALID, RELIABLE = 1, 2  # and bits 2..4: row 0..2 valid
NJOB = 32
NO_COUNT = 0xFFFFFFFF
STREAM_SUB = (0, 2, 3)  # the sampler's sub-fit index of rows all / forward / reverse
# job -> (row, column, k, index of the N used); job 31 reads N[0], the reference's data_forward quirk
JOBS = [(0, i, i % 15, i) for i in range(30)] + [(1, 0, 0, 0), (2, 0, 0, 0)]


def resample(w, R: int):
    """(idx[R], n_distinct) of the weights w[S]: c = cumsum(w) in float64, p_r =
    (r + 0.5) (c[-1] / R), idx[r] the least s with c_s > p_r."""
    c = np.cumsum(np.asarray(w, np.float64))
    p = (np.arange(R) + 0.5) * (c[-1] / R)
    idx = np.searchsorted(c, p, side="right")
    return idx.astype(np.int64), int(np.unique(idx).size)


def job_draws(oracle_lib, theta, job: int, N30, seed: int, g: int):
    """(counts[R] uint32 -- NO_COUNT where the draw is none or N = 0 --, m3[3],
    whether some draw is no count while N > 0) of job `job` on the resampled
    draws theta[R, 4] = (q, A, c, phi).  (At N = 2^32 - 1 NO_COUNT is a count
    too: what makes a draw none is its value, not the tap's.)"""
    row, col, k, ncol = JOBS[job]
    Nn = float(N30[ncol])
    frac, m3 = oracle_lib.nuts_predictive(theta, col, k, Nn, seed=seed, g=g, sub=STREAM_SUB[row])
    counts = np.full(len(frac), NO_COUNT, np.uint32)
    bad = False
    if Nn > 0:
        obs = np.rint(frac * Nn)
        ok = np.isfinite(frac) & (obs >= 0) & (obs <= Nn)
        counts[ok] = obs[ok].astype(np.uint32)
        bad = bool((~ok).any())
    else:
        m3 = np.full(3, np.nan)
    return counts, np.asarray(m3, float), bad


def summary(oracle_mod, counts, Nn: float):
    """np.median and numpyro's hpdi(0.68) of counts / N: NaN with N = 0 or a
    draw that is no count (the tap's NO_COUNT where it exceeds N)."""
    counts = np.asarray(counts, np.uint32)
    if Nn <= 0 or (counts.astype(np.float64) > Nn).any():
        return np.full(3, np.nan)
    f = np.sort(counts).astype(np.float64) / float(Nn)
    lo, hi = oracle_mod.hpdi(f, 0.68)
    return np.array([np.median(f), lo, hi])


def assemble(rows, S: int, R: int, N30, oracle_lib, seed: int, g: int):
    """The record from rows = 3 x (valid, khat, ess, w[S] or None, theta[S, 4] or
    None): dict rec[16], ppred[3, 30], index[3, R] (-1 in an invalid row),
    counts[32, R]."""
    rec = np.full(NFIELD, np.nan)
    ppred = np.full((3, 30), np.nan)
    index = np.full((3, R), -1, np.int64)
    counts = np.full((NJOB, R), NO_COUNT, np.uint32)
    m3 = np.full((NJOB, 3), np.nan)
    flags, n_bad = 0, 0
    tau = pref.khat_threshold(S)
    all_ok, all_rel = True, True
    for row, (valid, khat, ess, w, theta) in enumerate(rows):
        all_ok &= bool(valid)
        if not valid:
            continue
        flags |= 4 << row
        all_rel &= bool(khat <= tau)
        rec[KHAT + row], rec[ESS + row] = khat, ess
        idx, nd = resample(w, R)
        index[row] = idx
        rec[NDISTINCT + row] = nd
        th = np.asarray(theta, np.float64)[idx]
        for job, (jr, col, k, ncol) in enumerate(JOBS):
            if jr != row:
                continue
            counts[job], m3[job], bad = job_draws(oracle_lib, th, job, N30, seed, g)
            if bad:
                n_bad += 1
                assert np.isnan(m3[job]).all()
    ppred[:] = m3[:30].T
    rec[0:3] = m3[0]
    rec[3], rec[4] = m3[30, 0], m3[31, 0]
    rec[NNONCOUNT] = n_bad
    rec[FLAGS] = flags | (VALID if all_ok else 0) | (RELIABLE if all_ok and all_rel else 0)
    return {"rec": rec, "ppred": ppred, "index": index, "counts": counts}


def invalid_taxon(R: int):
    rec = np.full(NFIELD, np.nan)
    rec[FLAGS] = 0
    return {"rec": rec, "ppred": np.full((3, 30), np.nan), "index": np.full((3, R), -1, np.int64),
            "counts": np.full((NJOB, R), NO_COUNT, np.uint32)}


def pred_taxon(oracle_lib, y30, N30, out_rec, status: int, S: int, R: int, seed: int = 0, g: int = 0):
    """One taxon end to end on the reference's own draws and weights."""
    if status != 0:
        return invalid_taxon(R)
    rows = []
    for r in pref.psis_taxon(oracle_lib, y30, N30, out_rec, 0, S, seed=seed, g=g):
        rec = r["rec"]
        if not int(rec[pref.FLAGS]) & pref.VALID:
            rows.append((False, np.nan, np.nan, None, None))
            continue
        rows.append((True, float(rec[pref.KHAT]), float(rec[pref.ESS]), np.asarray(r["w"], np.float64),
                     pref.constrained(np.asarray(r["u"], np.float64)).astype(np.float64)))
    return assemble(rows, S, R, N30, oracle_lib, seed, g)


def pred_given(oracle_lib, N30, psis_rec, draws, S: int, R: int, seed: int = 0, g: int = 0):
    """The record from a taxon's mdfit_map_psis output: psis_rec[3, 16] and its
    draws tap draws[3, S, 6] = u[4], lw, w (the kernel's own weights and u)."""
    rows = []
    for row in range(3):
        if not int(psis_rec[row, pref.FLAGS]) & pref.VALID:
            rows.append((False, np.nan, np.nan, None, None))
            continue
        theta = pref.constrained(np.asarray(draws[row, :, :4], np.float64)).astype(np.float64)
        rows.append((True, float(psis_rec[row, pref.KHAT]), float(psis_rec[row, pref.ESS]),
                     np.asarray(draws[row, :, 5], np.float64), theta))
    return assemble(rows, S, R, N30, oracle_lib, seed, g)
