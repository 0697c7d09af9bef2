"""Reference of MDFIT-EVID v1 in numpy on np.longdouble (a
helper, no test), written from the specification, not from the kernel's code.
The proposals, draws, targets, smoothing and rounds are tests/map_waic_ref.py's,
tests/map_psis_ref.py's and tests/map_adapt_ref.py's; this module adds the
constants those drop, the log of the mean weight, its standard error and row 6,
and two independent truths: the null evidence by quadrature and the PMD
evidence by a large plain importance-sampling run."""

from __future__ import annotations

import functools
import json
from pathlib import Path

import numpy as np

from tests import map_adapt_ref as ad
from tests import map_psis_ref as pref
from tests import map_waic_ref as wref

LD = np.longdouble
NFIELD = 8
FIELDS = ["log_evidence", "se", "khat", "ess", "n_infeasible", "log_w_max", "best_round", "flags"]
COMPARE_FIELDS = ["log_bf", "log_bf_forward", "log_bf_reverse", "log_bf_asymmetry", "log_bf_se", "khat_max", "ess_min",
                  "flags"]
LOGZ, SE, KHAT, ESS, N_INF, LWMAX, ROUND, FLAGS = range(8)
VALID, RELIABLE, ADAPTED = 1, 2, 64
ROWS = wref.ROWS
NU = pref.NU


def _lgamma_half(n2: int):
    """lgamma(n2 / 2) in longdouble for a positive integer n2."""
    x, v = LD(n2) / 2, LD(0)
    while x > 1:
        x = x - 1
        v = v + np.log(x)
    return v + (np.log(np.sqrt(np.arccos(LD(-1)))) if x == LD(0.5) else LD(0))


def prior_constant(pmd: bool):
    """log of the normalising constants of the priors: Beta(2, 3) on q (and A)
    1 / B(2, 3) = 12, Beta(1, 9) on c 9, Exponential on delta its rate 1/1000."""
    k = np.log(LD(12)) - np.log(LD(1000))
    return k + np.log(LD(12)) + np.log(LD(9)) if pmd else k


def proposal_constant(prop):
    """log of the normalising constant of the proposal's density g(u): the
    d-variate Student-t's, minus the log determinant of the map t -> u_f (a
    Proposal: u_f = m + s * L^-T t; an Adapted one: u_f = m + d * F t), plus the
    log rate of the held c's exponential."""
    n = prop.idx.size
    k = _lgamma_half(NU + n) - _lgamma_half(NU) - LD(n) / 2 * np.log(NU * np.arccos(LD(-1)))
    if isinstance(prop, ad.Adapted):
        k = k - (np.log(prop.d).sum() + np.log(np.diag(prop.F)).sum())
    else:
        k = k - (np.log(prop.s).sum() - np.log(np.diag(prop.L)).sum())
    if prop.cheld:
        k = k + np.log(LD(prop.gc))
    return k


def log_mean_weight(lw):
    """(logz, se, khat, n_inf, w, ok) of raw log-weights lw[S] (float64): c +
    log(tot) - log S with c the largest finite lw and tot the sum of the
    smoothed weights exp(lw - c) before normalisation, se = sqrt(sum w^2 - 1/S)
    of the normalised ones, formed as sqrt(sum (w - 1/S)^2) -- the same number,
    since sum w = 1, without the cancellation that leaves 3e-11 of a difference
    of 1e-21 where the weights are uniform.  The smoothing is pref.psis_weights, which returns
    the normalised weights alone: a draw below the tail keeps exp(lw - c), so
    tot is the ratio of those draws' raw and normalised sums."""
    lw = np.asarray(lw, np.float64)
    S = lw.size
    w, khat, n_inf, ok = pref.psis_weights(lw)
    if not ok:
        return LD("nan"), LD("nan"), LD("nan"), n_inf, w, False
    inf = np.isneginf(lw)
    c = lw[~inf].max().astype(LD)
    r = lw.astype(LD) - c
    order = np.argsort(np.where(inf, LD(pref.FLOOR), r), kind="stable")
    body = order[:S - pref.tail_len(S)]
    body = body[~inf[body]]
    tot = np.exp(r[body]).sum() / w[body].sum()
    logz = c + np.log(tot) - np.log(LD(S))
    se = np.sqrt(((w - 1 / LD(S)) ** 2).sum())
    return logz, se, khat, n_inf, w, True


def invalid_record(mask: int):
    rec = np.full(NFIELD, np.nan, LD)
    rec[FLAGS] = mask << 2
    return rec


def row_record(lw, K, S: int, mask: int, best_round: int = 0):
    """One row from its raw log-weights and K = K_prior - K_prop -> (rec[8], w)."""
    logz, se, khat, n_inf, w, ok = log_mean_weight(lw)
    if not ok:
        return invalid_record(mask), w
    rec = np.full(NFIELD, np.nan, LD)
    rec[LOGZ] = K + logz
    rec[SE] = se
    rec[KHAT] = khat
    rec[ESS] = 1 / (w * w).sum()
    rec[N_INF] = n_inf
    rec[LWMAX] = K + np.asarray(lw, np.float64)[~np.isneginf(lw)].max().astype(LD)
    rec[ROUND] = best_round
    rec[FLAGS] = (VALID | (RELIABLE if khat <= pref.khat_threshold(S) else 0) | (mask << 2)
                  | (ADAPTED if best_round > 0 else 0))
    return rec, w


def compare(recs):
    """Row 6 from the six rows' records."""
    r6 = np.full(NFIELD, np.nan, LD)
    ok = [int(r[FLAGS]) & VALID for r in recs]
    lz = [r[LOGZ] for r in recs]
    r6[0] = lz[0] - lz[1]
    r6[1] = lz[2] - lz[4]
    r6[2] = lz[3] - lz[5]
    r6[3] = lz[0] - (lz[2] + lz[3])
    r6[4] = np.sqrt(recs[0][SE] ** 2 + recs[1][SE] ** 2)
    valid = [r for r, o in zip(recs, ok) if o]
    if valid:
        r6[5] = max(r[KHAT] for r in valid)
        r6[6] = min(r[ESS] for r in valid)
    allv = all(ok)
    r6[7] = (VALID if allv else 0) | (RELIABLE if allv and all(int(r[FLAGS]) & RELIABLE for r in recs) else 0)
    return r6


def status_bad():
    recs = np.full((7, NFIELD), np.nan, LD)
    recs[:, FLAGS] = 0
    return recs


def evidence_taxon(oracle_lib, y30, N30, rec, status: int, S: int, R: int = 0, seed: int = 0, g: int = 0, given=None):
    """One taxon end to end -> dict: rec[7, 8], rows (per row a dict: prop --
    the round-0 proposal --, best -- the proposal whose weights the record is
    of --, best_round, margin, K, lw, w).  R > 0: the PMD rows through
    map_adapt_ref's rounds.  given: None -- the reference's own draws -- or
    (u[6, S, 4], lw[6, S]) float64, the best round's draws and raw log-weights
    to use in its place (the constants stay the reference's own)."""
    if status != 0:
        return {"rec": status_bad(), "rows": [None] * 6}
    recs, rows = [], []
    for s in range(6):
        pmd = ROWS[s][0]
        prop = wref.proposal(oracle_lib, y30, N30, rec, s)
        info = {"prop": prop, "best": prop, "best_round": 0, "margin": np.inf}
        if not prop.valid:
            recs.append(invalid_record(prop.mask))
            rows.append(info)
            continue
        rnd = pref.randoms(oracle_lib, seed, g, s, S)
        if pmd and R > 0:
            res = ad.adapt_rounds(oracle_lib, y30, N30, wref.PMD_ROW[s], prop, rnd, S, R)
            best = res["best"]
            info.update(best=best["prop"], best_round=res["best_round"], margin=res["margin"])
            u64, lw = best["u64"], best["lw"]
        else:
            u, lg = prop.draw(*rnd)
            u64 = u.astype(np.float64)
            lw = (wref.log_target(oracle_lib, y30, N30, s, u64) - lg).astype(np.float64)
        info.update(u=u64)
        if given is not None:
            lw = np.asarray(given[1][s], float)
        K = prior_constant(pmd) - proposal_constant(info["best"])
        r, w = row_record(lw, K, S, prop.mask, info["best_round"])
        info.update(K=K, lw=lw, w=w)
        recs.append(r)
        rows.append(info)
    recs.append(compare(recs))
    return {"rec": np.stack(recs), "rows": rows}


# --------------------------------------------------------------------------
# truths
# --------------------------------------------------------------------------
def null_quadrature(oracle_lib, y30, N30, rec, s: int):
    """log Z of null row s (1, 4, 5) by tensor Gauss-Legendre in (logit q, log
    delta) over the mode +- 14 Laplace standard deviations, with 96^2 and 192^2
    nodes, which must agree to 1e-9.  Where they do not, the nodes are doubled
    again, to 768^2 at the most, and the last two rules must agree to 1e-9.
    (Taxon 9 of generate(300, 21), one position with 86 of 550 among positions
    with none: its all-position null posterior has a correlation of -0.87 and a
    flank that falls by 35 in log density within three standard deviations; 96^2
    and 192^2 differ by 4.8e-8 there, 192^2 and 384^2 by 4e-14; its reverse
    null needs 768^2.)"""
    prop = wref.null_proposal(oracle_lib, y30, N30, rec, s)
    assert prop.valid
    Li = pref._inv_lower(prop.L)
    sd = np.sqrt(np.diag((Li.T @ Li) * np.outer(prop.s, prop.s))).astype(float)
    mode = prop.u[[0, 3]]

    def rule(n):
        x, wq = np.polynomial.legendre.leggauss(n)
        u = np.zeros((n * n, 4))
        u[:, 0] = np.repeat(mode[0] + 14 * sd[0] * x, n)
        u[:, 3] = np.tile(mode[1] + 14 * sd[1] * x, n)
        t = wref.null_log_target(oracle_lib, y30, N30, s, u) + np.log(np.outer(wq, wq).ravel().astype(LD))
        m = t.max()
        return m + np.log(np.exp(t - m).sum()) + np.log(LD(14 * sd[0]) * LD(14 * sd[1])) + prior_constant(False)

    n = 192
    coarse, fine = rule(96), rule(192)
    while abs(coarse - fine) > 1e-9 and n < 768:
        n *= 2
        coarse, fine = fine, rule(n)
    assert abs(coarse - fine) <= 1e-9, (s, n, coarse, fine)
    return fine


def pmd_big_run(oracle_lib, y30, N30, s: int, prop, S: int = 200_000, rng=None, chunk: int = 50_000):
    """(log Z, se) of PMD row s (0, 2, 3) by plain importance sampling without
    smoothing: S draws of numpy's generator through the reference's proposal
    object, the log of the mean of the full weights and its own delta-method
    standard error."""
    rng = np.random.default_rng(0) if rng is None else rng
    K = prior_constant(True) - proposal_constant(prop)
    lws = []
    for lo in range(0, S, chunk):
        n = min(chunk, S - lo)
        z = rng.standard_normal((n, 4)).astype(LD)
        chi2 = rng.chisquare(NU, n).astype(LD)
        e = rng.exponential(size=n).astype(LD)
        u, lg = prop.draw(z, chi2, e)
        lws.append(wref.log_target(oracle_lib, y30, N30, s, u.astype(np.float64)) - lg)
    lw = np.concatenate(lws) + K
    m = lw.max()
    wt = np.exp(lw - m)
    tot = wt.sum()
    w = wt / tot
    return m + np.log(tot) - np.log(LD(S)), np.sqrt(max((w * w).sum() - 1 / LD(S), LD(0)))


TRUTH_TAXA = 16
TRUTH_SEED = 41
TRUTH_FILE = Path(__file__).resolve().parent / "golden" / "map_evidence_truth.json"


@functools.lru_cache(maxsize=None)
def batch_fit(oracle_lib):
    """generate(300, seed=21) fitted by the oracle: (batch, out, status); computed once."""
    from metadamage_amd.synthetic import generate

    b = generate(300, seed=21)
    out, _, st = oracle_lib.fit_batch(b.y, b.N)
    return b, out, st


def truth_row(oracle_lib, t: int, s: int):
    """(log Z, se) of row s of taxon t of batch_fit by the truth of its kind
    (se 0 for the quadrature), or None where the round-0 proposal is invalid."""
    b, out, st = batch_fit(oracle_lib)
    if st[t] != 0:
        return None
    y30, N30 = b.y[t, :30], b.N[t, :30]
    prop = wref.proposal(oracle_lib, y30, N30, out[t], s)
    if not prop.valid:
        return None
    if not ROWS[s][0]:
        return float(null_quadrature(oracle_lib, y30, N30, out[t], s)), 0.0
    lz, se = pmd_big_run(oracle_lib, y30, N30, s, prop, rng=np.random.default_rng([TRUTH_SEED, t, s]))
    return float(lz), float(se)


def load_truth():
    """The recorded truth_row of the first TRUTH_TAXA taxa: {(t, s): (log Z, se)}
    (tests/golden/map_evidence_truth.json; test_map_evidence.py holds it equal
    to the computation)."""
    rows = json.loads(TRUTH_FILE.read_text())["rows"]
    return {(int(r["taxon"]), int(r["row"])): (float.fromhex(r["log_z"]), float.fromhex(r["se"])) for r in rows}


def write_truth():
    from oracle.oracle import OracleLib

    o = OracleLib()
    rows = []
    for t in range(TRUTH_TAXA):
        for s in range(6):
            got = truth_row(o, t, s)
            if got is not None:
                rows.append({"taxon": t, "row": s, "log_z": got[0].hex(), "se": got[1].hex()})
                print(t, s, got, flush=True)
    TRUTH_FILE.write_text(json.dumps({"batch": "generate(300, seed=21)", "draws": 200000, "seed": TRUTH_SEED,
                                      "rows": rows}, indent=0) + "\n")


if __name__ == "__main__":
    write_truth()
