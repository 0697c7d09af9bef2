"""Reference of MDFIT-WAIC v1 in numpy on np.longdouble (a
helper, no test), written from the specification, not from the kernel's code.
The PMD rows are tests/map_psis_ref.py's (proposal, randoms, target,
smoothing); the null rows take the oracle's null objective at the mode rebuilt
from the record, laplace_ref's binding rule on q and delta, a bivariate
Student-t on (u0, u3) and the null target; the pointwise statistics are
whole-array weighted sums and row 6 the reference's n_sigma (oracle.py)."""

from __future__ import annotations

import numpy as np

from tests import laplace_ref
from tests import map_psis_ref as pref

LD = np.longdouble
NFIELD = 8
FIELDS = ["elpd_waic", "p_waic", "lppd", "khat", "ess", "n_infeasible", "p_waic_max", "flags"]
COMPARE_FIELDS = ["n_sigma_waic", "n_sigma_waic_forward", "n_sigma_waic_reverse", "asymmetry_waic", "khat_max",
                  "ess_min", "reserved", "flags"]
ELPD, PWAIC, LPPD, KHAT, ESS, N_INF, PMAX, FLAGS = range(8)
VALID, RELIABLE = 1, 2
NHALF = 15
# row s of the record (the diagnostic slot): (pmd, oracle subset); its stream's sub-fit index is s
ROWS = [(True, 0), (False, 0), (True, 1), (True, 2), (False, 1), (False, 2)]
PMD_ROW = {0: 0, 2: 1, 3: 2}  # record row -> map_psis_ref's row


def columns(s: int) -> range:
    return (range(0, 30), range(0, NHALF), range(NHALF, 30))[ROWS[s][1]]


class NullProposal(pref.Proposal):
    """A null sub-fit's proposal: the mode u = (logit q, 0, 0, log delta), the
    free set of coordinates 0 and 3, the Jacobi scale and the Cholesky factor
    of the scaled 2x2 block."""

    def __init__(self, u, g, H):
        self.u = np.asarray(u, float)
        free, self.near = laplace_ref.free_set(self.u, g, H)
        free = np.asarray(free, bool).copy()
        free[1] = free[2] = False  # not part of the model
        self.free = free
        self.mask = int(sum(1 << j for j in range(4) if free[j]))
        self.cheld = False
        self.gc = LD(0)
        self.idx = np.flatnonzero(free)
        self.valid = False
        if not (free[0] and free[3]):
            return
        Hf = np.asarray(H, float)[np.ix_(self.idx, self.idx)].astype(LD)
        if not (np.diag(Hf) > 0).all():
            return
        self.s = 1 / np.sqrt(np.diag(Hf))
        R = Hf * np.outer(self.s, self.s)
        L = np.zeros((2, 2), LD)
        for j in range(2):
            for m in range(j + 1):
                v = R[j, m] - (L[j, :m] * L[m, :m]).sum()
                if j == m:
                    if not v > laplace_ref.PIV_MIN:
                        return
                    L[j, m] = np.sqrt(v)
                else:
                    L[j, m] = v / L[m, m]
        self.L = L
        self.K = np.zeros(2, LD)
        self.valid = True


def null_proposal(oracle_lib, y30, N30, rec, s: int) -> NullProposal:
    d = rec[laplace_ref.F_DIAG + laplace_ref.DIAG_STRIDE * s:][:4]
    u = laplace_ref.rebuild_u(d[0], 0.5, 0.0, d[3])
    _, g, H, _ = oracle_lib.objective(1, ROWS[s][1], y30, N30, u)
    return NullProposal(u, g, H)


def pointwise_ll(oracle_lib, y30, N30, s: int, u):
    """l[S, n] (longdouble; NaN rows for infeasible PMD draws): the full
    beta-binomial log-pmf of float64 draws u[S, 4] at the row's points."""
    pmd = ROWS[s][0]
    u = np.asarray(u, float)
    cols = list(columns(s))
    f = pref.constrained(u)
    q, A, c, phi = f.T
    if pmd:
        with np.errstate(invalid="ignore"):
            feas = (c >= 0) & (A + c < 1)
        k = np.array([col % NHALF for col in cols], LD)
        D = A[:, None] * (1 - q[:, None]) ** k[None, :] + c[:, None]
    else:
        feas = np.ones(len(u), bool)
        D = np.broadcast_to(q[:, None], (len(u), len(cols))).copy()
    out = np.full(D.shape, np.nan, LD)
    if feas.any():
        Df = D[feas]
        ph = np.broadcast_to(phi[feas, None], Df.shape)
        yy = np.broadcast_to(np.asarray(y30, float)[cols][None, :], Df.shape)
        nn = np.broadcast_to(np.asarray(N30, float)[cols][None, :], Df.shape)
        out[feas] = oracle_lib.bb_logpmf_full(yy.ravel(), nn.ravel(), (Df * ph).astype(float).ravel(),
                                              ((1 - Df) * ph).astype(float).ravel()).reshape(Df.shape).astype(LD)
    return out


def null_log_target(oracle_lib, y30, N30, s: int, u):
    """log p(u)[S] of a null row: sum_i l_i + log q + 2 log(1 - q) - delta / 1000 + log[q (1 - q) delta]."""
    uf = np.asarray(u, float).astype(LD)
    ll = pointwise_ll(oracle_lib, y30, N30, s, u).sum(axis=1)
    lq, l1q = -np.log1p(np.exp(-uf[:, 0])), -np.log1p(np.exp(uf[:, 0]))
    delta = np.exp(uf[:, 3])
    return ll + (lq + 2 * l1q - delta / 1000) + (lq + l1q + uf[:, 3])


def log_target(oracle_lib, y30, N30, s: int, u):
    if ROWS[s][0]:
        return pref.log_target(oracle_lib, y30, N30, PMD_ROW[s], u)
    return null_log_target(oracle_lib, y30, N30, s, u)


def proposal(oracle_lib, y30, N30, rec, s: int):
    if ROWS[s][0]:
        return pref.proposal(oracle_lib, y30, N30, rec, PMD_ROW[s])
    return null_proposal(oracle_lib, y30, N30, rec, s)


def points(w, ll):
    """(lppd_i[n], p_i[n]) longdouble from normalised weights w[S] and l[S, n];
    draws of weight 0 take no part."""
    w = np.asarray(w, LD)
    use = w > 0
    ww, l = w[use], np.asarray(ll)[use].astype(LD)
    mx = l.max(axis=0)
    lppd = mx + np.log((ww[:, None] * np.exp(l - mx)).sum(axis=0))
    m = (ww[:, None] * l).sum(axis=0)
    p = (ww[:, None] * (l - m) ** 2).sum(axis=0)
    flat = (l == l[0]).all(axis=0)  # the same value in every draw: exact
    lppd = np.where(flat, l[0], lppd)
    p = np.where(flat, LD(0), p)
    return lppd, p


def row_record(lppd, p, w, khat, n_inf, S: int, mask: int):
    rec = np.full(NFIELD, np.nan, LD)
    rec[ELPD] = (lppd - p).sum()
    rec[PWAIC] = p.sum()
    rec[LPPD] = lppd.sum()
    rec[KHAT] = khat
    rec[ESS] = 1 / (np.asarray(w, LD) ** 2).sum()
    rec[N_INF] = n_inf
    rec[PMAX] = p.max()
    rec[FLAGS] = VALID | (RELIABLE if khat <= pref.khat_threshold(S) else 0) | (mask << 2)
    return rec


def invalid_record(mask: int):
    rec = np.full(NFIELD, np.nan, LD)
    rec[FLAGS] = mask << 2
    return rec


def n_sigma(a, b):
    """fits.py:194-227: (sum b - sum a) / sqrt(n var(a - b)), ddof 0."""
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    d = a - b
    with np.errstate(invalid="ignore", divide="ignore"):
        return (b.sum() - a.sum()) / np.sqrt(len(a) * ((d - d.mean()) ** 2).mean())


def compare(recs, waic_cols):
    """Row 6 from the six rows' records and their waic_i (None: invalid row)."""
    r6 = np.full(NFIELD, np.nan, LD)
    ok = [int(r[FLAGS]) & VALID for r in recs]

    def ns(a, b, need):
        if not all(ok[i] for i in need):
            return LD("nan")
        return n_sigma(a(), b())

    r6[0] = ns(lambda: waic_cols[0], lambda: waic_cols[1], (0, 1))
    r6[1] = ns(lambda: waic_cols[2], lambda: waic_cols[4], (2, 4))
    r6[2] = ns(lambda: waic_cols[3], lambda: waic_cols[5], (3, 5))
    r6[3] = ns(lambda: waic_cols[0], lambda: np.concatenate([waic_cols[2], waic_cols[3]]), (0, 2, 3))
    valid = [r for r, o in zip(recs, ok) if o]
    if valid:
        r6[4] = max(r[KHAT] for r in valid)
        r6[5] = min(r[ESS] for r in valid)
    r6[6] = 0
    allv = all(ok)
    r6[7] = (VALID if allv else 0) | (RELIABLE if allv and all(int(r[FLAGS]) & RELIABLE for r in recs) else 0)
    return r6


def row_from(oracle_lib, y30, N30, s: int, prop, u, lw, S: int):
    """One row from draws u[S, 4] and raw log-weights lw[S] (float64) ->
    (rec[8], pointwise[30, 2] (NaN outside the row), waic_i or None, w)."""
    pw = np.full((30, 2), np.nan, LD)
    if not prop.valid:
        return invalid_record(prop.mask), pw, None, None
    w, khat, n_inf, ok = pref.psis_weights(lw)
    if not ok:
        return invalid_record(prop.mask), pw, None, w
    ll = pointwise_ll(oracle_lib, y30, N30, s, u)
    lppd, p = points(w, ll)
    cols = list(columns(s))
    pw[cols, 0], pw[cols, 1] = lppd, p
    return row_record(lppd, p, w, khat, n_inf, S, prop.mask), pw, -2 * (lppd - p), w


def status_bad():
    recs = np.full((7, NFIELD), np.nan, LD)
    recs[:, FLAGS] = 0
    return recs


def waic_taxon(oracle_lib, y30, N30, rec, status: int, S: int, seed: int = 0, g: int = 0, given=None):
    """One taxon end to end -> dict: rec[7, 8], pointwise[6, 30, 2], rows (per
    row a dict: prop, u, lg, lw, w).  given: None -- the reference's own draws
    -- or (u[6, S, 4], lw[6, S]) float64, the draws and raw log-weights to use
    (NaN rows ignored where the proposal is invalid)."""
    if status != 0:
        return {"rec": status_bad(), "pointwise": np.full((6, 30, 2), np.nan, LD), "rows": [None] * 6}
    recs, pws, cols, rows = [], [], [], []
    for s in range(6):
        prop = proposal(oracle_lib, y30, N30, rec, s)
        info = {"prop": prop}
        if prop.valid:
            if given is None:
                z, chi2, e = pref.randoms(oracle_lib, seed, g, s, S)
                u, lg = prop.draw(z, chi2, e)
                u64 = u.astype(np.float64)
                lw = (log_target(oracle_lib, y30, N30, s, u64) - lg).astype(np.float64)
                info.update(u=u, lg=lg)
            else:
                u64, lw = np.asarray(given[0][s], float), np.asarray(given[1][s], float)
            r, pw, wc, w = row_from(oracle_lib, y30, N30, s, prop, u64, lw, S)
            info.update(lw=lw, w=w)
        else:
            r, pw, wc = invalid_record(prop.mask), np.full((30, 2), np.nan, LD), None
        recs.append(r)
        pws.append(pw)
        cols.append(wc)
        rows.append(info)
    recs.append(compare(recs, cols))
    return {"rec": np.stack(recs), "pointwise": np.stack(pws), "rows": rows}
