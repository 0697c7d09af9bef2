"""Reference of MDFIT-ADAPT v1 in numpy on np.longdouble (a
helper, no test), written from the specification on tests/map_psis_ref.py's
functions: round 0 is psis_taxon's, a round's refit the weighted moments of the
residuals as whole-array sums and the backward upper-triangular factor, the
redraw from the same randoms, the accept / stop rule."""

from __future__ import annotations

import numpy as np

from tests import map_psis_ref as ref

LD = np.longdouble
PIV_MIN = 1e-8
ADAPTED = 64
MAX_ROUNDS = 4


def refit_arrays(u, w, mask: int, cheld: bool, K):
    """Steps 2-3 on draws u[S, 4] (float64), weights w[S], the free mask, the
    c-held flag and the shift K[4] -> dict(m[4], d[4], F[4, 4], gc) in the
    kernel's layout (held coordinates: m = 0, d = 1, the identity's row and
    column; gc = 0 with c free), or None where the round stops."""
    w = np.asarray(w).astype(LD)
    use = w > 0
    idx = [j for j in range(4) if (mask >> j) & 1]
    n = len(idx)
    ww = w[use]
    uu = np.asarray(u, np.float64)[use].astype(LD)
    c_s = uu[:, 2] if cheld else np.zeros(len(uu), LD)
    Kf = np.asarray(K, np.float64).astype(LD)[idx] if cheld else np.zeros(n, LD)
    with np.errstate(all="ignore"):
        rho = uu[:, idx] - np.outer(c_s, Kf)
        m = (ww[:, None] * rho).sum(axis=0)
        e = rho - m
        C = (ww[:, None, None] * e[:, :, None] * e[:, None, :]).sum(axis=0)
        if not (np.diag(C) > 0).all():
            return None
        d = np.sqrt(np.diag(C))
        R = C / np.outer(d, d)
        F = np.zeros((n, n), LD)
        for j in range(n - 1, -1, -1):
            s = R[j, j] - (F[j, j + 1:] ** 2).sum()
            if not s > PIV_MIN:
                return None
            F[j, j] = np.sqrt(s)
            for i in range(j):
                F[i, j] = (R[i, j] - (F[i, j + 1:] * F[j, j + 1:]).sum()) / F[j, j]
        gc = LD(0)
        if cheld:
            cbar = (ww * c_s).sum()
            if not cbar > 0:
                return None
            gc = 1 / cbar
    out = {"m": np.zeros(4, LD), "d": np.ones(4, LD), "F": np.eye(4, dtype=LD), "gc": gc}
    out["m"][idx] = m
    out["d"][idx] = d
    out["F"][np.ix_(idx, idx)] = F
    with np.errstate(over="ignore"):  # (finite in longdouble alone is not finite)
        vals = np.concatenate([out["m"], out["d"], out["F"].ravel(), [gc]]).astype(float)
    return out if np.isfinite(vals).all() else None


class Adapted:
    """A refitted proposal: u_f = m (+ K c_s) + d * (F t), the held c from the
    exponential of rate gc; the mask, the held set and K are the base's."""

    def __init__(self, base, fit):
        self.base = base.base if isinstance(base, Adapted) else base
        b = self.base
        self.u, self.idx, self.mask, self.cheld, self.K, self.valid, self.near = (b.u, b.idx, b.mask, b.cheld, b.K,
                                                                                  b.valid, b.near)
        self.m = fit["m"][self.idx]
        self.d = fit["d"][self.idx]
        self.F = fit["F"][np.ix_(self.idx, self.idx)]
        self.gc = fit["gc"] if self.cheld else b.gc

    def centre(self, c_s):
        m = np.broadcast_to(self.m, (len(c_s), self.idx.size)).copy()
        if self.cheld:
            m = m + np.outer(c_s, self.K)
        return m

    def draw(self, z, chi2, e):
        S = len(chi2)
        t = z[:, self.idx] / np.sqrt(chi2 / ref.NU)[:, None]
        c_s = e / self.gc if self.cheld else np.zeros(S, LD)
        u = np.broadcast_to(self.u.astype(LD), (S, 4)).copy()
        u[:, self.idx] = self.centre(c_s) + (t @ self.F.T) * self.d
        lg = -LD(0.5) * (ref.NU + self.idx.size) * np.log1p((t * t).sum(axis=1) / ref.NU)
        if self.cheld:
            u[:, 2] = c_s
            lg = lg - e
        return u, lg

    def log_g_at(self, u):
        u = np.asarray(u, float).astype(LD)
        c_s = u[:, 2] if self.cheld else np.zeros(len(u), LD)
        x = (u[:, self.idx] - self.centre(c_s)) / self.d
        n = self.idx.size
        t = np.zeros_like(x)
        for j in range(n - 1, -1, -1):  # F t = x, F upper triangular
            t[:, j] = (x[:, j] - (t[:, j + 1:] * self.F[j, j + 1:]).sum(axis=1)) / self.F[j, j]
        lg = -LD(0.5) * (ref.NU + n) * np.log1p((t * t).sum(axis=1) / ref.NU)
        if self.cheld:
            lg = lg - c_s * self.gc
        return lg


def full_K(prop):
    K = np.zeros(4, LD)
    K[prop.idx] = prop.K
    return K


def refit(prop, u64, w):
    """The next round's proposal from the best round's (prop, float64 draws, weights), or None."""
    fit = refit_arrays(u64, w, prop.mask, prop.cheld, full_K(prop).astype(np.float64))
    return None if fit is None else Adapted(prop, fit)


def run_round(oracle_lib, y30, N30, row, prop, rnd):
    z, chi2, e = rnd
    u, lg = prop.draw(z, chi2, e)
    u64 = u.astype(np.float64)
    lp = ref.log_target(oracle_lib, y30, N30, row, u64)
    lw = (lp - lg).astype(np.float64)
    w, khat, n_inf, ok = ref.psis_weights(lw)
    return {"prop": prop, "u": u, "u64": u64, "lw": lw, "w": w, "khat": khat, "n_inf": n_inf, "ok": ok}


def adapt_rounds(oracle_lib, y30, N30, row, prop, rnd, S: int, R: int):
    """One valid-proposal PMD row through the rounds -> dict: rounds (every
    round run, round 0 first), best (its dict), best_round, tried, rec
    (longdouble[16], bit 6 included), adapt (4 floats), margin (the smallest
    distance of a decision -- khat against tau or against the best khat -- from
    its threshold)."""
    tau = ref.khat_threshold(S)
    r0 = run_round(oracle_lib, y30, N30, row, prop, rnd)
    res = {"rounds": [r0], "best": r0, "best_round": 0, "tried": 0, "margin": np.inf}
    if not r0["ok"]:
        res["rec"] = ref.invalid_record(prop.mask)
        res["adapt"] = np.full(4, np.nan)
        return res
    best = r0
    for r in range(1, R + 1):
        if best["khat"] <= tau:
            break
        nxt = refit(best["prop"], best["u64"], best["w"])
        if nxt is None:
            break
        cur = run_round(oracle_lib, y30, N30, row, nxt, rnd)
        res["rounds"].append(cur)
        res["tried"] = r
        if not cur["ok"] or not np.isfinite(float(cur["khat"])):
            break
        if np.isfinite(float(best["khat"])):
            res["margin"] = min(res["margin"], abs(float(cur["khat"] - best["khat"])))
        if not cur["khat"] < best["khat"]:
            break
        best = cur
        res["best_round"] = r
    res["margin"] = min(res["margin"], abs(float(best["khat"]) - tau))
    res["best"] = best
    rec = ref.estimates(best["w"], ref.constrained(best["u64"]), best["khat"], best["n_inf"], S, prop.mask)
    if res["best_round"] > 0:
        rec[ref.FLAGS] += ADAPTED
    res["rec"] = rec
    res["adapt"] = np.array([float(r0["khat"]), float(1 / (r0["w"] * r0["w"]).sum()), res["best_round"], res["tried"]])
    return res


def adapt_taxon(oracle_lib, y30, N30, rec, status: int, S: int, R: int, seed: int = 0, g: int = 0, rows=(0, 1, 2)):
    """One taxon end to end -> list over `rows` of dicts (adapt_rounds' keys, plus prop; an
    unsupported row or a status != 0: prop, rec and adapt alone)."""
    out = []
    for row in rows:
        if status != 0:
            r = np.full(ref.NFIELD, np.nan, LD)
            r[ref.FLAGS] = 0
            out.append({"prop": None, "rec": r, "adapt": np.full(4, np.nan)})
            continue
        prop = ref.proposal(oracle_lib, y30, N30, rec, row)
        if not prop.valid:
            out.append({"prop": prop, "rec": ref.invalid_record(prop.mask), "adapt": np.full(4, np.nan)})
            continue
        rnd = ref.randoms(oracle_lib, seed, g, ref.SUBFITS[row][1], S)
        res = adapt_rounds(oracle_lib, y30, N30, row, prop, rnd, S, R)
        res["prop"] = prop
        out.append(res)
    return out
