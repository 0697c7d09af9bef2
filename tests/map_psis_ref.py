"""Reference of MDFIT-PSIS v1 in numpy on np.longdouble (a
helper, no test), written from the specification, not from the kernel's code:
the Philox blocks through the CPU oracle, the mode's curvature and held set
through tests/laplace_ref.py, the target through the oracle's cancellation-free
beta-binomial log-pmf plus the priors of §3.1 and the Jacobian, the smoothing
with np.argsort(kind="stable"), the weighted estimates as whole-array sums."""

from __future__ import annotations

import math

import numpy as np

from tests import laplace_ref

LD = np.longdouble
NFIELD = 16
FIELDS = ["q_mean", "A_mean", "c_mean", "phi_mean", "D_max_mean", "q_std", "A_std", "c_std", "phi_std", "D_max_std",
          "rho_Ac", "significance", "khat", "ess", "n_infeasible", "flags"]
KHAT, ESS, N_INF, FLAGS = 12, 13, 14, 15
VALID, RELIABLE = 1, 2
DOMAIN = 0xFFFC0000  # counter word 2 of draw s is DOMAIN + s; word 3 the block 0..3
SUBFITS = laplace_ref.SUBFITS  # (oracle subset, diag sub-fit) of rows all / forward / reverse
NU = 4
FLOOR = -800.0
NHALF = 15


def tail_len(S: int) -> int:
    return min(S // 5, math.isqrt(9 * S - 1) + 1)  # min(floor(S / 5), ceil(3 sqrt S))


def khat_threshold(S: int) -> float:
    return min(1.0 - 1.0 / math.log10(S), 0.7)


# --------------------------------------------------------------------------
# random numbers
# --------------------------------------------------------------------------
def _u53(a, b):
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    return ((a >> 5).astype(LD) * LD(67108864.0) + (b >> 6).astype(LD)) / LD(9007199254740992.0)


def randoms(oracle_lib, seed: int, g: int, sub: int, S: int):
    """(z[S, 4], chi2[S], e[S]) of the stream (seed, global taxon g, diag
    sub-fit sub): per draw four blocks -- two Box-Muller pairs (cos, sin), the
    chi-square's two uniforms, the exponential's uniform; a uniform is 1 - u53,
    in (0, 1]."""
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32)
    ctr = np.zeros(4, np.uint32)
    ctr[0] = g & 0xFFFFFFFF
    ctr[1] = (((g >> 32) & 0xFFFFFFFF) + (sub << 24)) & 0xFFFFFFFF
    o = np.zeros(4, np.uint32)
    fn = oracle_lib.lib.oracle_philox
    cp, kp, op = ctr.ctypes.data, key.ctypes.data, o.ctypes.data
    blocks = np.zeros((S, 4, 4), np.uint32)
    for s in range(S):
        ctr[2] = DOMAIN + s
        for b in range(4):
            ctr[3] = b
            fn(cp, kp, op)
            blocks[s, b] = o
    ua, ub = _u53(blocks[:, :, 0], blocks[:, :, 1]), _u53(blocks[:, :, 2], blocks[:, :, 3])  # [S, 4] each
    two_pi = 2 * np.arccos(LD(-1))
    r = np.sqrt(-2 * np.log(1 - ua[:, :2]))
    z = np.empty((S, 4), LD)
    z[:, 0::2] = r * np.cos(two_pi * ub[:, :2])
    z[:, 1::2] = r * np.sin(two_pi * ub[:, :2])
    chi2 = -2 * (np.log(1 - ua[:, 2]) + np.log(1 - ub[:, 2]))
    e = -np.log(1 - ua[:, 3])
    return z, chi2, e


# --------------------------------------------------------------------------
# proposal
# --------------------------------------------------------------------------
class Proposal:
    """One sub-fit's proposal: the mode u, the free set, the Jacobi scale s and
    the Cholesky factor L of the scaled free block, the held c's gradient and
    the shift K = -C_ff H_fc of the free block's centre."""

    def __init__(self, u, g, H, free, near, lap_valid):
        self.u = np.asarray(u, float)
        self.free = np.asarray(free, bool)
        self.near = bool(near)
        self.mask = int(sum(1 << j for j in range(4) if self.free[j]))
        self.cheld = not self.free[2]
        c_low = self.u[2] - laplace_ref.KULO[2] <= laplace_ref.KEPSBIND[2]
        self.valid = bool(lap_valid and self.free[0] and self.free[1] and self.free[3] and (not self.cheld or c_low))
        self.gc = LD(g[2])
        self.idx = np.flatnonzero(self.free)
        if not self.valid:
            return
        n = self.idx.size
        Hf = np.asarray(H, float)[np.ix_(self.idx, self.idx)].astype(LD)
        self.s = 1 / np.sqrt(np.diag(Hf))
        R = Hf * np.outer(self.s, self.s)
        L = np.zeros((n, n), LD)
        for j in range(n):
            for m in range(j + 1):
                v = R[j, m] - (L[j, :m] * L[m, :m]).sum()
                L[j, m] = np.sqrt(v) if j == m else v / L[m, m]
        self.L = L
        self.K = np.zeros(n, LD)
        if self.cheld:
            Li = _inv_lower(L)
            C = (Li.T @ Li) * np.outer(self.s, self.s)
            self.K = -C @ np.asarray(H, float)[self.idx, 2].astype(LD)

    def centre(self, c_s):
        """m_f[S, n] of the free block for the draws' held-c values c_s[S]."""
        m = np.broadcast_to(self.u[self.idx].astype(LD), (len(c_s), self.idx.size)).copy()
        if self.cheld:
            m = m + np.outer(c_s, self.K)
        return m

    def draw(self, z, chi2, e):
        """(u[S, 4], log g[S]) in longdouble from the stream's randoms."""
        S = len(chi2)
        t = z[:, self.idx] / np.sqrt(chi2 / NU)[:, None]
        c_s = e / self.gc if self.cheld else np.zeros(S, LD)
        # u_f = m_f + D^-1/2 L^-T t: back substitution, row by row from the last
        n = self.idx.size
        x = np.zeros((S, n), LD)
        for j in range(n - 1, -1, -1):
            x[:, j] = (t[:, j] - (x[:, j + 1:] * self.L[j + 1:, j]).sum(axis=1)) / self.L[j, j]
        u = np.broadcast_to(self.u.astype(LD), (S, 4)).copy()
        u[:, self.idx] = self.centre(c_s) + x * self.s
        lg = -LD(0.5) * (NU + n) * np.log1p((t * t).sum(axis=1) / NU)
        if self.cheld:
            u[:, 2] = c_s
            lg = lg - e
        return u, lg

    def log_g_at(self, u):
        """log g of given draws u[S, 4] (float64): t = L' D^1/2 (u_f - m_f)."""
        u = np.asarray(u, float).astype(LD)
        c_s = u[:, 2] if self.cheld else np.zeros(len(u), LD)
        x = (u[:, self.idx] - self.centre(c_s)) / self.s
        t = x @ self.L  # (L' x)_j = sum_p L[p, j] x_p
        lg = -LD(0.5) * (NU + self.idx.size) * np.log1p((t * t).sum(axis=1) / NU)
        if self.cheld:
            lg = lg - c_s * self.gc
        return lg


def _inv_lower(L):
    n = L.shape[0]
    M = np.zeros_like(L)
    for m in range(n):
        M[m, m] = 1 / L[m, m]
        for j in range(m + 1, n):
            M[j, m] = -(L[j, m:j] * M[m:j, m]).sum() / L[j, j]
    return M


def proposal(oracle_lib, y30, N30, rec, row: int) -> Proposal:
    """The proposal of PMD row `row` (0 all, 1 forward, 2 reverse) from the MAP
    record rec[80]: the oracle's g and H at the rebuilt mode, laplace_ref's held
    set and validity."""
    subset, k = SUBFITS[row]
    u = laplace_ref.record_u(rec, k)
    _, g, H, _ = oracle_lib.objective(0, subset, y30, N30, u)
    free, near = laplace_ref.free_set(u, g, H)
    J, dmax = laplace_ref.jacobian(u)
    lap = laplace_ref.stats(H, free, J, dmax)
    return Proposal(u, g, H, free, near, int(lap[7]) & laplace_ref.VALID)


# --------------------------------------------------------------------------
# target
# --------------------------------------------------------------------------
def columns(row: int) -> range:
    return (range(0, 30), range(0, NHALF), range(NHALF, 30))[row]


def constrained(u):
    """(q, A, c, phi)[S, 4] longdouble of u[S, 4]."""
    u = np.asarray(u).astype(LD)
    q = 1 / (1 + np.exp(-u[:, 0]))
    A = 1 / (1 + np.exp(-u[:, 1]))
    return np.stack([q, A, u[:, 2], np.exp(u[:, 3]) + 2], axis=1)


def log_target(oracle_lib, y30, N30, row: int, u):
    """log p(u)[S] (longdouble; -inf where c < 0 or A + c >= 1) of float64
    draws u[S, 4]: the full beta-binomial log-pmf of the row's points, the
    priors Beta(2, 3) on q and A, Beta(1, 9) on c, Exponential(1/1000) on
    delta (constants dropped), and log[q(1-q) A(1-A) delta]."""
    u = np.asarray(u, float)
    S = len(u)
    f = constrained(u)
    q, A, c, phi = f.T
    delta = phi - 2
    with np.errstate(invalid="ignore"):
        feas = (c >= 0) & (A + c < 1)
    out = np.full(S, -np.inf, LD)
    if not feas.any():
        return out
    cols = list(columns(row))
    k = np.array([col % NHALF for col in cols], LD)
    D = A[feas, None] * (1 - q[feas, None]) ** k[None, :] + c[feas, None]
    ph = np.broadcast_to(phi[feas, None], D.shape)
    yy = np.broadcast_to(np.asarray(y30, float)[cols][None, :], D.shape)
    nn = np.broadcast_to(np.asarray(N30, float)[cols][None, :], D.shape)
    ll = oracle_lib.bb_logpmf_full(yy.ravel(), nn.ravel(), (D * ph).astype(float).ravel(),
                                   ((1 - D) * ph).astype(float).ravel()).reshape(D.shape).astype(LD).sum(axis=1)
    uf = u[feas].astype(LD)
    lq, l1q = -np.log1p(np.exp(-uf[:, 0])), -np.log1p(np.exp(uf[:, 0]))
    lA, l1A = -np.log1p(np.exp(-uf[:, 1])), -np.log1p(np.exp(uf[:, 1]))
    prior = lq + 2 * l1q + lA + 2 * l1A + 8 * np.log1p(-c[feas]) - delta[feas] / 1000
    jac = lq + l1q + lA + l1A + uf[:, 3]
    out[feas] = ll + prior + jac
    return out


# --------------------------------------------------------------------------
# smoothing and estimates
# --------------------------------------------------------------------------
def gpd_fit(x):
    """(khat, sigma) of the ascending excesses x: Zhang & Stephens (2009) with loo's priors."""
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


def psis_weights(lw):
    """(w[S], khat, n_infeasible, valid) of raw log-weights lw[S] (float64; -inf
    infeasible): longdouble.  Invalid -- w and khat NaN -- with a NaN or +inf, or
    when the draw that sets the tail's cut-off is infeasible."""
    lw = np.asarray(lw, np.float64)
    S = lw.size
    inf = np.isneginf(lw)
    bad = (np.full(S, np.nan, LD), LD("nan"), int(inf.sum()), False)
    if np.isnan(lw).any() or np.isposinf(lw).any() or inf.all():
        return bad
    r = lw.astype(LD) - lw[~inf].max().astype(LD)
    rank_value = np.where(inf, LD(FLOOR), r)
    order = np.argsort(rank_value, kind="stable")
    M = tail_len(S)
    if inf[order[S - M - 1]]:
        return bad
    sv = rank_value[order]
    eu = np.exp(sv[S - M - 1])
    x = np.maximum(np.exp(sv[S - M:]) - eu, 0)
    khat = LD("inf")
    out = r.copy()
    if x[-1] == 0:
        khat = LD(0)
    elif x[(M + 2) // 4 - 1] > 0:
        khat, sigma = gpd_fit(x)
        if np.isfinite(khat):
            l1 = np.log1p(-(np.arange(M, dtype=LD) + LD(0.5)) / M)
            if abs(khat) < 30 * np.finfo(np.float64).eps:
                qq = -sigma * l1
            else:
                qq = sigma * np.expm1(-khat * l1) / khat
            out[order[S - M:]] = np.minimum(np.log(qq + eu), 0)
    w = np.exp(out)
    return w / w.sum(), khat, int(inf.sum()), True


def estimates(w, f, khat, n_inf, S: int, mask: int):
    """The record (longdouble[16]) from normalised weights w[S] and draws f[S, 4] = (q, A, c, phi)."""
    rec = np.full(NFIELD, np.nan, LD)
    w = np.asarray(w, LD)
    use = w > 0
    ww = w[use]
    f = np.asarray(f)[use].astype(LD)
    f5 = np.concatenate([f, (f[:, 1] + f[:, 2])[:, None]], axis=1)
    mean = (ww[:, None] * f5).sum(axis=0)
    d = f5 - mean
    var = (ww[:, None] * d * d).sum(axis=0)
    rec[0:5] = mean
    rec[5:10] = np.sqrt(var)
    if var[1] > 0 and var[2] > 0:
        rec[10] = (ww * d[:, 1] * d[:, 2]).sum() / np.sqrt(var[1] * var[2])
    if var[4] > 0:
        rec[11] = mean[4] / np.sqrt(var[4])
    rec[KHAT] = khat
    rec[ESS] = 1 / (w * w).sum()
    rec[N_INF] = n_inf
    rec[FLAGS] = VALID | (RELIABLE if khat <= khat_threshold(S) else 0) | (mask << 2)
    return rec


def invalid_record(mask: int):
    rec = np.full(NFIELD, np.nan, LD)
    rec[FLAGS] = mask << 2
    return rec


def record_from(prop: Proposal, u, lw, S: int):
    """The record from draws u[S, 4] and raw log-weights lw[S] (float64)."""
    if not prop.valid:
        return invalid_record(prop.mask), None
    w, khat, n_inf, ok = psis_weights(lw)
    if not ok:
        return invalid_record(prop.mask), w
    return estimates(w, constrained(np.asarray(u, float)), khat, n_inf, S, prop.mask), w


def psis_taxon(oracle_lib, y30, N30, rec, status: int, S: int, seed: int = 0, g: int = 0, rows=(0, 1, 2)):
    """One taxon end to end -> list over `rows` of dicts: prop, u, lg, lp, lw (float64), w, rec."""
    res = []
    for row in rows:
        if status != 0:
            r = np.full(NFIELD, np.nan, LD)
            r[FLAGS] = 0
            res.append({"prop": None, "rec": r})
            continue
        prop = proposal(oracle_lib, y30, N30, rec, row)
        if not prop.valid:
            res.append({"prop": prop, "rec": invalid_record(prop.mask)})
            continue
        z, chi2, e = randoms(oracle_lib, seed, g, SUBFITS[row][1], S)
        u, lg = prop.draw(z, chi2, e)
        u64 = u.astype(np.float64)
        lp = log_target(oracle_lib, y30, N30, row, u64)
        lw = (lp - lg).astype(np.float64)
        r, w = record_from(prop, u64, lw, S)
        res.append({"prop": prop, "u": u, "lg": lg, "lp": lp, "lw": lw, "w": w, "rec": r})
    return res
