"""Reference for the Laplace standard errors of the MAP modes (a helper, no test).

numpy only.  H and g come from the CPU oracle's objective at the u rebuilt from
a given record's diagnostic slots; the held-set rule (the optimiser's
Bertsekas rule, free_set in csrc/mdfit_model.h), the Jacobi scaling, the
validity rule and the delta method are restated here on their own
(DESIGN.md §3.7).  An mpmath twin of the linear algebra (50 digits) serves the
tests of the device's and the host's 4x4 routine.
"""

from __future__ import annotations

import numpy as np

F_DIAG, DIAG_STRIDE = 32, 8
KULO = np.array([-25.0, -25.0, 0.0, -25.0])
KUHI = np.array([25.0, 25.0, 0.999, 20.0])
KEPSBIND = np.array([1e-3, 1e-3, 1e-4, 1e-3])
KEPSACT = 1e-8
PIV_MIN = 1e-8
VALID = 16
FIELDS = ["q_std", "A_std", "c_std", "phi_std", "D_max_std", "rho_Ac", "significance", "flags"]
SUBFITS = [(0, 0), (1, 2), (2, 3)]  # (oracle subset, diag sub-fit) of lap rows all / forward / reverse


def rebuild_u(q, A, c, phi):
    """u = (logit q, logit A, c, log(phi - 2)) clamped into the optimiser's box."""
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.array([np.log(q) - np.log1p(-q), np.log(A) - np.log1p(-A), c, np.log(phi - 2.0)])
    return np.minimum(np.maximum(u, KULO), KUHI)


def record_u(rec, diag_subfit):
    d = rec[F_DIAG + DIAG_STRIDE * diag_subfit:][:4]
    return rebuild_u(d[0], d[1], d[2], d[3])


def free_set(u, g, H, eps=KEPSBIND):
    """(free[4], near): the coordinates the binding rule leaves free, in the
    rule's own FP64 comparisons; near: some comparison it took lies within 1e-6
    relative of its threshold (the decision is then not the data's)."""
    u, g = np.asarray(u, float), np.asarray(g, float)
    free = np.ones(4, bool)
    near = False

    def close(a, b):
        return abs(a - b) <= 1e-6 * max(abs(a), abs(b))

    for j in range(4):
        dlo, dhi = u[j] - KULO[j], KUHI[j] - u[j]
        atlo, athi = dlo <= eps[j], dhi <= eps[j]
        hjj = H[j, j]
        hnp = hjj <= 0.0
        glo, ghi = g[j] > -KEPSACT, g[j] < KEPSACT
        slo, shi = g[j] + KEPSACT > hjj * dlo, -g[j] + KEPSACT > hjj * dhi
        bind = (atlo and glo and (hnp or slo)) or (athi and ghi and (hnp or shi))
        free[j] = not bind
        near = near or close(dlo, eps[j]) or close(dhi, eps[j])
        if atlo:
            near = near or close(g[j], -KEPSACT) or close(g[j] + KEPSACT, hjj * dlo)
        if athi:
            near = near or close(g[j], KEPSACT) or close(-g[j] + KEPSACT, hjj * dhi)
    return free, near


def jacobian(u):
    """(J[4], D_max): dtheta/du = (q(1-q), A(1-A), 1, delta) and A + c at u."""
    q = 1.0 / (1.0 + np.exp(-u[0]))
    A = 1.0 / (1.0 + np.exp(-u[1]))
    omq = 1.0 / (1.0 + np.exp(u[0]))
    omA = 1.0 / (1.0 + np.exp(u[1]))
    return np.array([q * omq, A * omA, 1.0, np.exp(u[3])]), A + u[2]


def _record(C, free, J, dmax):
    rec = np.full(8, np.nan)
    Cf = np.zeros((4, 4))
    idx = np.flatnonzero(free)
    Cf[np.ix_(idx, idx)] = C
    rec[:4] = J * np.sqrt(np.diag(Cf))
    var = J[1] ** 2 * Cf[1, 1] + Cf[2, 2] + 2.0 * J[1] * Cf[1, 2]
    rec[4] = np.sqrt(max(var, 0.0))
    if free[1] and free[2]:
        rec[5] = Cf[1, 2] / np.sqrt(Cf[1, 1] * Cf[2, 2])
    if rec[4] > 0.0:
        rec[6] = dmax / rec[4]
    return rec


def stats(H, free, J, dmax):
    """One Laplace record (FIELDS) from H (4x4), the free mask, J and D_max."""
    free = np.asarray(free, bool)
    mask = int(sum(1 << j for j in range(4) if free[j]))
    bad = np.full(8, np.nan)
    bad[7] = mask
    idx = np.flatnonzero(free)
    if idx.size == 0:
        return bad
    Hf = np.asarray(H, float)[np.ix_(idx, idx)]
    dg = np.diag(Hf)
    if not (dg > 0.0).all():
        return bad
    s = 1.0 / np.sqrt(dg)
    R = Hf * np.outer(s, s)
    try:
        L = np.linalg.cholesky(R)
    except np.linalg.LinAlgError:
        return bad
    if not (np.diag(L) ** 2 > PIV_MIN).all():
        return bad
    C = np.linalg.inv(R) * np.outer(s, s)
    rec = _record(C, free, J, dmax)
    rec[7] = mask | VALID
    return rec


def stats_mp(H, free, J, dmax, dps=50):
    """stats() in mpmath at `dps` digits -> (record as float64[8], kappa, amp):
    kappa the 2-norm condition number of the scaled free block, amp the
    cancellation factor (J_A^2 C_AA + C_cc + 2|J_A C_Ac|) / var_D of D_max_std.
    The validity rule is the caller's: the record is computed whenever the free
    block factors."""
    import mpmath as mp

    free = np.asarray(free, bool)
    idx = [j for j in range(4) if free[j]]
    n = len(idx)
    with mp.workdps(dps):
        Hf = mp.matrix(n, n)
        for a, j in enumerate(idx):
            for b, m in enumerate(idx):
                Hf[a, b] = mp.mpf(float(H[j][m]))
        s = [1 / mp.sqrt(Hf[a, a]) for a in range(n)]
        R = mp.matrix(n, n)
        for a in range(n):
            for b in range(n):
                R[a, b] = Hf[a, b] * s[a] * s[b]
        ev = mp.eigsy(R, eigvals_only=True)
        ev = [ev[i] for i in range(n)]
        kappa = float(max(ev) / min(ev))
        Ri = mp.inverse(R)
        C = mp.matrix(4, 4)
        for a, j in enumerate(idx):
            for b, m in enumerate(idx):
                C[j, m] = Ri[a, b] * s[a] * s[b]
        Jm = [mp.mpf(float(x)) for x in J]
        rec = np.full(8, np.nan)
        for j in range(4):
            rec[j] = float(Jm[j] * mp.sqrt(C[j, j]))
        var = Jm[1] ** 2 * C[1, 1] + C[2, 2] + 2 * Jm[1] * C[1, 2]
        gross = Jm[1] ** 2 * C[1, 1] + C[2, 2] + 2 * abs(Jm[1] * C[1, 2])
        amp = float(gross / var) if var > 0 else float("inf")
        sd = mp.sqrt(var) if var > 0 else mp.mpf(0)
        rec[4] = float(sd)
        if free[1] and free[2]:
            rec[5] = float(C[1, 2] / mp.sqrt(C[1, 1] * C[2, 2]))
        if sd > 0:
            rec[6] = float(mp.mpf(float(dmax)) / sd)
        rec[7] = int(sum(1 << j for j in range(4) if free[j])) | VALID
    return rec, kappa, amp


def laplace_taxon(oracle_lib, y30, N30, rec, status):
    """The three Laplace records of one taxon from its MAP record `rec`
    (float64[80]) -> (lap[3, 8], near[3], hmax[3]): oracle H and g at the
    rebuilt u, then free_set / stats above.  status != 0: NaN, flags 0."""
    lap = np.full((3, 8), np.nan)
    near = np.zeros(3, bool)
    hmax = np.zeros(3)
    if status != 0:
        lap[:, 7] = 0.0
        return lap, near, hmax
    for r, (subset, k) in enumerate(SUBFITS):
        u = record_u(rec, k)
        _, g, H, _ = oracle_lib.objective(0, subset, y30, N30, u)
        free, near[r] = free_set(u, g, H)
        J, dmax = jacobian(u)
        lap[r] = stats(H, free, J, dmax)
        hmax[r] = np.abs(H).max()
    return lap, near, hmax


def laplace_batch(oracle_lib, y, N, out, status):
    """laplace_taxon over a batch -> (lap[T, 3, 8], near[T, 3])."""
    T = len(status)
    lap = np.empty((T, 3, 8))
    near = np.zeros((T, 3), bool)
    for t in range(T):
        lap[t], near[t], _ = laplace_taxon(oracle_lib, y[t, :30], N[t, :30], out[t], int(status[t]))
    return lap, near
