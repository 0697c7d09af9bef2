"""MDFIT-AUTO v1 (mdfit_auto_route) restated in numpy: the
routing rule and the composition of a settled taxon's record, plus the crafted
records the CPU and GPU tests run through the host build and the device kernel.
Written from the issue's rule, not from csrc/mdfit_auto.h."""

from __future__ import annotations

import numpy as np

NOUT, NPSIS, NWAIC = 80, 16, 8
OK, MAXITER, NONFINITE, INVALID = 0, 1, 2, 3
R_WAIC, R_PSIS, R_STATUS, R_INVALID, R_SAMPLE = 1, 2, 4, 8, 7
# result columns (enum mdfit_field)
F = {"n_sigma": 1, "q_mean": 4, "concentration_mean": 5, "D_max_marginalized_mean": 6, "n_sigma_forward": 15,
     "q_mean_forward": 17, "n_sigma_reverse": 18, "q_mean_reverse": 20, "asymmetry": 21}
COMPOSED = sorted(F.values())
# (column, source record, row, field): psis fields q_mean 0, phi_mean 3, D_max_mean 4; waic row 6 fields 0..3
COPIES = [(F["q_mean"], "psis", 0, 0), (F["concentration_mean"], "psis", 0, 3),
          (F["D_max_marginalized_mean"], "psis", 0, 4), (F["q_mean_forward"], "psis", 1, 0),
          (F["q_mean_reverse"], "psis", 2, 0), (F["n_sigma"], "waic", 6, 0), (F["n_sigma_forward"], "waic", 6, 1),
          (F["n_sigma_reverse"], "waic", 6, 2), (F["asymmetry"], "waic", 6, 3)]


def _bits(f) -> int:
    """A flags field (an integer stored as double); what is no such integer has no bit."""
    f = float(f)
    return int(f) if 0.0 <= f < 4294967296.0 else 0


def route_one(status: int, psis: np.ndarray, waic: np.ndarray) -> int:
    if status == INVALID:
        return R_INVALID
    r = 0
    if not _bits(waic[6, NWAIC - 1]) & 2:
        r |= R_WAIC
    if any((_bits(psis[k, NPSIS - 1]) & 3) != 3 for k in range(3)):
        r |= R_PSIS
    if status in (MAXITER, NONFINITE):
        r |= R_STATUS
    return r


def auto_route(status, psis, waic, out):
    """(route int32[T], composed copy of out[T, NOUT]) of status[T], psis[T, 3,
    16], waic[T, 7, 8]."""
    status, psis, waic = np.asarray(status), np.asarray(psis), np.asarray(waic)
    out = np.array(out, dtype=np.float64, copy=True)
    route = np.array([route_one(int(status[t]), psis[t], waic[t]) for t in range(len(status))], dtype=np.int32)
    for t in np.flatnonzero(route == 0):
        for col, src, row, field in COPIES:
            out[t, col] = (psis if src == "psis" else waic)[t, row, field]
    return route, out


def crafted():
    """status[T], psis[T, 3, 16], waic[T, 7, 8], out[T, 80]: every combination of
    (status 0..3) x (waic row 6 flags 0, 1, 3) x (psis rows: all reliable / row 1
    valid but unreliable / row 2 invalid with NaN statistics / row 0 flags NaN),
    with distinct finite payloads elsewhere -- NaN, -0.0 and inf among the
    copied fields --, NaN statistics in invalid rows, and the NaN record of a
    status-3 taxon."""
    rng = np.random.default_rng(20261020)
    rows = []
    for status in (OK, MAXITER, NONFINITE, INVALID):
        for wflags in (0.0, 1.0, 3.0):
            for pkind in range(4):
                rows.append((status, wflags, pkind))
    T = len(rows)
    st = np.array([r[0] for r in rows], dtype=np.int32)
    psis = rng.normal(size=(T, 3, NPSIS))
    waic = rng.normal(size=(T, 7, NWAIC))
    out = rng.normal(size=(T, NOUT))
    for t, (status, wflags, pkind) in enumerate(rows):
        psis[t, :, NPSIS - 1] = 3.0 + 60.0  # valid, reliable, four free bits
        waic[t, :6, NWAIC - 1] = 3.0 + 60.0
        waic[t, 6, NWAIC - 1] = wflags
        if wflags == 0.0:  # an invalid comparison row: NaN statistics
            waic[t, 6, :6] = np.nan
        if pkind == 1:
            psis[t, 1, NPSIS - 1] = 1.0 + 60.0
        elif pkind == 2:
            psis[t, 2, :NPSIS - 1] = np.nan
            psis[t, 2, NPSIS - 1] = 60.0
        elif pkind == 3:
            psis[t, 0, NPSIS - 1] = np.nan
        if status == INVALID:
            out[t] = np.nan
            psis[t, :, :NPSIS - 1] = np.nan
            psis[t, :, NPSIS - 1] = 0.0
            waic[t, :, :NWAIC - 1] = np.nan
            waic[t, :, NWAIC - 1] = 0.0
    # special values among what a route-0 taxon copies (rows[3] ... are (OK, 3.0, 0) -> index 8)
    t0 = rows.index((OK, 3.0, 0))
    psis[t0, 0, 0] = -0.0
    psis[t0, 1, 0] = np.inf
    waic[t0, 6, 3] = np.nan
    waic[t0, 6, 1] = 5e-324
    return st, psis, waic, out
