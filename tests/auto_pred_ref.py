"""MDFIT-AUTO v1.1 (mdfit_auto_route_pred) restated in numpy (a
helper, no test): v1's routing rule (tests/auto_ref.py) with the pred record's
bit, and the composition of a settled taxon's record -- v1's nine columns, the
five predictive columns and the 90 prediction floats.  Written from the issue's
rule, not from csrc/mdfit_auto.h."""

from __future__ import annotations

import itertools

import numpy as np

from tests import auto_ref as v1

NOUT, NPSIS, NWAIC, NPRED_REC, NPRED_FLOATS = v1.NOUT, v1.NPSIS, v1.NWAIC, 16, 90
R_PRED, R_SAMPLE_PRED = 16, 23
PRED_FLAGS, PRED_NNONCOUNT = 15, 14
# result columns (enum mdfit_field) <- prec fields 0..4
F_PRED = {"D_max": 0, "D_max_lower_hpdi": 2, "D_max_upper_hpdi": 3, "D_max_forward": 16, "D_max_reverse": 19}
PRED_COPIES = [(F_PRED["D_max"], 0), (F_PRED["D_max_lower_hpdi"], 1), (F_PRED["D_max_upper_hpdi"], 2),
               (F_PRED["D_max_forward"], 3), (F_PRED["D_max_reverse"], 4)]
COMPOSED = sorted(v1.COMPOSED + list(F_PRED.values()))  # the 14 columns


def route_one(status: int, psis, waic, prec) -> int:
    if status == v1.INVALID:
        return v1.R_INVALID
    r = v1.route_one(status, psis, waic)
    if not v1._bits(prec[PRED_FLAGS]) & 2 or not float(prec[PRED_NNONCOUNT]) == 0.0:
        r |= R_PRED
    return r


def auto_route_pred(status, psis, waic, prec, ppred, out, pred=None):
    """(route int32[T], composed copy of out[T, NOUT], composed copy of pred[T, 90]
    or None) of status[T], psis[T, 3, 16], waic[T, 7, 8], prec[T, 16], ppred[T, 90]."""
    status, psis, waic, prec = np.asarray(status), np.asarray(psis), np.asarray(waic), np.asarray(prec)
    ppred = np.asarray(ppred, np.float32).reshape(len(status), NPRED_FLOATS)
    out = np.array(out, dtype=np.float64, copy=True)
    if pred is not None:
        pred = np.array(pred, dtype=np.float32, copy=True).reshape(len(status), NPRED_FLOATS)
    route = np.array([route_one(int(status[t]), psis[t], waic[t], prec[t]) for t in range(len(status))],
                     dtype=np.int32)
    for t in np.flatnonzero(route == 0):
        for col, src, row, field in v1.COPIES:
            out[t, col] = (psis if src == "psis" else waic)[t, row, field]
        for col, field in PRED_COPIES:
            out[t, col] = prec[t, field]
        if pred is not None:
            pred[t] = ppred[t]
    return route, out, pred


def crafted():
    """status[T], psis[T, 3, 16], waic[T, 7, 8], prec[T, 16], ppred[T, 90],
    out[T, 80], pred[T, 90]: status 0..3 x (waic row 6 reliable or not) x (psis
    reliable or not) x (pred flags 3, 1, NaN, -2, 2^32 + 3, 67) x (n_noncount 0,
    1, NaN) -- every combination of the five route causes --, distinct finite
    payloads elsewhere, NaN, -0.0, inf and a subnormal among what is copied."""
    rng = np.random.default_rng(20261021)
    rows = list(itertools.product((v1.OK, v1.MAXITER, v1.NONFINITE, v1.INVALID), (3.0, 1.0), (True, False),
                                  (3.0, 1.0, np.nan, -2.0, 4294967299.0, 67.0), (0.0, 1.0, np.nan)))
    T = len(rows)
    st = np.array([r[0] for r in rows], dtype=np.int32)
    psis = rng.normal(size=(T, 3, NPSIS))
    waic = rng.normal(size=(T, 7, NWAIC))
    prec = rng.normal(size=(T, NPRED_REC))
    ppred = rng.normal(size=(T, NPRED_FLOATS)).astype(np.float32)
    out = rng.normal(size=(T, NOUT))
    pred = rng.normal(size=(T, NPRED_FLOATS)).astype(np.float32)
    for t, (status, wflags, prel, pflags, nnon) in enumerate(rows):
        psis[t, :, NPSIS - 1] = 3.0 + 60.0
        if not prel:
            psis[t, 1, NPSIS - 1] = 1.0 + 60.0
        waic[t, :6, NWAIC - 1] = 3.0 + 60.0
        waic[t, 6, NWAIC - 1] = wflags
        prec[t, PRED_FLAGS] = pflags
        prec[t, PRED_NNONCOUNT] = nnon
        if status == v1.INVALID:
            out[t] = np.nan
            pred[t] = np.nan
    t0 = rows.index((v1.OK, 3.0, True, 3.0, 0.0))
    prec[t0, 0], prec[t0, 1], prec[t0, 3], prec[t0, 4] = -0.0, np.nan, np.inf, 5e-324
    ppred[t0, 0], ppred[t0, 1], ppred[t0, 89] = np.nan, -0.0, np.float32(1e-45)
    return st, psis, waic, prec, ppred, out, pred
