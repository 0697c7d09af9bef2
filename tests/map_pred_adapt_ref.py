"""Reference of mdfit_map_pred_adapt (MDFIT-AUTO v1.1) in numpy
(a helper, no test): tests/map_adapt_ref.adapt_taxon's best-round draws and
weights fed to tests/map_pred_ref.pred_given, the adapt rows beside them and
MDFIT_FLAG_ADAPTED on the record when some valid row's best round is > 0."""

from __future__ import annotations

import numpy as np

from tests import map_adapt_ref as ad
from tests import map_pred_ref as mref
from tests import map_psis_ref as pref


def pred_adapt_taxon(oracle_lib, y30, N30, out_rec, status: int, S: int, R: int, rounds: int, seed: int = 0,
                     g: int = 0):
    """One taxon end to end on the reference's own rounds: map_pred_ref's dict
    (rec, ppred, index, counts) plus adapt[3, 4] and best_round[3] (-1: invalid)."""
    if status != 0:
        got = mref.invalid_taxon(R)
        got["adapt"], got["best_round"] = np.full((3, 4), np.nan), np.full(3, -1)
        return got
    rows = ad.adapt_taxon(oracle_lib, y30, N30, out_rec, status, S, rounds, seed=seed, g=g)
    psis_rec = np.full((3, pref.NFIELD), np.nan)
    draws = np.full((3, S, 6), np.nan)
    best_round = np.full(3, -1)
    for r, res in enumerate(rows):
        psis_rec[r] = np.asarray(res["rec"]).astype(np.float64)
        if int(psis_rec[r, pref.FLAGS]) & pref.VALID:
            b = res["best"]
            draws[r, :, :4], draws[r, :, 4], draws[r, :, 5] = b["u64"], b["lw"], np.asarray(b["w"], np.float64)
            best_round[r] = res["best_round"]
    got = mref.pred_given(oracle_lib, N30, psis_rec, draws, S, R, seed=seed, g=g)
    if (best_round > 0).any():
        got["rec"][mref.FLAGS] += ad.ADAPTED
    got["adapt"] = np.array([np.asarray(res["adapt"], np.float64) for res in rows])
    got["best_round"] = best_round
    return got
