"""CPU tests of the predictive kernel with the proposal rounds
(mdfit_map_pred_adapt, MDFIT-AUTO v1.1): the C-ABI entry point
without a device and the reference (tests/map_pred_adapt_ref.py) -- with no
rounds it is map_pred_ref.pred_taxon exactly, and with three rounds the pred
record turns reliable for taxa whose round-0 record is not."""

from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import map_adapt_ref as ad
from tests import map_pred_adapt_ref as paref
from tests import map_pred_ref as mref
from tests import map_psis_ref as pref

ROOT = Path(__file__).resolve().parents[1]
S_A, R_PRED, ROUNDS, SEED = 256, 100, 3, 0


def test_entry_point_declared_exported_and_argument_checked():
    from metadamage_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mdfit.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+mdfit_map_pred_adapt\s*\(", text)
    assert f"#define MDFIT_ABI_VERSION {_lib.ABI_VERSION}" in text and _lib.ABI_VERSION == 3
    assert "mdfit_map_pred_adapt" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                        check=True).stdout
    assert re.search(r"\bT mdfit_map_pred_adapt\b", nm)
    dummy = ctypes.c_void_p(16)
    none4, d4 = (None, None, None, None), (dummy, dummy, dummy, dummy)
    f = lib.mdfit_map_pred_adapt
    assert f(*none4, 0, 256, 1000, 3, 0, 0, None, None, None, None, None, None) == 0
    assert f(*none4, -1, 256, 1000, 3, 0, 0, None, None, None, None, None, None) == -1
    assert b"n_taxa" in lib.mdfit_last_error()
    for S in (24, 1025):
        assert f(*d4, 1, S, 1000, 3, 0, 0, dummy, dummy, None, None, None, None) == -1
        assert b"num_draws" in lib.mdfit_last_error()
    for R in (24, 1025):
        assert f(*d4, 1, 256, R, 3, 0, 0, dummy, dummy, None, None, None, None) == -1
        assert b"num_pred" in lib.mdfit_last_error()
    for rounds in (-1, _lib.ADAPT_MAX_ROUNDS + 1):
        assert f(*d4, 1, 256, 1000, rounds, 0, 0, dummy, dummy, None, None, None, None) == -1
        assert b"adapt_rounds" in lib.mdfit_last_error()
    assert f(*d4, 1, 256, 1000, 3, 0, 0, dummy, None, None, None, None, None) == -1  # rec is required
    assert b"null" in lib.mdfit_last_error()
    assert f(*d4, 1, 256, 1000, 3, 0, 0, None, dummy, None, None, None, None) == -1  # ppred is required
    assert f(*d4, (1 << 25) + 1, 256, 1000, 3, 0, 0, dummy, dummy, None, None, None, None) == -1
    assert b"2^25" in lib.mdfit_last_error()


@pytest.fixture(scope="module")
def batch(oracle_lib):
    from metadamage_amd.synthetic import generate

    b = generate(300, seed=21)
    out, _, st = oracle_lib.fit_batch(b.y, b.N)
    return b, out, st


def test_no_rounds_is_the_plain_reference_exactly(batch, oracle_lib):
    b, out, st = batch
    n_valid = 0
    for t in range(12):
        args = (oracle_lib, b.y[t, :30], b.N[t, :30], out[t], int(st[t]), S_A, R_PRED)
        want = mref.pred_taxon(*args, seed=SEED, g=t)
        got = paref.pred_adapt_taxon(*args, 0, seed=SEED, g=t)
        for key in ("rec", "ppred", "index", "counts"):
            assert np.array_equal(got[key], want[key], equal_nan=key in ("rec", "ppred")), (t, key)
        valid = got["best_round"] >= 0
        assert (got["best_round"][valid] == 0).all() and not int(got["rec"][mref.FLAGS]) & ad.ADAPTED
        # adapt reads (khat, ess, 0, 0)
        np.testing.assert_array_equal(got["adapt"][valid, 0], got["rec"][mref.KHAT:mref.KHAT + 3][valid])
        np.testing.assert_array_equal(got["adapt"][valid, 2:], 0.0)
        np.testing.assert_allclose(got["adapt"][valid, 1], got["rec"][mref.ESS:mref.ESS + 3][valid], rtol=1e-13)
        n_valid += int(valid.sum())
    assert n_valid >= 30


def test_rounds_turn_the_pred_record_reliable(batch, oracle_lib):
    """DESIGN.md §3.12 records 153 -> 23 PMD rows over tau on this batch at S =
    256, R = 3; here the first 24 taxa: every taxon whose three rows are valid,
    with some round-0 khat over tau and every best khat at or below it, must
    come out of pred_adapt_taxon reliable and adapted -- and there is one."""
    b, out, st = batch
    tau = pref.khat_threshold(S_A)
    rescued = []
    for t in range(24):
        rows = ad.adapt_taxon(oracle_lib, b.y[t, :30], b.N[t, :30], out[t], int(st[t]), S_A, ROUNDS, seed=SEED, g=t)
        if not all("rounds" in r and r["rounds"][0]["ok"] for r in rows):
            continue
        k0 = [float(r["rounds"][0]["khat"]) for r in rows]
        kb = [float(r["best"]["khat"]) for r in rows]
        if max(k0) > tau and max(kb) <= tau:
            rescued.append(t)
    assert rescued, "no taxon of the first 24 is rescued by the rounds"
    for t in rescued[:2]:
        args = (oracle_lib, b.y[t, :30], b.N[t, :30], out[t], int(st[t]), S_A, R_PRED)
        r0 = paref.pred_adapt_taxon(*args, 0, seed=SEED, g=t)
        r3 = paref.pred_adapt_taxon(*args, ROUNDS, seed=SEED, g=t)
        f0, f3 = int(r0["rec"][mref.FLAGS]), int(r3["rec"][mref.FLAGS])
        assert f0 & mref.VALID and not f0 & mref.RELIABLE and not f0 & ad.ADAPTED, (t, f0)
        assert f3 & mref.VALID and f3 & mref.RELIABLE and f3 & ad.ADAPTED, (t, f3)
        assert (r3["best_round"] > 0).any() and np.array_equal(r3["adapt"][:, 0], r0["adapt"][:, 0])
        for row in np.flatnonzero(r3["best_round"] == 0):  # a row the rounds left alone keeps its index
            assert np.array_equal(r3["index"][row], r0["index"][row]), (t, row)
        assert np.isfinite(r3["rec"][:5]).all() and r3["rec"][1] <= r3["rec"][0] <= r3["rec"][2]
