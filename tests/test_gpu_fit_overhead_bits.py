"""The fit kernel returns the records, predictions and status of the commit
before its pad lanes were given a neutral lg3 argument, bit for bit, in both
lane layouts.

The 96-taxon batch (tools/record_fit_overhead_golden.py: the 29 taxa of
map_boundary_cases.json -- polish phase, saddle escape, gradient fallback,
flat-tail rescue -- among 67 crafted ones) holds the cases where the pad's
argument matters: a0 = D(1) phi below 10 with every real y >= 10 and with
some y < 10, b0 below 10, phi below 10 (the pad's phi triple must still take
lg3's shift), y = 0 at far positions.  With 96 taxa every queue of the
one-point-per-lane layout holds 12: its waves fit two PMD or two null models.
The first 91 taxa alone give queues of 11, where a wave holds the last PMD
fit beside the first null fit; both calls are in the fixture.

The fixture tests/golden/fit_overhead_records.npz was recorded from the parent
commit on a GPU by tools/record_fit_overhead_golden.py, never from the code
under test.  The CPU test here checks on the oracle's modes that the batch
holds every argument case.  Of the rare paths the oracle's record reports only
the polish phase (and each sub-fit's evaluation count and status): that one is
asserted.  The saddle escape, the gradient fallback and the flat-tail rescue
are not flagged in the record, so those taxa are chosen by provenance -- each
boundary case's "source" in map_boundary_cases.json says which path it was
collected for and that it ended with status 1 before that path existed -- and
the test asserts what follows from it: every one of them now ends with status
0, after a chain too long for a plain Newton descent.
"""

from __future__ import annotations

import importlib.util

import numpy as np
import pytest

from tests.helpers import GOLDEN

ROOT = GOLDEN.parents[1]


def _tool():
    # the batch is defined once, in the tool that recorded the fixture
    path = ROOT / "tools" / "record_fit_overhead_golden.py"
    spec = importlib.util.spec_from_file_location("record_fit_overhead_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "fit_overhead_records.npz")


@pytest.fixture(scope="module")
def batch():
    return TOOL.batch(ROOT)


def test_fixture_is_the_parents(golden):
    assert (GOLDEN / "fit_overhead_records.npz").stat().st_size < 1_000_000
    assert len(str(golden["commit"])) == 40
    n, m = TOOL.N_TAXA, TOOL.N_ODD
    assert (n, m) == (96, 91) and any((m * (q + 1) // 8 - m * q // 8) % 2 for q in range(8))
    assert golden["out"].shape == (n, 80) and golden["out"].dtype == np.float64
    assert golden["pred"].shape[0] == n and golden["status"].shape == (n,)
    assert golden["out_odd"].shape == (m, 80) and golden["status_odd"].shape == (m,)
    diag = golden["out"][:, 32:80].reshape(n, 6, 8)
    assert int((diag[:, :, 7] == 1).sum()) >= 10  # polished sub-fits
    assert int((diag[:, :, 5] >= 30).sum()) >= 20  # long chains


def test_batch_holds_every_case_at_the_oracles_modes(batch):
    from oracle.oracle import OracleLib

    y, N, mm = batch
    assert y.shape == (96, 32)
    out, _, st = OracleLib().fit_batch(y, N, mm)
    diag = np.asarray(out)[:, 32:80].reshape(96, 6, 8)  # per sub-fit: q, A, c, phi, F, evals, status, polished
    q, A, c, phi = (diag[:, :, j] for j in range(4))
    pmd = np.array([True, False, True, True, False, False])
    D1 = np.where(pmd[None, :], A + c, q)  # D at |z| = 1: the pad lane's
    a0, b0 = D1 * phi, (1.0 - D1) * phi
    yy = y[:, :30].astype(np.float64)
    ymin = yy.min(1)
    P = 0  # the PMD all-position fit
    assert ((a0[:, P] < 10) & (ymin >= 10)).sum() >= 3  # the pad alone would take the shift of lg3(y + a)
    assert ((a0[:, P] < 10) & (ymin < 10)).sum() >= 3  # real points take it too
    assert (b0[:, P] < 10).sum() >= 3 and ((b0[:, P] < 10) & (phi[:, P] >= 10)).sum() >= 3
    assert (phi[:, P] < 10).sum() >= 3  # the phi triple itself shifts
    assert ((a0[:, 1] < 10).sum() >= 3) and ((b0[:, 1] < 10).sum() >= 3)  # null fits: the pad's triples are read
    far = np.r_[10:15, 25:30]
    assert ((yy[:, far] == 0).sum(1) >= 3).sum() >= 10  # y = 0 at far positions
    # the rare paths.  Asserted on the oracle: the polish phase (its flag), status
    # and chain lengths.  By provenance only (see the docstring): which taxa take
    # the saddle escape, the gradient fallback and the flat-tail rescue
    rows = TOOL.boundary_rows(ROOT)
    assert len(rows) == 29
    kinds = {k: [t for t, n in rows.items() if n.startswith(k)] for k in ("c5_", "c5g_", "m1s3g_", "s101_t4066", "m1s3_")}
    assert all(kinds.values())  # flat-tail rescue, gradient fallback (two sources), saddle escape, polish
    assert (st[list(rows)] == 0).all()  # each of them converges only through its path
    assert int((diag[list(rows), :, 7] == 1).sum()) >= 10
    assert diag[kinds["m1s3_"][0], :, 7].any() and diag[kinds["s101_t4066"][0], 2, 5] >= 20
    for k in ("c5_", "c5g_", "m1s3g_"):  # each needed its path to converge: no short chain among them
        assert all(diag[t, :, 5].max() >= 30 for t in kinds[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("ppl", ["1", "2"])
def test_records_equal_the_parent_commits(golden, batch, monkeypatch, ppl):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    from metadamage_amd import engine

    monkeypatch.setenv("MDFIT_FIT_PPL", ppl)
    y, N, mm = batch
    for n, suffix in ((TOOL.N_TAXA, ""), (TOOL.N_ODD, "_odd")):
        out, pred, status = engine.fit_batch(y[:n], N[:n], mm[:n])
        out = np.asarray(out, np.float64)
        pred = np.asarray(pred, np.float32)
        ref_out, ref_pred, ref_status = golden["out" + suffix], golden["pred" + suffix], golden["status" + suffix]
        bad = out.view(np.uint64) != ref_out.view(np.uint64)
        badp = pred.view(np.uint32) != ref_pred.view(np.uint32)
        print(f"PPL {ppl}, {n} taxa: {int(bad.sum())} of {bad.size} record values and {int(badp.sum())} of {badp.size} "
              f"predictions differ (taxa {np.flatnonzero(bad.any(1))[:8].tolist()}, "
              f"columns {np.flatnonzero(bad.any(0))[:8].tolist()})")
        assert out.tobytes() == ref_out.tobytes()
        assert pred.tobytes() == ref_pred.tobytes()
        assert np.array_equal(np.asarray(status), ref_status)
