"""The fit kernel's Newton logic reproduces the records of the commit before
its restructuring bit for bit, in both lane layouts.

The batch is small but reaches the rare paths of the logic: long chains,
backtracking, the polish phase, the saddle escape, the gradient fallback and
the flat-tail rescue (the 29 taxa of map_boundary_cases.json; the 512
synthetic taxa alone never enter the polish phase).  The fixture
tests/golden/fit_logic_records.npz was recorded from the parent commit by
tools/record_fit_logic_golden.py, never from the code under test.
"""

from __future__ import annotations

import importlib.util

import numpy as np
import pytest

from tests.helpers import GOLDEN


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN / "fit_logic_records.npz")
    return g["out"], g["status"]


@pytest.fixture(scope="module")
def batch():
    # the batch is defined once, in the tool that recorded the fixture
    path = GOLDEN.parents[1] / "tools" / "record_fit_logic_golden.py"
    spec = importlib.util.spec_from_file_location("record_fit_logic_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.batch(GOLDEN.parents[1])


def test_fixture_reaches_the_rare_paths(golden):
    out, status = golden
    assert out.shape == (541, 80) and out.dtype == np.float64 and status.shape == (541,)
    diag = out[:, 32:80].reshape(541, 6, 8)
    assert int((diag[:, :, 7] == 1).sum()) >= 20  # polished sub-fits
    assert int((diag[:, :, 5] >= 30).sum()) >= 10  # long chains


@pytest.mark.gpu
@pytest.mark.parametrize("ppl", ["1", "2"])
def test_records_equal_the_parent_commits(golden, batch, monkeypatch, ppl):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    from metadamage_amd import engine

    ref_out, ref_status = golden
    monkeypatch.setenv("MDFIT_FIT_PPL", ppl)
    out, _, status = engine.fit_batch(*batch)
    out = np.asarray(out, np.float64)
    assert out.shape == ref_out.shape
    bad = ~((out == ref_out) | (np.isnan(out) & np.isnan(ref_out)))
    print(f"PPL {ppl}: {int(bad.sum())} of {bad.size} record values differ "
          f"(taxa {np.flatnonzero(bad.any(1))[:8].tolist()}, columns {np.flatnonzero(bad.any(0))[:8].tolist()})")
    assert np.array_equal(out, ref_out, equal_nan=True)
    assert np.array_equal(np.asarray(status), ref_status)
