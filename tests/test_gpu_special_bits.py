"""The log / lnGamma primitives of csrc/mdfit_special.h return, on the GPU, the
bits of the commit before lg3's evaluation was trimmed (flog_pos for the logs
whose argument is positive by construction, the shift recursion from its j = 0
step's result): flog, lg3 in both forms, lgdiff and lrise through
mdfit_primitive, at the x values of their grids in primitives_golden.npz, the
edges of the shift (0, the smallest subnormal, 10 and its neighbours) and, for
lrise, counts n against s on both sides of s <= n + 1.

The fixture tests/golden/special_bits_parent.npz was recorded from the parent
commit on a GPU by tools/record_special_bits_golden.py, never from the code
under test.
"""

from __future__ import annotations

import importlib.util

import numpy as np
import pytest

from tests.helpers import GOLDEN

ROOT = GOLDEN.parents[1]


def _tool():
    # the points are defined once, in the tool that recorded the fixture
    path = ROOT / "tools" / "record_special_bits_golden.py"
    spec = importlib.util.spec_from_file_location("record_special_bits_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "special_bits_parent.npz")


def test_fixture_covers_every_point(golden):
    assert (GOLDEN / "special_bits_parent.npz").stat().st_size < 1_000_000
    for sel in TOOL.GRIDS:
        x, x2 = TOOL.points(ROOT, sel)
        assert 0 < x.size < 4000 and golden[f"bits_{sel}"].shape == x.shape
        assert golden[f"bits_{sel}"].dtype == np.uint64
        assert (x2 is None) == (sel not in (TOOL.LGDIFF, TOOL.LRISE))
    x, _ = TOOL.points(ROOT, TOOL.LG3_L)
    assert (x < 10.0).sum() > 1000 and (x >= 10.0).sum() > 800 and (x == 0.0).any()
    n, s = TOOL.points(ROOT, TOOL.LRISE)
    assert (s <= n + 1.0).sum() > 100 and (s > n + 1.0).sum() > 100 and (n == 0.0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("sel", sorted(TOOL.GRIDS), ids=lambda s: TOOL.NAMES[s])
def test_primitive_returns_the_parent_commits_bits(golden, sel):
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    from metadamage_amd import engine

    x, x2 = TOOL.points(ROOT, sel)
    got = np.asarray(engine.primitive(sel, x, x2), np.float64).view(np.uint64)
    want = golden[f"bits_{sel}"]
    bad = np.flatnonzero(got != want)
    print(f"{TOOL.NAMES[sel]}: {bad.size} of {x.size} points differ from the parent's bits"
          + (f" (x {x[bad][:5].tolist()}, got {got[bad][:5].view(np.float64).tolist()}, "
             f"parent {want[bad][:5].view(np.float64).tolist()})" if bad.size else ""))
    assert bad.size == 0
