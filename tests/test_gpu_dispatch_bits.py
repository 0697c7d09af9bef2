"""The whole dispatch -- every post-fit block with every tail that rides it,
through the host route (fits.fit_packed on one GPU: fit_batch_host, or
fit_auto_chunks for auto) and the device-destination route (the gather records,
the dispatch into them, their staging and unpacking) -- returns, on the GPU, the
bits of the commit before the tails became entries of blocks.TAILS: every
returned array in full, NaN payloads included, and the same number and order of
arrays, on 13 taxa of generate(13, seed=21) and one crafted taxon with y > N, in
three uneven chunks (MDFIT_CHUNK_TAXA = 5), at seed 0, index_base 7, 65
importance draws, 100 predictive draws, two rounds where rounds are on and the
threshold 0.02.

The fixture tests/golden/dispatch_parent.npz was recorded from the parent
commit on a GPU by tools/record_dispatch_golden.py, never from the code under
test; the inputs, the configurations and the calls are that tool's.
"""

from __future__ import annotations

import importlib.util

import numpy as np
import pytest

from tests.helpers import GOLDEN

ROOT = GOLDEN.parents[1]
PARENT = "c89a910"


def _tool():
    # the inputs and the calls are defined once, in the tool that recorded the fixture
    path = ROOT / "tools" / "record_dispatch_golden.py"
    spec = importlib.util.spec_from_file_location("record_dispatch_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()
CASES = [(name, route) for name in TOOL.CONFIGS for route in TOOL.ROUTES]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN / "dispatch_parent.npz")


def test_fixture_names_the_parent_and_holds_every_run(golden):
    assert (GOLDEN / "dispatch_parent.npz").stat().st_size < 1_000_000
    assert str(golden["commit"]).startswith(PARENT)
    assert len(TOOL.CONFIGS) == 18 and TOOL.CHUNK_TAXA == 5
    T = TOOL.N_SYNTHETIC + 1
    assert T == 14
    for name, route in CASES:
        n = int(golden[f"{name}/{route}/n"])
        block, tails = TOOL.CONFIGS[name]
        assert n == 3 + (block is not None) + len(tails), (name, route)
        status = golden[f"{name}/{route}/2"]
        assert status.shape == (T,) and status[-1] != 0 and (status[:-1] == 0).sum() > T // 2
        for i in range(n):
            a = golden[f"{name}/{route}/{i}"]
            assert a.shape[0] == T and a.dtype.kind == "i", (name, route, i)
    assert {k for k in golden.files if k != "commit"} == {
        f"{name}/{route}/{i}" for name, route in CASES for i in ("n", *range(int(golden[f"{name}/{route}/n"])))}


@pytest.fixture(scope="module")
def computed():
    """Every configuration through both routes on the fixture's taxa, once."""
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    m = TOOL.modules()
    got = TOOL.run(m, *TOOL.inputs(m.synthetic))
    for arrays in got.values():
        for a in arrays:
            a.setflags(write=False)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name, route", CASES)
def test_dispatch_returns_the_parent_commits_bits(golden, computed, name, route):
    got = computed[name, route]
    assert len(got) == int(golden[f"{name}/{route}/n"])  # the same number of arrays, in the same order
    bad = []
    for i, a in enumerate(got):
        have, want = TOOL.bits(a), golden[f"{name}/{route}/{i}"]
        assert have.shape == want.shape and have.dtype == want.dtype, (name, route, i)
        n = int((have != want).sum())
        print(f"{name} / {route} / array {i}: {n} of {have.size} words differ from the parent's bits")
        if n:
            bad.append(i)
    assert not bad, bad
