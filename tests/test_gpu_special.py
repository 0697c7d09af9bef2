"""GPU tests of the device primitives of csrc/mdfit_special.h, one launch of
mdfit_primitive per selector over every point of tests/golden/
primitives_golden.npz (mpmath references; the test itself needs numpy alone):
the kernel meets the bars derived in DESIGN.md §3.4.1 (tests/special_cases.py),
which tests/test_special_host.py shows the host build of the same header to
meet; the functions without a reciprocal and with contraction off (flog_t,
fexp_t) return the host build's bits."""

from __future__ import annotations

import numpy as np
import pytest

from tests import special_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    from metadamage_amd import engine as eng

    return eng


@pytest.fixture(scope="module")
def fixture():
    return sc.load_fixture()


@pytest.mark.parametrize("sel", sorted(sc.SELECTORS), ids=lambda s: sc.NAMES[s])
def test_primitive_meets_its_bar_at_every_fixture_point(engine, fixture, sel):
    grids, key = sc.grids_of(fixture, sel)
    binary = sel in (sc.LGDIFF, sc.LRISE)
    x = np.concatenate([d["x"] for _, d in grids])
    x2 = np.concatenate([d["x2"] for _, d in grids]) if binary else None
    got_all = engine.primitive(sel, x, x2)
    assert got_all.shape == x.shape
    worst, lo = (0.0, "", -1), 0
    differ, far = 0, 0
    for name, d in grids:
        got = got_all[lo:lo + d["x"].size]
        lo += d["x"].size
        ratio, i = sc.check(sel, got, d["x"], d.get("x2"), d[f"ref_{key}"], d[f"res_{key}"], d.get("mag"),
                            d.get(f"ressub_{key}"))
        if ratio > worst[0]:
            worst = (ratio, name, i)
        host = d[f"host_{sel}"]
        nan = np.isnan(host)
        assert np.array_equal(np.isnan(got), nan), name
        same = got.view(np.int64) == host.view(np.int64)
        if sel in sc.BIT_IDENTICAL:
            assert same[~nan].all(), (sc.NAMES[sel], name, d["x"][~nan & ~same][:5], got[~nan & ~same][:5],
                                      host[~nan & ~same][:5])
        fin = ~nan & ~same & np.isfinite(got) & np.isfinite(host)
        differ += int((~nan & ~same).sum())
        if fin.any():
            far = max(far, int(sc.ulp_distance(got[fin], host[fin]).max()))
    print(f"{sc.NAMES[sel]}: {x.size} points, worst error {worst[0]:.3f} of its bar ({worst[1]}[{worst[2]}]); "
          f"{differ} points differ from the host build, by at most {far} ulp")
    assert worst[0] <= 1.0, worst


def test_unary_primitive_ignores_a_missing_x2_and_empty_input(engine):
    assert engine.primitive(sc.FLOG, np.array([])).size == 0
    x = np.array([1.0, np.e, 10.0])
    np.testing.assert_array_equal(engine.primitive(sc.FLOG, x), engine.primitive(sc.FLOG, x, np.zeros(3)))
    # more than one block, no multiple of its size
    x = np.linspace(0.5, 3.0, 1000)
    # fexp_t's 1.5 ulp and one ulp for numpy's exp: 2.5 * 2^-52
    np.testing.assert_allclose(engine.primitive(sc.FEXP_T, x), np.exp(x), rtol=5.6e-16)
