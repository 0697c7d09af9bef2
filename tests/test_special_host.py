"""CPU tests of the device primitives of csrc/mdfit_special.h (rcp, flog,
flog_t, flog1p, fexp, fexp_t, lg3, stirling_rem, lgdiff, lrise): the host
build of the unmodified header (tests/special_host_main.cpp through
tests/host_shim) against the mpmath references of tests/golden/
primitives_golden.npz, at the bars derived in DESIGN.md §3.4.1
(tests/special_cases.py).  This is where each bar is shown to be reachable by
correct arithmetic; tests/test_gpu_special.py holds the kernel to the same bars."""

from __future__ import annotations

import ctypes
import importlib.util
import re

import numpy as np
import pytest

from tests import special_cases as sc

ROOT = sc.ROOT


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return sc.build_host(tmp_path_factory.mktemp("special_host"))


@pytest.fixture(scope="module")
def fixture():
    return sc.load_fixture()


def _golden_module():
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_golden_primitives",
                                                  ROOT / "tests" / "golden" / "make_golden_primitives.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# --------------------------------------------------------------------------
# ABI
# --------------------------------------------------------------------------
def test_entry_point_declared_exported_and_argument_checked():
    from metadamage_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mdfit.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+mdfit_primitive\s*\(", text)
    enum = re.search(r"enum mdfit_primitive_id \{(.*?)\}", text, re.S).group(1)
    ids = {name: int(val) for name, val in re.findall(r"MDFIT_P_([A-Z0-9_]+) = (\d+)", enum)}
    assert ids == {"RCP": sc.RCP, "RCP1": sc.RCP1, "FLOG": sc.FLOG, "FLOG_T": sc.FLOG_T,
                   "FLOG_T_ZERO": sc.FLOG_T_ZERO, "FLOG1P": sc.FLOG1P, "FEXP": sc.FEXP, "FEXP_T": sc.FEXP_T,
                   "LG3_L": sc.LG3_L, "LG3_P": sc.LG3_P, "LG3_Q": sc.LG3_Q, "LG3_FAST_L": sc.LG3_FAST_L,
                   "LG3_FAST_P": sc.LG3_FAST_P, "STIRLING_REM": sc.STIRLING_REM, "LGDIFF": sc.LGDIFF,
                   "LRISE": sc.LRISE, "COUNT": 17}
    assert "mdfit_primitive" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    dummy = ctypes.c_void_p(16)
    for which in (0, 17, -1):
        assert lib.mdfit_primitive(which, dummy, dummy, 1, dummy, None) == -1
        assert b"which" in lib.mdfit_last_error()
    assert lib.mdfit_primitive(sc.FLOG, dummy, None, -1, dummy, None) == -1
    assert lib.mdfit_primitive(sc.FLOG, None, None, 1, dummy, None) == -1
    assert lib.mdfit_primitive(sc.FLOG, dummy, None, 1, None, None) == -1
    assert lib.mdfit_primitive(sc.LRISE, dummy, None, 1, dummy, None) == -1  # a binary primitive needs x2
    assert lib.mdfit_primitive(sc.FLOG, dummy, None, (1 << 31) + 1, dummy, None) == -1
    for which in range(1, 17):
        assert lib.mdfit_primitive(which, None, None, 0, None, None) == 0


# --------------------------------------------------------------------------
# the host build against the fixture
# --------------------------------------------------------------------------
@pytest.mark.parametrize("sel", sorted(sc.SELECTORS), ids=lambda s: sc.NAMES[s])
def test_host_build_meets_its_bar_at_every_fixture_point(host_program, fixture, tmp_path, sel):
    """Every point of every grid, specials by value; and the host results the
    fixture stores (the device is compared with them) are this build's."""
    grids, key = sc.grids_of(fixture, sel)
    assert grids
    worst = (0.0, "", -1)
    for name, d in grids:
        got = sc.run_host(host_program, sel, d["x"], d.get("x2"), tmp_path)
        assert sc.same_value(got, d[f"host_{sel}"]).all() and \
            (np.signbit(got) == np.signbit(d[f"host_{sel}"]))[~np.isnan(got)].all(), name
        ratio, i = sc.check(sel, got, d["x"], d.get("x2"), d[f"ref_{key}"], d[f"res_{key}"], d.get("mag"),
                            d.get(f"ressub_{key}"))
        if ratio > worst[0]:
            worst = (ratio, name, i)
    print(f"{sc.NAMES[sel]}: worst error {worst[0]:.3f} of its bar ({worst[1]}[{worst[2]}])")
    assert worst[0] <= 1.0, worst


def test_fexp_t_tail_is_the_subnormal_exponential(host_program, tmp_path):
    """Below -709.78 the result is subnormal: exp(-740) = 4.2e-322 and
    exp(-745.1) = 4.9e-324 (with ki clamped short of the subnormal exponents
    they came out near 5.6e-309), and at most a spacing and a half off."""
    got = sc.run_host(host_program, sc.FEXP_T, [-740.0, -745.1, -745.2, np.nextafter(-745.2, -np.inf)], None,
                      tmp_path)
    assert abs(got[0] - 4.2e-322) <= 1.5 * sc.SUB and abs(got[1] - 4.9e-324) <= 1.5 * sc.SUB
    assert got[2] <= 1.5 * sc.SUB and got[3] == 0.0


def test_flog1p_below_half_a_rounding_is_the_argument(host_program, tmp_path):
    """1 + x == 1 for |x| <= 2^-54 (ties to even) and for 0 < x < 2^-53: the
    result is x itself.  A negative x in (-2^-53, -2^-54) rounds 1 + x to
    1 - 2^-53 and goes through the correction, held to the 3 ulp bar by the
    fixture's flog1p_tiny grid."""
    x = np.concatenate([10.0 ** np.linspace(-300, np.log10(2.0 ** -54), 400), [2.0 ** -54]])
    x = np.concatenate([x, -x, np.linspace(2.0 ** -54, 2.0 ** -53, 50, endpoint=False)])
    got = sc.run_host(host_program, sc.FLOG1P, x, None, tmp_path)
    assert np.array_equal(got, x)


# --------------------------------------------------------------------------
# a denser sweep against mpmath
# --------------------------------------------------------------------------
DENSE_CHEAP, DENSE_GAMMA, DENSE_BINARY = 100_000, 1_500, 1_000


def _dense(mg, family):
    n = DENSE_CHEAP
    if family == "rcp":
        x = mg.logu(101, 1e-300, 1e300, n)
        return np.concatenate([x, -x]), None
    if family == "flog":
        d = mg.logu(103, 1e-16, 0.45, n // 4)
        return np.concatenate([mg.logu(102, 1e-300, 1e300, n // 2), 1.0 + d, 1.0 - d]), None
    if family == "flog_t":
        # and the binades next to (0.5, 2), where the inner sum's rounding and the table's are largest against
        # the result's ulp (the host build reaches 0.999 ulp there over 2e6 points)
        return np.concatenate([mg.logu(105, 2.0, 1e300, n // 3), mg.logu(106, 1e-300, 0.5, n // 3),
                               mg.logu(107, 0.5, 2.0, n // 3), mg.unif(128, 0.25, 0.5, n // 4),
                               mg.unif(129, 2.0, 4.0, n // 4)]), None
    if family == "flog1p":
        x = mg.logu(108, 1e-300, 0.999, n // 3)
        return np.concatenate([x, -x, mg.logu(109, 1.0, 1e10, n // 3)]), None
    if family == "exp":
        return np.concatenate([mg.unif(110, -708.0, 709.0, n // 2), mg.unif(111, -1.0, 1.0, n // 4),
                               mg.unif(112, -745.2, -708.0, n // 4)]), None
    if family == "lg3":
        n = DENSE_GAMMA
        small = mg.logu(114, 1e-6, 10.0, n)
        return np.concatenate([mg.logu(113, 1e-100, 1e-6, n), np.minimum(small, np.nextafter(10.0, 0.0)),
                               mg.unif(115, 0.9, 2.1, n), mg.unif(116, 9.99, 10.01, n),
                               mg.logu(117, 10.0, 1e10, n), mg.logu(118, 1e10, 1e300, n)]), None
    if family == "stirling":
        return mg.logu(119, 10.0, 1e10, DENSE_GAMMA), None
    n = DENSE_BINARY
    if family == "lrise":
        rng = np.random.default_rng(122)
        return (np.concatenate([np.floor(mg.logu(120, 1.0, 4e9, n)), rng.integers(1, 13, n).astype(np.float64)]),
                np.concatenate([mg.logu(121, 1e-6, 1e6, n), mg.logu(123, 1e-6, 20.0, n)]))
    if family == "lgdiff":
        z = mg.logu(126, 1e-3, 4e9, n)
        u = np.random.default_rng(127).uniform(1e-9, 0.999, n)
        return (np.concatenate([mg.logu(124, 1e-3, 4e9, n), z]),
                np.concatenate([mg.logu(125, 1e-6, 4e9, n), -u * np.minimum(z, 1.0)]))
    raise KeyError(family)


@pytest.mark.parametrize("family", ["rcp", "flog", "flog_t", "flog1p", "exp", "lg3", "stirling", "lrise", "lgdiff"])
def test_host_build_meets_its_bars_on_a_dense_sweep(host_program, tmp_path, family):
    mg = _golden_module()
    x, x2 = _dense(mg, family)
    refs, mag = mg.references(family, x, x2)
    for sel, (fams, key) in sc.SELECTORS.items():
        if family not in fams:
            continue
        ref, res = mg._split(refs[key])
        ressub = mg.scaled_residual(refs[key], ref) if family == "exp" else None
        got = sc.run_host(host_program, sel, x, x2, tmp_path)
        ratio, i = sc.check(sel, got, x, x2, ref, res, mag, ressub)
        print(f"{sc.NAMES[sel]}: {x.size} points, worst error {ratio:.3f} of its bar (x = {x[i]!r}"
              + (f", x2 = {x2[i]!r})" if x2 is not None else ")"))
        assert ratio <= 1.0, (sc.NAMES[sel], x[i], None if x2 is None else x2[i], got[i], ref[i])


# --------------------------------------------------------------------------
# the sampler's potential at the edges: the oracle against the mpmath reference
# --------------------------------------------------------------------------
def test_oracle_potential_at_the_edges(oracle_lib, fixture):
    """The reference of test_gpu_nuts.py::test_potential_at_the_edges (mpmath's
    restatement of oracle/mdfit_nuts.c's nuts_potential, in the fixture) is
    the function the oracle computes: the oracle, on double lgamma_r, is within
    HALF the kernel's bar at every item (none exempted; the worst is 0.26 of
    the bar, a gradient component), and gives U = +inf, g = 0 on the
    infeasible one."""
    p = fixture["pot"]
    n = len(p["model"])
    assert 55 <= n <= 80 and np.isinf(p["U"]).sum() == 1
    worst = 0.0
    for k in range(n):
        U, g = oracle_lib.nuts_potential(int(p["model"][k]), int(p["subset"][k]), p["y"][k, :30], p["N"][k, :30],
                                         p["v"][k])
        if np.isinf(p["U"][k]):
            assert U == np.inf and (np.asarray(g) == 0).all()
            continue
        bar_u = sc.POT_C_U * p["U_mag"][k] + sc.POT_ABS
        bar_g = sc.POT_C_G * p["g_mag"][k] + sc.POT_ABS
        r = max(abs(U - p["U"][k]) / bar_u, float((np.abs(g - p["g"][k]) / bar_g).max()))
        worst = max(worst, r)
        assert r <= 0.5, (k, p["v"][k], U, p["U"][k], g, p["g"][k])
    print(f"oracle potential at the edges: worst error {worst:.3f} of the kernel's bar")


def test_fixture_regenerates_from_its_script(fixture, tmp_path):
    mg = _golden_module()
    out = tmp_path / "primitives_golden.npz"
    mg.build(out)
    new = np.load(out)
    old = np.load(sc.FIXTURE)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert np.array_equal(old[k], new[k], equal_nan=True), k
    assert sc.FIXTURE.stat().st_size < 1_000_000
    for k in old.files:
        if k.endswith("/x"):
            assert old[k].size <= 2048, k
