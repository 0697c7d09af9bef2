"""CPU test of the trimmed forms in csrc/mdfit_special.h, on the host build of
the unmodified header (tests/eval_trim_host_main.cpp through tests/host_shim):
each returns the bits of the form it replaces.

  * lg3<false>(x).l and lg3<true>(x).l are the same bits (what lets the polish
    phase hand lnGamma(a), lnGamma(b), lnGamma(phi) to lrise_lg), and lg3 with
    flog's special-case tail kept (kPos off) returns lg3's l, psi and psi1;
  * flog_pos is flog on [10, 1e300] and on the shift products of x in (0, 10);
  * the one-select form of flog(P) is flog(P) at P = 0 and at subnormal P;
  * lrise_lg(n, s, lgam(s)) is lrise(n, s).

The points are those of tests/test_gpu_special_bits.py (the x values of
primitives_golden.npz, the edges of the shift, the n x s cross), defined in
tools/record_special_bits_golden.py.
"""

from __future__ import annotations

import importlib.util
import subprocess

import numpy as np
import pytest

from tests import special_cases as sc

ROOT = sc.ROOT


def _tool():
    path = ROOT / "tools" / "record_special_bits_golden.py"
    spec = importlib.util.spec_from_file_location("record_special_bits_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("eval_trim_host") / "eval_trim_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", f"-I{ROOT / 'tests' / 'host_shim'}",
                    str(ROOT / "tests" / "eval_trim_host_main.cpp"), "-o", str(exe)], check=True)
    return exe


def run(exe, mode, x, x2, tmp):
    x = np.asarray(x, np.float64).ravel()
    x2 = np.zeros_like(x) if x2 is None else np.asarray(x2, np.float64).ravel()
    src = tmp / f"{mode}.txt"
    src.write_text(f"{x.size}\n" + "".join(f"{float(a).hex()} {float(b).hex()}\n" for a, b in zip(x, x2)))
    r = subprocess.run([str(exe), mode, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = [[int(t, 16) for t in line.split()] for line in r.stdout.splitlines()]
    got = np.array(rows, dtype=np.uint64)
    assert got.shape[0] == x.size
    return got


def same(x, a, b, what):
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, x[bad][:5].tolist(), a[bad][:5].view(np.float64).tolist(),
                           b[bad][:5].view(np.float64).tolist())


def test_lg3_forms_are_the_same_bits(program, tmp_path):
    x, _ = TOOL.points(ROOT, TOOL.LG3_L)
    assert (x == 0.0).any() and (x == 5e-324).any() and (x == 10.0).any()
    g = run(program, "lg3", x, None, tmp_path)
    same(x, g[:, 0], g[:, 1], "lg3<false>.l against lg3<true>.l")
    for j, name in ((1, "l"), (3, "p"), (5, "q")):
        same(x, g[:, j], g[:, j + 1], f"lg3.{name}, flog's tail kept")
    fin = x >= 1e-100  # (below ~1e-303 the shift product's reciprocal overflows: psi = -inf)
    assert np.isfinite(g[fin][:, [1, 3, 5]].view(np.float64)).all()


def test_flog_pos_is_flog_from_10_and_on_the_shift_products(program, tmp_path):
    fx = np.concatenate([TOOL.points(ROOT, TOOL.FLOG)[0], TOOL.points(ROOT, TOOL.LG3_L)[0]])
    rng = np.random.default_rng(7)
    big = np.concatenate([fx[(fx >= 10.0) & (fx <= 1e300)], 10.0 ** rng.uniform(1.0, 300.0, 2000), [10.0, 1e300]])
    g = run(program, "log", big, None, tmp_path)
    same(big, g[:, 0], g[:, 1], "flog_pos against flog on [10, 1e300]")
    small = fx[(fx > 0.0) & (fx < 10.0)]
    assert small.size > 1000 and small.min() == 5e-324
    g = run(program, "prod", small, None, tmp_path)
    P = g[:, 0].view(np.float64)
    assert (P > 0.0).all() and P.max() < 3.4e11 and (P < 2.3e-308).any()  # subnormal products too
    same(small, g[:, 1], g[:, 2], "the one-select form against flog on the shift products")


def test_one_select_form_is_flog_at_zero_and_subnormals(program, tmp_path):
    sub = TOOL.fixture_x(ROOT, "flog_sub")
    P = np.concatenate([[0.0, 5e-324, 2.2250738585072009e-308], sub])
    assert (sub < 2.2250738585072014e-308).all()
    g = run(program, "sel", P, None, tmp_path)
    same(P, g[:, 0], g[:, 1], "the one-select form against flog")
    assert g[0, 1].view(np.float64) == -np.inf


def test_lrise_with_a_known_lgamma_is_lrise(program, tmp_path):
    n, s = TOOL.points(ROOT, TOOL.LRISE)
    cn, cs = TOOL.rise_cross()
    assert cn.size == 42 and np.array_equal(n[-42:], cn) and np.array_equal(s[-42:], cs)
    g = run(program, "lrise", n, s, tmp_path)
    same(n, g[:, 0], g[:, 1], "lrise_lg against lrise")
    assert (g[n == 0.0, 1] == 0).all()
