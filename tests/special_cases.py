"""Shared by the pointwise tests of csrc/mdfit_special.h (test_special_host.py,
test_gpu_special.py) and the fixture's script (golden/make_golden_primitives.py):
the selectors, which grids of the fixture each one runs on, the derived error
bars (DESIGN.md §3.4.1 -- none is measured from the code under test), the host
build, and the error measure.  Needs numpy alone."""

from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
FIXTURE = ROOT / "tests" / "golden" / "primitives_golden.npz"

# enum mdfit_primitive_id (include/mdfit.h)
RCP, RCP1, FLOG, FLOG_T, FLOG_T_ZERO, FLOG1P, FEXP, FEXP_T = 1, 2, 3, 4, 5, 6, 7, 8
LG3_L, LG3_P, LG3_Q, LG3_FAST_L, LG3_FAST_P, STIRLING_REM, LGDIFF, LRISE = 9, 10, 11, 12, 13, 14, 15, 16
NAMES = {RCP: "rcp", RCP1: "rcp1", FLOG: "flog", FLOG_T: "flog_t<false>", FLOG_T_ZERO: "flog_t<true>",
         FLOG1P: "flog1p", FEXP: "fexp", FEXP_T: "fexp_t", LG3_L: "lg3.l", LG3_P: "lg3.p", LG3_Q: "lg3.q",
         LG3_FAST_L: "lg3<fast>.l", LG3_FAST_P: "lg3<fast>.p", STIRLING_REM: "stirling_rem", LGDIFF: "lgdiff",
         LRISE: "lrise"}

# selector -> (the grid families it runs on, the reference it is held to)
SELECTORS = {RCP: (("rcp",), "f"), RCP1: (("rcp",), "f"), FLOG: (("flog",), "f"), FLOG_T: (("flog_t",), "f"),
             FLOG_T_ZERO: (("flog_t", "flog_t0"), "f"), FLOG1P: (("flog1p",), "f"), FEXP: (("exp",), "f"),
             FEXP_T: (("exp",), "f"), LG3_L: (("lg3",), "l"), LG3_P: (("lg3",), "p"), LG3_Q: (("lg3",), "q"),
             LG3_FAST_L: (("lg3",), "l"), LG3_FAST_P: (("lg3",), "p"), STIRLING_REM: (("stirling",), "f"),
             LGDIFF: (("lgdiff",), "f"), LRISE: (("lrise",), "f")}
# family -> the selectors whose host-build results the fixture stores
HOST_BITS = {}
for _sel, (_fams, _) in SELECTORS.items():
    for _f in _fams:
        HOST_BITS.setdefault(_f, []).append(_sel)
# contract(off), no reciprocal: the device's bits are the host build's
BIT_IDENTICAL = (FLOG_T, FLOG_T_ZERO, FEXP_T)

FAMILY_OF_GRID = {"rcp": "rcp", "flog_": "flog", "flogt_sub": "flog_t0", "flogt_special": "flog_t0",
                  "flogt_": "flog_t", "flog1p_": "flog1p", "exp_": "exp", "lg3_": "lg3", "stirling": "stirling",
                  "lrise_": "lrise", "lgdiff_": "lgdiff"}


def family_of(grid: str) -> str:
    for prefix, fam in FAMILY_OF_GRID.items():
        if grid.startswith(prefix):
            return fam
    raise KeyError(grid)


# --------------------------------------------------------------------------
# the bars
# --------------------------------------------------------------------------
ULP1 = 2.0 ** -52     # one ulp, relative, at the bottom of a binade (the largest an ulp gets)
U = 2.0 ** -53        # one rounding
SUB = 2.0 ** -1074    # the spacing of subnormals

FLOG_T_ABS = 2.3e-16  # flog_t on (0.5, 2): table 5.6e-17 + one rounding at |ln x| < 0.7 (1.1e-16) + the
#                       polynomial's last rounding at |r| < 2^-9 (< 1e-18) + the inner sum's (|.| < 0.7 / 2: 5.6e-17)
LG3_L_ABS, LG3_L_REL = 2.5e-14, 4.5e-16   # lnGamma below 10
LG3_L_BIG = 1e-15                         # lnGamma from 10, relative
# psi below 10: s1 = dP * iP = sum 1 / (x + j) carries 17 (dP: 9 fma roundings and the 8 of the P it adds) + 9
# (P) + 1 (the rounded x + j) + 2 (rcp, one ulp) + 1 (the product) = 30 roundings, taken as 32 U; psi(x + 10)
# itself: the log's ulp at < 4 (4.4e-16), the rounded x + 10 (psi1 <= 0.105 times 1.8e-15 = 1.9e-16) and three
# roundings at <= 3 (1e-15): 1.7e-15.  |err| <= 32 U s1 + 1.7e-15; over x in (0, 10) the largest of that over
# max(1, |psi(x)|) is 1.36e-14, at x = 0.785 (|psi| = 1).  The fast form's rcp1 (10 ulp = 20 U in place of
# rcp's 2 U) makes it 50 U s1 + 1.7e-15 + 1.1e-16 (its r / 2 <= 0.05 at 20 U): 2.04e-14 at the same x.
LG3_P_C, LG3_P_FAST_C = 1.4e-14, 2.1e-14
# psi1 below 10: s1^2 carries 2 * 30 = 60 U; d2P * iP 9 + 17 (d2P: its own fma roundings and dP's) + 9 (P) + 2
# (rcp) + 1 (the rounded x + j) = 38 U; the fma and the sum 2 U of the result: |err| <= 60 U s1^2 + 38 U
# (s1^2 - s2) + 2 U s2 + 4e-17 (psi1(x + 10) <= 0.105 at 3 U), s2 = sum 1 / (x + j)^2.  Over x in (0, 10) the
# largest of that over max(1, psi1(x)) is 6.05e-14, at x = 1.426 (psi1 = 1); towards 0 it falls to 60 U = 6.9e-15.
LG3_Q_C = 6.1e-14
LG3_PQ_BIG = 2.5 * ULP1    # psi, psi1 from 10: the log's ulp (times ln x / psi <= 1.03) or rcp's, two fma
#                            roundings, psi's truncation (B16 / (16 x^16): < 0.1 ulp at 10): 2.2 ulp
# the series stop at B14; the first term left out bounds the truncation of an alternating asymptotic series.
# For psi1 it is B16 / x^17 (3 ulp of psi1(10) = 0.105, gone by x = 13); for the Stirling remainder
# B16 / (16 * 15 x^15) (2.96e-17 at 10, where the remainder is 8.3e-3: 16 of ITS ulps, 0.002 ulp of lnGamma)
B16 = 3617.0 / 510.0
LG3_P_FAST_BIG = 2.75 * ULP1  # + rcp1's 20 U on r / 2 <= 0.05, against psi >= 2.25: 0.44 U
LG3_FAST_L_EXTRA = 2.3e-16 + 2e-17  # the table log's absolute bar where P is in (0.5, 2); rcp1 on r sl <= 1 / 120
STIRLING_C = 4 * ULP1
# lgdiff's Stirling branch, in ulps of each term (the golden script's `mag`): t = log1p(h rcp(z)) carries
# 1.5 (the argument; log1p's condition is <= 1 there) + 3 (flog1p) and the factor z - 1/2 + h two roundings
# (1) and the fma (1/2): 6 on (z - 1/2 + h) t; h (ln z - 1): the log's ulp on |h| ln z and two roundings on
# |h| |ln z - 1|; each remainder 4 (stirling_rem) + 1/2 (the rounded z + h) + 1/2 (their difference): 5; the
# two sums 1/2 each of the result.  Below 10: the two lnGamma bars, the rounded z + h through psi, the difference.
LGDIFF_T1_ULPS, LGDIFF_SR_ULPS = 6.0, 5.0
BINARY_ABS = 1e-15


# the sampler's potential at the edges (test_potential_at_the_edges): |dU| <= POT_C_U U_mag + POT_ABS and
# |dg_j| <= POT_C_G g_mag_j + POT_ABS, the magnitudes from the fixture.  c_U: the fast lnGamma's bar as a
# relative figure (1e-15 of the value from 10; below 10 (2.53e-14 + 4.5e-16 |f|) against the up to 58 of the
# terms it sums, counted in U_mag: 8.9e-16) plus 180 summation roundings (30 points of six terms) of 2^-53;
# c_g: the fast psi's 2.1e-14 max(1, |psi|) the same way
POT_C_U = 1e-15 + 180 * U
POT_C_G = 2.1e-14 + 180 * U
POT_ABS = 1e-12


def ulp_of(f):
    """The ulp of |f| at normal spacing (continued below the normal range); 0 at 0."""
    f = np.abs(np.asarray(f, np.float64))
    with np.errstate(all="ignore"):
        _, e = np.frexp(np.where(np.isfinite(f), f, 1.0))
        return np.where(f == 0.0, 0.0, np.ldexp(1.0, e - 53))


def bar_lg3_l(x, f, fast):
    x, f = np.asarray(x, np.float64), np.abs(np.asarray(f, np.float64))
    return np.where(x < 10.0, LG3_L_ABS + (LG3_FAST_L_EXTRA if fast else 0.0) + LG3_L_REL * f,
                    LG3_L_BIG * f + (2e-17 if fast else 0.0))


def bar_lg3_p(x, f, fast):
    x, f = np.asarray(x, np.float64), np.abs(np.asarray(f, np.float64))
    return np.where(x < 10.0, (LG3_P_FAST_C if fast else LG3_P_C) * np.maximum(1.0, f),
                    (LG3_P_FAST_BIG if fast else LG3_PQ_BIG) * f)


def bar_lg3_q(x, f):
    x, f = np.asarray(x, np.float64), np.abs(np.asarray(f, np.float64))
    with np.errstate(all="ignore"):
        return np.where(x < 10.0, LG3_Q_C * np.maximum(1.0, f), LG3_PQ_BIG * f + B16 * np.maximum(x, 10.0) ** -17.0)


def expected(sel, x, x2, ref, mag=None):
    """(bar, exact, want): the absolute error allowed at each point; where
    `exact`, the function must return `want` itself (specials, saturation),
    compared by value and NaN pattern."""
    x = np.asarray(x, np.float64)
    ref = np.asarray(ref, np.float64).copy()
    exact = ~np.isfinite(ref)
    if sel == RCP:
        bar = 1.0 * ulp_of(ref)
    elif sel == RCP1:
        bar = 10.0 * ulp_of(ref)
    elif sel == FLOG:
        bar = 1.0 * ulp_of(ref)
    elif sel in (FLOG_T, FLOG_T_ZERO):
        bar = np.where((x >= 2.0) | (x <= 0.5), 1.0 * ulp_of(ref), FLOG_T_ABS)
    elif sel == FLOG1P:
        bar = 3.0 * ulp_of(ref)
        exact |= np.abs(x) < 2.0 ** -54  # 1 + x == 1: the argument itself
        ref = np.where(np.abs(x) < 2.0 ** -54, x, ref)
    elif sel == FEXP:
        bar = np.maximum(2.5 * ulp_of(ref), 1.5 * SUB)
        exact |= x < -745.2
        ref[x < -745.2] = 0.0
    elif sel == FEXP_T:
        bar = np.maximum(1.5 * ulp_of(ref), 1.5 * SUB)
        exact |= (x < -745.2) | (x > 709.78)
        ref[x < -745.2] = 0.0
        ref[x > 709.78] = np.inf
    elif sel in (LG3_L, LG3_FAST_L):
        bar = bar_lg3_l(x, ref, sel == LG3_FAST_L)
    elif sel in (LG3_P, LG3_FAST_P):
        bar = bar_lg3_p(x, ref, sel == LG3_FAST_P)
    elif sel == LG3_Q:
        bar = bar_lg3_q(x, ref)
    elif sel == STIRLING_REM:
        bar = STIRLING_C * np.abs(ref) + B16 / 240.0 * x ** -15.0
    elif sel in (LGDIFF, LRISE):
        bar = ULP1 * np.asarray(mag, np.float64) + BINARY_ABS
        if sel == LRISE:
            exact |= x == 0.0
    else:
        raise KeyError(sel)
    return np.where(exact, 0.0, bar), exact, ref


def errors(got, ref, res):
    """|got - (ref + res)|, exact to a rounding of the residual."""
    with np.errstate(all="ignore"):
        return np.abs((np.asarray(got, np.float64) - ref) - res)


def same_value(a, b):
    """Equal by value and NaN pattern (+0 == -0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def ulp_distance(a, b):
    """Distance in representable doubles between finite a and b of one sign."""
    ia = np.asarray(a, np.float64).view(np.int64)
    ib = np.asarray(b, np.float64).view(np.int64)
    return np.abs(ia - ib)


TINY = 2.0 ** -1000  # below it the fixture's residual is the scaled one (res * 2^1074)


def check(sel, got, x, x2, ref, res, mag=None, res_sub=None):
    """Worst error over bar of selector `sel` at the points (asserting the
    exact ones), and the index of the worst point.  res_sub: the residual in
    units of the subnormal spacing, used where |ref| < TINY (a double cannot
    hold a residual below that spacing)."""
    bar, exact, want = expected(sel, x, x2, ref, mag)
    got = np.asarray(got, np.float64)
    bad = exact & ~same_value(got, want)
    assert not bad.any(), (NAMES[sel], "exact", np.asarray(x)[bad][:5], got[bad][:5], want[bad][:5])
    use = ~exact
    if not use.any():
        return 0.0, -1
    err = np.where(use, errors(got, want, res), 0.0)
    assert np.isfinite(got[use]).all(), (NAMES[sel], np.asarray(x)[use][~np.isfinite(got[use])][:5])
    with np.errstate(all="ignore"):
        if res_sub is not None:
            tiny = use & (np.abs(want) < TINY)
            err = np.where(tiny, np.abs(np.ldexp(got - want, 1074) - res_sub), err)
            bar = np.where(tiny, np.ldexp(bar, 1074), bar)
        ratio = np.where(use, np.where(err == 0.0, 0.0, err / bar), 0.0)
    i = int(np.argmax(ratio))
    return float(ratio[i]), i


# --------------------------------------------------------------------------
# the host build
# --------------------------------------------------------------------------
def build_host(outdir: Path, header_dir: Path | None = None, sanitize: bool = False) -> Path:
    """tests/special_host_main.cpp on the unmodified csrc/mdfit_special.h through
    the include-path stand-in tests/host_shim."""
    exe = Path(outdir) / "special_host"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", f"-I{ROOT / 'tests' / 'host_shim'}"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run([*cmd, str(ROOT / "tests" / "special_host_main.cpp"), "-o", str(exe)], check=True)
    return exe


def _tok(v):
    return float(v).hex() if np.isfinite(v) else ("nan" if np.isnan(v) else ("inf" if v > 0 else "-inf"))


def run_host(exe: Path, sel: int, x, x2, tmp: Path) -> np.ndarray:
    x = np.asarray(x, np.float64).ravel()
    x2 = np.zeros_like(x) if x2 is None else np.asarray(x2, np.float64).ravel()
    src = Path(tmp) / f"primitive_{sel}.txt"
    src.write_text(f"{sel} {x.size}\n" + "".join(f"{_tok(a)} {_tok(b)}\n" for a, b in zip(x, x2)))
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = np.array([float.fromhex(t) for t in r.stdout.split()], np.float64)
    assert got.size == x.size
    return got


def load_fixture():
    g = np.load(FIXTURE)
    grids = {}
    for key in g.files:
        name, _, field = key.partition("/")
        grids.setdefault(name, {})[field] = g[key]
    return grids


def grids_of(fixture, sel):
    fams, key = SELECTORS[sel]
    return [(name, d) for name, d in fixture.items() if name != "pot" and family_of(name) in fams], key
