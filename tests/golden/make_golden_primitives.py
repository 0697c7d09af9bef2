#!/usr/bin/env python
"""Regenerates tests/golden/primitives_golden.npz: arguments and references of
the device primitives of csrc/mdfit_special.h (rcp, flog, flog_t, flog1p, fexp,
fexp_t, lg3, stirling_rem, lgdiff, lrise) and of the sampler's potential at the
edges of its domain, from mpmath at 300 bits.  Seeded: a rerun writes the same
arrays.

Per grid `g` (GRIDS below):
  g/x, g/x2           the arguments (x2 for the binary functions)
  g/ref_K, g/res_K    reference K rounded to the nearest double, and the signed
                      residual (reference - ref) rounded to a double, so that an
                      error (got - ref) - res is exact to ~1e-16 of an ulp
  g/ressub_K          exp: where |ref| < 2^-1000, the residual times 2^1074 (a
                      double cannot hold a residual below the subnormal spacing)
  g/mag               lgdiff, lrise: the error-weighted magnitude of the terms
                      summed in the branch taken, in ulps
  g/host_S            the host build's result (tests/special_host_main.cpp) of
                      selector S, for the functions whose device bits must equal it
and for the potential (`pot/...`): the items, v, U, g[4], U_mag, g_mag[4].

Usage: python tests/golden/make_golden_primitives.py [out.npz]
"""

from __future__ import annotations

import sys
import tempfile
from pathlib import Path

import numpy as np
from mpmath import mp, mpf

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import special_cases as sc  # noqa: E402

mp.prec = 300
SEED = 20261020
NPT = 400  # points per random grid (at most 2048; the fixture stays under 1 MB)


def _rng(k):
    return np.random.default_rng([SEED, k])


def logu(k, lo, hi, n=NPT, ends=True):
    x = 10.0 ** _rng(k).uniform(np.log10(lo), np.log10(hi), n)
    x = np.clip(x, lo, hi)
    if ends:
        x[0], x[-1] = lo, hi
    return x


def unif(k, lo, hi, n=NPT):
    x = _rng(k).uniform(lo, hi, n)
    x[0], x[-1] = lo, hi
    return x


def pm1(x):
    """x and its two neighbours."""
    x = np.asarray(x, np.float64)
    return np.concatenate([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


def grids():
    """name -> (family, x, x2 or None)."""
    g = {}
    x = logu(1, 1e-300, 1e300)
    g["rcp"] = ("rcp", np.concatenate([x, -x]), None)
    # log
    g["flog_wide"] = ("flog", logu(2, 1e-300, 1e300), None)
    d = logu(3, 1e-16, 0.45)
    g["flog_near1"] = ("flog", np.concatenate([1.0 + d, 1.0 - d]), None)
    sub = 10.0 ** _rng(4).uniform(-323.3, -307.66, NPT)
    sub = np.minimum(sub, np.nextafter(2.2250738585072014e-308, 0.0))
    sub[0], sub[-1] = 5e-324, np.nextafter(2.2250738585072014e-308, 0.0)
    g["flog_sub"] = ("flog", sub, None)
    g["flog_special"] = ("flog", np.array([0.0, -0.0, np.inf, -1.0, np.nan]), None)
    # table log: both forms on the first four, the kZero form alone on the rest
    g["flogt_big"] = ("flog_t", logu(5, 2.0, 1e300), None)
    g["flogt_small"] = ("flog_t", logu(6, 1e-300, 0.5), None)
    g["flogt_near1"] = ("flog_t", logu(7, 0.5, 2.0), None)
    j = np.arange(256)
    for e in (-1, 0, 3, 33):
        g[f"flogt_edges_e{e}"] = ("flog_t", pm1(np.ldexp(1.0 + j / 256.0, e)), None)
    g["flogt_sub"] = ("flog_t0", sub.copy(), None)
    g["flogt_special"] = ("flog_t0", np.concatenate([[0.0], pm1([2.2250738585072014e-308])]), None)
    # log1p
    x = logu(8, 1e-300, 0.999)
    g["flog1p_small"] = ("flog1p", np.concatenate([x, -x]), None)
    g["flog1p_big"] = ("flog1p", logu(9, 1.0, 1e10), None)
    g["flog1p_tiny"] = ("flog1p", pm1([2.0 ** -54, -(2.0 ** -54), 2.0 ** -53, -(2.0 ** -53)]), None)
    # exp: fexp and fexp_t on the same points
    g["exp_wide"] = ("exp", unif(10, -708.0, 709.0), None)
    g["exp_unit"] = ("exp", unif(11, -1.0, 1.0), None)
    ln2 = 0.6931471805599453
    g["exp_bounds"] = ("exp", pm1((np.arange(-256, 256) + 0.5) * (ln2 / 256.0)), None)
    g["exp_halves"] = ("exp", pm1(np.arange(-2040, 2048, 24) * (ln2 / 2.0)), None)
    g["exp_tail"] = ("exp", np.concatenate([unif(12, -745.2, -708.0, 300),
                                            [-745.2, -745.1332, -745.14, -709.78, -709.79, -740.0, -745.1,
                                             np.nextafter(-745.2, -np.inf), -746.0, -1000.0]]), None)
    g["exp_top"] = ("exp", np.array([709.77, 709.78, 709.7800001]), None)
    g["exp_special"] = ("exp", np.array([np.nan, np.inf, -np.inf, np.nextafter(709.8, np.inf), 720.0]), None)
    # lnGamma / psi / psi1: both forms
    g["lg3_tiny"] = ("lg3", logu(13, 1e-100, 1e-6), None)
    x = logu(14, 1e-6, 10.0)
    x[-1] = np.nextafter(10.0, 0.0)
    g["lg3_small"] = ("lg3", x, None)
    g["lg3_zeros"] = ("lg3", unif(15, 0.9, 2.1), None)
    g["lg3_branch"] = ("lg3", np.concatenate([unif(16, 9.99, 10.01), pm1([10.0])]), None)
    g["lg3_big"] = ("lg3", logu(17, 10.0, 1e10), None)
    g["lg3_huge"] = ("lg3", logu(18, 1e10, 1e300), None)
    g["stirling"] = ("stirling", logu(19, 10.0, 1e10), None)
    # lrise(n, s)
    g["lrise_big"] = ("lrise", np.floor(logu(20, 1.0, 4e9)), logu(21, 1e-6, 1e6))
    g["lrise_small"] = ("lrise", _rng(22).integers(1, 13, NPT).astype(np.float64), logu(23, 1e-6, 20.0))
    g["lrise_zero"] = ("lrise", np.zeros(6), np.array([1e-6, 0.5, 1.0, 3.0, 1e3, 1e6]))
    # lgdiff(z, h)
    g["lgdiff_pos"] = ("lgdiff", logu(24, 1e-3, 4e9), logu(25, 1e-6, 4e9))
    z = logu(26, 1e-3, 4e9)
    u = _rng(27).uniform(0.0, 0.999, NPT)
    u = np.where(u == 0.0, 0.5, u)
    g["lgdiff_neg"] = ("lgdiff", z, -u * np.minimum(z, 1.0))
    for name, (_, x, _) in g.items():
        assert x.size <= 2048, name
    return g


def _split(vals):
    """mpf values -> (nearest double, residual as a double)."""
    ref = np.empty(len(vals))
    res = np.zeros(len(vals))
    for i, v in enumerate(vals):
        if isinstance(v, float):  # a special value
            ref[i] = v
            continue
        f = float(v)
        ref[i] = f
        if np.isfinite(f):
            res[i] = float(v - mpf(f))
    return ref, res


def scaled_residual(vals, ref):
    """Subnormal results: the residual in units of their spacing, where |ref| < sc.TINY (0 elsewhere)."""
    tiny = np.isfinite(ref) & (np.abs(ref) < sc.TINY)
    return np.array([float((v - mpf(float(r))) * mpf(2) ** 1074) if t and not isinstance(v, float) else 0.0
                     for v, r, t in zip(vals, ref, tiny)])


def _special_log(x):
    if np.isnan(x) or x < 0:
        return float("nan")
    if x == 0:
        return float("-inf")
    if np.isinf(x):
        return float("inf")
    return None


def ref_exp(x):
    if np.isnan(x):
        return float("nan")
    if x == np.inf:
        return float("inf")
    if x == -np.inf:
        return 0.0
    v = mp.exp(mpf(float(x)))
    if v > mpf(sys.float_info.max) + mpf(2) ** 970:  # rounds to +inf
        return float("inf")
    return v


HALF_LOG_2PI = mp.log(2 * mp.pi) / 2


def sr(z):
    """Stirling remainder lnGamma(z) - [(z - 1/2) ln z - z + ln(2 pi) / 2]."""
    z = mpf(z)
    return mp.loggamma(z) - ((z - mpf(0.5)) * mp.log(z) - z + HALF_LOG_2PI)


def lgam_units(z):
    """The accurate lnGamma's bar at z in ulps (2^-52) (sc.bar_lg3_l)."""
    return float(sc.bar_lg3_l(float(z), float(mp.loggamma(mpf(z))), fast=False) / sc.ULP1)


def lgdiff_ref_mag(z, h, h_err=0.0):
    """lnGamma(z + h) - lnGamma(z) and the magnitude of lgdiff's error in ulps
    on the branch the code takes (the branch test is the code's: on the double
    z + h).  h_err: the absolute rounding error the caller made in h."""
    zz, hh = mpf(float(z)), mpf(float(h))
    ref = mp.loggamma(zz + hh) - mp.loggamma(zz)
    z1 = float(z) + float(h)
    if z >= 10.0 and z1 >= 10.0:
        t1 = (zz - mpf(0.5) + hh) * mp.log1p(hh / zz)
        t2a, t2b = abs(hh) * mp.log(zz), abs(hh) * abs(mp.log(zz) - 1)
        mag = (sc.LGDIFF_T1_ULPS * abs(t1) + t2a + t2b + sc.LGDIFF_SR_ULPS * (abs(sr(z1)) + abs(sr(zz)))
               + abs(ref))
    else:
        mag = (lgam_units(z1) + lgam_units(z) + mpf(0.5) * abs(mpf(z1) * mp.psi(0, mpf(z1))) + mpf(0.5) * abs(ref))
    mag += mpf(h_err) / mpf(sc.ULP1) * abs(mp.psi(0, zz + hh))
    return ref, float(mag)


def lrise_ref_mag(n, s):
    if n == 0.0:
        return mpf(0), 0.0
    nn, ss = mpf(float(n)), mpf(float(s))
    ref = mp.loggamma(nn + ss) - mp.loggamma(nn + 1) - mp.loggamma(ss)
    if s <= n + 1.0:
        h = s - 1.0  # rounded when s < 1/2
        _, mag = lgdiff_ref_mag(n + 1.0, h, h_err=abs(float(mpf(h) - (ss - 1))))
        mag += lgam_units(s)
    else:
        _, mag = lgdiff_ref_mag(s, n)
        mag += lgam_units(n + 1.0)
    return ref, mag + 0.5 * abs(float(ref))


def references(family, x, x2):
    """{key: list of mpf or special floats} and the optional mag array."""
    out, mag = {}, None
    if family == "rcp":
        out["f"] = [1 / mpf(float(v)) for v in x]
    elif family in ("flog", "flog_t", "flog_t0"):
        out["f"] = [_special_log(v) if _special_log(v) is not None else mp.log(mpf(float(v))) for v in x]
    elif family == "flog1p":
        out["f"] = [mp.log1p(mpf(float(v))) for v in x]
    elif family == "exp":
        out["f"] = [ref_exp(v) for v in x]
    elif family == "lg3":
        out["l"] = [mp.loggamma(mpf(float(v))) for v in x]
        out["p"] = [mp.psi(0, mpf(float(v))) for v in x]
        out["q"] = [mp.psi(1, mpf(float(v))) for v in x]
    elif family == "stirling":
        out["f"] = [sr(float(v)) for v in x]
    elif family == "lgdiff":
        both = [lgdiff_ref_mag(a, b) for a, b in zip(x, x2)]
        out["f"], mag = [b[0] for b in both], np.array([b[1] for b in both])
    elif family == "lrise":
        both = [lrise_ref_mag(a, b) for a, b in zip(x, x2)]
        out["f"], mag = [b[0] for b in both], np.array([b[1] for b in both])
    else:
        raise KeyError(family)
    return out, mag


# --------------------------------------------------------------------------
# the sampler's potential at the edges of its domain
# --------------------------------------------------------------------------
def potential_items():
    """(model, subset, y[n][32], N[n][32], v[n][4]): five count rows crossed with
    v at the corners of both models, and one infeasible item (the last)."""
    rows_y = np.zeros((5, 32), np.uint32)
    rows_N = np.zeros((5, 32), np.uint32)
    rows_N[0, :30] = 4_000_000_000                    # near the uint32 ceiling, y = N / 100
    rows_y[0, :30] = 40_000_000
    base = (1000 + 37 * np.arange(30)).astype(np.uint32)
    rows_N[1, :30] = base                             # ragged: no coverage at positions 5..11
    rows_y[1, :30] = base // 7
    rows_N[1, 5:12] = 0
    rows_y[1, 5:12] = 0
    rows_N[2, :30] = base                             # y == N
    rows_y[2, :30] = base
    rows_N[3, :30] = base                             # y == 0
    rows_N[4, :30] = 1                                # minimal coverage
    rows_y[4, :30] = np.arange(30) % 2
    corners = (-12.0, 0.0, 6.0)
    deltas = (-20.0, 0.0, 7.0, 12.0)
    feasible = [(a, c) for a in corners for c in corners
                if 1.0 / (1.0 + np.exp(-a)) + 1.0 / (1.0 + np.exp(-c)) < 1.0]
    assert feasible == [(-12.0, -12.0), (-12.0, 0.0), (-12.0, 6.0), (0.0, -12.0), (6.0, -12.0)]
    items = []
    pmd = [(q, a, c, d) for q in corners for (a, c) in feasible for d in deltas]
    null = [(q, 0.0, 0.0, d) for q in corners for d in deltas]
    for i, v in enumerate(pmd):
        items.append((0, i % 3, i % 5, v))
    for i, v in enumerate(null):
        items.append((1, (i + 1) % 3, i % 5, v))
    items.append((0, 0, 1, (0.0, 3.0, 3.0, 5.0)))     # A + c >= 1: U = +inf, g = 0
    model = np.array([m for m, _, _, _ in items], np.int32)
    subset = np.array([s for _, s, _, _ in items], np.int32)
    row = [r for _, _, r, _ in items]
    return model, subset, rows_y[row], rows_N[row], np.array([v for _, _, _, v in items], np.float64)


def _lg_mag(x):
    """Magnitude of the terms lg3 sums for lnGamma(x): below 10 lnGamma(x + 10) and ln P(x)."""
    if x >= 10:
        return abs(mp.loggamma(x))
    P = mpf(1)
    for j in range(10):
        P *= x + j
    return abs(mp.loggamma(x + 10)) + abs(mp.log(P))


def potential_reference(model, subset, y, N, v):
    """oracle/mdfit_nuts.c's nuts_potential in mpmath: U, g[4] and the magnitudes
    U_mag, g_mag[4] (sums of the absolute values of the summed terms times
    their coefficients; a psi term counts as max(1, |psi|), its bar's form)."""
    v = [mpf(float(t)) for t in v]
    pmd = model == 0
    sig = lambda t: 1 / (1 + mp.exp(-t))  # noqa: E731
    lsig = lambda t: -mp.log(1 + mp.exp(-t))  # noqa: E731
    q, lq, l1q = sig(v[0]), lsig(v[0]), lsig(-v[0])
    delta = mp.exp(v[3])
    phi = delta + 2
    A = c = mpf(0)
    lp = 2 * lq + 3 * l1q + v[3] - delta / 1000
    lp_mag = 2 * abs(lq) + 3 * abs(l1q) + abs(v[3]) + delta / 1000
    gq, gA, gc, gd = 2 - 5 * q, mpf(0), mpf(0), 1 - delta / 1000
    if pmd:
        A, c = sig(v[1]), sig(v[2])
        lA, l1A, lc, l1c = lsig(v[1]), lsig(-v[1]), lsig(v[2]), lsig(-v[2])
        lp += 2 * lA + 3 * l1A + lc + 9 * l1c
        lp_mag += 2 * abs(lA) + 3 * abs(l1A) + abs(lc) + 9 * abs(l1c)
        gA, gc = 2 - 5 * A, 1 - 10 * c
        if float(A) + float(c) >= 1.0:
            return float("inf"), [0.0] * 4, 0.0, [0.0] * 4
    lo, hi = (15 if subset == 2 else 0), (15 if subset == 1 else 30)
    pm = lambda t: max(mpf(1), abs(t))  # noqa: E731
    ell = ell_mag = mpf(0)
    s = [mpf(0)] * 4   # sDq, sDA, sDc, sF
    sm = [mpf(0)] * 4
    psi_phi, lg_phi = mp.psi(0, phi), mp.loggamma(phi)
    for i in range(lo, hi):
        k = i if i < 15 else i - 15
        if pmd:
            w = (1 - q) ** k
            D, dq, dA = A * w + c, (-A * k * (1 - q) ** (k - 1) if k > 0 else mpf(0)), w
        else:
            D, dq, dA = q, mpf(1), mpf(0)
        yy, nn = mpf(int(y[i])), mpf(int(N[i]))
        a, b = D * phi, (1 - D) * phi
        args = (yy + a, a, nn - yy + b, b, nn + phi, phi)
        ell += (mp.loggamma(args[0]) - mp.loggamma(a) + mp.loggamma(args[2]) - mp.loggamma(b)
                - mp.loggamma(args[4]) + lg_phi)
        ell_mag += sum(_lg_mag(t) for t in args)
        ps = [mp.psi(0, t) for t in args[:5]] + [psi_phi]
        Pa, Pb = ps[0] - ps[1], ps[2] - ps[3]
        lD = phi * (Pa - Pb)
        lD_mag = phi * (pm(ps[0]) + pm(ps[1]) + pm(ps[2]) + pm(ps[3]))
        for j, f in enumerate((dq, dA, mpf(1))):
            s[j] += lD * f
            sm[j] += lD_mag * abs(f)
        s[3] += D * Pa + (1 - D) * Pb + psi_phi - ps[4]
        sm[3] += D * (pm(ps[0]) + pm(ps[1])) + (1 - D) * (pm(ps[2]) + pm(ps[3])) + pm(ps[5]) + pm(ps[4])
    U = -(ell + lp)
    J = (q * (1 - q), A * (1 - A), c * (1 - c), delta)
    pr = (gq, gA, gc, gd)
    pr_mag = (2 + 5 * q, 2 + 5 * A, 1 + 10 * c, 1 + delta / 1000)
    g = [-(s[j] * J[j] + pr[j]) for j in range(4)]
    g_mag = [sm[j] * J[j] + pr_mag[j] for j in range(4)]
    if not pmd:
        g[1] = g[2] = g_mag[1] = g_mag[2] = mpf(0)
    return float(U), [float(t) for t in g], float(ell_mag + lp_mag), [float(t) for t in g_mag]


def potential_fixture():
    model, subset, y, N, v = potential_items()
    refs = [potential_reference(int(m), int(s), yy, nn, vv) for m, s, yy, nn, vv in zip(model, subset, y, N, v)]
    return {"pot/model": model, "pot/subset": subset, "pot/y": y, "pot/N": N, "pot/v": v,
            "pot/U": np.array([r[0] for r in refs]), "pot/g": np.array([r[1] for r in refs]),
            "pot/U_mag": np.array([r[2] for r in refs]), "pot/g_mag": np.array([r[3] for r in refs])}


def build(out_path: Path) -> dict:
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = sc.build_host(Path(tmp))
        for name, (family, x, x2) in grids().items():
            res[f"{name}/x"] = x
            if x2 is not None:
                res[f"{name}/x2"] = x2
            refs, mag = references(family, x, x2)
            for key, vals in refs.items():
                res[f"{name}/ref_{key}"], res[f"{name}/res_{key}"] = _split(vals)
                if family == "exp":
                    res[f"{name}/ressub_{key}"] = scaled_residual(vals, res[f"{name}/ref_{key}"])
            if mag is not None:
                res[f"{name}/mag"] = mag
            for sel in sc.HOST_BITS.get(family, ()):
                res[f"{name}/host_{sel}"] = sc.run_host(exe, sel, x, x2, Path(tmp))
    res.update(potential_fixture())
    np.savez_compressed(out_path, **res)
    return res


if __name__ == "__main__":
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(__file__).with_name("primitives_golden.npz")
    r = build(out)
    print(f"wrote {out}: {len(r)} arrays, {sum(v.nbytes for v in r.values())} bytes raw, {out.stat().st_size} on disk")
