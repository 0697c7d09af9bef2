#!/usr/bin/env python
"""Regenerates tests/golden/nuts_post_waic.npz: waic_i of the crafted cases of
tests/nuts_post_cases.py at S <= 130, from mpmath at 60 digits by the two-pass
formula of fits.py:126-172 (logsumexp - log S, population variance), with
loggamma on the float64 arguments a = D phi, b = (1 - D) phi, y + a, N - y + b,
N + phi, a + b exactly as the specification forms them (D in float64 too).

Per case `<group>/<S>`:
  .../hash   sha256 of the case's arrays (tests/nuts_post_cases.case_hash): the
             test refuses a fixture made from other inputs
  .../waic   float64 [T][6][30]: the reference rounded to the nearest double; NaN
             at the columns a sub-fit has not and where the float64 value class
             is not finite (an argument of lnGamma 0, a NaN draw)
  .../mag    float64 [T][6][30][5], what the error bar needs:
             max over the draws of e_lp = sum over the nine lnGamma terms f of
             2.5e-14 + 4.5e-16 |f|; sd(lp); |lppd|; var(lp); mean |lp|

Usage: python tests/golden/make_golden_nuts_post.py [out.npz]
"""

from __future__ import annotations

import functools
import sys
from pathlib import Path

import numpy as np
from mpmath import mp, mpf

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import nuts_post_cases as cases  # noqa: E402
from tests import nuts_post_ref as ref  # noqa: E402

mp.dps = 60


@functools.lru_cache(maxsize=1 << 20)
def lg(x: float):
    return mp.loggamma(mpf(x))


def eps_f(f) -> float:
    return 2.5e-14 + 4.5e-16 * abs(float(f))


def point(y, N, D, phi):
    """(waic_i, e_lp max, sd, |lppd|, var, mean |lp|) of one column's series."""
    y, N = float(y), float(N)
    lc = [lg(N + 1.0), lg(y + 1.0), lg(N - y + 1.0)]
    lps, e_max = [], 0.0
    for Ds, ps in zip(D, phi):
        Ds, ps = float(Ds), float(ps)
        a, b = Ds * ps, (1.0 - Ds) * ps
        t = [lg(y + a), lg(a), lg(N - y + b), lg(b), lg(N + ps), lg(a + b)]
        lps.append(lc[0] - lc[1] - lc[2] + t[0] - t[1] + t[2] - t[3] - t[4] + t[5])
        e_max = max(e_max, sum(eps_f(f) for f in lc + t))
    S = len(lps)
    mx = max(lps)
    lppd = mx + mp.log(sum(mp.exp(v - mx) for v in lps)) - mp.log(S)
    mean = sum(lps) / S
    var = sum((v - mean) ** 2 for v in lps) / S
    waic = -2 * (lppd - var)
    return float(waic), e_max, float(mp.sqrt(var)), abs(float(lppd)), float(var), float(sum(abs(v) for v in lps) / S)


def build():
    out = {}
    for group in cases.GROUPS:
        for S in cases.S_MPMATH:
            x, status, y, N, names = cases.case(group, S)
            T = x.shape[0]
            cls = ref.waic_class(x, y, N)
            waic = np.full((T, 6, ref.NPOS), np.nan)
            mag = np.full((T, 6, ref.NPOS, 5), np.nan)
            for t in range(T):
                if (y[t, :ref.NPOS] > N[t, :ref.NPOS]).any():
                    continue
                for k in range(6):
                    for col in ref.points_of(k):
                        if not np.isfinite(cls[t, k, col]):
                            continue
                        D = ref.d_of(x[t, k], k in ref.PMD_SUBFITS, col)
                        r = point(y[t, col], N[t, col], D, x[t, k, :, 3])
                        waic[t, k, col], mag[t, k, col] = r[0], r[1:]
                lg.cache_clear()
            out[f"{group}/{S}/hash"] = np.array(cases.case_hash(group, S))
            out[f"{group}/{S}/waic"] = waic
            out[f"{group}/{S}/mag"] = mag
            print(group, S, "done", flush=True)
    return out


if __name__ == "__main__":
    dst = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(__file__).with_name("nuts_post_waic.npz")
    np.savez_compressed(dst, **build())
    print("wrote", dst, dst.stat().st_size, "bytes")
