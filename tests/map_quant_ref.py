"""Reference of MDFIT-QUANT v1: the weighted order statistics
of one series in Python integers, written from the specification and
independent of csrc/mdfit_mapquant.h, and the crafted series the CPU and GPU
tests share (tests/test_map_quant.py on the host program,
tests/test_gpu_map_quant.py on mdfit_weighted_order_stats)."""

from __future__ import annotations

import functools
import math

import numpy as np

NFIELD = 16
FIELDS = ["D_max_median", "D_max_lo", "D_max_hi", "D_max_q05", "D_max_q95", "D_max_p_above", "q_median", "q_lo",
          "q_hi", "A_median", "c_median", "phi_median", "khat", "ess", "n_window", "flags"]
NRES = 8  # median, lo, hi, q05, q95, p_above, n_window, ok
MEDIAN, LO, HI, Q05, Q95, P_ABOVE, N_WINDOW, OK = range(8)
SCALE = 1 << 52
S_VALUES = (25, 26, 64, 65, 100, 256, 1000, 1024)
KINDS = ("equal", "ties", "zero_nan", "point09", "two_points", "d0_on_draw", "all_zero", "pareto0.5", "pareto0.9",
         "nan_with_mass", "bad_weight")
SEED = 47


def fixed_weights(w) -> list[int]:
    """k_s = rint(w_s 2^52) as Python integers (w in [0, 1]: the product is exact, rint rounds half to even)."""
    return [int(np.rint(np.float64(x) * np.float64(SCALE))) if 0.0 < x <= 1.0 else 0 for x in np.asarray(w, np.float64)]


def order_stats(v, w, d0: float) -> np.ndarray:
    """res[8] float64 of the series v[S] with weights w[S]."""
    v = np.asarray(v, np.float64)
    w = np.asarray(w, np.float64)
    S = len(v)
    bad = np.full(NRES, np.nan)
    bad[OK] = 0.0
    if not all(0.0 <= x <= 1.0 for x in w):  # (a NaN fails both comparisons)
        return bad
    k = fixed_weights(w)
    K = sum(k)
    if K == 0 or any(k[s] > 0 and not math.isfinite(v[s]) for s in range(S)):
        return bad
    # ascending by (value, draw index); a draw without mass has the key +inf
    order = sorted(range(S), key=lambda s: (v[s] if k[s] > 0 else math.inf, s))
    sv = [v[s] if k[s] > 0 else math.inf for s in order]
    sk = [k[s] for s in order]
    cum, run = [], 0
    for x in sk:
        run += x
        cum.append(run)

    def first(pred):
        return next(j for j in range(S) if pred(cum[j]))

    res = np.empty(NRES)
    res[MEDIAN] = 0.5 * (np.float64(sv[first(lambda c: 2 * c >= K)]) + np.float64(sv[first(lambda c: 2 * c > K)]))
    res[Q05] = sv[first(lambda c: 100 * c >= 5 * K)]
    res[Q95] = sv[first(lambda c: 100 * c >= 95 * K)]
    best = None
    for i in range(S):
        if sk[i] == 0:
            continue
        before = cum[i - 1] if i > 0 else 0
        j = next((j for j in range(i, S) if 100 * (cum[j] - before) > 68 * K), None)
        if j is None:
            continue
        width = np.float64(sv[j]) - np.float64(sv[i])
        if best is None or width < best[0]:  # ascending i: ties go to the lowest
            best = (width, i, j)
    _, i, j = best
    res[LO], res[HI] = sv[i], sv[j]
    res[N_WINDOW] = sum(1 for x in sk[i:j + 1] if x > 0)
    above = sum(k[s] for s in range(S) if k[s] > 0 and v[s] > d0)
    res[P_ABOVE] = np.float64(above) / np.float64(K)  # (both below 2^63; Python's int -> float rounds to nearest)
    res[OK] = 1.0
    return res


def record_stats(values, w, d0: float) -> np.ndarray:
    """Fields 0..11 and 14 of a sub-fit's record (NaN elsewhere) from its values tap values[S, 5] = D_max, q, A,
    c, phi and weights w[S]."""
    rec = np.full(NFIELD, np.nan)
    D = order_stats(values[:, 0], w, d0)
    q = order_stats(values[:, 1], w, d0)
    rec[0:6] = D[[MEDIAN, LO, HI, Q05, Q95, P_ABOVE]]
    rec[6:9] = q[[MEDIAN, LO, HI]]
    for j in range(3):
        rec[9 + j] = order_stats(values[:, 2 + j], w, d0)[MEDIAN]
    rec[14] = D[N_WINDOW]
    return rec


def series(kind: str, S: int, rng):
    """(v[S], w[S], d0) float64 of one crafted series."""
    from tests import map_psis_cases, map_psis_ref

    v = rng.uniform(0.0, 0.3, S)
    d0 = 0.1
    if kind == "equal":
        w = np.full(S, 1.0 / S)
    elif kind == "ties":  # a coarse grid of values under uneven weights
        v = np.rint(v * 40.0) / 40.0
        w = rng.uniform(0.1, 1.0, S)
        w /= w.sum()
    elif kind == "zero_nan":  # draws without mass holding NaN, infinities and huge values
        w = rng.uniform(0.1, 1.0, S)
        dead = rng.permutation(S)[: S // 3]
        w[dead] = 0.0
        w /= w.sum()
        v[dead] = np.resize(np.array([np.nan, np.inf, -np.inf, 1e300, -1e300]), len(dead))
    elif kind == "point09":  # one draw holds the median and the whole window
        w = np.full(S, 0.1 / (S - 1))
        w[rng.integers(S)] = 0.9
    elif kind == "two_points":  # two masses of 0.45 far apart, the rest spread thin
        w = np.full(S, 0.1 / (S - 2))
        a, b = rng.permutation(S)[:2]
        w[[a, b]] = 0.45
        v[a], v[b] = 0.02, 0.29
    elif kind == "d0_on_draw":  # the threshold equals a draw's value: the comparison is strict
        w = rng.uniform(0.1, 1.0, S)
        w /= w.sum()
        d0 = float(v[rng.integers(S)])
    elif kind == "all_zero":
        w = np.zeros(S)
    elif kind.startswith("pareto"):  # the smoothed weights of a heavy-tailed importance ratio
        lw = map_psis_cases.series(kind, S, rng)
        w = np.asarray(map_psis_ref.psis_weights(lw)[0], np.float64)
    elif kind == "nan_with_mass":  # a draw with mass that is not finite
        w = np.full(S, 1.0 / S)
        v[rng.integers(S)] = np.nan
    elif kind == "bad_weight":  # a weight that is none
        w = np.full(S, 1.0 / S)
        w[rng.integers(S)] = np.resize(np.array([np.nan, -0.25, 1.5]), S)[S % 3]
    else:
        raise ValueError(kind)
    return v, w, d0


@functools.lru_cache(maxsize=None)
def case(S: int):
    """(v[n, S], w[n, S], d0[n], kinds, want[n, 8]) of every kind at S; the reference computed once."""
    rng = np.random.default_rng([SEED, S])
    got = [series(k, S, rng) for k in KINDS]
    v = np.stack([g[0] for g in got])
    w = np.stack([g[1] for g in got])
    d0 = np.array([g[2] for g in got])
    want = np.stack([order_stats(a, b, c) for a, b, c in zip(v, w, d0)])
    for a in (v, w, d0, want):
        a.setflags(write=False)
    return v, w, d0, KINDS, want


def bits(a) -> np.ndarray:
    """The bit patterns of float64 values, every NaN as one pattern."""
    a = np.array(a, np.float64)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)
