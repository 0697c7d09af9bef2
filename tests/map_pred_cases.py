"""Crafted weight and count series for MDFIT-PPRED v1 (a helper, no test),
shared by tests/test_map_pred.py (the host build) and
tests/test_gpu_map_pred.py (mdfit_resample)."""

from __future__ import annotations

import numpy as np

S_VALUES = (25, 64, 65, 256, 1024)
R_VALUES = (25, 100, 1000, 1024)


def weight_series(S: int, R: int):
    """[(kind, w[S])]: equal weights; one draw holding all the weight; a third
    of the weights 0 with leading and trailing zeros; weights of 1e-300 beside
    1; weights whose cumulative sums fall exactly on the p_r; smoothed-looking
    random weights."""
    rng = np.random.default_rng(1000 * S + R)
    out = [("equal", np.full(S, 1.0 / S))]
    one = np.zeros(S)
    one[(7 * S) // 11] = 1.0
    out.append(("one", one))
    third = rng.random(S) + 0.01
    third[rng.permutation(S)[: S // 3]] = 0.0
    third[:3] = 0.0
    third[-4:] = 0.0
    out.append(("third_zero", third / third.sum()))
    tiny = np.where(rng.random(S) < 0.5, 1e-300, 1.0)
    tiny[0], tiny[-1] = 1e-300, 1e-300
    tiny[S // 2] = 1.0
    out.append(("tiny", tiny))
    # integer weights summing to 2 R: c[-1] / R = 2 and p_r = 2 r + 1 exactly, and every odd cumulative sum is a p_r
    exact = np.zeros(S)
    exact[0] = 1.0
    exact[1:] = rng.multinomial(2 * R - 1, np.full(S - 1, 1.0 / (S - 1)))
    assert exact.sum() == 2 * R
    out.append(("on_p", exact))
    lw = rng.standard_normal(S) * 2.0
    w = np.exp(lw - lw.max())
    out.append(("random", w / w.sum()))
    return out


def all_weight_series():
    """[(S, R, kind, w)] over S_VALUES x R_VALUES and the pairs R = S."""
    items = []
    for S in S_VALUES:
        for R in tuple(R_VALUES) + ((S,) if S not in R_VALUES else ()):
            items += [(S, R, kind, w) for kind, w in weight_series(S, R)]
    return items


def count_series():
    """[(kind, R, N, counts[R] uint32)]: ties, all-equal counts, N = 1, R odd and even, N = 4e9."""
    rng = np.random.default_rng(7)
    out = []
    for R in (25, 100, 999, 1000, 1024):
        out.append(("ties", R, 40.0, rng.integers(0, 6, R).astype(np.uint32)))
        out.append(("equal", R, 12345.0, np.full(R, 77, np.uint32)))
        out.append(("n1", R, 1.0, rng.integers(0, 2, R).astype(np.uint32)))
        out.append(("wide", R, 1.0e6, rng.binomial(1000000, 0.03, R).astype(np.uint32)))
        out.append(("big", R, 4.0e9, rng.integers(0, 4000000000, R, dtype=np.int64).astype(np.uint32)))
        two = np.where(np.arange(R) % 2 == 0, 3, 900).astype(np.uint32)  # two clusters: the window's first minimum
        out.append(("two", R, 1000.0, two))
    return out
