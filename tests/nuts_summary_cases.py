"""Crafted draws for the posterior-summary tests (tests/test_nuts_summary.py on
the host program, tests/test_gpu_nuts_summary.py on the kernel): the draws of
tests/nuts_diag_cases.py -- iid, AR(1), alternating, constant, 1e8 offset and
trend series, one NaN draw, one failed chain -- at the shapes where the sort and
the window search change path, plus the ramp, whose windows all tie."""

from __future__ import annotations

import functools

import numpy as np

from tests import nuts_diag_cases as diag_cases
from tests import nuts_summary_ref as ref

# 1024 and 1025 straddle the sort's padding; 2 and 3 have a single HPDI window
S_VALUES = (2, 3, 4, 5, 63, 64, 65, 127, 129, 1000, 1001, 1024, 1025, 4096)
# (S, T): every S at T = 3; T = 1 and T = 67 (more rows than one block) at small S
SHAPES = tuple((S, 3) for S in S_VALUES) + ((5, 1), (1000, 1), (65, 67))
SEED = 17
kind_of = diag_cases.kind_of
faults = diag_cases.faults
# the ramp: a permutation of 0 .. S-1, so every window of L + 1 sorted draws is
# exactly L wide and only the lowest-index rule gives [0, L].  Row (0, 0), a PMD
# sub-fit: q, A and phi are ramps and c is 0, so D_max = A is one too; row (0,
# 1), a null sub-fit: q (its D_max) and phi
RAMP_ROWS = ((0, 0), (0, 1))


def window(S: int) -> int:
    return int(0.68 * S)


@functools.lru_cache(maxsize=None)
def case(S: int, T: int):
    """(samples[T, 6, S, 4] float64, chain_status[T, 6] float64) of one shape."""
    x0, status = diag_cases.case(S, T)
    x = x0.copy()
    rng = np.random.default_rng([SEED, S, T])
    for t, k in RAMP_ROWS:
        for j in (0, 1, 3):
            x[t, k, :, j] = rng.permutation(S).astype(np.float64)
        x[t, k, :, 2] = 0.0
    x[0, 1, :, 1] = 0.0  # (a null sub-fit stores A = c = 0)
    x.setflags(write=False)
    return x, status


@functools.lru_cache(maxsize=None)
def reference(S: int, T: int):
    """summ[T, 6, 16] longdouble of the shape's case; computed once."""
    x, status = case(S, T)
    want = ref.summary_rows(x, status)
    want.setflags(write=False)
    return want
