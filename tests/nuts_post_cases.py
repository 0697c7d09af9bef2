"""Crafted inputs for the tests of the NUTS post kernel (tests/test_nuts_post.py
on the oracle, tests/test_gpu_nuts_post.py on mdfit_nuts_post): draws, y, N and
chain status at the smallest sizes at which each part of the record assembly
can go wrong.  Three launches ("groups") of 7 or 8 taxa each,
at every sample count of S_VALUES:

  rows    the data rows under typical scattered draws
  series  the draw series on typical data (the predictive sampler's branches)
  paths   NaN draws, identical PMD / null likelihoods, -inf likelihoods, a
          failed chain, y > N

The draws of a job are seeded per (group, S): a rerun builds the same arrays.
"""

from __future__ import annotations

import functools
import hashlib

import numpy as np

NPOS, NHALF, LD = 30, 15, 32
PMD_SUBFITS = (0, 2, 3)
# 2, 3: the least; 63 .. 65: the lanes (cnt = 0 lanes below 64); 100: a usual
# small run; 511 .. 513: the LDS sort against the register sort; 1000: the
# default; 1024 / 1025: the register sort's end and the padding; 4096: the bound
S_VALUES = (2, 3, 63, 64, 65, 100, 511, 512, 513, 1000, 1024, 1025, 4096)
S_MPMATH = tuple(S for S in S_VALUES if S <= 130)  # the cases of tests/golden/nuts_post_waic.npz
GROUPS = ("rows", "series", "paths")
SEED = 41
K = np.tile(np.arange(NHALF), 2)  # |z| - 1 of column i

ROWS = ("typical", "N1", "N2", "N4e9", "Nmax", "y0", "yN", "ragged")
SERIES = ("const", "phi2", "phi1e6", "boost", "tiny", "zeroD", "clampD", "straddle")
PATHS = ("flip", "nan", "same", "neginf", "failed", "invalid", "constbig")
TAXA = {"rows": ROWS, "series": SERIES, "paths": PATHS}
UMAX = 4294967295
SMALL_N = (1, 2, 3, 5, 8, 13, 20, 30, 40, 40)  # the chi-square columns of the constant-theta taxon
POST_SEED = 20261020  # the predictive streams' seed of every crafted call (fixed: the draws are part of the case)


def _typical_draws(rng, S, q0, A0, c0, p0, rel=1.0):
    """x[6, S, 4]: scattered draws about (q0, A0, c0, p0); null chains D = q small."""
    x = np.zeros((6, S, 4))
    for k in range(6):
        x[k, :, 3] = p0 * np.exp(0.2 * rel * rng.standard_normal(S))
        if k in PMD_SUBFITS:
            x[k, :, 0] = np.clip(q0 + 0.05 * rel * rng.standard_normal(S), 0.01, 0.99)
            x[k, :, 1] = np.clip(A0 + 0.02 * rel * rng.standard_normal(S), 0.001, 0.9)
            x[k, :, 2] = np.clip(c0 + 0.002 * rel * rng.standard_normal(S), 0.0005, 0.09)
        else:
            x[k, :, 0] = np.clip(0.03 + 0.004 * rel * rng.standard_normal(S), 0.001, 0.99)
    return x


def _d_of(x0, k=K):
    """D[S, 30] of PMD draws x0[S, 4], as the specification forms it (clamped to [0, 1])."""
    D = x0[:, 1:2] * (1.0 - x0[:, 0:1]) ** k[None, :] + x0[:, 2:3]
    return np.clip(D, 0.0, 1.0)


def _typical_data(rng, x, lo=50, hi=5000):
    N = np.zeros(LD, np.uint32)
    y = np.zeros(LD, np.uint32)
    N[:NPOS] = rng.integers(lo, hi, NPOS)
    D = np.nan_to_num(_d_of(x[0, :1])[0], nan=0.1)
    y[:NPOS] = rng.binomial(N[:NPOS], D)
    return y, N


def _taxon(group: str, name: str, S: int, rng):
    """(x[6, S, 4], status[6], y[32], N[32]) of one crafted taxon."""
    status = np.zeros(6)
    x = _typical_draws(rng, S, rng.uniform(0.2, 0.6), rng.uniform(0.05, 0.3), rng.uniform(0.005, 0.02),
                       10 ** rng.uniform(1.5, 3))
    y, N = _typical_data(rng, x)
    if group == "rows":
        D0 = _d_of(x[0, :1])[0]
        if name == "N1":  # every fraction 0 or 1: the HPDI windows tie massively
            N[:NPOS] = 1
            y[:NPOS] = rng.binomial(1, np.maximum(D0, 0.3))
        elif name == "N2":
            N[:NPOS] = 2
            y[:NPOS] = rng.binomial(2, np.maximum(D0, 0.3))
        elif name == "N4e9":
            N[:NPOS] = 4_000_000_000
            y[:NPOS] = np.rint(4.0e9 * D0).astype(np.uint32)
        elif name == "Nmax":  # the sort's pad value is a legal count here
            for col in (0, NHALF):
                N[col] = UMAX
                y[col] = np.uint32(int(UMAX * D0[col]))
            x[3, ::2, 1], x[3, ::2, 2] = 0.97, 0.06  # D = 1 at k = 0: job 31 draws the count 0xFFFFFFFF itself
        elif name == "y0":
            y[:] = 0
        elif name == "yN":
            y[:] = N
        elif name == "ragged":
            for col in (0, 3, 14, 15, 22, 29):
                N[col] = 0
                y[col] = 0
    elif group == "series":
        if name == "const":  # iid Beta-Binomial predictive counts; N <= 40 at the first columns
            x[:] = x[:, :1]
            N[:len(SMALL_N)] = SMALL_N
            y[:NPOS] = rng.binomial(N[:NPOS], _d_of(x[0, :1])[0])
        elif name == "phi2":
            x[..., 3] = 2.0 + 10.0 ** rng.uniform(-6, -1, (6, S))
        elif name == "phi1e6":
            x[..., 3] = 1.0e6
        elif name == "boost":  # D phi < 1 at the far positions, > 1 at the near ones
            x[..., 0] = np.clip(0.5 + 0.05 * rng.standard_normal((6, S)), 0.3, 0.7)
            x[..., 1] = 0.3
            x[..., 2] = 0.001
            x[..., 3] = 40.0 * np.exp(0.2 * rng.standard_normal((6, S)))
            for k in (1, 4, 5):
                x[k, :, 0] = 0.01  # the null chains too: D phi = 0.4
            y, N = _typical_data(rng, x)
        elif name == "tiny":  # D phi ~ 1e-9
            for k in PMD_SUBFITS:
                x[k, :, 1] = 1.0e-12 * rng.uniform(0.5, 2.0, S)
                x[k, :, 2] = 1.0e-12 * rng.uniform(0.5, 2.0, S)
                x[k, :, 3] = 500.0
            y[:] = 0
            y[1] = 1
        elif name == "zeroD":  # A = c = 0: D = 0 exactly, alpha = 0
            for k in PMD_SUBFITS:
                x[k, :, 1] = 0.0
                x[k, :, 2] = 0.0
            y[:] = 0
            y[2] = 3  # lp = -inf there, NaN (inf - inf) where y = 0
        elif name == "clampD":  # A + c > 1: D clamped to 1 at the near positions
            for k in PMD_SUBFITS:
                x[k, :, 1] = 0.97 + 0.01 * rng.uniform(size=S)
                x[k, :, 2] = 0.06 + 0.01 * rng.uniform(size=S)
                x[k, :, 0] = 0.5
            y, N = _typical_data(rng, x)
        elif name == "straddle":  # N min(p, 1 - p) about 10: inversion and BTRS both
            for k in PMD_SUBFITS:
                x[k, :, 0] = 0.25
                x[k, :, 1] = 0.12 + 0.01 * rng.standard_normal(S)
                x[k, :, 2] = 0.012
                x[k, :, 3] = 300.0
            N[:NPOS] = np.rint(10.0 / _d_of(x[0, :1])[0]).astype(np.uint32)
            y[:NPOS] = rng.binomial(N[:NPOS], _d_of(x[0, :1])[0])
    elif group == "paths":
        if name == "flip":  # p > 0.5
            for k in PMD_SUBFITS:
                x[k, :, 0] = 0.05
                x[k, :, 1] = np.clip(0.75 + 0.03 * rng.standard_normal(S), 0.5, 0.9)
                x[k, :, 2] = 0.05
            y, N = _typical_data(rng, x)
        elif name == "nan":  # one NaN draw in the forward PMD chain: job 30 only
            x[2, S // 2, 1] = np.nan
        elif name == "same":  # null chains = PMD chains with A = 0: identical likelihoods
            for kp, kn in ((0, 1), (2, 4), (3, 5)):
                x[kp, :, 1] = 0.0
                x[kp, :, 2] = np.clip(0.03 + 0.004 * rng.standard_normal(S), 0.001, 0.99)
                x[kn] = 0.0
                x[kn, :, 0] = x[kp, :, 2]
                x[kn, :, 3] = x[kp, :, 3]
        elif name == "neginf":  # every draw of null-rev has D = 0 (lp = -inf where y > 0); null-fwd some
            x[5, :, 0] = 0.0
            x[4, ::3, 0] = 0.0
            y[:NPOS] = np.maximum(y[:NPOS], 1)
        elif name == "failed":  # two chains failed: the status is the larger
            status[1] = 1.0
            status[3] = 2.0
        elif name == "invalid":
            y[7] = N[7] + 1
        elif name == "constbig":  # constant theta at large N: the moments' check
            x[:] = x[:, :1]
            N[:NPOS] = rng.integers(200_000, 400_000, NPOS)
            N[0], N[1] = 2_000_000_000, 500_000_000
            y[:NPOS] = np.rint(N[:NPOS] * _d_of(x[0, :1])[0]).astype(np.uint32)
    return x, status, y, N


@functools.lru_cache(maxsize=None)
def case(group: str, S: int):
    """(x[T, 6, S, 4], status[T, 6], y[T, 32] uint32, N[T, 32] uint32, names)."""
    names = TAXA[group]
    xs, sts, ys, Ns = [], [], [], []
    for t, name in enumerate(names):
        rng = np.random.default_rng([SEED, GROUPS.index(group), S, t])
        x, st, y, N = _taxon(group, name, S, rng)
        xs.append(x), sts.append(st), ys.append(y), Ns.append(N)
    out = (np.stack(xs), np.stack(sts), np.stack(ys), np.stack(Ns))
    for a in out:
        a.setflags(write=False)
    return out + (names,)


def case_hash(group: str, S: int) -> str:
    """Digest of the case's arrays: the mpmath fixture names the inputs it was made from."""
    x, st, y, N, _ = case(group, S)
    h = hashlib.sha256()
    for a in (x, st, y, N):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def diag_slots(status):
    """diag[T, 6, 4] = the chain slots 4..7 (step, leapfrogs, status, divergences) a caller seeds."""
    T = status.shape[0]
    d = np.zeros((T, 6, 4))
    d[:, :, 0] = 0.25 + 0.01 * np.arange(6)[None, :]
    d[:, :, 1] = 7.0
    d[:, :, 2] = status
    d[:, :, 3] = np.arange(T)[:, None] % 3
    return d


def mm_of(group: str, S: int):
    """Mismatch counts mm[T, 30, 12] uint32 for the noise columns."""
    T = len(TAXA[group])
    rng = np.random.default_rng([SEED, 99, GROUPS.index(group), S])
    return rng.integers(1, 2000, (T, NPOS, 12)).astype(np.uint32)


# ---------------------------------------------------------------------------
# regime classes of the predictive draws (by the draw's own parameters)
# ---------------------------------------------------------------------------
CLASSES = ("boost", "tiny_alpha", "inversion", "btrs_small", "btrs_large", "flip", "clamped")
JOB_CHAIN = tuple([0] * NPOS + [2, 3])
JOB_COL = tuple(list(range(NPOS)) + [0, 0])


def draw_classes(x, N):
    """cls[T, 32, S, 7] bool: the classes each predictive draw belongs to (a draw
    may be in several), from D and phi of the draw and the job's N: boost (alpha
    or beta < 1), tiny alpha (< 1e-6), inversion (N min(D, 1 - D) < 10), BTRS at
    N <= 1e6 and at N >= 1e8, flip (D > 0.5), clamped D (the raw D outside [0, 1]
    or on its ends)."""
    T, _, S, _ = x.shape
    cls = np.zeros((T, 32, S, len(CLASSES)), bool)
    for j in range(32):
        th = x[:, JOB_CHAIN[j]]
        k = K[JOB_COL[j]]
        with np.errstate(invalid="ignore"):
            raw = th[..., 1] * (1.0 - th[..., 0]) ** k + th[..., 2]
            D = np.clip(raw, 0.0, 1.0)
            a, b = D * th[..., 3], (1.0 - D) * th[..., 3]
            n = N[:, JOB_COL[j]].astype(float)[:, None]
            npq = n * np.minimum(D, 1.0 - D)
            clamped = (raw <= 0.0) | (raw >= 1.0)
            cls[:, j, :, 6] = clamped
            cls[:, j, :, 0] = ~clamped & ((a < 1.0) | (b < 1.0))
            cls[:, j, :, 1] = ~clamped & ((a < 1.0e-6) | (b < 1.0e-6))
            cls[:, j, :, 2] = ~clamped & (npq < 10.0)
            cls[:, j, :, 3] = ~clamped & (npq >= 10.0) & (n <= 1.0e6)
            cls[:, j, :, 4] = ~clamped & (npq >= 10.0) & (n >= 1.0e8)
            cls[:, j, :, 5] = ~clamped & (D > 0.5)
    return cls


@functools.lru_cache(maxsize=None)
def oracle_post(group: str, S: int):
    """(out, pred, status, waic, counts, flags) of oracle_nuts_post on the case; computed once."""
    from oracle.oracle import OracleLib

    x, status, y, N, _ = case(group, S)
    got = OracleLib().nuts_post(y, N, x, diag=diag_slots(status), mm=mm_of(group, S), seed=POST_SEED, taps=True)
    for a in got:
        a.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def waic64(group: str, S: int):
    """(waic[T, 6, 30], mag[T, 6, 30, 5]) of the case in float64 (nuts_post_ref.waic_class),
    NaN for the taxa whose record is not assembled; computed once."""
    from tests import nuts_post_ref as ref

    x, status, y, N, _ = case(group, S)
    ok = (status == 0).all(axis=1) & ~(y[:, :NPOS] > N[:, :NPOS]).any(axis=1)
    w = np.full((x.shape[0], 6, NPOS), np.nan)
    mag = np.full((x.shape[0], 6, NPOS, 5), np.nan)
    w[ok], mag[ok] = ref.waic_class(x[ok], y[ok], N[ok], with_mag=True)
    w.setflags(write=False), mag.setflags(write=False)
    return w, mag
