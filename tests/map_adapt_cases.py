"""Crafted series for the proposal refit of MDFIT-ADAPT v1 (a helper, no test):
shared by the host-program test (tests/test_map_adapt.py) and the device test
(tests/test_gpu_map_adapt.py), with the reference's answer and the error
measure both use."""

from __future__ import annotations

import numpy as np

from tests import map_adapt_ref as ad

S_VALUES = (25, 64, 65, 256, 1024)
KINDS = ("free4", "free4_heavy", "held3", "held3_heavy", "one_draw", "const_coord", "zero_nan", "zero_nan_held",
         "cbar_tiny", "cbar_zero", "cbar_subnormal")
STOPS = ("one_draw", "const_coord", "cbar_zero", "cbar_subnormal")


def series(S: int, reps: int = 3):
    """(u[n, S, 4], w[n, S], mask[n], cheld[n], K[n, 4], kinds[n]): reps of every kind."""
    rng = np.random.default_rng(1000 + S)
    us, ws, masks, chs, Ks, kinds = [], [], [], [], [], []
    for rep in range(reps):
        for kind in KINDS:
            held = kind in ("held3", "held3_heavy", "zero_nan_held", "cbar_tiny", "cbar_zero", "cbar_subnormal")
            A = rng.normal(size=(4, 4)) * np.array([0.3, 0.5, 0.02, 1.0])[:, None]
            u = np.array([-1.0, -2.0, 0.05, 5.0]) + rng.standard_t(4, size=(S, 4)) @ A.T
            K = np.zeros(4)
            if held:
                u[:, 2] = rng.exponential(size=S) / 300.0
                K[[0, 1, 3]] = rng.normal(size=3) * 5.0
            lw = rng.normal(size=S) * (3.0 if "heavy" in kind else 1.0)
            w = np.exp(lw - lw.max())
            if kind == "one_draw":
                w = np.zeros(S)
                w[rng.integers(S)] = 1.0
            if kind == "const_coord":
                u[:, 3] = 0.0  # (exactly: its mean and every residual are 0 in any arithmetic)
            if kind in ("zero_nan", "zero_nan_held"):
                dead = rng.permutation(S)[: S // 3]
                w[dead] = 0.0
                u[dead] = np.nan
            if kind == "cbar_tiny":
                u[:, 2] *= 1e-200
            if kind == "cbar_zero":
                u[:, 2] = 0.0
            if kind == "cbar_subnormal":
                u[:, 2] = 5e-324  # (1 / c-bar overflows)
            w = w / w.sum()
            us.append(u)
            ws.append(w)
            masks.append(11 if held else 15)
            chs.append(1 if held else 0)
            Ks.append(K)
            kinds.append(kind)
    return (np.array(us), np.array(ws), np.array(masks, np.int32), np.array(chs, np.int32), np.array(Ks), kinds)


def reference(u, w, mask, cheld, K):
    """List of refit_arrays' dicts (None: the round stops)."""
    return [ad.refit_arrays(u[i], w[i], int(mask[i]), bool(cheld[i]), K[i]) for i in range(len(w))]


def errors(got, want):
    """Worst error over the series that do not stop: got = (m, d, F, gc) arrays,
    want = reference().  m absolute over max(1, |m|), d and gc relative, F
    absolute (its entries lie in [-1, 1])."""
    m, d, F, gc = got
    worst = {"m": 0.0, "d": 0.0, "F": 0.0, "gc": 0.0}
    for i, r in enumerate(want):
        if r is None:
            continue
        worst["m"] = max(worst["m"], float((np.abs(m[i] - r["m"]) / np.maximum(1, np.abs(r["m"]))).max()))
        worst["d"] = max(worst["d"], float((np.abs(d[i] - r["d"]) / r["d"]).max()))
        worst["F"] = max(worst["F"], float(np.abs(F[i] - r["F"]).max()))
        if r["gc"] != 0:
            worst["gc"] = max(worst["gc"], float(abs(gc[i] - r["gc"]) / r["gc"]))
        else:
            assert gc[i] == 0.0
    return worst
