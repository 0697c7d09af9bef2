"""The CPU oracle's MAP objective, gradient and Hessian (evaluate() of
oracle/mdfit_oracle.c) against the analytic formulas of DESIGN.md §3.1-3.2 in
mpmath (tests/golden/objective_golden.npz, written by make_golden_objective.py;
the items and the bars' constants in tests/objective_cases.py, DESIGN.md
§3.4.2).  No bar holds a number taken from the oracle or the kernel.  The
oracle is held to HALF the bar, as §3.4.1 holds it; tests/test_gpu_map_objective.py
holds the kernel to the whole bar on the same items."""

from __future__ import annotations

import numpy as np
import pytest

from tests import objective_cases as oc


@pytest.fixture(scope="module")
def fx():
    return oc.load()


@pytest.fixture(scope="module")
def oracle_X(fx, oracle_lib):
    """The oracle on every item, flat [n][NX]."""
    with np.errstate(all="ignore"):
        rows = [oracle_lib.objective(int(m), int(s), y[:30], N[:30], u)
                for m, s, y, N, u in zip(fx["model"], fx["subset"], fx["y"], fx["N"], fx["u"])]
    return oc.flat(*(np.array([r[j] for r in rows]) for j in range(4)))


def test_fixture_belongs_to_these_cases(fx):
    """The npz was written from the items and constants objective_cases.py holds now."""
    assert str(fx["digest"]) == oc.digest()
    model, subset, row, u, group = oc.items()
    for key, a in (("model", model), ("subset", subset), ("row", row), ("u", u), ("group", group)):
        assert np.array_equal(fx[key], a), key
    assert str(fx["null_omd"]) == oc.NULL_OMD
    # the groups are what they say: every group but the overflow corner keeps D and the gap off the floor
    fin = fx["group"] != oc.INFEASIBLE
    safe = fin & (fx["group"] != oc.OVERFLOW)
    # (in the overflow corner some true entries of H lie beyond the doubles: +-inf in `ref`)
    assert (fx["ref"][~fin, 0] == np.inf).all() and np.isfinite(fx["ref"][safe]).all()
    assert np.isfinite(fx["ref"][fin][:, 0]).all()
    assert (fx["min_D"][safe] >= oc.D_FLOOR).all() and (fx["gap"][safe] >= oc.GAP_FLOOR).all()
    assert (fx["min_D"][fx["group"] == oc.OVERFLOW] < oc.D_FLOOR).all()
    assert np.bincount(fx["group"]).tolist() == [108, 126, 3, 6]
    assert np.isfinite(fx["bar"][safe]).all() and (fx["bar"][fin] >= oc.ABS).all()


def test_oracle_within_half_the_bar(fx, oracle_X):
    """Every entry of F, g, H and ell within half its bar on every item whose
    D and 1 - A - c stay off the floor (interior and edge items)."""
    sel = np.flatnonzero((fx["group"] == oc.INTERIOR) | (fx["group"] == oc.EDGE))
    frac = oc.fractions(oracle_X, fx["ref"], fx["res"], fx["bar"])
    for grp in (oc.INTERIOR, oc.EDGE):
        for model in (oc.PMD, oc.NULL):
            s = np.flatnonzero((fx["group"] == grp) & (fx["model"] == model))
            oc.report(f"oracle, {oc.GROUPS[grp]}, {'PMD' if model == oc.PMD else 'null'}", oc.worst(frac, s))
    oc.report(f"oracle, null at logit q in (12, 25), bar '{oc.NULL_OMD}'", oc.worst(frac, oc.null_corner(fx)))
    assert np.isfinite(oracle_X[sel]).all()
    bad = np.argwhere(frac[sel] > 0.5)
    assert bad.size == 0, [(int(sel[i]), int(j), float(frac[sel[i], j])) for i, j in bad[:10]]


def test_oracle_exact_zeros_and_symmetry(fx, oracle_X):
    fin = fx["group"] != oc.INFEASIBLE
    X = oracle_X[fin]
    ell = X[:, oc.SL_ELL]
    sub = fx["subset"][fin]
    pos = np.arange(30)
    outside = ((sub[:, None] == 1) & (pos >= 15)) | ((sub[:, None] == 2) & (pos < 15))
    empty = fx["N"][fin][:, :30] == 0
    assert (ell[outside | empty] == 0.0).all()  # (compared by value; a NaN would fail)
    null = fx["model"][fin] == oc.NULL
    g, H = X[null][:, oc.SL_G], X[null][:, oc.SL_H].reshape(-1, 4, 4)
    assert (g[:, 1:3] == 0.0).all() and (H[:, 1:3, :] == 0.0).all() and (H[:, :, 1:3] == 0.0).all()
    H = X[:, oc.SL_H].reshape(-1, 4, 4)
    Ht = H.transpose(0, 2, 1)
    assert ((H == Ht) | (np.isnan(H) & np.isnan(Ht))).all()


def test_oracle_infeasible_items(fx, oracle_X):
    bad = fx["group"] == oc.INFEASIBLE
    assert bad.sum() == 3
    assert (oracle_X[bad, 0] == np.inf).all()
    assert (oracle_X[bad][:, 1:21] == 0.0).all()  # g and H, as evaluate() returns them


def test_oracle_overflow_corner(fx, oracle_X):
    """min D_i < 1e-150: phi^2 psi1(a) leaves the doubles, and some true entries
    of H lie beyond them.  F stays finite and within its bar; an entry of g or
    H is within its bar or non-finite.  The whole bar, not half of it as on the
    finite-reference items: the oracle forms (1-q)^k as exp(k ln(1-q)), which
    carries 3 roundings times |k ln(1-q)|, up to 350 here, into D_i and through
    psi(a) ~ -1/a into g_c -- 0.58 of the bar, whose eps_D is the kernel's
    product form's.  The fit records of tests/golden pin the
    oracle's bits, so that form stays."""
    sel = np.flatnonzero(fx["group"] == oc.OVERFLOW)
    frac = oc.fractions(oracle_X, fx["ref"], fx["res"], fx["bar"])
    assert np.isfinite(oracle_X[sel, 0]).all() and (frac[sel, 0] <= 1.0).all(), frac[sel, 0]
    gh = slice(1, 21)
    nonfinite = ~np.isfinite(oracle_X[sel][:, gh])
    for i, nf in zip(sel, nonfinite):
        names = [f"g{j}" for j in range(4)] + [f"H{j}{m}" for j in range(4) for m in range(4)]
        print(f"overflow corner, item {i}, u = {fx['u'][i].tolist()}: non-finite",
              [n for n, b in zip(names, nf) if b] or "none")
    worst = np.where(nonfinite, 0.0, frac[sel][:, gh])
    print(f"overflow corner: worst finite entry of g, H at {worst.max():.3f} of the bar, F at {frac[sel, 0].max():.3f}")
    ok = nonfinite | (frac[sel][:, gh] <= 1.0)
    assert ok.all(), [(int(sel[i]), int(j), float(frac[sel[i], 1 + j])) for i, j in np.argwhere(~ok)[:10]]


def test_the_bars_have_teeth(fx):
    """Each planted wrong Hessian (without the J2 G chain term; without the
    lD Dqq term; the prior's -8/(1-c)^2 taken as -8/(1-c)) lies outside the
    FULL bar, in some entry, on at least 90 % of the PMD interior items.  The
    third plant equals the true Hessian where c = 0 (1 - c = 1): it is counted
    over the items with c > 0."""
    it = fx["planted_item"]
    assert np.array_equal(it, np.flatnonzero((fx["group"] == oc.INTERIOR) & (fx["model"] == oc.PMD)))
    assert len(it) == 54
    ref, res, bar = fx["ref"][it][:, oc.SL_H], fx["res"][it][:, oc.SL_H], fx["bar"][it][:, oc.SL_H]
    for p, name in enumerate(("no J2 G term", "no lD Dqq term", "prior -8/(1-c)")):
        frac = oc.fractions(fx["planted"][:, p], ref, res, bar)
        caught = (frac > 1.0).any(1)
        use = fx["u"][it, 2] > 0.0 if p == 2 else np.ones(len(it), bool)
        print(f"planted '{name}': outside the bar on {caught[use].sum()} of {use.sum()} items, "
              f"median excess {np.median(frac.max(1)[use]):.3g} bars")
        assert use.sum() >= 27
        assert caught[use].mean() >= 0.9, (name, caught[use].mean())
