"""The fit kernel's MAP objective, gradient and Hessian (make_theta, point_args,
point_finish, finish_eval of csrc/mdfit_model.h, through mdfit_objective and
mdfit_objective_form) against the analytic formulas of DESIGN.md §3.1-3.2 in
mpmath, on the items of tests/objective_cases.py at the bars of DESIGN.md
§3.4.2 -- the whole bar here, half of it for the oracle
(tests/test_map_objective.py).  One launch over all items per form, one wave
per item.  Run on an MI355X: pytest -m gpu."""

from __future__ import annotations

import numpy as np
import pytest

from tests import objective_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    from metadamage_amd import engine as eng

    return eng


@pytest.fixture(scope="module")
def fx():
    return oc.load()


@pytest.fixture(scope="module")
def forms(engine, fx):
    """{form: flat [n][NX]} of the plain entry (None) and every form of mdfit_objective_form."""
    return {f: oc.flat(*engine.objective(fx["model"], fx["subset"], fx["y"], fx["N"], fx["u"], form=f))
            for f in (None, 0, 1, 2, 3, 4, 5, 6, 7)}


def test_kernel_within_the_bar(fx, forms):
    X = forms[None]
    frac = oc.fractions(X, fx["ref"], fx["res"], fx["bar"])
    for grp in (oc.INTERIOR, oc.EDGE):
        for model in (oc.PMD, oc.NULL):
            s = np.flatnonzero((fx["group"] == grp) & (fx["model"] == model))
            oc.report(f"kernel, {oc.GROUPS[grp]}, {'PMD' if model == oc.PMD else 'null'}", oc.worst(frac, s))
    oc.report(f"kernel, null at logit q in (12, 25), bar '{oc.NULL_OMD}'", oc.worst(frac, oc.null_corner(fx)))
    sel = np.flatnonzero((fx["group"] == oc.INTERIOR) | (fx["group"] == oc.EDGE))
    assert np.isfinite(X[sel]).all()
    bad = np.argwhere(frac[sel] > 1.0)
    assert bad.size == 0, [(int(sel[i]), int(j), float(frac[sel[i], j])) for i, j in bad[:10]]
    # infeasible: F = +inf is all the header promises
    assert (X[fx["group"] == oc.INFEASIBLE, 0] == np.inf).all()
    # the overflow corner (min D_i < 1e-150): F finite and within its bar, g and H within theirs or non-finite
    ov = np.flatnonzero(fx["group"] == oc.OVERFLOW)
    assert np.isfinite(X[ov, 0]).all() and (frac[ov, 0] <= 1.0).all(), frac[ov, 0]
    gh = slice(1, 21)
    nonfinite = ~np.isfinite(X[ov][:, gh])
    names = [f"g{j}" for j in range(4)] + [f"H{j}{m}" for j in range(4) for m in range(4)]
    for i, nf in zip(ov, nonfinite):
        print(f"overflow corner, item {i}, u = {fx['u'][i].tolist()}: non-finite",
              [n for n, b in zip(names, nf) if b] or "none")
    worst = np.where(nonfinite, 0.0, frac[ov][:, gh])
    print(f"overflow corner: worst finite entry of g, H at {worst.max():.3f} of the bar, F at {frac[ov, 0].max():.3f}")
    ok = nonfinite | (frac[ov][:, gh] <= 1.0)
    assert ok.all(), [(int(ov[i]), int(j), float(frac[ov[i], 1 + j])) for i, j in np.argwhere(~ok)[:10]]


def test_kernel_exact_zeros_and_symmetry(fx, forms):
    fin = fx["group"] != oc.INFEASIBLE
    X = forms[None][fin]
    sub = fx["subset"][fin]
    pos = np.arange(30)
    outside = ((sub[:, None] == 1) & (pos >= 15)) | ((sub[:, None] == 2) & (pos < 15))
    empty = fx["N"][fin][:, :30] == 0
    assert (X[:, oc.SL_ELL][outside | empty] == 0.0).all()
    null = fx["model"][fin] == oc.NULL
    g, H = X[null][:, oc.SL_G], X[null][:, oc.SL_H].reshape(-1, 4, 4)
    assert (g[:, 1:3] == 0.0).all() and (H[:, 1:3, :] == 0.0).all() and (H[:, :, 1:3] == 0.0).all()
    H = X[:, oc.SL_H].reshape(-1, 4, 4)
    assert np.array_equal(H.view(np.int64), np.ascontiguousarray(H.transpose(0, 2, 1)).view(np.int64))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_forms_return_the_plain_bits(fx, forms):
    """null_row (pad-lane triples) and whole_pair (xrow triples) are "bitwise lg3
    of the same argument": F, g, H and ell equal the plain form's bits; accf
    changes the value term alone: g and H equal the plain form's bits."""
    plain = forms[None]
    n_null = int((fx["model"] == oc.NULL).sum())
    n_all = int((fx["subset"] == 0).sum())
    assert n_null > 50 and n_all > 50  # the forms have items to act on
    for f in (0, oc.FORM_NULL_ROW, oc.FORM_WHOLE_PAIR, oc.FORM_NULL_ROW | oc.FORM_WHOLE_PAIR):
        diff = _bits(forms[f]) != _bits(plain)
        assert not diff.any(), (f, np.argwhere(diff)[:10].tolist())
    gh = slice(1, 21)
    for f in (1, 3, 5, 7):
        diff = _bits(forms[f][:, gh]) != _bits(plain[:, gh])
        assert not diff.any(), (f, np.argwhere(diff)[:10].tolist())
        # and the value term does not depend on where the triples came from
        v = np.r_[0, 21:51]
        diff = _bits(forms[f][:, v]) != _bits(forms[1][:, v])
        assert not diff.any(), (f, np.argwhere(diff)[:10].tolist())


def test_form_argument_errors(engine, fx):
    with pytest.raises(Exception):
        engine.objective(fx["model"][:1], fx["subset"][:1], fx["y"][:1], fx["N"][:1], fx["u"][:1], form=8)
    with pytest.raises(Exception):
        engine.objective(fx["model"][:1], fx["subset"][:1], fx["y"][:1], fx["N"][:1], fx["u"][:1], form=-1)


def test_accf_value_against_the_full_logpmf(fx, forms):
    """The polish form's F and ell are the full log-pmf objective (ln C(N, y)
    included): against mpmath at lrise's bar (special_cases.py) summed over the
    three terms per point, the sums' roundings and cond(F)."""
    v = np.r_[0, 21:51]
    got = forms[oc.FORM_ACCF][:, v]
    fin = np.flatnonzero(fx["group"] != oc.INFEASIBLE)
    frac = oc.fractions(got, fx["accf_ref"], fx["accf_res"], fx["accf_bar"])[fin]
    iF, iE = int(frac[:, 0].argmax()), int(frac[:, 1:].max(1).argmax())
    print(f"accf: worst error as a fraction of the bar: F {frac[iF, 0]:.3f} (item {fin[iF]}), "
          f"ell {frac[iE, 1:].max():.3f} (item {fin[iE]})")
    assert np.isfinite(got[fin]).all()
    bad = np.argwhere(frac > 1.0)
    assert bad.size == 0, [(int(fin[i]), int(j), float(frac[i, j])) for i, j in bad[:10]]
    assert (forms[oc.FORM_ACCF][fx["group"] == oc.INFEASIBLE, 0] == np.inf).all()
