"""GPU tests of mdfit_map_evidence (MDFIT-EVID v1): the
diagnostics, draws and adapt record against mdfit_map_waic_adapt bit for bit,
the evidence against tests/map_evidence_ref.py fed the kernel's draws and
against quadrature and a large importance-sampling run, the log mean weight on
crafted series, the edge cases, the invariance of the record under every way of
calling, and the CLI path."""

from __future__ import annotations

import ctypes
import json

import numpy as np
import pandas as pd
import pytest

from tests import map_evidence_ref as ref
from tests import map_psis_cases as cases
from tests import map_psis_ref as pref
from tests import map_waic_ref as wref
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

S_A = 256
T_A = 64
SEED = 0
LD = np.longdouble
# measured on the MI355X over the first 64 taxa of generate(300, 21) at S = 256
# and the first 8 at S = 25, 65 and 1024, without rounds and with three (the
# worst of the eight runs), asserted at ten times it: the
# kernel's record against the reference fed the kernel's u and lw, absolute over
# max(1, |.|).  (378 + 378 + 6 x 48 rows compared, none left out.)  Without
# rounds log_evidence and log_w_max are at 4.5e-14 and the comparisons, which
# are differences of two log Z of a few hundred measured against max(1, |log
# BF|), at 1.7e-12.  With rounds they carry K_prop of the refitted proposal,
# whose scale and factor the reference forms from its own refit of its own
# draws: 5.8e-14 at S = 256, 1.5e-13 at S = 1024, 2.9e-13 at S = 65 and 1.0e-11
# at S = 25, where a covariance of four coordinates comes from 25 draws and the
# 1e-12-sized differences between the device's and the oracle's log-weights are
# amplified by its condition; the comparisons follow (8.4e-10 at S = 25, 8.4e-12
# at S = 256).
MEASURED = {"log_evidence": 1.02e-11, "se": 1.29e-15, "log_w_max": 1.03e-11, "compare": 8.42e-10}


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    return torch


def _map_fit(torch, y, N, mm=None, **opts):
    from metadamage_amd import _lib, engine

    ty, tN, tm = engine.to_device_counts(y, N, mm)
    res = engine.fit_batch_device(ty, tN, tm, _lib.default_opts(mode=_lib.MODE_MAP, **opts))
    torch.cuda.synchronize()
    return ty, tN, res


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _sub(res, lo, hi):
    from metadamage_amd import engine

    return engine.FitBatch(res.out[lo:hi], None, res.status[lo:hi], None)


def _run(torch, ty, tN, res, S, T=None, R=0, seed=SEED, base=0):
    """mdfit_map_evidence_adapt with draws and the adapt record on the first T taxa -> host arrays."""
    from metadamage_amd import engine

    T = int(ty.shape[0]) if T is None else T
    evid, dr, adapt = engine.map_evidence_device(ty[:T], tN[:T], _sub(res, 0, T), S, seed, base, draws=True,
                                                 adapt_rounds=R, adapt=True)
    torch.cuda.synchronize()
    return evid.cpu().numpy(), dr.cpu().numpy(), adapt.cpu().numpy()


def _run_waic(torch, ty, tN, res, S, T, R):
    from metadamage_amd import engine

    waic, dr, adapt = engine.map_waic_device(ty[:T], tN[:T], _sub(res, 0, T), S, SEED, 0, draws=True, adapt_rounds=R,
                                             adapt=True)
    torch.cuda.synchronize()
    return waic.cpu().numpy(), dr.cpu().numpy(), adapt.cpu().numpy()


@pytest.fixture(scope="module")
def batch_a(torch_dev):
    """generate(300, seed=21) fitted by one MAP call; the evidence of its first
    64 taxa at S = 256 with the draws, without rounds (mdfit_map_evidence) and
    with three (computed once, read only)."""
    from metadamage_amd import engine
    from metadamage_amd.synthetic import generate

    torch = torch_dev
    b = generate(300, seed=21)
    ty, tN, res = _map_fit(torch, b.y, b.N, b.mm)
    before = (res.out.clone(), res.pred.clone(), res.status.clone())
    plain, plain_dr = engine.map_evidence_device(ty[:T_A], tN[:T_A], _sub(res, 0, T_A), S_A, SEED, 0, draws=True)
    torch.cuda.synchronize()
    host = {"b": b, "plain": plain.cpu().numpy(), "plain_draws": plain_dr.cpu().numpy()}
    for R in (0, 3):
        host[f"evid{R}"], host[f"draws{R}"], host[f"adapt{R}"] = _run(torch, ty, tN, res, S_A, T_A, R)
    # out, pred and status are read only
    assert torch.equal(before[0].view(torch.int64), res.out.view(torch.int64))
    assert torch.equal(before[1].view(torch.int32), res.pred.view(torch.int32)) and torch.equal(before[2], res.status)
    host.update(out=res.out.cpu().numpy(), st=res.status.cpu().numpy())
    for a in host.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    host.update(ty=ty, tN=tN, res=res)
    return host


# --------------------------------------------------------------------------
# the diagnostics, the draws and the adapt record are mdfit_map_waic_adapt's
# --------------------------------------------------------------------------
@pytest.mark.parametrize("R", (0, 3))
def test_rows_are_map_waic_adapt_bit_for_bit(torch_dev, batch_a, R):
    waic, wdr, wad = _run_waic(torch_dev, batch_a["ty"], batch_a["tN"], batch_a["res"], S_A, T_A, R)
    evid, dr, adapt = batch_a[f"evid{R}"], batch_a[f"draws{R}"], batch_a[f"adapt{R}"]
    for name, fe, fw in (("khat", ref.KHAT, wref.KHAT), ("ess", ref.ESS, wref.ESS), ("n_inf", ref.N_INF, wref.N_INF),
                         ("flags", ref.FLAGS, wref.FLAGS)):
        assert np.array_equal(_bits(evid[:, :6, fe]), _bits(waic[:, :6, fw])), name
    assert np.array_equal(_bits(dr), _bits(wdr)) and np.array_equal(_bits(adapt), _bits(wad))
    # row 6: khat_max, ess_min and the flags are the waic record's too
    assert np.array_equal(_bits(evid[:, 6, 5:8]), _bits(waic[:, 6, [4, 5, 7]]))
    fl = evid[:, :6, ref.FLAGS].astype(int)
    n_valid = int((fl & ref.VALID).sum())
    print(f"R = {R}: {n_valid} of 384 rows valid, {int(((fl & 3) == 3).sum())} reliable, "
          f"{int((fl & ref.ADAPTED != 0).sum())} adapted")
    assert n_valid >= 340
    valid = (fl & ref.VALID) != 0
    assert np.array_equal(evid[:, :6, ref.ROUND][valid] > 0, (fl & ref.ADAPTED != 0)[valid])
    assert (evid[:, [1, 4, 5], ref.ROUND][valid[:, [1, 4, 5]]] == 0).all()  # the null rows are not adapted
    if R == 0:  # mdfit_map_evidence_adapt without rounds writes mdfit_map_evidence's bits
        assert np.array_equal(_bits(evid), _bits(batch_a["plain"]))
        assert np.array_equal(_bits(dr), _bits(batch_a["plain_draws"]))
        assert (evid[:, :6, ref.ROUND][valid] == 0).all()
    else:
        pmd = [0, 2, 3]
        assert np.array_equal(evid[:, pmd, ref.ROUND][valid[:, pmd]], adapt[:, :, 2][valid[:, pmd]])


# --------------------------------------------------------------------------
# against the reference
# --------------------------------------------------------------------------
def _compare_with_reference(oracle_lib, b, out, st, evid, dr, S, T, R, worst):
    """Every taxon t < T: flags and NaN pattern equal, errors into `worst`.
    Returns (rows compared, rows left out as too close to a decision)."""
    tau = pref.khat_threshold(S)
    compared = excluded = 0
    for t in range(T):
        y30, N30 = b.y[t, :30], b.N[t, :30]
        if st[t] != 0:
            assert np.isnan(evid[t, :, :7]).all() and (evid[t, :, 7] == 0).all() and np.isnan(dr[t]).all()
            continue
        fed = ref.evidence_taxon(oracle_lib, y30, N30, out[t], 0, S, R, seed=SEED, g=t,
                                 given=(dr[t, :, :, :4], dr[t, :, :, 4]))
        near = False
        for s in range(6):
            got, want, info = evid[t, s], fed["rec"][s], fed["rows"][s]
            prop = info["prop"]
            if prop.near or info["margin"] <= 1e-6:  # a held/free or khat decision within 1e-6 of its threshold
                near = True
                excluded += 1
                continue
            assert (int(got[ref.FLAGS]) >> 2) & 15 == prop.mask, (t, s, got[ref.FLAGS], prop.mask)
            if not int(want[ref.FLAGS]) & ref.VALID:
                assert int(got[ref.FLAGS]) == prop.mask << 2 and np.isnan(got[:7]).all(), (t, s, got)
                assert np.isnan(dr[t, s, :, 5]).all()
                continue
            khat_ref = float(want[ref.KHAT])
            if np.isfinite(khat_ref) and abs(khat_ref - tau) <= 1e-6:
                near = True
                excluded += 1
                continue
            compared += 1
            assert int(got[ref.FLAGS]) == int(want[ref.FLAGS]), (t, s, got, want)
            assert got[ref.ROUND] == float(want[ref.ROUND]) and got[ref.N_INF] == float(want[ref.N_INF])
            assert abs(dr[t, s, :, 5].sum() - 1.0) < 1e-12
            for name, j in (("log_evidence", ref.LOGZ), ("se", ref.SE), ("log_w_max", ref.LWMAX)):
                worst[name] = max(worst[name], float(abs(got[j] - want[j]) / max(1, abs(want[j]))))
        if near:
            continue
        g6, w6 = evid[t, 6], fed["rec"][6]
        assert int(g6[ref.FLAGS]) == int(w6[ref.FLAGS]), (t, g6, w6)
        for j in range(7):
            assert np.isnan(g6[j]) == np.isnan(float(w6[j])), (t, j, g6, w6)
            if not np.isnan(g6[j]):
                worst["compare"] = max(worst["compare"], float(abs(g6[j] - w6[j]) / max(1, abs(w6[j]))))
    return compared, excluded


def _assert_worst(worst):
    for name, v in worst.items():
        assert v <= 10.0 * MEASURED[name], (name, v)


@pytest.mark.parametrize("R", (0, 3))
def test_batch_a_vs_reference(batch_a, oracle_lib, R):
    worst = dict.fromkeys(MEASURED, 0.0)
    compared, excluded = _compare_with_reference(oracle_lib, batch_a["b"], batch_a["out"], batch_a["st"],
                                                 batch_a[f"evid{R}"], batch_a[f"draws{R}"], S_A, T_A, R, worst)
    print(f"S = {S_A}, R = {R}, {T_A} taxa: {compared} rows compared, {excluded} left out; worst error: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert compared >= 340 and excluded <= 4  # of 384
    _assert_worst(worst)


@pytest.mark.parametrize("R", (0, 3))
@pytest.mark.parametrize("S", (25, 65, 1024))
def test_other_draw_counts_vs_reference(torch_dev, batch_a, oracle_lib, S, R):
    """A five-draw tail, one full trip plus one draw, and the largest LDS."""
    T = 8
    evid, dr, _ = _run(torch_dev, batch_a["ty"], batch_a["tN"], batch_a["res"], S, T, R)
    worst = dict.fromkeys(MEASURED, 0.0)
    compared, excluded = _compare_with_reference(oracle_lib, batch_a["b"], batch_a["out"], batch_a["st"], evid, dr, S,
                                                 T, R, worst)
    print(f"S = {S}, R = {R}, {T} taxa: {compared} rows compared, {excluded} left out; worst error: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert compared >= 36  # of 48
    _assert_worst(worst)


def test_device_evidence_meets_quadrature_and_big_run(batch_a, oracle_lib):
    """The kernel's log_evidence with the reference's se, on the first 16 taxa,
    against the recorded truths (tests/golden/map_evidence_truth.json, which
    tests/test_map_evidence.py holds equal to the computation): every valid,
    reliable row (S = 256, no rounds) within 5 standard errors.  With three
    rounds the comparison is printed, not asserted, for the reason given at
    tests/test_map_evidence.py::test_reference_meets_quadrature_and_big_run."""
    from tests.test_map_evidence import truth_check

    truth = ref.load_truth()
    b = batch_a["b"]
    for R in (0, 3):
        evid, dr = batch_a[f"evid{R}"], batch_a[f"draws{R}"]
        records = []
        for t in range(ref.TRUTH_TAXA):
            fed = ref.evidence_taxon(oracle_lib, b.y[t, :30], b.N[t, :30], batch_a["out"][t], int(batch_a["st"][t]),
                                     S_A, R, seed=SEED, g=t, given=(dr[t, :, :, :4], dr[t, :, :, 4]))
            rec = np.array(evid[t, :6], dtype=np.float64)
            rec[:, ref.SE] = fed["rec"][:6, ref.SE].astype(np.float64)
            records.append(rec)
        compared, worst, over = truth_check(records, truth, f"device R={R}", enforce=R == 0)
        print(f"R = {R}: {compared} of 96 rows compared, worst |z| {worst:.2f}, over 5: {over}")
        assert R != 0 or compared >= 64


# --------------------------------------------------------------------------
# the log mean weight on crafted series
# --------------------------------------------------------------------------
def _log_mean_weight(torch, lw):
    from metadamage_amd import _lib

    n, S = lw.shape
    t = torch.as_tensor(np.ascontiguousarray(lw), device="cuda")
    o = torch.full((3, n), -7.0, dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().mdfit_log_mean_weight(ctypes.c_void_p(t.data_ptr()), n, S, ctypes.c_void_p(o[0].data_ptr()),
                                                 ctypes.c_void_p(o[1].data_ptr()), ctypes.c_void_p(o[2].data_ptr()),
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return o.cpu().numpy()


@pytest.mark.parametrize("S", cases.S_VALUES)
def test_log_mean_weight_vs_reference(torch_dev, S):
    from tests.test_map_evidence import HOST_TOL, check_log_mean_weight, half_infeasible

    lw, kinds = cases.weights_case(S)
    lw = np.concatenate([lw, half_infeasible(S)[None, :]])
    logz, se, khat = _log_mean_weight(torch_dev, lw)
    worst = check_log_mean_weight(S, lw, kinds, logz, se, khat)
    print(f"S={S}: worst error " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    # (the bounds of the host program, derived there from the arithmetic; khat: the device's pinned tolerance of
    # tests/test_gpu_map_psis.py is for the same function)
    assert worst["logz"] <= HOST_TOL["logz"] and worst["se"] <= HOST_TOL["se"] and worst["khat"] <= 1e-11


# --------------------------------------------------------------------------
# edges
# --------------------------------------------------------------------------
def test_edges(torch_dev, batch_a, oracle_lib, ref_golden):
    from metadamage_amd import engine

    torch = torch_dev
    b = batch_a["b"]
    S = 64
    # the whole batch at S = 64: where a null row is invalid, and where a PMD c is held on 0
    full = engine.map_evidence_device(batch_a["ty"], batch_a["tN"], _sub(batch_a["res"], 0, 300), S, SEED, 0)
    torch.cuda.synchronize()
    full = full.cpu().numpy()
    fl = full[:, :, ref.FLAGS].astype(int)
    fitted = np.flatnonzero(batch_a["st"] == 0)
    bad_null = [(t, s) for t in fitted for s in (1, 4, 5) if not fl[t, s] & ref.VALID]
    assert bad_null
    for t, s in bad_null:
        assert np.isnan(full[t, s, :7]).all() and np.isnan(full[t, 6, {1: 0, 4: 1, 5: 2}[s]])
        assert fl[t, s] == fl[t, s] & 60 and not fl[t, 6] & ref.VALID and not fl[t, 6] & ref.RELIABLE
        if fl[t, 0] & fl[t, 1] & ref.VALID:  # log_bf and its se need rows 0 and 1 only
            assert np.isfinite(full[t, 6, [0, 4]]).all()
    held = [(t, s) for t in fitted for s in (0, 2, 3) if fl[t, s] & ref.VALID and not (fl[t, s] >> 2) & 4]
    print(f"c held on 0 in {len(held)} valid PMD rows")
    assert len(held) >= 5
    # rows with c held on 0, where the exponential's rate is part of K_prop, against the reference fed the kernel's lw
    T_H = sorted({t for t, _ in held})[:6]
    n_held = 0
    worst = 0.0
    for t in T_H:
        one, dr, _ = _run(torch, batch_a["ty"][t:t + 1], batch_a["tN"][t:t + 1], _SubRes(batch_a["res"], t), S, 1, 0,
                          base=t)
        assert np.array_equal(_bits(one[0]), _bits(full[t]))
        fed = ref.evidence_taxon(oracle_lib, b.y[t, :30], b.N[t, :30], batch_a["out"][t], 0, S, 0, seed=SEED, g=t,
                                 given=(dr[0, :, :, :4], dr[0, :, :, 4]))
        for s in (0, 2, 3):
            info, want = fed["rows"][s], fed["rec"][s]
            if (t, s) in held and not info["prop"].near and int(want[ref.FLAGS]) & ref.VALID:
                assert info["prop"].cheld and np.isfinite(full[t, s, [0, 1, 3, 4, 5]]).all()
                worst = max(worst, float(abs(full[t, s, ref.LOGZ] - want[ref.LOGZ]) / max(1, abs(want[ref.LOGZ]))))
                n_held += 1
    print(f"{n_held} valid rows with c held compared, worst log_evidence error {worst:.2e}")
    assert n_held >= 3 and worst <= 10.0 * MEASURED["log_evidence"]
    # the null rows' free bits are those of q and delta alone; no null row is adapted
    assert ((fl[:, [1, 4, 5]] >> 2) & 6 == 0).all() and (fl[:, [1, 4, 5]] & ref.ADAPTED == 0).all()

    # the boundary cases: rows invalid for a held coordinate have NaN statistics and their free bits alone
    cases_b = json.loads((GOLDEN / "map_boundary_cases.json").read_text())
    nb = len(cases_b)
    y = np.zeros((nb + 2, 32), np.uint32)
    N = np.zeros((nb + 2, 32), np.uint32)
    for i, c in enumerate(cases_b.values()):
        y[i, :30], N[i, :30] = c["y"], c["N"]
    N[nb:, :30] = 1000  # no damage at all; one count at the last position of each strand
    y[nb + 1, [14, 29]] = 3
    ty, tN, res = _map_fit(torch, y, N)
    evid, dr, adapt = _run(torch, ty, tN, res, S, nb + 2, 3)
    st = res.status.cpu().numpy()
    fb = evid[:, :, ref.FLAGS].astype(int)
    n_inv = n_a = 0
    for t in np.flatnonzero(st == 0):
        for s in (0, 2, 3):
            mask = (fb[t, s] >> 2) & 15
            if mask & 11 != 11:  # q, A or phi held: unsupported
                assert fb[t, s] == mask << 2 and np.isnan(evid[t, s, :7]).all() and np.isnan(dr[t, s]).all(), (t, s)
                assert np.isnan(adapt[t, {0: 0, 2: 1, 3: 2}[s]]).all()
                n_inv += 1
                n_a += int(mask & 2 == 0)
    print(f"boundary cases: {n_inv} PMD rows invalid for a held q, A or phi ({n_a} with A held)")
    assert n_inv >= 8

    # a crafted batch: y > N; ragged rows with N = 0 columns; N = 4e9; a strand without data; MAXITER
    T = 5
    y = np.zeros((T, 32), np.uint32)
    N = np.zeros((T, 32), np.uint32)
    y[:, :30], N[:, :30] = b.y[3, :30], b.N[3, :30]
    y[0, 4] = N[0, 4] + 1  # y > N at one position
    dead = [12, 13, 14, 27, 28, 29]
    y[1, dead] = N[1, dead] = 0  # ragged: the last positions of both strands without data
    N[2, :30] = ref_golden["data_ancient__N"][0]
    y[2, :30] = ref_golden["data_ancient__y"][0]
    k = int(4.0e9 // N[2, :30].max())
    N[2, :30] *= np.uint32(k)
    y[2, :30] *= np.uint32(k)
    assert 3.9e9 < N[2, :30].max() <= 4.0e9
    y[3, 0:15] = N[3, 0:15] = 0  # the forward strand without data
    ty, tN, res = _map_fit(torch, y, N)
    before = res.out.clone()
    evid, dr, _ = _run(torch, ty, tN, res, S, T, 0)
    assert torch.equal(before.view(torch.int64), res.out.view(torch.int64))
    st = res.status.cpu().numpy()
    assert st[0] == 3 and (st[[1, 2, 4]] == 0).all(), st
    assert np.isnan(evid[0, :, :7]).all() and (evid[0, :, 7] == 0).all() and np.isnan(dr[0]).all()
    f1 = evid[1, :, ref.FLAGS].astype(int)
    assert (f1[:2] & ref.VALID).all() and np.isfinite(evid[1, 6, 0]) and np.isfinite(evid[1, 6, 4])
    # a column with N = 0 has log-pmf 0: the ragged taxon's evidence is that of its live columns
    fed = ref.evidence_taxon(oracle_lib, y[1, :30], N[1, :30], res.out[1].cpu().numpy(), 0, S, 0, seed=SEED, g=1,
                             given=(dr[1, :, :, :4], dr[1, :, :, 4]))
    for s in range(6):
        if f1[s] & ref.VALID and not fed["rows"][s]["prop"].near:
            assert abs(evid[1, s, ref.LOGZ] - float(fed["rec"][s][ref.LOGZ])) <= 10.0 * MEASURED["log_evidence"] * max(
                1, abs(evid[1, s, ref.LOGZ]))
    f2 = evid[2, :, ref.FLAGS].astype(int)
    assert (f2[:6] & ref.VALID).sum() >= 4 and np.isfinite(evid[2, 6, 0])
    for s in range(6):
        if f2[s] & ref.VALID:
            assert np.isfinite(evid[2, s, [0, 1, 3, 4, 5, 6]]).all() and evid[2, s, ref.ESS] > 1
    assert evid[2, 6, 0] > 0  # (the ancient file's deep taxon, its counts scaled up: the damage model wins)
    if st[3] == 0:  # a strand without data: its rows have every point N = 0, the likelihood is 1
        f3 = evid[3, :, ref.FLAGS].astype(int)
        print(f"forward strand without data: flags {f3}")
        for s in (2, 4):
            assert not f3[s] & ref.VALID or np.isfinite(evid[3, s, ref.LOGZ])
    ty2, tN2, r2 = _map_fit(torch, y[1:3], N[1:3], max_iter=1)
    st2 = r2.status.cpu().numpy()
    assert (st2 == 1).all(), st2  # MDFIT_MAXITER
    e2, d2, a2 = _run(torch, ty2, tN2, r2, S, 2, 3)
    assert np.isnan(e2[:, :, :7]).all() and (e2[:, :, 7] == 0).all() and np.isnan(d2).all() and np.isnan(a2).all()


class _SubRes:
    """The records of taxon t alone, as _run slices them."""

    def __init__(self, res, t):
        self.out, self.status = res.out[t:t + 1], res.status[t:t + 1]


# --------------------------------------------------------------------------
# invariance
# --------------------------------------------------------------------------
def test_record_does_not_depend_on_the_call(torch_dev, monkeypatch, batch_a):
    torch = torch_dev
    from metadamage_amd import _lib, distributed as d, engine

    b, res = batch_a["b"], batch_a["res"]
    ty, tN = batch_a["ty"][:T_A], batch_a["tN"][:T_A]
    out0, st0 = res.out.clone(), res.status.clone()

    def host(x):
        torch.cuda.synchronize()
        return x.cpu().numpy()

    for R in (0, 3):
        base = batch_a[f"evid{R}"]
        kw = {"adapt_rounds": R} if R else {}

        def call(lo, hi, index_base, seed=SEED, **more):
            got = engine.map_evidence_device(ty[lo:hi], tN[lo:hi], _sub(res, lo, hi), S_A, seed, index_base, **kw,
                                             **more)
            return got[0] if isinstance(got, tuple) else got

        # without the draws; into a buffer of garbage
        assert np.array_equal(_bits(host(call(0, T_A, 0))), _bits(base))
        junk = torch.full((T_A, _lib.NEVIDROW, _lib.NMAPEVID), 1.0e300, dtype=torch.float64, device=ty.device)
        call(0, T_A, 0, evid=junk)
        assert np.array_equal(_bits(host(junk)), _bits(base))
        # T = 1, 3 and 65
        for T in (1, 3):
            assert np.array_equal(_bits(host(call(0, T, 0))), _bits(base[:T])), T
        g65 = engine.map_evidence_device(batch_a["ty"][:65], batch_a["tN"][:65], _sub(res, 0, 65), S_A, SEED, 0, **kw)
        assert np.array_equal(_bits(host(g65[0] if isinstance(g65, tuple) else g65)[:T_A]), _bits(base))
        # two calls split at an odd taxon with index_base
        a, c, wrong = call(0, 31, 0), call(31, T_A, 31), call(31, T_A, 0)
        assert np.array_equal(_bits(host(torch.cat([a, c]))), _bits(base))
        assert not np.array_equal(_bits(host(wrong)), _bits(base[31:]))  # (the streams are the global taxon's)
        assert not np.array_equal(_bits(host(call(0, T_A, 0, seed=SEED + 1))), _bits(base))
        # a non-default stream
        s1 = torch.cuda.Stream()
        s1.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s1):
            on_s1 = call(0, T_A, 0, stream=s1)
        s1.synchronize()
        assert np.array_equal(_bits(host(on_s1)), _bits(base))
        # after a poisoning of the LDS
        _lib.check(_lib.load().mdfit_poison_lds(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        assert np.array_equal(_bits(host(call(0, T_A, 0))), _bits(base))
        # under graph capture, replayed once
        s = torch.cuda.Stream()
        dst = torch.zeros((T_A, _lib.NEVIDROW, _lib.NMAPEVID), dtype=torch.float64, device=ty.device)
        adst = torch.zeros((T_A, 3, _lib.NMAPADAPT), dtype=torch.float64, device=ty.device) if R else None
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call(0, T_A, 0, evid=dst, stream=torch.cuda.current_stream(), **({"adapt": adst} if R else {}))
        dst.fill_(0.0)
        g.replay()
        assert np.array_equal(_bits(host(dst)), _bits(base))
    # out and status are unchanged by all of it
    assert torch.equal(out0.view(torch.int64), res.out.view(torch.int64)) and torch.equal(st0, res.status)
    # through the chunked dispatch in two chunks, and into the gather record of a world of one
    opts = _lib.default_opts(mode=_lib.MODE_MAP)
    y, N, mm = b.y[:T_A], b.N[:T_A], b.mm[:T_A]
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "32")
    assert len(engine.plan_chunks(T_A, opts, with_evidence=True)) == 2
    base32 = batch_a["evid0"].astype(np.float32)
    o4, p4, s4, e4 = engine.fit_batch_host(y, N, mm, opts, evidence=True, psis_draws=S_A)
    assert e4.shape == (T_A, 7, 8) and e4.dtype == np.float32
    assert np.array_equal(e4.view(np.int32), base32.view(np.int32))
    plain3 = engine.fit_batch_host(y, N, mm, opts)
    assert len(plain3) == 3
    for x, z in zip(plain3, (o4, p4, s4)):
        assert x.dtype == z.dtype and np.array_equal(x, z, equal_nan=True)
    o5, p5, s5, e5, a5 = engine.fit_batch_host(y, N, mm, opts, evidence=True, psis_draws=S_A, psis_adapt=3)
    assert np.array_equal(e5.view(np.int32), batch_a["evid3"].astype(np.float32).view(np.int32))
    assert a5.shape == (T_A, 2) and np.array_equal(o5, o4, equal_nan=True)
    rec = d.alloc_records(T_A, torch.device("cuda", torch.cuda.current_device()), with_evidence=True)
    assert rec.buf.numel() == T_A * (d.REC_BYTES + d.REC_EVID) and rec.waic is None
    fitter = engine.ChunkedFitter(32, opts=opts, dest_on_device=True, with_evidence=True, psis_draws=S_A)
    fitter.run_into_device(y, N, mm, opts, engine.FitBatch(rec.out, rec.pred, rec.status, evid=rec.evid),
                           chunks=engine.plan_chunks(T_A, opts, chunk_taxa=32))
    buf = rec.stage()
    torch.cuda.synchronize()
    og, pg, sg, eg = d.unpack_gathered(d.gather_records(buf, T_A, 0, 1), T_A, 1, with_evidence=True)
    assert np.array_equal(eg.view(np.int32), base32.view(np.int32))
    assert np.array_equal(og, d.round_like_gather(batch_a["out"][:T_A]), equal_nan=True) and np.array_equal(sg, s4)


def test_rejections(torch_dev, batch_a):
    from metadamage_amd import _lib, engine

    ty, tN, res = batch_a["ty"], batch_a["tN"], batch_a["res"]
    for S in (24, 1025):
        with pytest.raises(_lib.MdfitError, match="num_draws"):
            engine.map_evidence_device(ty[:2], tN[:2], _sub(res, 0, 2), S)
        with pytest.raises(_lib.MdfitError, match="num_draws"):
            engine.map_evidence_device(ty[:2], tN[:2], _sub(res, 0, 2), S, adapt_rounds=2)
    for R in (-1, 5):
        with pytest.raises(_lib.MdfitError, match="adapt_rounds"):
            engine.map_evidence_device(ty[:2], tN[:2], _sub(res, 0, 2), 64, adapt_rounds=R)
    with pytest.raises(ValueError, match="MODE_MAP"):
        engine.ChunkedFitter(8, opts=_lib.default_opts(mode=_lib.MODE_NUTS), with_evidence=True)
    with pytest.raises(ValueError, match="mutually exclusive"):
        engine.ChunkedFitter(8, opts=_lib.default_opts(mode=_lib.MODE_MAP), with_evidence=True, with_waic=True)


# --------------------------------------------------------------------------
# the CLI
# --------------------------------------------------------------------------
def test_cli_map_evidence(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import fits, io
    from metadamage_amd.cli import cli_app
    from tests.test_map_evidence import NEW_COLUMNS

    def run(out_dir, *args):
        r = CliRunner().invoke(cli_app, ["fit", "--out-dir", str(out_dir), *args, str(GOLDEN / "data_ancient.txt")])
        assert r.exit_code == 0, (r.output, r.exception)
        return io.Parquet(out_dir / "fit_results" / "data_ancient.parquet")

    out_dir = tmp_path / "out"
    pq = run(out_dir, "--inference", "map-evidence", "--psis-adapt", "3")
    df = pq.load()
    assert len(df.columns) == 44 and list(df.columns[30:]) == NEW_COLUMNS + fits.ADAPT_COLUMNS
    meta = pq.load_metadata()
    assert meta["inference"] == "map-evidence" and int(meta["psis_draws"]) == 256 and int(meta["psis_adapt"]) == 3
    valid = df["map_evidence_valid"].to_numpy() == 1
    assert valid.any()
    assert np.isfinite(df.loc[valid, NEW_COLUMNS[:-2]].to_numpy()).all()
    # the ancient file's deep taxa: the damage model wins
    deep = valid & (df["D_max"].to_numpy() > 0.1)
    assert deep.any() and (df.loc[deep, "log_bf"] > 0).all() and (df.loc[deep, "damage_probability"] > 0.5).all()
    assert (df.loc[valid, "evidence_ess_min"] > 1).all() and (df.loc[valid, "log_bf_se"] >= 0).all()
    plain = run(tmp_path / "plain", "--inference", "map").load()
    assert len(plain.columns) == 30
    pd.testing.assert_frame_equal(df[plain.columns], plain)  # the 25 result columns (and the names) are the MAP call's
    pa = io.Parquet(out_dir / "fit_predictions" / "data_ancient.parquet").load()
    pb = io.Parquet(tmp_path / "plain" / "fit_predictions" / "data_ancient.parquet").load()
    pd.testing.assert_frame_equal(pa, pb)
    f = out_dir / "fit_results" / "data_ancient.parquet"
    m1 = f.stat().st_mtime_ns
    run(out_dir, "--inference", "map-evidence", "--psis-adapt", "3")  # cache hit: file untouched
    assert f.stat().st_mtime_ns == m1
    pq2 = run(out_dir, "--inference", "map-evidence")  # without rounds: the cache is not reused
    assert f.stat().st_mtime_ns != m1 and "psis_adapt" not in pq2.load_metadata()
    assert list(pq2.load().columns[30:]) == NEW_COLUMNS
