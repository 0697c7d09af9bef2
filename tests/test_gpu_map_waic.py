"""GPU tests of mdfit_map_waic (MDFIT-WAIC v1): the PMD rows
against mdfit_map_psis bit for bit, the draws, log-weights, records and
pointwise statistics against tests/map_waic_ref.py, the edge cases, the
invariance of the record under every way of calling, and the CLI path."""

from __future__ import annotations

import ctypes

import numpy as np
import pandas as pd
import pytest

from tests import map_psis_ref as pref
from tests import map_waic_ref as ref
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

S_A = 256
T_A = 64
SEED = 0
# measured on the MI355X over the first 64 taxa of generate(300, 21) at S = 256
# and the first 8 at S = 25, 65 and 1024 (the worst of the four runs; DESIGN.md
# §3.9), asserted at ten times it.  u and lw of the null rows: against the
# reference's own draws (absolute over max(1, |u|)) and against its log p - log
# g at the kernel's u (absolute over max(1, |lw|)).  Everything else against the
# reference fed the kernel's u and lw: lppd_i absolute over max(1, |lppd_i|),
# p_i relative, the row's sums relative, khat absolute, the comparisons of row
# 6 absolute over max(1, |.|).
# (378 + 3 x 48 rows compared, none left out.  lppd_i and p_i carry the 1e-12-sized
# differences between the device's and the oracle's log-pmf, p_i relative to a
# variance of a few 1e-2; the accumulation itself is 1e-15, test_map_waic.py.)
MEASURED = {"u": 3.86e-12, "lw": 5.10e-12, "lppd_i": 2.33e-12, "p_i": 7.00e-11, "elpd_waic": 2.15e-13,
            "p_waic": 3.79e-12, "lppd": 1.98e-13, "khat": 9.89e-15, "ess": 1.08e-14, "p_waic_max": 9.05e-12,
            "compare": 2.04e-11}


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


def _run(torch, ty, tN, res, S, T=None, seed=SEED, base=0):
    """mdfit_map_waic with pointwise and draws on the first T taxa -> host arrays."""
    from metadamage_amd import engine

    T = int(ty.shape[0]) if T is None else T
    sub = engine.FitBatch(res.out[:T], None, res.status[:T], None)
    waic, pw, dr = engine.map_waic_device(ty[:T], tN[:T], sub, S, seed, base, pointwise=True, draws=True)
    torch.cuda.synchronize()
    return waic.cpu().numpy(), pw.cpu().numpy(), dr.cpu().numpy()


@pytest.fixture(scope="module")
def batch_a(torch_dev):
    """generate(300, seed=21) fitted by one MAP call; mdfit_map_waic on its
    first 64 taxa at S = 256 with the pointwise values and the draws (computed
    once, read only)."""
    from metadamage_amd.synthetic import generate

    torch = torch_dev
    b = generate(300, seed=21)
    ty, tN, res = _map_fit(torch, b.y, b.N, b.mm)
    before = (res.out.clone(), res.pred.clone(), res.status.clone())
    waic, pw, dr = _run(torch, ty, tN, res, S_A, T_A)
    # out, pred and status are read only
    assert torch.equal(before[0].view(torch.int64), res.out.view(torch.int64))
    assert torch.equal(before[1].view(torch.int32), res.pred.view(torch.int32)) and torch.equal(before[2], res.status)
    host = {"b": b, "out": res.out.cpu().numpy(), "st": res.status.cpu().numpy(), "waic": waic, "pw": pw, "draws": dr}
    for a in host.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    host.update(ty=ty, tN=tN, res=res)
    return host


# --------------------------------------------------------------------------
# the PMD rows are mdfit_map_psis's
# --------------------------------------------------------------------------
def test_pmd_rows_are_map_psis_bit_for_bit(torch_dev, batch_a):
    from metadamage_amd import engine

    torch = torch_dev
    ty, tN, res = batch_a["ty"], batch_a["tN"], batch_a["res"]
    sub = engine.FitBatch(res.out[:T_A], None, res.status[:T_A], None)
    psis, pdr = engine.map_psis_device(ty[:T_A], tN[:T_A], sub, S_A, SEED, 0, draws=True)
    torch.cuda.synchronize()
    psis, pdr = psis.cpu().numpy(), pdr.cpu().numpy()
    waic, dr = batch_a["waic"], batch_a["draws"]
    n_valid = 0
    for r, s in enumerate((0, 2, 3)):
        for name, fp, fw in (("khat", pref.KHAT, ref.KHAT), ("ess", pref.ESS, ref.ESS), ("n_inf", pref.N_INF, ref.N_INF)):
            assert np.array_equal(_bits(psis[:, r, fp]), _bits(waic[:, s, fw])), (name, s)
        assert np.array_equal(psis[:, r, pref.FLAGS], waic[:, s, ref.FLAGS]), s  # valid, reliable, the free bits
        assert np.array_equal(_bits(pdr[:, r]), _bits(dr[:, s])), s  # u, lw, w
        n_valid += int((psis[:, r, pref.FLAGS].astype(int) & 1).sum())
    assert n_valid >= 170  # of 192


# --------------------------------------------------------------------------
# against the reference
# --------------------------------------------------------------------------
def _rel(a, b):
    return float(abs(a - b) / abs(b)) if b != 0 else float(abs(a))


def _compare_with_reference(oracle_lib, b, out, st, waic, pw, dr, S, T, worst):
    """Every taxon t < T: flags and NaN pattern equal, errors into `worst`.
    Returns (rows compared, rows left out as too close to a decision)."""
    tau = pref.khat_threshold(S)
    compared = excluded = 0
    for t in range(T):
        y30, N30 = b.y[t, :30], b.N[t, :30]
        own = ref.waic_taxon(oracle_lib, y30, N30, out[t], int(st[t]), S, seed=SEED, g=t)
        if st[t] != 0:
            assert np.isnan(waic[t, :, :7]).all() and (waic[t, :, 7] == 0).all()
            assert np.isnan(pw[t]).all() and np.isnan(dr[t]).all()
            continue
        fed = ref.waic_taxon(oracle_lib, y30, N30, out[t], 0, S, seed=SEED, g=t, given=(dr[t, :, :, :4], dr[t, :, :, 4]))
        near = False
        for s in range(6):
            got, want, info = waic[t, s], fed["rec"][s], fed["rows"][s]
            prop = info["prop"]
            if prop.near:  # a held/free decision within 1e-6 of its threshold: not the data's
                near = True
                excluded += 1
                continue
            assert (int(got[ref.FLAGS]) >> 2) & 15 == prop.mask, (t, s, got[ref.FLAGS], prop.mask)
            if not int(want[ref.FLAGS]) & ref.VALID:
                assert int(got[ref.FLAGS]) == prop.mask << 2 and np.isnan(got[:7]).all(), (t, s, got)
                assert np.isnan(pw[t, s]).all() and np.isnan(dr[t, s, :, 5]).all()
                if not prop.valid:
                    assert np.isnan(dr[t, s]).all()
                continue
            khat_ref = float(want[ref.KHAT])
            if np.isfinite(khat_ref) and abs(khat_ref - tau) <= 1e-6:
                near = True
                excluded += 1
                continue
            compared += 1
            assert int(got[ref.FLAGS]) == int(want[ref.FLAGS]), (t, s, got, want)
            ku, klw, kw = dr[t, s, :, :4], dr[t, s, :, 4], dr[t, s, :, 5]
            if not ref.ROWS[s][0]:  # a null row: the draws and the log-weights (the PMD rows are map_psis's)
                assert (ku[:, 1] == 0).all() and (ku[:, 2] == 0).all()
                ou = own["rows"][s]["u"]
                worst["u"] = max(worst["u"], float((np.abs(ku - ou) / np.maximum(1, np.abs(ou))).max()))
                lw_ref = ref.log_target(oracle_lib, y30, N30, s, ku) - prop.log_g_at(ku)
                assert np.isfinite(klw).all() and got[ref.N_INF] == 0
                worst["lw"] = max(worst["lw"], float((np.abs(klw - lw_ref) / np.maximum(1, np.abs(lw_ref))).max()))
            assert abs(kw.sum() - 1.0) < 1e-12 and got[ref.N_INF] == float(want[ref.N_INF])
            cols = list(ref.columns(s))
            inside = np.zeros(30, bool)
            inside[cols] = True
            assert np.isnan(pw[t, s, ~inside]).all() and np.isfinite(pw[t, s, inside]).all()
            wl, wp = fed["pointwise"][s, cols, 0], fed["pointwise"][s, cols, 1]
            gl, gp = pw[t, s, cols, 0], pw[t, s, cols, 1]
            worst["lppd_i"] = max(worst["lppd_i"], float((np.abs(gl - wl) / np.maximum(1, np.abs(wl))).max()))
            zero = wp == 0
            assert (gp[zero] == 0).all() and (gl[zero] == wl[zero]).all()
            if (~zero).any():
                worst["p_i"] = max(worst["p_i"], float((np.abs(gp[~zero] - wp[~zero]) / np.abs(wp[~zero])).max()))
            for name, j in (("elpd_waic", ref.ELPD), ("p_waic", ref.PWAIC), ("lppd", ref.LPPD), ("ess", ref.ESS),
                            ("p_waic_max", ref.PMAX)):
                worst[name] = max(worst[name], _rel(got[j], want[j]))
            if np.isfinite(khat_ref):
                worst["khat"] = max(worst["khat"], float(abs(got[ref.KHAT] - want[ref.KHAT])))
            else:
                assert got[ref.KHAT] == khat_ref
        if near:
            continue
        g6, w6 = waic[t, 6], fed["rec"][6]
        assert int(g6[ref.FLAGS]) == int(w6[ref.FLAGS]) and g6[6] == 0.0, (t, g6, w6)
        for j in range(6):
            assert np.isnan(g6[j]) == np.isnan(float(w6[j])), (t, j, g6, w6)
            if not np.isnan(g6[j]):
                worst["compare"] = max(worst["compare"], float(abs(g6[j] - w6[j]) / max(1, abs(w6[j]))))
    return compared, excluded


def _assert_worst(worst):
    for name, v in worst.items():
        assert v <= 10.0 * MEASURED[name], (name, v)


def test_batch_a_vs_reference(batch_a, oracle_lib):
    worst = dict.fromkeys(MEASURED, 0.0)
    compared, excluded = _compare_with_reference(oracle_lib, batch_a["b"], batch_a["out"], batch_a["st"],
                                                 batch_a["waic"], batch_a["pw"], batch_a["draws"], S_A, T_A, worst)
    print(f"S = {S_A}, {T_A} taxa: {compared} rows compared, {excluded} left out; worst error: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert compared >= 340 and excluded <= 4  # of 384
    _assert_worst(worst)


@pytest.mark.parametrize("S", (25, 65, 1024))
def test_other_draw_counts_vs_reference(torch_dev, batch_a, oracle_lib, S):
    """A five-draw tail, one full trip plus one draw, and the largest LDS."""
    T = 8
    waic, pw, dr = _run(torch_dev, batch_a["ty"], batch_a["tN"], batch_a["res"], S, T)
    worst = dict.fromkeys(MEASURED, 0.0)
    compared, excluded = _compare_with_reference(oracle_lib, batch_a["b"], batch_a["out"], batch_a["st"], waic, pw, dr,
                                                 S, T, worst)
    print(f"S = {S}, {T} taxa: {compared} rows compared, {excluded} left out; worst error: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert compared >= 36  # of 48
    _assert_worst(worst)


# --------------------------------------------------------------------------
# edges
# --------------------------------------------------------------------------
def test_edges(torch_dev, batch_a, oracle_lib, ref_golden):
    from metadamage_amd import engine

    torch = torch_dev
    b = batch_a["b"]
    S = 64
    # the whole batch at S = 64: where a null row is invalid, and where a PMD c is held on 0
    sub = engine.FitBatch(batch_a["res"].out, None, batch_a["res"].status, None)
    full = engine.map_waic_device(batch_a["ty"], batch_a["tN"], sub, S, SEED, 0)
    torch.cuda.synchronize()
    full = full.cpu().numpy()
    fl = full[:, :, ref.FLAGS].astype(int)
    fitted = np.flatnonzero(batch_a["st"] == 0)
    assert fitted.size >= 295 and 18 in fitted
    bad_null = [(t, s) for t in fitted for s in (1, 4, 5) if not fl[t, s] & ref.VALID]
    print(f"invalid null rows: {bad_null}")
    # (the oracle and the device: 6 rows in the 5 taxa 18, 19, 25, 92 and 193)
    assert bad_null and len(bad_null) <= 12 and len({t for t, _ in bad_null}) >= 3
    assert any(t == 18 for t, _ in bad_null)
    for t, s in bad_null:
        assert s in (4, 5) and (fl[t, s] >> 2) & 8 == 0, (t, s, fl[t, s])  # delta is held; never the all-position null
        assert np.isnan(full[t, s, :7]).all() and np.isnan(full[t, 6, 1 if s == 4 else 2])
        assert not fl[t, 6] & ref.VALID and not fl[t, 6] & ref.RELIABLE
        if fl[t, 0] & fl[t, 1] & ref.VALID:
            assert np.isfinite(full[t, 6, 0])  # n_sigma_waic needs rows 0 and 1 only
    held = [(t, s) for t in fitted for s in (0, 2, 3) if fl[t, s] & ref.VALID and not (fl[t, s] >> 2) & 4]
    print(f"c held on 0 in {len(held)} valid PMD rows")
    assert len(held) >= 5
    for t, s in held:
        # (khat may be +inf -- the tail's first-quartile excess 0 under many infeasible draws -- in a valid row)
        others = [j for j in range(7) if j != ref.KHAT]
        assert np.isfinite(full[t, s, others]).all() and not np.isnan(full[t, s, ref.KHAT]) and full[t, s, ref.PWAIC] > 0
    # the null rows' free bits are those of q and delta alone
    assert ((fl[:, [1, 4, 5]] >> 2) & 6 == 0).all() and ((fl[fitted][:, [1, 4, 5]] >> 2) & 9 != 0).any()
    # taxon 18 and the first held-c taxon against the reference: flags and the NaN pattern
    t_held = held[0][0]
    for t in (18, t_held):
        want = ref.waic_taxon(oracle_lib, b.y[t, :30], b.N[t, :30], batch_a["out"][t], 0, S, seed=SEED, g=t)
        if any(r["prop"].near for r in want["rows"]):
            continue
        w = want["rec"].astype(float)
        assert np.array_equal(np.isnan(full[t]), np.isnan(w)), (t, full[t], w)
        assert np.array_equal(fl[t, :6] >> 2, w[:6, ref.FLAGS].astype(int) >> 2) and (fl[t] & 1 == w[:, 7].astype(int) & 1).all()

    # a crafted batch: y > N; ragged rows with N = 0 columns; N = 4e9
    T = 4
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
    y[3, 15:30] = N[3, 15:30] = 0  # the reverse strand without data
    ty, tN, res = _map_fit(torch, y, N)
    before = res.out.clone()
    waic, pw, dr = _run(torch, ty, tN, res, S, T)
    assert torch.equal(before.view(torch.int64), res.out.view(torch.int64))
    st = res.status.cpu().numpy()
    assert st[0] == 3 and (st[1:] == 0).all(), st
    assert np.isnan(waic[0, :, :7]).all() and (waic[0, :, 7] == 0).all() and np.isnan(pw[0]).all() and np.isnan(dr[0]).all()
    f1 = waic[1, :, ref.FLAGS].astype(int)
    for s in range(6):
        cols = list(ref.columns(s))
        if f1[s] & ref.VALID:
            inside = [c for c in dead if c in cols]
            assert (pw[1, s, inside] == 0.0).all(), (s, pw[1, s, inside])  # lppd_i = p_i = 0 exactly
            live = [c for c in cols if c not in dead]
            assert (pw[1, s, live, 0] < 0).all() and (pw[1, s, live, 1] > 0).all()
    assert (f1[:2] & ref.VALID).all() and np.isfinite(waic[1, 6, 0])
    f2 = waic[2, :, ref.FLAGS].astype(int)
    assert (f2[:6] & ref.VALID).sum() >= 4 and np.isfinite(waic[2, 6, 0])
    for s in range(6):
        if f2[s] & ref.VALID:
            others = [j for j in range(7) if j != ref.KHAT]
            assert np.isfinite(waic[2, s, others]).all() and waic[2, s, ref.PWAIC] > 0 and waic[2, s, ref.ESS] > 1
    # N = 4e9 against the reference fed the kernel's draws: the device's pointwise log-pmf is pinned to 1e-9 of
    # max(1, |l|) against the oracle's up to N = 4e9 (test_gpu_parity.py), and lppd_i is a weighted log-mean-exp
    # of those values -- its error is at most the largest of theirs
    fed = ref.waic_taxon(oracle_lib, y[2, :30], N[2, :30], res.out[2].cpu().numpy(), 0, S, seed=SEED, g=2,
                         given=(dr[2, :, :, :4], dr[2, :, :, 4]))
    for s in range(6):
        if f2[s] & ref.VALID and int(fed["rec"][s, ref.FLAGS]) & ref.VALID:
            cols = list(ref.columns(s))
            wl = fed["pointwise"][s, cols, 0]
            e = float((np.abs(pw[2, s, cols, 0] - wl) / np.maximum(1, np.abs(wl))).max())
            print(f"N = 4e9, row {s}: max |lppd_i - ref| / max(1, |lppd_i|) {e:.2e}")
            assert e <= 1e-9
    # a strand without data: its rows have every point N = 0
    f3 = waic[3, :, ref.FLAGS].astype(int)
    for s in (3, 5):
        if f3[s] & ref.VALID:
            assert (pw[3, s, 15:30] == 0.0).all() and waic[3, s, ref.ELPD] == 0.0


# --------------------------------------------------------------------------
# invariance
# --------------------------------------------------------------------------
def test_record_does_not_depend_on_the_call(torch_dev, monkeypatch, batch_a):
    torch = torch_dev
    from metadamage_amd import _lib, distributed as d, engine

    b, ty, tN, res = batch_a["b"], batch_a["ty"], batch_a["tN"], batch_a["res"]
    ty, tN = ty[:T_A], tN[:T_A]
    base = batch_a["waic"]
    out0, st0 = res.out.clone(), res.status.clone()

    def sub(lo, hi):
        return engine.FitBatch(res.out[lo:hi], None, res.status[lo:hi], None)

    def host(x):
        torch.cuda.synchronize()
        return x.cpu().numpy()

    # without the taps, with one of them
    assert np.array_equal(_bits(host(engine.map_waic_device(ty, tN, sub(0, T_A), S_A, SEED, 0))), _bits(base))
    w1, p1 = engine.map_waic_device(ty, tN, sub(0, T_A), S_A, SEED, 0, pointwise=True)
    assert np.array_equal(_bits(host(w1)), _bits(base))
    assert np.array_equal(_bits(host(p1)), _bits(batch_a["pw"]))
    w2, d2 = engine.map_waic_device(ty, tN, sub(0, T_A), S_A, SEED, 0, draws=True)
    assert np.array_equal(_bits(host(w2)), _bits(base)) and np.array_equal(_bits(host(d2)), _bits(batch_a["draws"]))
    # T = 1, 3 (and 64 above; 65 below): the first taxa of the batch
    for T in (1, 3):
        got = host(engine.map_waic_device(ty[:T], tN[:T], sub(0, T), S_A, SEED, 0))
        assert np.array_equal(_bits(got), _bits(base[:T])), T
    ty65, tN65 = batch_a["ty"][:65], batch_a["tN"][:65]
    got65 = host(engine.map_waic_device(ty65, tN65, sub(0, 65), S_A, SEED, 0))
    assert np.array_equal(_bits(got65[:T_A]), _bits(base))
    # two calls split with index_base
    a = engine.map_waic_device(ty[:30], tN[:30], sub(0, 30), S_A, SEED, 0)
    c = engine.map_waic_device(ty[30:], tN[30:], sub(30, T_A), S_A, SEED, 30)
    wrong = engine.map_waic_device(ty[30:], tN[30:], sub(30, T_A), S_A, SEED, 0)
    assert np.array_equal(_bits(host(torch.cat([a, c]))), _bits(base))
    assert not np.array_equal(_bits(host(wrong)), _bits(base[30:]))  # (the streams are the global taxon's)
    other = host(engine.map_waic_device(ty, tN, sub(0, T_A), S_A, SEED + 1, 0))
    assert not np.array_equal(_bits(other), _bits(base))
    # after a poisoning of the LDS
    _lib.check(_lib.load().mdfit_poison_lds(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert np.array_equal(_bits(host(engine.map_waic_device(ty, tN, sub(0, T_A), S_A, SEED, 0))), _bits(base))
    # under graph capture and replay
    s = torch.cuda.Stream()
    dst = torch.zeros((T_A, _lib.NWAICROW, _lib.NMAPWAIC), dtype=torch.float64, device=ty.device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        engine.map_waic_device(ty, tN, sub(0, T_A), S_A, SEED, 0, waic=dst, stream=torch.cuda.current_stream())
    for _ in range(2):
        dst.fill_(0.0)
        g.replay()
        assert np.array_equal(_bits(host(dst)), _bits(base))
    # out and status are unchanged by all of it
    assert torch.equal(out0.view(torch.int64), res.out.view(torch.int64)) and torch.equal(st0, res.status)
    # through the chunked dispatch in two chunks, and into the gather record of a world of one
    opts = _lib.default_opts(mode=_lib.MODE_MAP)
    base32 = base.astype(np.float32)
    y, N, mm = b.y[:T_A], b.N[:T_A], b.mm[:T_A]
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "32")
    assert len(engine.plan_chunks(T_A, opts, with_waic=True)) == 2
    o4, p4, s4, w4 = engine.fit_batch_host(y, N, mm, opts, waic=True, psis_draws=S_A)
    assert w4.shape == (T_A, 7, 8) and w4.dtype == np.float32
    assert np.array_equal(w4.view(np.int32), base32.view(np.int32))
    plain3 = engine.fit_batch_host(y, N, mm, opts)
    assert len(plain3) == 3
    for x, z in zip(plain3, (o4, p4, s4)):
        assert x.dtype == z.dtype and np.array_equal(x, z, equal_nan=True)
    rec = d.alloc_records(T_A, torch.device("cuda", torch.cuda.current_device()), with_waic=True)
    assert rec.buf.numel() == T_A * (d.REC_BYTES + d.REC_WAIC)
    fitter = engine.ChunkedFitter(32, opts=opts, dest_on_device=True, with_waic=True, psis_draws=S_A)
    fitter.run_into_device(y, N, mm, opts, engine.FitBatch(rec.out, rec.pred, rec.status, waic=rec.waic),
                           chunks=engine.plan_chunks(T_A, opts, chunk_taxa=32))
    buf = rec.stage()
    torch.cuda.synchronize()
    og, pg, sg, wg = d.unpack_gathered(d.gather_records(buf, T_A, 0, 1), T_A, 1, with_waic=True)
    assert np.array_equal(wg.view(np.int32), base32.view(np.int32))
    assert np.array_equal(og, d.round_like_gather(batch_a["out"][:T_A]), equal_nan=True) and np.array_equal(sg, s4)
    assert np.array_equal(pg, p4, equal_nan=True)


def test_rejections(torch_dev, batch_a):
    from metadamage_amd import _lib, engine

    ty, tN, res = batch_a["ty"], batch_a["tN"], batch_a["res"]
    for S in (24, 1025):
        with pytest.raises(_lib.MdfitError, match="num_draws"):
            engine.map_waic_device(ty[:2], tN[:2], engine.FitBatch(res.out[:2], None, res.status[:2], None), S)
    with pytest.raises(ValueError, match="MODE_MAP"):
        engine.ChunkedFitter(8, opts=_lib.default_opts(mode=_lib.MODE_NUTS), with_waic=True)
    with pytest.raises(ValueError, match="mutually exclusive"):
        engine.ChunkedFitter(8, opts=_lib.default_opts(mode=_lib.MODE_MAP), with_waic=True, with_psis=True)


# --------------------------------------------------------------------------
# the CLI
# --------------------------------------------------------------------------
def test_cli_map_waic(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import io
    from metadamage_amd.cli import cli_app
    from tests.test_map_waic import NEW_COLUMNS

    def run(out_dir, *args):
        r = CliRunner().invoke(cli_app, ["fit", "--out-dir", str(out_dir), *args, str(GOLDEN / "data_ancient.txt")])
        assert r.exit_code == 0, (r.output, r.exception)
        return io.Parquet(out_dir / "fit_results" / "data_ancient.parquet")

    out_dir = tmp_path / "out"
    pq = run(out_dir, "--inference", "map-waic")
    df = pq.load()
    assert len(df.columns) == 42 and list(df.columns[30:]) == NEW_COLUMNS
    meta = pq.load_metadata()
    assert meta["inference"] == "map-waic" and int(meta["psis_draws"]) == 256
    valid = df["map_waic_valid"].to_numpy() == 1
    assert valid.any()
    assert np.isfinite(df.loc[valid, NEW_COLUMNS[:-2]].to_numpy()).all()
    assert (df.loc[valid, "p_waic"] > 0).all() and (df.loc[valid, "waic_ess_min"] > 1).all()
    plain = run(tmp_path / "plain", "--inference", "map").load()
    assert len(plain.columns) == 30
    pd.testing.assert_frame_equal(df[plain.columns], plain)  # the 25 result columns (and the names) are the MAP call's
    pa = io.Parquet(out_dir / "fit_predictions" / "data_ancient.parquet").load()
    pb = io.Parquet(tmp_path / "plain" / "fit_predictions" / "data_ancient.parquet").load()
    pd.testing.assert_frame_equal(pa, pb)
    f = out_dir / "fit_results" / "data_ancient.parquet"
    m1 = f.stat().st_mtime_ns
    run(out_dir, "--inference", "map-waic")  # cache hit: file untouched
    assert f.stat().st_mtime_ns == m1
    pq2 = run(out_dir, "--inference", "map-waic", "--psis-draws", "64")  # other draws: the cache is not reused
    assert f.stat().st_mtime_ns != m1 and int(pq2.load_metadata()["psis_draws"]) == 64
    assert not np.array_equal(pq2.load()["n_sigma_waic"].to_numpy(), df["n_sigma_waic"].to_numpy())
