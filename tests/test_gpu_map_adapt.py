"""GPU tests of mdfit_map_psis_adapt, mdfit_map_waic_adapt and
mdfit_adapt_proposal (MDFIT-ADAPT v1): adapt_rounds = 0 against
the v1 entries, the rounds' decisions, draws and records against
tests/map_adapt_ref.py, the refit on crafted series, the agreement of the two
entries, the invariance of the records under every way of calling, and the auto
call with adapted proposals."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import map_adapt_cases as cases
from tests import map_adapt_ref as ad
from tests import map_psis_ref as ref

pytestmark = pytest.mark.gpu

S_A, R_A, SEED, T_A = 256, 3, 0, 64
# The worst errors measured on the MI355X over the four shapes of
# test_rounds_vs_reference, asserted at ten times them: the
# best round's u against the reference's own draws (absolute over max(1, |u|)),
# its raw log-weight against the reference's log p - log g at the kernel's u
# (absolute over max(1, |lw|)), each statistic against the reference fed the
# kernel's u and lw (relative; khat absolute), khat and ess of round 0 in the
# adapt record against the reference fed the round-0 draws of the adapt_rounds =
# 0 call.  u and lw of a later round inherit the refit's agreement with the
# reference (the crafted series below) times the offsets of a heavy-tailed draw;
# the worst u and lw are S = 25's, where 25 weights fix a 4 x 4 covariance.
E2E_MEASURED = {"u": 1.24e-9, "lw": 4.21e-11, "mean": 7.85e-16, "std": 1.41e-15, "rho_Ac": 2.46e-12,
                "significance": 1.34e-15, "khat": 1.44e-15, "ess": 3.53e-15, "khat0": 9.89e-15, "ess0": 1.08e-14}
# mdfit_adapt_proposal against the reference on the crafted series, measured likewise
PROPOSAL_MEASURED = {"m": 3.61e-16, "d": 1.92e-16, "F": 2.81e-13, "gc": 2.31e-16}


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    return torch


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _np(*ts):
    return tuple(t.cpu().numpy() for t in ts)


@pytest.fixture(scope="module")
def batch(torch_dev):
    """The first 64 taxa of generate(300, seed=21) fitted by one MAP call; the
    v1 records, the adapt_rounds = 0 records and the R = 3 records of both
    entries at S = 256, each with its draws (computed once, read only)."""
    from metadamage_amd import _lib, engine
    from metadamage_amd.synthetic import generate

    torch = torch_dev
    b = generate(300, seed=21)
    y, N, mm = b.y[:T_A], b.N[:T_A], b.mm[:T_A]
    ty, tN, tm = engine.to_device_counts(y, N, mm)
    res = engine.fit_batch_device(ty, tN, tm, _lib.default_opts(mode=_lib.MODE_MAP))
    torch.cuda.synchronize()
    h = {"y": y, "N": N, "mm": mm, "out": res.out.cpu().numpy(), "st": res.status.cpu().numpy()}
    h["v1_psis"], h["v1_draws"] = _np(*engine.map_psis_device(ty, tN, res, S_A, SEED, 0, draws=True))
    h["v1_waic"], h["v1_pw"], h["v1_wdraws"] = _np(*engine.map_waic_device(ty, tN, res, S_A, SEED, 0, pointwise=True,
                                                                           draws=True))
    h["p0"], h["p0_draws"], h["p0_adapt"] = _np(*engine.map_psis_device(ty, tN, res, S_A, SEED, 0, draws=True,
                                                                        adapt=True))
    h["w0"], h["w0_pw"], h["w0_draws"], h["w0_adapt"] = _np(*engine.map_waic_device(
        ty, tN, res, S_A, SEED, 0, pointwise=True, draws=True, adapt=True))
    h["p3"], h["p3_draws"], h["p3_adapt"] = _np(*engine.map_psis_device(ty, tN, res, S_A, SEED, 0, draws=True,
                                                                        adapt_rounds=R_A))
    h["w3"], h["w3_pw"], h["w3_draws"], h["w3_adapt"] = _np(*engine.map_waic_device(
        ty, tN, res, S_A, SEED, 0, pointwise=True, draws=True, adapt_rounds=R_A))
    torch.cuda.synchronize()
    for k, a in h.items():
        if k not in ("y", "N", "mm"):  # (the counts go back to the device: torch wants them writable)
            a.setflags(write=False)
    h.update(ty=ty, tN=tN, tm=tm, res=res)
    return h


# --------------------------------------------------------------------------
# 5. adapt_rounds = 0 is v1
# --------------------------------------------------------------------------
def test_zero_rounds_is_v1(batch):
    h = batch
    assert np.array_equal(_bits(h["p0"]), _bits(h["v1_psis"])) and np.array_equal(_bits(h["p0_draws"]),
                                                                                  _bits(h["v1_draws"]))
    assert np.array_equal(_bits(h["w0"]), _bits(h["v1_waic"])) and np.array_equal(_bits(h["w0_pw"]), _bits(h["v1_pw"]))
    assert np.array_equal(_bits(h["w0_draws"]), _bits(h["v1_wdraws"]))
    valid = (h["v1_psis"][:, :, ref.FLAGS].astype(int) & ref.VALID) != 0
    assert valid.sum() >= 180
    for a in (h["p0_adapt"], h["w0_adapt"]):
        assert a.shape == (T_A, 3, 4) and np.isnan(a[~valid]).all()
        assert np.array_equal(_bits(a[valid][:, 0]), _bits(h["v1_psis"][valid][:, ref.KHAT]))
        assert np.array_equal(_bits(a[valid][:, 1]), _bits(h["v1_psis"][valid][:, ref.ESS]))
        assert (a[valid][:, 2:] == 0).all()
    assert not (h["p0"][:, :, ref.FLAGS].astype(int) & ad.ADAPTED).any()


# --------------------------------------------------------------------------
# 6. against the reference
# --------------------------------------------------------------------------
def _compare(h, T, S, R, oracle_lib, worst, checks):
    """Rows of the first T taxa: the kernel's R-round records (psis, draws,
    adapt) and round-0 draws against the reference.  -> (compared, left out,
    best rounds seen)."""
    tau = ref.khat_threshold(S)
    psis, draws, adapt, draws0 = h["p3"], h["p3_draws"], h["p3_adapt"], h["p0_draws"]
    compared = excluded = ref_near = 0
    seen = set()
    for t in range(T):
        rows = ad.adapt_taxon(oracle_lib, h["y"][t, :30], h["N"][t, :30], h["out"][t], int(h["st"][t]), S, R,
                              seed=SEED, g=t)
        for r, res in enumerate(rows):
            got, ga = psis[t, r], adapt[t, r]
            prop = res["prop"]
            if h["st"][t] != 0:
                assert got[ref.FLAGS] == 0 and np.isnan(got[:15]).all() and np.isnan(ga).all()
                continue
            if prop.near:  # a held/free decision within 1e-6 of its threshold: not the data's
                excluded += 1
                continue
            assert (int(got[ref.FLAGS]) >> 2) & 15 == prop.mask, (t, r)
            if not prop.valid or not res["rounds"][0]["ok"]:
                assert int(got[ref.FLAGS]) == prop.mask << 2 and np.isnan(got[:15]).all() and np.isnan(ga).all(), (t, r)
                continue
            if res["margin"] <= 1e-6:  # a khat decision of the reference within 1e-6
                excluded += 1
                ref_near += 1
                continue
            compared += 1
            best = res["best"]
            seen.add(res["best_round"])
            # the decisions
            assert ga[2] == res["best_round"] and ga[3] == res["tried"], (t, r, ga, res["best_round"], res["tried"])
            assert int(got[ref.FLAGS]) == int(res["rec"][ref.FLAGS]), (t, r, got[ref.FLAGS], res["rec"][ref.FLAGS])
            assert got[ref.N_INF] == best["n_inf"], (t, r)
            ku, klw, kw = draws[t, r, :, :4], draws[t, r, :, 4], draws[t, r, :, 5]
            # the best round's draws against the reference's own
            e = float((np.abs(ku - best["u"]) / np.maximum(1, np.abs(best["u"]))).max())
            worst["u"] = max(worst["u"], e)
            checks.append(("u", e, t, r, "u"))
            # its raw log-weights against log p - log g at the kernel's u
            lw_ref = ref.log_target(oracle_lib, h["y"][t, :30], h["N"][t, :30], r, ku) - best["prop"].log_g_at(ku)
            inf = np.isneginf(lw_ref.astype(float))
            assert np.array_equal(np.isneginf(klw), inf), (t, r)
            e = float((np.abs(klw[~inf] - lw_ref[~inf]) / np.maximum(1, np.abs(lw_ref[~inf]))).max())
            worst["lw"] = max(worst["lw"], e)
            checks.append(("lw", e, t, r, "lw"))
            # the record against the reference fed the kernel's u and lw
            want, _ = ref.record_from(prop, ku, klw, S)
            assert int(want[ref.FLAGS]) & ref.VALID
            assert abs(kw.sum() - 1.0) < 1e-12 and (kw[inf] == 0).all()
            for j, name in enumerate(ref.FIELDS[:14]):
                a, w_ = got[j], float(want[j])
                key = "mean" if j < 5 else ("std" if j < 10 else name)
                assert np.isnan(a) == np.isnan(w_), (t, r, name, a, w_)
                if np.isnan(w_) or np.isinf(w_):
                    assert np.isnan(w_) or a == w_
                    continue
                e = abs(a - want[j]) if name == "khat" else (abs(a) if w_ == 0.0 else abs(a - want[j]) / abs(want[j]))
                worst[key] = max(worst[key], float(e))
                checks.append((key, float(e), t, r, name))
            # round 0 in the adapt record against the reference fed the round-0 draws
            w0, k0, _, ok0 = ref.psis_weights(draws0[t, r, :, 4])
            assert ok0
            for key, a, w_ in (("khat0", ga[0], k0), ("ess0", ga[1], 1 / (w0 * w0).sum())):
                if np.isinf(float(w_)):
                    assert a == float(w_)
                    continue
                e = float(abs(a - w_)) if key == "khat0" else float(abs(a - w_) / w_)
                worst[key] = max(worst[key], e)
                checks.append((key, e, t, r, key))
    return compared, excluded, ref_near, seen


def _assert_tolerances(worst, checks):
    for key, e, t, r, name in checks:
        assert e <= 10.0 * E2E_MEASURED[key], (key, e, t, r, name)
    # a final-u error above 1e-6 would be a finding to explain, not a tolerance to set
    assert worst["u"] <= 1e-6


def test_rounds_vs_reference(batch, oracle_lib):
    worst = dict.fromkeys(E2E_MEASURED, 0.0)
    checks = []
    compared, excluded, ref_near, seen = _compare(batch, T_A, S_A, R_A, oracle_lib, worst, checks)
    print(f"T = {T_A}, S = {S_A}: {compared} rows compared, {excluded} left out; best rounds {sorted(seen)}; worst "
          "error: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert ref_near == 0 and excluded <= 0.02 * 3 * T_A and compared >= 180
    assert seen == {0, 1, 2, 3}  # every way out of the loop is taken
    p3 = batch["p3"]
    over0 = int((batch["p3_adapt"][:, :, 0] > ref.khat_threshold(S_A)).sum())
    over1 = int(((p3[:, :, ref.FLAGS].astype(int) & 3) == 1).sum())
    print(f"rows over tau: {over0} -> {over1}")
    assert over0 == 37 and over1 == 6  # (the reference's counts on these taxa)
    _assert_tolerances(worst, checks)


@pytest.mark.parametrize("S", (25, 65, 1024))
def test_rounds_vs_reference_other_draws(torch_dev, batch, oracle_lib, S):
    from metadamage_amd import engine

    T = 8
    ty, tN, res = batch["ty"][:T], batch["tN"][:T], batch["res"]
    sub = engine.FitBatch(res.out[:T], None, res.status[:T], None)
    h = {k: batch[k] for k in ("y", "N", "out", "st")}
    h["p3"], h["p3_draws"], h["p3_adapt"] = _np(*engine.map_psis_device(ty, tN, sub, S, SEED, 0, draws=True,
                                                                        adapt_rounds=R_A))
    _, h["p0_draws"], _ = _np(*engine.map_psis_device(ty, tN, sub, S, SEED, 0, draws=True, adapt=True))
    worst = dict.fromkeys(E2E_MEASURED, 0.0)
    checks = []
    compared, excluded, ref_near, seen = _compare(h, T, S, R_A, oracle_lib, worst, checks)
    print(f"T = {T}, S = {S}: {compared} rows compared, {excluded} left out; best rounds {sorted(seen)}; worst "
          "error: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert ref_near == 0 and excluded == 0 and compared >= 20
    _assert_tolerances(worst, checks)


@pytest.mark.parametrize("S", cases.S_VALUES)
def test_adapt_proposal_vs_reference(torch_dev, S):
    from metadamage_amd import engine

    u, w, mask, cheld, K, kinds = cases.series(S)
    want = cases.reference(u, w, mask, cheld, K)
    m, d, F, gc, ok = engine.adapt_proposal(u, w, mask, cheld, K)
    for i, kind in enumerate(kinds):
        assert bool(ok[i]) == (want[i] is not None) == (kind not in cases.STOPS), (kind, ok[i])
        if not ok[i]:
            assert np.isnan(m[i]).all() and np.isnan(d[i]).all() and np.isnan(F[i]).all() and np.isnan(gc[i])
    worst = cases.errors((m, d, F, gc), want)
    print(f"S={S}: worst error " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= 10.0 * PROPOSAL_MEASURED[name], (name, v)


# --------------------------------------------------------------------------
# 7. the two entries agree
# --------------------------------------------------------------------------
def test_psis_and_waic_rows_agree(batch):
    h = batch
    from metadamage_amd import _lib

    P = ref

    wf = _lib.MAPWAIC_FIELDS.index
    for p, pa, w, wa in ((h["p3"], h["p3_adapt"], h["w3"], h["w3_adapt"]), (h["p0"], h["p0_adapt"], h["w0"],
                                                                           h["w0_adapt"])):
        rows = w[:, [0, 2, 3]]
        for pf, name in ((P.KHAT, "khat"), (P.ESS, "ess"), (P.N_INF, "n_infeasible"), (P.FLAGS, "flags")):
            assert np.array_equal(_bits(p[:, :, pf]), _bits(rows[:, :, wf(name)])), name
        assert np.array_equal(_bits(pa), _bits(wa))
    adapted = (h["p3"][:, :, ref.FLAGS].astype(int) & ad.ADAPTED) != 0
    assert adapted.sum() >= 25 and np.array_equal(adapted, h["p3_adapt"][:, :, 2] > 0)
    # the null rows are mdfit_map_waic's; so is every PMD row the rounds left alone
    for a, b in ((h["w3"], h["v1_waic"]), (h["w3_pw"], h["v1_pw"]), (h["w3_draws"], h["v1_wdraws"])):
        assert np.array_equal(_bits(a[:, [1, 4, 5]]), _bits(b[:, [1, 4, 5]]))
        pm = a[:, [0, 2, 3]], b[:, [0, 2, 3]]
        assert np.array_equal(_bits(pm[0][~adapted]), _bits(pm[1][~adapted]))
    assert np.array_equal(_bits(h["p3"][~adapted]), _bits(h["v1_psis"][~adapted]))
    # an adapted PMD row's WAIC is that of other weights
    assert (h["w3"][:, [0, 2, 3]][adapted][:, 0] != h["v1_waic"][:, [0, 2, 3]][adapted][:, 0]).all()
    # the waic entry's draws of a PMD row are the psis entry's best round
    assert np.array_equal(_bits(h["w3_draws"][:, [0, 2, 3]]), _bits(h["p3_draws"]))


# --------------------------------------------------------------------------
# 8. the records do not depend on the call
# --------------------------------------------------------------------------
def test_records_do_not_depend_on_the_call(torch_dev, batch):
    torch = torch_dev
    from metadamage_amd import _lib, engine

    h = batch
    ty, tN, res = h["ty"], h["tN"], h["res"]
    base_p, base_a, base_w = h["p3"], h["p3_adapt"], h["w3"]

    def sub(lo, hi):
        return engine.FitBatch(res.out[lo:hi], None, res.status[lo:hi], None)

    def run(lo, hi, index_base, **kw):
        p, a = engine.map_psis_device(ty[lo:hi], tN[lo:hi], sub(lo, hi), S_A, SEED, index_base, adapt_rounds=R_A, **kw)
        w, a2 = engine.map_waic_device(ty[lo:hi], tN[lo:hi], sub(lo, hi), S_A, SEED, index_base, adapt_rounds=R_A,
                                       **kw)
        torch.cuda.synchronize()
        return _np(p, a, w, a2)

    def same(got, lo, hi):
        p, a, w, a2 = got
        return (np.array_equal(_bits(p), _bits(base_p[lo:hi])) and np.array_equal(_bits(a), _bits(base_a[lo:hi]))
                and np.array_equal(_bits(w), _bits(base_w[lo:hi])) and np.array_equal(_bits(a2), _bits(base_a[lo:hi])))

    # without the draws (the fixture's calls wrote them); T = 1, 3 and the whole batch of 64 ...
    for T in (1, 3, T_A):
        assert same(run(0, T, 0), 0, T), T
    # ... and T = 65: one taxon more, the first 64 unchanged
    y65 = np.concatenate([h["y"], h["y"][:1]])
    N65 = np.concatenate([h["N"], h["N"][:1]])
    t65y, t65N, _ = engine.to_device_counts(y65, N65, None)
    r65 = engine.FitBatch(torch.cat([res.out, res.out[:1]]), None, torch.cat([res.status, res.status[:1]]), None)
    p65, a65 = engine.map_psis_device(t65y, t65N, r65, S_A, SEED, 0, adapt_rounds=R_A)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(p65[:T_A].cpu().numpy()), _bits(base_p))
    assert np.array_equal(_bits(a65[:T_A].cpu().numpy()), _bits(base_a))
    # two calls split with index_base
    assert same(run(0, 30, 0), 0, 30) and same(run(30, T_A, 30), 30, T_A)
    assert not same(run(30, T_A, 0), 30, T_A)  # (the streams are the global taxon's)
    # without the adapt record: the entry called with adapt = NULL
    lib = _lib.load()
    p = torch.zeros((T_A, 3, _lib.NMAPPSIS), dtype=torch.float64, device=ty.device)
    w = torch.zeros((T_A, _lib.NWAICROW, _lib.NMAPWAIC), dtype=torch.float64, device=ty.device)
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.mdfit_map_psis_adapt(vp(ty.data_ptr()), vp(tN.data_ptr()), vp(res.out.data_ptr()),
                                        vp(res.status.data_ptr()), T_A, S_A, R_A, SEED, 0, vp(p.data_ptr()), None, None,
                                        stream))
    _lib.check(lib.mdfit_map_waic_adapt(vp(ty.data_ptr()), vp(tN.data_ptr()), vp(res.out.data_ptr()),
                                        vp(res.status.data_ptr()), T_A, S_A, R_A, SEED, 0, vp(w.data_ptr()), None, None,
                                        None, stream))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(base_p)) and np.array_equal(_bits(w.cpu().numpy()),
                                                                                    _bits(base_w))
    # after a poisoning of the LDS
    _lib.check(lib.mdfit_poison_lds(stream))
    assert same(run(0, T_A, 0), 0, T_A)
    # under graph capture and one replay
    s = torch.cuda.Stream()
    dp = torch.zeros_like(p)
    da = torch.zeros((T_A, 3, _lib.NMAPADAPT), dtype=torch.float64, device=ty.device)
    dw = torch.zeros_like(w)
    da2 = torch.zeros_like(da)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cur = torch.cuda.current_stream()
        engine.map_psis_device(ty, tN, res, S_A, SEED, 0, psis=dp, stream=cur, adapt_rounds=R_A, adapt=da)
        engine.map_waic_device(ty, tN, res, S_A, SEED, 0, waic=dw, stream=cur, adapt_rounds=R_A, adapt=da2)
    for t in (dp, da, dw, da2):
        t.fill_(0.0)
    g.replay()
    torch.cuda.synchronize()
    assert same(_np(dp, da, dw, da2), 0, T_A)


# --------------------------------------------------------------------------
# 9. auto
# --------------------------------------------------------------------------
def test_auto_with_adapted_proposals(torch_dev):
    from metadamage_amd import _lib, engine
    from metadamage_amd.synthetic import generate
    from tests.test_gpu_auto import BASE3, N3, S3, W3

    torch = torch_dev
    T = 48
    b = generate(300, seed=21)
    ty, tN, tm = engine.to_device_counts(b.y[:T], b.N[:T], b.mm[:T])
    opts = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=W3, num_samples=N3, seed=0, index_base=BASE3)
    o_map, o_nuts = engine.auto_opts(opts)
    r0, route0, _ = engine.fit_auto_device(ty, tN, tm, opts, S3)
    r3, route3, auto3 = engine.fit_auto_device(ty, tN, tm, opts, S3, psis_adapt=R_A)
    m = engine.fit_batch_device(ty, tN, tm, o_map)
    psis, pa = engine.map_psis_device(ty, tN, m, S3, 0, BASE3, adapt_rounds=R_A)
    waic, _ = engine.map_waic_device(ty, tN, m, S3, 0, BASE3, adapt_rounds=R_A)
    nuts = engine.fit_batch_device(ty, tN, tm, o_nuts)
    torch.cuda.synchronize()
    assert r0.adapt is None
    s0 = (route0.cpu().numpy() & _lib.ROUTE_SAMPLE) != 0
    s3 = (route3.cpu().numpy() & _lib.ROUTE_SAMPLE) != 0
    print(f"sampled {int(s0.sum())} -> {int(s3.sum())} of {T}")
    assert not (s3 & ~s0).any() and s3.sum() < s0.sum() and (~s3).sum() >= 4
    out, psis, waic, pa = _np(r3.out, psis, waic, pa)
    # a sampled row is the plain NUTS call's
    assert np.array_equal(_bits(out[s3]), _bits(nuts.out.cpu().numpy()[s3]))
    assert np.array_equal(r3.pred.cpu().numpy()[s3].view(np.int32), nuts.pred.cpu().numpy()[s3].view(np.int32))
    assert np.array_equal(r3.status.cpu().numpy()[s3], nuts.status.cpu().numpy()[s3])
    # a settled row: the nine columns are copies of the adapted records, the rest the MAP call's
    u = ~s3
    F, P = _lib.RESULT_FIELDS.index, _lib.MAPPSIS_FIELDS.index
    nine = {F("q_mean"): psis[:, 0, P("q_mean")], F("concentration_mean"): psis[:, 0, P("phi_mean")],
            F("D_max_marginalized_mean"): psis[:, 0, P("D_max_mean")], F("q_mean_forward"): psis[:, 1, P("q_mean")],
            F("q_mean_reverse"): psis[:, 2, P("q_mean")], F("n_sigma"): waic[:, 6, 0],
            F("n_sigma_forward"): waic[:, 6, 1], F("n_sigma_reverse"): waic[:, 6, 2], F("asymmetry"): waic[:, 6, 3]}
    for col, v in nine.items():
        assert np.array_equal(_bits(out[u, col]), _bits(v[u])), col
    rest = [c for c in range(_lib.NOUT) if c not in nine]
    assert np.array_equal(_bits(out[u][:, rest]), _bits(m.out.cpu().numpy()[u][:, rest]))
    # some settled taxon was settled by an adapted row
    assert ((psis[u][:, :, ref.FLAGS].astype(int) & ad.ADAPTED) != 0).any()
    # the block that leaves the device
    a = r3.adapt.cpu().numpy()
    assert a.dtype == np.float32 and a.shape == (T, _lib.NADAPTOUT)
    with np.errstate(invalid="ignore"):
        want = np.stack([np.nanmax(np.where(np.isnan(pa[:, :, 0]), -np.inf, pa[:, :, 0]), axis=1),
                         np.nanmax(np.where(np.isnan(pa[:, :, 2]), -np.inf, pa[:, :, 2]), axis=1)], axis=1)
    want[np.isneginf(want)] = np.nan
    assert np.array_equal(a.view(np.int32), want.astype(np.float32).view(np.int32))
    assert auto3.shape == (T, _lib.NAUTO)


# --------------------------------------------------------------------------
# the chunked dispatch, the gather record and the CLI
# --------------------------------------------------------------------------
def _summary(a):
    with np.errstate(invalid="ignore"):
        s = np.stack([np.where(np.isnan(a[:, :, 0]), -np.inf, a[:, :, 0]).max(axis=1),
                      np.where(np.isnan(a[:, :, 2]), -np.inf, a[:, :, 2]).max(axis=1)], axis=1)
    s[np.isneginf(s)] = np.nan
    return s.astype(np.float32)


def test_two_chunks_and_the_gather_record(torch_dev, batch, monkeypatch):
    torch = torch_dev
    from metadamage_amd import _lib, distributed as d, engine

    h = batch
    opts = _lib.default_opts(mode=_lib.MODE_MAP)
    want_p, want_w = h["p3"].astype(np.float32), h["w3"].astype(np.float32)
    want_a = _summary(h["p3_adapt"])
    assert np.isfinite(want_a).all() and want_a[:, 1].max() == 3
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "32")
    assert len(engine.plan_chunks(T_A, opts, with_psis=True)) == 2
    o5, p5, s5, ps5, a5 = engine.fit_batch_host(h["y"], h["N"], h["mm"], opts, psis=True, psis_draws=S_A,
                                                psis_adapt=R_A)
    assert ps5.dtype == np.float32 and a5.dtype == np.float32 and a5.shape == (T_A, _lib.NADAPTOUT)
    assert np.array_equal(ps5.view(np.int32), want_p.view(np.int32))
    assert np.array_equal(a5.view(np.int32), want_a.view(np.int32))
    o6, p6, s6, w6, a6 = engine.fit_batch_host(h["y"], h["N"], h["mm"], opts, waic=True, psis_draws=S_A,
                                               psis_adapt=R_A)
    assert np.array_equal(w6.view(np.int32), want_w.view(np.int32))
    assert np.array_equal(a6.view(np.int32), want_a.view(np.int32))
    # without rounds: today's four arrays, the v1 records
    got4 = engine.fit_batch_host(h["y"], h["N"], h["mm"], opts, psis=True, psis_draws=S_A)
    assert len(got4) == 4 and np.array_equal(got4[3].view(np.int32), h["v1_psis"].astype(np.float32).view(np.int32))
    for x, z in zip(got4[:3], (o5, p5, s5)):
        assert np.array_equal(x, z, equal_nan=True)
    # into the gather record of a world of one
    rec = d.alloc_records(T_A, torch.device("cuda", torch.cuda.current_device()), with_psis=True, with_adapt=True)
    fitter = engine.ChunkedFitter(32, opts=opts, dest_on_device=True, with_psis=True, psis_draws=S_A, psis_adapt=R_A)
    fitter.run_into_device(h["y"], h["N"], h["mm"], opts,
                           engine.FitBatch(rec.out, rec.pred, rec.status, psis=rec.psis, adapt=rec.adapt),
                           chunks=engine.plan_chunks(T_A, opts, chunk_taxa=32))
    buf = rec.stage()
    torch.cuda.synchronize()
    og, pg, sg, psg, ag = d.unpack_gathered(d.gather_records(buf, T_A, 0, 1), T_A, 1, with_psis=True, with_adapt=True)
    assert np.array_equal(psg.view(np.int32), want_p.view(np.int32))
    assert np.array_equal(ag.view(np.int32), want_a.view(np.int32)) and np.array_equal(sg, s5)
    # the auto call in two chunks
    o_auto = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=20, num_samples=20, seed=0)
    one = engine.fit_auto_chunks(h["y"], h["N"], h["mm"], o_auto, S_A, psis_adapt=R_A)
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "0")
    two = engine.fit_auto_chunks(h["y"], h["N"], h["mm"], o_auto, S_A, psis_adapt=R_A)
    assert len(one) == len(two) == 5
    for x, z in zip(one, two):
        assert x.dtype == z.dtype and np.array_equal(x, z, equal_nan=True)
    assert np.array_equal(one[4].view(np.int32), want_a.view(np.int32))


def test_cli_psis_adapt(tmp_path):
    import pandas as pd
    from typer.testing import CliRunner

    from metadamage_amd import fits, io
    from metadamage_amd.cli import cli_app
    from tests.helpers import GOLDEN

    def run(out_dir, *args):
        r = CliRunner().invoke(cli_app, ["fit", "--out-dir", str(out_dir), *args, str(GOLDEN / "data_ancient.txt")])
        assert r.exit_code == 0, (r.output, r.exception)
        return io.Parquet(out_dir / "fit_results" / "data_ancient.parquet")

    for inference in ("map-psis", "map-waic", "auto"):
        plain = run(tmp_path / f"{inference}-plain", "--inference", inference)
        zero = run(tmp_path / f"{inference}-zero", "--inference", inference, "--psis-adapt", "0")
        pq = run(tmp_path / f"{inference}-three", "--inference", inference, "--psis-adapt", "3")
        df0, dfz, df = plain.load(), zero.load(), pq.load()
        pd.testing.assert_frame_equal(dfz, df0)  # psis_adapt 0: today's frame and metadata
        mz, mp = zero.load_metadata(), plain.load_metadata()
        assert sorted(mz) == sorted(mp) and "psis_adapt" not in mp  # (the same keys; out_dir differs by design)
        assert {k: v for k, v in mz.items() if k != "out_dir"} == {k: v for k, v in mp.items() if k != "out_dir"}
        assert int(pq.load_metadata()["psis_adapt"]) == 3
        assert list(df.columns) == list(df0.columns) + fits.ADAPT_COLUMNS
        assert df["pareto_k_initial"].dtype == np.float32 and df["psis_adapt_rounds"].dtype == np.uint32
        assert np.isfinite(df["pareto_k_initial"]).all() and (df["psis_adapt_rounds"] <= 3).all()
        # the MAP fit's columns do not change with the rounds
        if inference != "auto":
            pd.testing.assert_frame_equal(df[df0.columns[:30]], df0[df0.columns[:30]])
    f = tmp_path / "map-psis-three" / "fit_results" / "data_ancient.parquet"
    m1 = f.stat().st_mtime_ns
    run(tmp_path / "map-psis-three", "--inference", "map-psis", "--psis-adapt", "3")  # cache hit: file untouched
    assert f.stat().st_mtime_ns == m1
    run(tmp_path / "map-psis-three", "--inference", "map-psis")  # other rounds: the cache is not reused
    assert f.stat().st_mtime_ns != m1
