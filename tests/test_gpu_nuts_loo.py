"""GPU tests of mdfit_nuts_loo and mdfit_psis (MDFIT-LOO v1):
the estimator on crafted series and the whole pass on crafted draws written
straight into a workspace against tests/nuts_loo_ref.py, that the pass only
reads and is deterministic, beside mdfit_nuts_diag and mdfit_nuts_summary on one
workspace, on the device's own small chains, the chunked, sharded and CLI paths
of `--inference nuts-loo`, and what n_sigma_loo means beside the WAIC n_sigma."""

from __future__ import annotations

import ctypes
import itertools
import os
import socket

import numpy as np
import pandas as pd
import pytest

from tests import nuts_loo_cases as cases
from tests import nuts_loo_ref as ref
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

# Ten times the worst error measured on the MI355X against nuts_loo_ref
# (longdouble), never looser than 1e-9 for an elpd.  khat is
# compared absolutely (O(1), 0 included; it passes through the grid's softmax);
# where the reference gives +-inf or exactly 0 it must be equal.
# mdfit_psis: identical series in, so every rank decision is the reference's.
MEASURED_PSIS = {"elpd": 5.36e-15, "khat": 9.09e-15}
TOL_PSIS = {k: min(10.0 * v, 1e-9) for k, v in MEASURED_PSIS.items()}
# mdfit_nuts_loo against the reference fed the reference's own log-likelihoods
# (scipy gammaln on float64 arguments, combined in longdouble): the difference
# is the two log-likelihoods', cases.LL_ERROR, largest at the N ~ 1e6 position.
# Relative, but khat_i and khat_max absolute; p_loo (lppd - elpd) and the four
# comparisons are differences of sums and lose what their cancellation takes.
# khat_i is worst at S = 65, where M = 13 excesses carry the fit (5.1e-9 at S = 1000).
MEASURED_LOO = {"elpd_i": 3.21e-10, "khat_i": 4.55e-8, "elpd_loo": 2.79e-11, "p_loo": 2.12e-10, "elpd_se": 1.82e-10,
                "khat_max": 8.21e-10, "lppd": 1.35e-11, "n_sigma": 2.30e-9}
TOL_LOO = {k: (min(10.0 * v, 1e-9) if k in ("elpd_i", "elpd_loo", "lppd") else 10.0 * v)
           for k, v in MEASURED_LOO.items()}
# the device's log-likelihood against the reference's, relative to max(1, |l|)
MEASURED_LL = 6.0e-10


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    return torch


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# --------------------------------------------------------------------------
# mdfit_psis: the estimator on identical series
# --------------------------------------------------------------------------
@pytest.mark.parametrize("S,n", cases.PSIS_SHAPES)
def test_psis_vs_reference(torch_dev, S, n):
    from metadamage_amd import engine
    from tests.test_nuts_loo import compare_to_reference

    ll, kinds = cases.psis_case(S, n)
    want_e, want_k = cases.psis_reference(S, n)
    e, k = engine.psis(np.array(ll))
    e2, k2 = engine.psis(np.array(ll))
    assert np.array_equal(e.view(np.int64), e2.view(np.int64)) and np.array_equal(k.view(np.int64), k2.view(np.int64))
    print(f"S={S} n={len(kinds)}", end=": ")
    compare_to_reference(e, k, want_e, want_k, TOL_PSIS)
    for i, kind in enumerate(kinds):
        if kind == "const":
            assert k[i] == (0.0 if S >= 25 else np.inf) and e[i] == ll[i, 0]
        if S < 25 or (kind == "xstar0" and S >= 25):
            assert k[i] == np.inf


def test_psis_special_values_and_poison(torch_dev):
    from metadamage_amd import _lib, engine

    sp = cases.special_series()
    got = {}
    for name, l in sp:
        e, k = engine.psis(l[None, :])
        _lib.check(_lib.load().mdfit_poison_lds(_stream(torch_dev)))
        e2, k2 = engine.psis(l[None, :])
        assert np.array_equal(e.view(np.int64), e2.view(np.int64)), name
        assert np.array_equal(k.view(np.int64), k2.view(np.int64)), name
        got[name] = (e[0], k[0])
    for name in ("nan", "-inf", "+inf"):
        assert np.isnan(got[name][0]) and np.isnan(got[name][1]), name
    assert got["const"] == (-1.5, 0.0)
    assert got["flat_tail"][1] == 0.0 and got["xstar0"][1] == np.inf
    assert got["S24"][1] == np.inf and got["S2"][1] == np.inf
    for name in ("flat_tail", "xstar0", "ties", "S24", "S2"):
        we, wk = ref.psis(dict(sp)[name])
        assert abs(got[name][0] - we) <= TOL_PSIS["elpd"] * abs(we), name
        if np.isfinite(wk) and wk != 0:
            assert abs(got[name][1] - wk) <= TOL_PSIS["khat"], name


# --------------------------------------------------------------------------
# mdfit_nuts_loo on crafted draws
# --------------------------------------------------------------------------
def crafted_on_device(torch, x, status, y, N):
    """§9.2's crafted workspace -- the draws x[T, 6, S, 4] and records whose chain
    status slots are status[T, 6] -- and the device counts: (ty, tN, res, opts)."""
    from metadamage_amd import engine
    from tests.test_gpu_nuts_summary import crafted_on_device as summary_crafted

    res, opts = summary_crafted(torch, np.array(x), status)
    ty, tN, _ = engine.to_device_counts(np.array(y), np.array(N))
    return ty, tN, res, opts


def run_loo(torch, x, status, y, N, poison=False):
    """mdfit_nuts_loo on crafted draws -> host (loo[T, 7, 8], pointwise[T, 6, 30,
    2]) float64; checks on the way that the call only reads and that a second
    call gives the same bits."""
    from metadamage_amd import _lib, engine

    ty, tN, res, opts = crafted_on_device(torch, x, status, y, N)
    T = x.shape[0]
    before = [t.clone() for t in (res.out, res.pred, res.status, res.workspace, ty, tN)]
    if poison:
        _lib.check(_lib.load().mdfit_poison_lds(_stream(torch)))
    loo, pw = engine.nuts_loo_device(ty, tN, res, T, opts, pointwise=True)
    again, pw2 = engine.nuts_loo_device(ty, tN, res, T, opts, pointwise=True)
    no_pw = engine.nuts_loo_device(ty, tN, res, T, opts)
    torch.cuda.synchronize()
    for b, a in zip(before, (res.out, res.pred, res.status, res.workspace, ty, tN)):
        assert torch.equal(b.view(torch.uint8), a.view(torch.uint8))
    assert torch.equal(loo.view(torch.int64), again.view(torch.int64))
    assert torch.equal(loo.view(torch.int64), no_pw.view(torch.int64))
    assert torch.equal(pw.view(torch.int64), pw2.view(torch.int64))
    return loo.cpu().numpy(), pw.cpu().numpy()


@pytest.fixture(scope="module")
def crafted(torch_dev):
    """Every crafted shape through the kernel once: {(S, T): (loo, pointwise)}, read only."""
    got = {}
    for S, T in cases.LOO_SHAPES:
        loo, pw = run_loo(torch_dev, *cases.loo_case(S, T))
        loo.setflags(write=False)
        pw.setflags(write=False)
        got[(S, T)] = (loo, pw)
    return got


def _rel(got, want):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(got.astype(ref.LD) - want) / np.abs(want)


def device_loglik(torch, x, y, N):
    """The device's own l[T, 6, 30, S]: every draw replicated into a two-draw
    chain of its own, whose constant series is not smoothed and has elpd_i = l
    exactly."""
    from metadamage_amd import engine

    T, K, S, _ = x.shape
    xx = np.repeat(np.transpose(x, (0, 2, 1, 3)).reshape(T * S, K, 1, 4), 2, axis=2)
    ty, tN, res, opts = crafted_on_device(torch, xx, np.zeros((T * S, K)), np.repeat(y, S, axis=0),
                                          np.repeat(N, S, axis=0))
    _, pw = engine.nuts_loo_device(ty, tN, res, T * S, opts, pointwise=True)
    torch.cuda.synchronize()
    return np.transpose(pw.cpu().numpy()[..., 0].reshape(T, S, K, 30), (0, 2, 3, 1))


@pytest.mark.parametrize("S,T", cases.LOO_SHAPES)
def test_device_loglik_within_the_precondition(torch_dev, S, T):
    """The precondition's figure: the device's log-likelihood lies within
    cases.LL_ERROR of the reference's; at N = 0 it is exactly 0."""
    x, status, y, N = cases.loo_case(S, T)
    dl = device_loglik(torch_dev, x, y, N)
    wl = ref.loo_rows(x, status, y, N)[2]
    fin = np.isfinite(wl.astype(np.float64))
    assert np.array_equal(np.isfinite(dl), fin)
    err = np.abs(dl[fin].astype(ref.LD) - wl[fin]) / np.maximum(1, np.abs(wl[fin]))
    print(f"S={S} T={T}: device log-likelihood worst error {float(err.max()):.2e}")
    assert MEASURED_LL <= cases.LL_ERROR and err.max() <= cases.LL_ERROR
    assert (dl[0, :2, 4] == 0.0).all() and N[0, 4] == 0


@pytest.mark.parametrize("S,T", cases.LOO_SHAPES)
def test_crafted_draws_vs_reference(crafted, S, T):
    loo, pw = crafted[(S, T)]
    want, wpw, exempt = cases.loo_reference(S, T)
    n_series = sum(len(ref.points_of(k)) for k in range(6)) * T
    assert exempt.sum() <= cases.MAX_EXEMPT * n_series, (int(exempt.sum()), n_series)
    w64, wpw64 = want.astype(np.float64), wpw.astype(np.float64)
    assert np.array_equal(np.isnan(loo), np.isnan(w64)) and np.array_equal(np.isnan(pw), np.isnan(wpw64))
    assert np.array_equal(loo[:, :, ref.FLAGS], w64[:, :, ref.FLAGS])
    x, status, y, N = cases.loo_case(S, T)
    # the crafted faults: a failed chain, a NaN draw; the other rows valid
    assert loo[T - 1, 4, 7] == 0.0 and loo[T - 1, 3, 7] == 0.0 and loo[T - 1, 6, 7] == 0.0
    assert loo[:, :6, 7].sum() == 6 * T - 2 and (loo[:T - 1, 6, 7] == 1.0).all()
    worst = {}
    use = ~exempt & ~np.isnan(wpw64[..., 0])
    zero = use & (wpw64[..., 0] == 0)  # (the N = 0 position in the four sub-fits that hold it: met exactly)
    assert (pw[..., 0][zero] == 0.0).all() and zero.sum() == 4
    worst["elpd_i"] = float(_rel(pw[..., 0][use & ~zero], wpw[..., 0][use & ~zero]).max())
    kw = wpw64[..., 1]
    special = use & (np.isinf(kw) | (kw == 0))
    assert np.array_equal(pw[..., 1][special], kw[special])
    assert pw[0, 0, 4, 1] == 0.0 and pw[0, 0, 4, 0] == 0.0  # N = 0: l = 0, a constant tail
    fin = use & ~special
    worst["khat_i"] = float(np.abs(pw[..., 1][fin].astype(ref.LD) - wpw[..., 1][fin]).max())
    rows = ~exempt.any(axis=2) & (w64[:, :6, ref.FLAGS] == 1.0)
    for name, f in (("elpd_loo", ref.ELPD), ("p_loo", ref.P_LOO), ("elpd_se", ref.ELPD_SE), ("lppd", ref.LPPD)):
        worst[name] = float(_rel(loo[:, :6, f][rows], want[:, :6, f][rows]).max())
    km = want[:, :6, ref.KHAT_MAX][rows]
    kfin = np.isfinite(km.astype(np.float64))
    assert np.array_equal(loo[:, :6, ref.KHAT_MAX][rows][~kfin], km.astype(np.float64)[~kfin])
    worst["khat_max"] = float(np.abs(loo[:, :6, ref.KHAT_MAX][rows][kfin].astype(ref.LD) - km[kfin]).max())
    assert np.array_equal(loo[:, :6, ref.KHAT_ARGMAX][rows], w64[:, :6, ref.KHAT_ARGMAX][rows])
    assert np.array_equal(loo[:, :6, ref.N_BAD][rows], w64[:, :6, ref.N_BAD][rows])
    taxa = rows.all(axis=1)
    cmp4 = slice(ref.N_SIGMA, ref.ASYMMETRY + 1)
    ok6 = ~np.isnan(w64[taxa][:, 6, cmp4])
    worst["n_sigma"] = float(_rel(loo[taxa][:, 6, cmp4][ok6], want[taxa][:, 6, cmp4][ok6]).max())
    assert np.array_equal(loo[taxa][:, 6, ref.ALL_N_BAD], w64[taxa][:, 6, ref.ALL_N_BAD])
    assert (loo[:, 6, 6][~np.isnan(loo[:, 6, 6])] == 0.0).all()
    print(f"S={S} T={T} worst error: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= TOL_LOO[name], (name, v)


def test_invalid_taxon_gives_seven_nan_rows(torch_dev):
    x, status, y, N = cases.loo_case(65, 3)
    y = np.array(y)
    y[1, 3] = N[1, 3] + 1  # status 3 in a fit
    loo, pw = run_loo(torch_dev, x, status, y, N)
    assert np.isnan(loo[1, :, :7]).all() and (loo[1, :, 7] == 0.0).all() and np.isnan(pw[1]).all()
    assert (loo[0, :, 7] == 1.0).all()


def test_poisoned_lds_same_bits(torch_dev, crafted):
    for S, T in cases.LOO_SHAPES:
        loo, pw = run_loo(torch_dev, *cases.loo_case(S, T), poison=True)
        assert np.array_equal(loo.view(np.int64), crafted[(S, T)][0].view(np.int64))
        assert np.array_equal(pw.view(np.int64), crafted[(S, T)][1].view(np.int64))


def test_record_does_not_depend_on_the_batch(torch_dev, crafted):
    S, T = 65, 3
    x, status, y, N = cases.loo_case(S, T)
    for t in range(T):
        loo, pw = run_loo(torch_dev, x[t:t + 1], status[t:t + 1], y[t:t + 1], N[t:t + 1])
        assert np.array_equal(loo[0].view(np.int64), crafted[(S, T)][0][t].view(np.int64)), t
        assert np.array_equal(pw[0].view(np.int64), crafted[(S, T)][1][t].view(np.int64)), t
    big = [np.concatenate([a] * 23) for a in (x, status, y, N)]  # 69 taxa: more blocks than a few
    loo, pw = run_loo(torch_dev, *big)
    assert np.array_equal(loo.view(np.int64), np.concatenate([crafted[(S, T)][0]] * 23).view(np.int64))


def test_diag_summary_loo_in_every_order(torch_dev, crafted):
    """The three passes are independent: any order on one finished call's
    workspace gives each its solo bits."""
    torch = torch_dev
    from metadamage_amd import engine

    S, T = 65, 3
    case = cases.loo_case(S, T)
    ty, tN, res, opts = crafted_on_device(torch, *case)
    solo = {"diag": engine.nuts_diag_device(crafted_on_device(torch, *case)[2], T, opts),
            "summary": engine.nuts_summary_device(crafted_on_device(torch, *case)[2], T, opts),
            "loo": torch.tensor(np.array(crafted[(S, T)][0]), device=ty.device)}
    run = {"diag": lambda: engine.nuts_diag_device(res, T, opts),
           "summary": lambda: engine.nuts_summary_device(res, T, opts),
           "loo": lambda: engine.nuts_loo_device(ty, tN, res, T, opts)}
    for order in itertools.permutations(("diag", "summary", "loo")):
        got = {name: run[name]() for name in order}
        torch.cuda.synchronize()
        for name in order:
            assert torch.equal(got[name].view(torch.int64), solo[name].view(torch.int64)), (order, name)


# --------------------------------------------------------------------------
# real chains, small
# --------------------------------------------------------------------------
def _small_opts():
    from metadamage_amd import _lib

    return _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=100, num_samples=200)


@pytest.fixture(scope="module")
def small_chains(torch_dev):
    """generate(8, seed=21) fitted by one NUTS call (warmup 100, samples 200)
    and its PSIS-LOO records and pointwise values."""
    torch = torch_dev
    from metadamage_amd import engine
    from metadamage_amd.synthetic import generate

    b = generate(8, seed=21)
    opts = _small_opts()
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    res = engine.fit_batch_device(ty, tN, tm, opts)
    loo, pw = engine.nuts_loo_device(ty, tN, res, 8, opts, pointwise=True)
    torch.cuda.synchronize()
    out, st = res.out.cpu().numpy(), res.status.cpu().numpy()
    loo, pw = loo.cpu().numpy(), pw.cpu().numpy()
    for a in (out, st, loo, pw):
        a.setflags(write=False)
    return b, out, st, loo, pw


def test_real_chains(small_chains):
    b, out, st, loo, pw = small_chains
    assert (st == 0).all() and (loo[:, :, 7] == 1.0).all(), (st, loo[:, :, 7])
    assert np.isfinite(loo[:, :6, :7]).all() or np.isinf(loo[:, :6, ref.KHAT_MAX]).any()
    r = loo[:, :6]
    # lppd - elpd_loo = p_loo > 0: leaving a point out never raises its density.  The three are sums
    # of the same 15 or 30 pointwise values in one order: equal to a few roundings of |lppd|
    assert (r[..., ref.P_LOO] > 0.0).all()
    np.testing.assert_allclose(r[..., ref.LPPD] - r[..., ref.ELPD], r[..., ref.P_LOO], rtol=0,
                               atol=1e-12 * np.abs(r[..., ref.LPPD]).max())
    tau = ref.khat_threshold(200)
    for k in range(6):
        cols = list(ref.points_of(k))
        outside = np.setdiff1d(np.arange(30), cols)
        assert np.isnan(pw[:, k, outside]).all() and np.isfinite(pw[:, k, cols, 0]).all()
        np.testing.assert_allclose(pw[:, k, cols, 0].sum(axis=1), r[:, k, ref.ELPD], rtol=1e-12)
        np.testing.assert_array_equal(pw[:, k, cols, 1].max(axis=1), r[:, k, ref.KHAT_MAX])
        np.testing.assert_array_equal(np.asarray(cols)[pw[:, k, cols, 1].argmax(axis=1)], r[:, k, ref.KHAT_ARGMAX])
        np.testing.assert_array_equal((pw[:, k, cols, 1] > tau).sum(axis=1), r[:, k, ref.N_BAD])
        e = pw[:, k, cols, 0]
        np.testing.assert_allclose(np.sqrt(len(cols) * e.var(axis=1)), r[:, k, ref.ELPD_SE], rtol=1e-10)
    # row 6 from the pointwise values by the reference's formula (sums of 15 or 30 doubles and one
    # cancelling difference of them: 1e-9 covers the rounding of either summation order)
    for t in range(8):
        lp = np.full((6, 30), np.nan)
        for k in range(6):
            lp[k, list(ref.points_of(k))] = 0.0  # (lppd is not part of row 6)
        want = ref.rows_from_pointwise(pw[t].astype(ref.LD), lp, np.ones(6, bool), 200)[6].astype(np.float64)
        np.testing.assert_allclose(loo[t, 6, :4], want[:4], rtol=1e-9, atol=1e-9)
        assert loo[t, 6, ref.ALL_KHAT_MAX] == r[t, :, ref.KHAT_MAX].max()
        assert loo[t, 6, ref.ALL_N_BAD] == r[t, :, ref.N_BAD].sum() and loo[t, 6, 6] == 0.0


def test_feature_is_additive_and_chunks_agree(torch_dev, monkeypatch, small_chains):
    from metadamage_amd import _lib, engine, fits

    b, out, st, loo, pw = small_chains
    opts = _small_opts()
    p = fits.Packed(b.tax_id, b.tax_id.astype(str), np.full(8, "species"), b.N_alignments, b.y, b.N, b.mm)
    plain = fits.fit_packed(p, opts, shard=False)
    with_loo = fits.fit_packed(p, opts, shard=False, loo=True)
    assert len(plain) == 3 and len(with_loo) == 4
    for a, c in zip(plain, with_loo):
        assert a.dtype == c.dtype and np.array_equal(a.view(np.uint8), c.view(np.uint8))
    assert np.array_equal(plain[0], out[:, :25], equal_nan=True) and np.array_equal(plain[2], st)
    want32 = loo.astype(np.float32)
    assert with_loo[3].dtype == np.float32 and with_loo[3].shape == (8, 7, 8)
    assert np.array_equal(with_loo[3].view(np.int32), want32.view(np.int32))
    # three chunks reuse the one workspace: each chunk's pass runs before the next chunk's fit
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "3")
    assert len(engine.plan_chunks(8, opts)) == 3
    o3, p3, s3, d3 = engine.fit_batch_host(b.y, b.N, b.mm, opts, loo=True)
    assert np.array_equal(d3.view(np.int32), want32.view(np.int32))
    assert np.array_equal(o3, plain[0], equal_nan=True) and np.array_equal(s3, st)
    fitter = engine.ChunkedFitter(3, opts=opts, with_loo=True)
    o4, p4, s4, d4 = fitter.run(b.y, b.N, b.mm, opts)
    assert np.array_equal(d4.view(np.int32), want32.view(np.int32))
    with pytest.raises(ValueError):
        fitter.run(b.y, b.N, b.mm, _lib.default_opts(mode=_lib.MODE_MAP))
    with pytest.raises(ValueError):
        engine.fit_batch_host(b.y, b.N, b.mm, opts, loo=True, summary=True)
    import types

    df = fits.make_df_fit_results(p, with_loo[0], st == 0, types.SimpleNamespace(shortname="x"), loo=with_loo[3])
    assert (df["nuts_loo_valid"] == 1).all()
    np.testing.assert_array_equal(df["elpd_loo"].to_numpy(), want32[:, 0, 0])
    np.testing.assert_array_equal(df["n_sigma_loo"].to_numpy(), want32[:, 6, 0])


# --------------------------------------------------------------------------
# sharded: two gloo ranks on the one GPU
# --------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank(rank, world, port, T, q):
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from metadamage_amd import _lib, fits
        from metadamage_amd.synthetic import generate

        b = generate(T, seed=23)
        p = fits.Packed(b.tax_id, b.tax_id.astype(str), np.full(T, "species"), b.N_alignments, b.y, b.N, b.mm)
        opts = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=20, num_samples=40)
        res = fits.fit_packed(p, opts, shard=True, loo=True)
        q.put((rank, None if res is None else [np.asarray(a) for a in res]))
    except Exception as e:  # surfaced by the parent
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_sharded_loo_equals_single_process(torch_dev):
    import torch.multiprocessing as mp

    from metadamage_amd import _lib, fits
    from metadamage_amd.distributed import round_like_gather
    from metadamage_amd.synthetic import generate

    T = 61  # ragged shards: 31 + 30
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, T, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = dict(q.get(timeout=600) for _ in procs)
    for pr in procs:
        pr.join(timeout=120)
    assert got[1] is None, got[1]
    assert not isinstance(got[0], str), got[0]
    out, pred, st, loo = got[0]
    b = generate(T, seed=23)
    p = fits.Packed(b.tax_id, b.tax_id.astype(str), np.full(T, "species"), b.N_alignments, b.y, b.N, b.mm)
    opts = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=20, num_samples=40)
    ref_out, ref_pred, ref_st, ref_loo = fits.fit_packed(p, opts, shard=False, loo=True)
    assert loo.shape == (T, 7, 8) and loo.dtype == np.float32
    assert np.array_equal(loo.view(np.int32), ref_loo.view(np.int32))
    assert np.array_equal(st, ref_st) and np.array_equal(pred, ref_pred, equal_nan=True)
    assert np.array_equal(out, round_like_gather(ref_out), equal_nan=True)


# --------------------------------------------------------------------------
# CLI
# --------------------------------------------------------------------------
def test_cli_nuts_loo(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import io
    from metadamage_amd.cli import cli_app
    from tests.test_nuts_loo import FLOAT_COLUMNS, UINT_COLUMNS

    def run(out_dir, inference):
        r = CliRunner().invoke(cli_app, ["fit", "--out-dir", str(out_dir), "--inference", inference, "--max-fits", "10",
                                         str(GOLDEN / "data_ancient.txt")])
        assert r.exit_code == 0, (r.output, r.exception)
        return io.Parquet(out_dir / "fit_results" / "data_ancient.parquet")

    pq = run(tmp_path / "loo", "nuts-loo")
    df = pq.load()
    assert len(df.columns) == 43 and list(df.columns[30:]) == FLOAT_COLUMNS + UINT_COLUMNS
    assert pq.load_metadata()["inference"] == "nuts-loo"
    plain = run(tmp_path / "plain", "nuts").load()
    assert len(plain.columns) == 30
    pd.testing.assert_frame_equal(df[plain.columns], plain)  # value for value
    assert (df["nuts_loo_valid"] == 1).all()
    for c in UINT_COLUMNS:
        assert df[c].dtype == np.uint32, c
    for c in FLOAT_COLUMNS:
        assert df[c].dtype == np.float32 and not df[c].isna().any(), c
    assert (df["p_loo"] > 0).all() and (df["p_loo_null"] > 0).all() and (df["elpd_loo_se"] > 0).all()
    assert (df["elpd_loo"] < 0).all() and (df["elpd_loo_null"] < 0).all()


# --------------------------------------------------------------------------
# what it means: n_sigma_loo beside the record's WAIC n_sigma
# --------------------------------------------------------------------------
# n_sigma_loo / n_sigma on the 16 deep ancient taxa, measured on the oracle's
# 500 + 1000 chains on the CPU (oracle.lppd_and_waic against nuts_loo_ref.psis on
# one set of log-likelihoods), over the taxa without a bad point,
# two seeds; and the largest change of a taxon's ratio from one seed to the other
RATIO_BAND = (0.9858, 1.0019)
RATIO_SEED_SPREAD = 0.070


def test_n_sigma_loo_tracks_waic_n_sigma(torch_dev):
    """The 16 deep ancient taxa of test_laplace.test_reference_vs_nuts_posterior_std
    at 500 + 1000 draws: where no point is bad, n_sigma_loo / n_sigma lies in the
    band the oracle's chains show, widened by their seed-to-seed spread."""
    torch = torch_dev
    from metadamage_amd import _lib, engine
    from metadamage_amd.synthetic import generate

    b = generate(400, seed=21)
    deep = np.flatnonzero(b.truth["ancient"] & (b.N[:, :30].mean(axis=1) > 3e3))[:16]
    assert deep.size == 16
    ty, tN, tm = engine.to_device_counts(b.y[deep], b.N[deep], b.mm[deep])
    nuts = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=500, num_samples=1000)
    res = engine.fit_batch_device(ty, tN, tm, nuts)
    loo = engine.nuts_loo_device(ty, tN, res, 16, nuts)
    torch.cuda.synchronize()
    loo, out = loo.cpu().numpy(), res.out.cpu().numpy()
    assert (res.status.cpu().numpy() == 0).all() and (loo[:, :, 7] == 1.0).all()
    good = (loo[:, 0, ref.N_BAD] == 0) & (loo[:, 1, ref.N_BAD] == 0)
    ratio = loo[:, 6, ref.N_SIGMA] / out[:, _lib.RESULT_FIELDS.index("n_sigma")]
    print("n_sigma_loo / n_sigma: %d of 16 taxa without a bad point, %.3f-%.3f (all: %.3f-%.3f); khat_max %.2f-%.2f"
          % (good.sum(), ratio[good].min() if good.any() else np.nan, ratio[good].max() if good.any() else np.nan,
             ratio.min(), ratio.max(), loo[:, 6, ref.ALL_KHAT_MAX].min(), loo[:, 6, ref.ALL_KHAT_MAX].max()))
    lo, hi = RATIO_BAND[0] - RATIO_SEED_SPREAD, RATIO_BAND[1] + RATIO_SEED_SPREAD
    assert good.any()
    assert (ratio[good] >= lo).all() and (ratio[good] <= hi).all(), ratio
