"""GPU tests of mdfit_nuts_summary (MDFIT-SUMM v1): the kernel
on crafted draws written straight into a workspace against
tests/nuts_summary_ref.py, that it only reads and is deterministic, beside
mdfit_nuts_diag on one workspace, on the device's own small chains, the
chunked, sharded and CLI paths of `--inference nuts-summary`, and what its
spread means beside the Laplace standard errors."""

from __future__ import annotations

import ctypes
import os
import socket

import numpy as np
import pandas as pd
import pytest

from tests import nuts_summary_cases as cases
from tests import nuts_summary_ref as ref
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

# Against nuts_summary_ref (longdouble): ten times the worst error per moment
# field (relative; rho_Ac absolute) measured on the MI355X over every crafted
# shape and the small real chains, never looser than 1e-9.
# The order statistics get no tolerance: equal by value.
# D_max_mean and significance are largest where a crafted series' mean is nearly
# 0 and its sum cancels (the (65, 67) shape); 3.6e-14 elsewhere.
MEASURED = {"q_std": 9.55e-16, "A_std": 1.73e-15, "c_std": 9.61e-16, "phi_std": 1.54e-15, "D_max_std": 1.37e-15,
            "D_max_mean": 2.88e-12, "rho_Ac": 1.44e-15, "significance": 2.88e-12}
TOL = {k: min(10.0 * v, 1e-9) for k, v in MEASURED.items()}


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    return torch


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def crafted_on_device(torch, x, status):
    """A workspace holding the draws x[T, 6, S, 4] and records whose chain
    status slots are status[T, 6] (everything else zero): (res, opts)."""
    from metadamage_amd import _lib, engine

    T, _, S, _ = x.shape
    opts = _lib.default_opts(mode=_lib.MODE_NUTS, num_samples=S)
    res = engine.alloc_outputs(T, opts=opts)
    res.out.zero_()
    res.pred.zero_()
    res.status.zero_()
    res.workspace.zero_()
    res.out[:, _lib.F_DIAG + 6::_lib.DIAG_STRIDE] = torch.tensor(np.asarray(status), device=res.out.device)
    engine.samples_view(res, T, opts).copy_(torch.tensor(np.asarray(x)))
    return res, opts


def run_summary(torch, x, status, poison=False):
    """mdfit_nuts_summary on crafted draws -> host summ[T, 6, 16] float64; checks
    on the way that the call only reads and that a second call gives the same bits."""
    from metadamage_amd import _lib, engine

    res, opts = crafted_on_device(torch, x, status)
    T = x.shape[0]
    before = [t.clone() for t in (res.out, res.pred, res.status, res.workspace)]
    if poison:
        _lib.check(_lib.load().mdfit_poison_lds(_stream(torch)))
    summ = engine.nuts_summary_device(res, T, opts)
    again = engine.nuts_summary_device(res, T, opts)
    torch.cuda.synchronize()
    for b, a in zip(before, (res.out, res.pred, res.status, res.workspace)):
        assert torch.equal(b.view(torch.uint8), a.view(torch.uint8))
    assert torch.equal(summ.view(torch.int64), again.view(torch.int64))
    return summ.cpu().numpy()


@pytest.fixture(scope="module")
def crafted(torch_dev):
    """Every crafted shape through the kernel once: {(S, T): summ}, read only."""
    got = {}
    for S, T in cases.SHAPES:
        x, status = cases.case(S, T)
        got[(S, T)] = run_summary(torch_dev, x, status)
        got[(S, T)].setflags(write=False)
    return got


def _compare(got, want, label):
    from tests.test_nuts_summary import compare_to_reference

    print(label, end=": ")
    return compare_to_reference(got, want, TOL)


@pytest.mark.parametrize("S,T", cases.SHAPES)
def test_crafted_draws_vs_reference(crafted, S, T):
    from tests.test_nuts_summary import check_crafted_properties

    got = crafted[(S, T)]
    _compare(got, cases.reference(S, T), f"S={S} T={T}")
    check_crafted_properties(got, S, T)  # invalid rows, constants, null rows, the ramp's [0, L]


def test_poisoned_lds_same_bits(torch_dev, crafted):
    for S, T in ((65, 67), (1025, 3), (4096, 3)):
        x, status = cases.case(S, T)
        got = run_summary(torch_dev, x, status, poison=True)
        assert np.array_equal(got.view(np.int64), crafted[(S, T)].view(np.int64))


def test_record_does_not_depend_on_the_batch(torch_dev, crafted):
    x, status = cases.case(65, 67)
    for t in (0, 1, 2, 31, 66):
        one = run_summary(torch_dev, x[t:t + 1], status[t:t + 1])
        assert np.array_equal(one[0].view(np.int64), crafted[(65, 67)][t].view(np.int64)), t


def test_diag_then_summary_on_one_workspace(torch_dev, crafted):
    """The two passes are independent: either order on one finished call's
    workspace gives each its solo bits."""
    torch = torch_dev
    from metadamage_amd import engine

    S, T = 129, 3
    x, status = cases.case(S, T)
    res, opts = crafted_on_device(torch, x, status)
    solo_diag = engine.nuts_diag_device(crafted_on_device(torch, x, status)[0], T, opts)
    d1 = engine.nuts_diag_device(res, T, opts)
    s1 = engine.nuts_summary_device(res, T, opts)
    d2 = engine.nuts_diag_device(res, T, opts)  # ... and the other way round
    torch.cuda.synchronize()
    assert np.array_equal(s1.cpu().numpy().view(np.int64), crafted[(S, T)].view(np.int64))
    assert torch.equal(d1.view(torch.int64), solo_diag.view(torch.int64))
    assert torch.equal(d2.view(torch.int64), solo_diag.view(torch.int64))


# --------------------------------------------------------------------------
# real chains, small
# --------------------------------------------------------------------------
def _small_opts():
    from metadamage_amd import _lib

    return _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=100, num_samples=200)


@pytest.fixture(scope="module")
def small_chains(torch_dev):
    """generate(8, seed=21) fitted by one NUTS call (warmup 100, samples 200),
    its summary records and draws, and the reference on those draws."""
    torch = torch_dev
    from metadamage_amd import _lib, engine
    from metadamage_amd.synthetic import generate

    b = generate(8, seed=21)
    opts = _small_opts()
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    res = engine.fit_batch_device(ty, tN, tm, opts)
    summ = engine.nuts_summary_device(res, 8, opts)
    torch.cuda.synchronize()
    out, pred, st = res.out.cpu().numpy(), res.pred.cpu().numpy(), res.status.cpu().numpy()
    draws = engine.samples_view(res, 8, opts).cpu().numpy()
    summ = summ.cpu().numpy()
    want = ref.summary_rows(draws, out[:, _lib.F_DIAG + 6::_lib.DIAG_STRIDE])
    for a in (out, pred, st, draws, summ, want):
        a.setflags(write=False)
    return b, out, pred, st, draws, summ, want


def test_real_chains_vs_reference(small_chains):
    b, out, pred, st, draws, summ, want = small_chains
    assert (st == 0).all() and (summ[:, :, 15] == 1.0).all(), (st, summ[:, :, 15])
    _compare(summ, want, "real chains")
    for k in range(6):
        r = summ[:, k]
        if k in ref.PMD_SUBFITS:
            assert np.isfinite(r[:, :15]).all() and (r[:, 0:5] > 0.0).all()
            assert (np.abs(r[:, ref.RHO]) <= 1.0).all()
        else:  # null sub-fits store A = c = 0: constant series
            assert (draws[:, k, :, 1:3] == 0.0).all()
            assert (r[:, 1:3] == 0.0).all() and np.isnan(r[:, ref.RHO]).all()
            assert np.array_equal(r[:, [4, ref.D_MEDIAN, ref.D_LO, ref.D_HI]],
                                  r[:, [0, ref.Q_MEDIAN, ref.Q_LO, ref.Q_HI]])
            assert np.isfinite(np.delete(r, ref.RHO, axis=1)).all()
        assert (r[:, ref.D_LO] <= r[:, ref.D_MEDIAN]).all() and (r[:, ref.D_MEDIAN] <= r[:, ref.D_HI]).all()
    # the record's own posterior mean of D_max is the mean of the same draws
    np.testing.assert_allclose(summ[:, 0, ref.D_MEAN], (draws[:, 0, :, 1] + draws[:, 0, :, 2]).mean(axis=1), rtol=1e-12)


def test_feature_is_additive_and_chunks_agree(torch_dev, monkeypatch, small_chains):
    from metadamage_amd import _lib, engine, fits

    b, out, pred, st, draws, summ, want = small_chains
    opts = _small_opts()
    p = fits.Packed(b.tax_id, b.tax_id.astype(str), np.full(8, "species"), b.N_alignments, b.y, b.N, b.mm)
    plain = fits.fit_packed(p, opts, shard=False)
    with_summ = fits.fit_packed(p, opts, shard=False, summary=True)
    assert len(plain) == 3 and len(with_summ) == 4
    for a, c in zip(plain, with_summ):
        assert a.dtype == c.dtype and np.array_equal(a.view(np.uint8), c.view(np.uint8))
    assert np.array_equal(plain[0], out[:, :25], equal_nan=True) and np.array_equal(plain[2], st)
    want32 = summ.astype(np.float32)
    assert with_summ[3].dtype == np.float32 and with_summ[3].shape == (8, 6, 16)
    assert np.array_equal(with_summ[3].view(np.int32), want32.view(np.int32))
    # three chunks reuse the one workspace: each chunk's summary runs before the next chunk's fit
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "3")
    assert len(engine.plan_chunks(8, opts)) == 3
    o3, p3, s3, d3 = engine.fit_batch_host(b.y, b.N, b.mm, opts, summary=True)
    assert np.array_equal(d3.view(np.int32), want32.view(np.int32))
    assert np.array_equal(o3, plain[0], equal_nan=True) and np.array_equal(s3, st)
    fitter = engine.ChunkedFitter(3, opts=opts, with_summary=True)
    o4, p4, s4, d4 = fitter.run(b.y, b.N, b.mm, opts)
    assert np.array_equal(d4.view(np.int32), want32.view(np.int32))
    with pytest.raises(ValueError):
        fitter.run(b.y, b.N, b.mm, _lib.default_opts(mode=_lib.MODE_MAP))
    with pytest.raises(ValueError):
        engine.fit_batch_host(b.y, b.N, b.mm, opts, summary=True, diag=True)
    import types

    df = fits.make_df_fit_results(p, with_summ[0], st == 0, types.SimpleNamespace(shortname="x"), summ=with_summ[3])
    assert (df["nuts_summary_valid"] == 1).all()
    np.testing.assert_array_equal(df["D_max_std"].to_numpy(), want32[:, 0, 4])


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
        res = fits.fit_packed(p, opts, shard=True, summary=True)
        q.put((rank, None if res is None else [np.asarray(a) for a in res]))
    except Exception as e:  # surfaced by the parent
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_sharded_summary_equals_single_process(torch_dev):
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
    out, pred, st, summ = got[0]
    b = generate(T, seed=23)
    p = fits.Packed(b.tax_id, b.tax_id.astype(str), np.full(T, "species"), b.N_alignments, b.y, b.N, b.mm)
    opts = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=20, num_samples=40)
    ref_out, ref_pred, ref_st, ref_summ = fits.fit_packed(p, opts, shard=False, summary=True)
    assert summ.shape == (T, 6, 16) and summ.dtype == np.float32
    assert np.array_equal(summ.view(np.int32), ref_summ.view(np.int32))
    assert np.array_equal(st, ref_st) and np.array_equal(pred, ref_pred, equal_nan=True)
    assert np.array_equal(out, round_like_gather(ref_out), equal_nan=True)


# --------------------------------------------------------------------------
# CLI
# --------------------------------------------------------------------------
def test_cli_nuts_summary(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import io
    from metadamage_amd.cli import cli_app
    from tests.test_nuts_summary import FLOAT_COLUMNS, UINT_COLUMNS

    def run(out_dir, inference):
        r = CliRunner().invoke(cli_app, ["fit", "--out-dir", str(out_dir), "--inference", inference, "--max-fits", "10",
                                         str(GOLDEN / "data_ancient.txt")])
        assert r.exit_code == 0, (r.output, r.exception)
        return io.Parquet(out_dir / "fit_results" / "data_ancient.parquet")

    pq = run(tmp_path / "summary", "nuts-summary")
    df = pq.load()
    assert len(df.columns) == 49 and list(df.columns[30:]) == FLOAT_COLUMNS + UINT_COLUMNS
    assert pq.load_metadata()["inference"] == "nuts-summary"
    plain = run(tmp_path / "plain", "nuts").load()
    assert len(plain.columns) == 30
    pd.testing.assert_frame_equal(df[plain.columns], plain)  # value for value
    assert (df["nuts_summary_valid"] == 1).all() and df["nuts_summary_valid"].dtype == np.uint32
    for c in FLOAT_COLUMNS:
        assert df[c].dtype == np.float32 and np.isfinite(df[c]).all(), c
    assert (df["D_max_posterior_lower_hpdi"] <= df["D_max_posterior_median"]).all()
    assert (df["D_max_posterior_median"] <= df["D_max_posterior_upper_hpdi"]).all()
    assert (df["q_lower_hpdi"] <= df["q_median"]).all() and (df["q_median"] <= df["q_upper_hpdi"]).all()
    assert (df["D_max_std"] > 0).all() and (df["significance"] > 0).all() and (df["rho_Ac"].abs() <= 1).all()


# --------------------------------------------------------------------------
# what the spread means: beside the Laplace standard errors
# --------------------------------------------------------------------------
def test_laplace_std_vs_posterior_std(torch_dev):
    """The 16 deep ancient taxa of test_laplace.test_reference_vs_nuts_posterior_std,
    fitted on the device once by MAP + mdfit_map_laplace and once by NUTS 500 +
    1000 + mdfit_nuts_summary: Laplace D_max_std / summary D_max_std and phi_std
    / phi_std lie in [0.7, 1.3] -- the project's own band (the oracle alone
    measures 0.83-1.03 and 0.93-1.09; it leaves ~15 % for a 1000-draw std's
    Monte Carlo error)."""
    torch = torch_dev
    from metadamage_amd import _lib, engine
    from metadamage_amd.synthetic import generate

    b = generate(400, seed=21)
    deep = np.flatnonzero(b.truth["ancient"] & (b.N[:, :30].mean(axis=1) > 3e3))[:16]
    assert deep.size == 16
    ty, tN, tm = engine.to_device_counts(b.y[deep], b.N[deep], b.mm[deep])
    res_map = engine.fit_batch_device(ty, tN, tm, _lib.default_opts(mode=_lib.MODE_MAP))
    lap = engine.map_laplace_device(ty, tN, res_map)
    nuts = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=500, num_samples=1000)
    res = engine.fit_batch_device(ty, tN, tm, nuts)
    summ = engine.nuts_summary_device(res, 16, nuts)
    torch.cuda.synchronize()
    lap, summ = lap.cpu().numpy(), summ.cpu().numpy()
    assert (res_map.status.cpu().numpy() == 0).all() and (res.status.cpu().numpy() == 0).all()
    fl, fs = _lib.LAPLACE_FIELDS.index, _lib.NUTSSUMM_FIELDS.index
    assert ((lap[:, 0, fl("flags")].astype(np.int64) & _lib.LAPLACE_VALID) != 0).all()
    assert (summ[:, 0, fs("flags")] == 1.0).all()
    ratios = np.stack([lap[:, 0, fl("D_max_std")] / summ[:, 0, fs("D_max_std")],
                       lap[:, 0, fl("phi_std")] / summ[:, 0, fs("phi_std")]], axis=1)
    print("Laplace / NUTS summary std: D_max %.2f-%.2f, phi %.2f-%.2f" % (ratios[:, 0].min(), ratios[:, 0].max(),
                                                                          ratios[:, 1].min(), ratios[:, 1].max()))
    assert (ratios >= 0.7).all() and (ratios <= 1.3).all(), ratios
