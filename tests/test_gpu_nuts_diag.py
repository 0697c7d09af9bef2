"""GPU tests of mdfit_nuts_diag (MDFIT-DIAG v1): the kernel on
crafted draws written straight into a workspace against tests/nuts_diag_ref.py,
that it only reads and is deterministic, on the device's own small chains, and
the chunked, sharded and CLI paths of `--inference nuts-diag`."""

from __future__ import annotations

import ctypes
import os
import socket

import numpy as np
import pandas as pd
import pytest

from tests import nuts_diag_cases as cases
from tests import nuts_diag_ref as ref
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

# Against nuts_diag_ref (longdouble): ten times the worst relative error per
# field measured on the MI355X over every crafted shape and the small real
# chains, never looser than 1e-9.
MEASURED = {"ess_q": 1.37e-15, "ess_A": 2.29e-15, "ess_c": 1.65e-15, "ess_phi": 1.52e-14, "ess_D_max": 5.13e-15,
            "rhat_q": 4.03e-16, "rhat_A": 3.49e-16, "rhat_c": 4.66e-16, "rhat_phi": 3.63e-16, "rhat_D_max": 4.03e-16,
            "mcse_D_max": 2.51e-15}
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


def run_diag(torch, x, status, poison=False):
    """mdfit_nuts_diag on crafted draws -> host diag[T, 6, 12] float64; checks
    on the way that the call only reads and that a second call gives the same bits."""
    from metadamage_amd import _lib, engine

    res, opts = crafted_on_device(torch, x, status)
    T = x.shape[0]
    before = [t.clone() for t in (res.out, res.pred, res.status, res.workspace)]
    if poison:
        _lib.check(_lib.load().mdfit_poison_lds(_stream(torch)))
    diag = engine.nuts_diag_device(res, T, opts)
    again = engine.nuts_diag_device(res, T, opts)
    torch.cuda.synchronize()
    for b, a in zip(before, (res.out, res.pred, res.status, res.workspace)):
        assert torch.equal(b.view(torch.uint8), a.view(torch.uint8))
    assert torch.equal(diag.view(torch.int64), again.view(torch.int64))
    return diag.cpu().numpy()


@pytest.fixture(scope="module")
def crafted(torch_dev):
    """Every crafted shape through the kernel once: {(S, T): diag}, read only."""
    got = {}
    for S, T in cases.SHAPES:
        x, status = cases.case(S, T)
        got[(S, T)] = run_diag(torch_dev, x, status)
        got[(S, T)].setflags(write=False)
    return got


def _compare(got, want, label):
    from tests.test_nuts_diag import compare_to_reference

    print(label, end=": ")
    return compare_to_reference(got, want, TOL)


@pytest.mark.parametrize("S,T", cases.SHAPES)
def test_crafted_draws_vs_reference(crafted, S, T):
    want, tr = cases.reference(S, T)
    assert cases.decision_margin_ok(tr) == []  # the stopping decisions are the data's, not rounding's
    got = crafted[(S, T)]
    _compare(got, want, f"S={S} T={T}")
    (tn, kn), (ts, ks) = cases.faults(T)
    valid = np.ones((T, 6), bool)
    valid[tn, kn] = valid[ts, ks] = False
    assert np.isnan(got[~valid][:, :11]).all() and (got[~valid][:, 11] == 0.0).all()
    assert (got[valid][:, 11] == 1.0).all()
    if S < 4:  # h = 1: no split R-hat while the ESS is defined
        assert np.isnan(got[valid][:, ref.RHAT:ref.RHAT + 5]).all()
    x, _ = cases.case(S, T)
    for t in range(T):
        for k in range(6):
            if not valid[t, k]:
                continue
            for j in range(4):
                kind = cases.kind_of(t, k, j)
                e, r = got[t, k, ref.ESS + j], got[t, k, ref.RHAT + j]
                if kind == "const":
                    assert np.isnan(e) and np.isnan(r)
                    continue
                assert np.isfinite(e) and e > 0.0
                if S >= 63 and kind == "alt":
                    assert abs(e - S * np.log10(S)) <= 1e-9 * e  # the cap
                if S >= 1000 and kind == "arneg05":
                    assert e > S
                if S >= 1000 and kind == "trend":
                    assert r > 2.0
                if S >= 1000 and kind in ("iid", "offset"):
                    assert 0.5 * S < e <= S * np.log10(S) and abs(r - 1.0) < 0.02  # (offset: fails without centring)
            if k not in ref.PMD_SUBFITS:  # D_max of a null sub-fit is its q
                assert np.array_equal(got[t, k, [4, 9]], got[t, k, [0, 5]], equal_nan=True)


def test_poisoned_lds_same_bits(torch_dev, crafted):
    for S, T in ((65, 67), (4096, 3)):
        x, status = cases.case(S, T)
        got = run_diag(torch_dev, x, status, poison=True)
        assert np.array_equal(got.view(np.int64), crafted[(S, T)].view(np.int64))


def test_record_does_not_depend_on_the_batch(torch_dev, crafted):
    x, status = cases.case(65, 67)
    for t in (0, 1, 2, 31, 66):
        one = run_diag(torch_dev, x[t:t + 1], status[t:t + 1])
        assert np.array_equal(one[0].view(np.int64), crafted[(65, 67)][t].view(np.int64)), t


# --------------------------------------------------------------------------
# real chains, small
# --------------------------------------------------------------------------
def _small_opts():
    from metadamage_amd import _lib

    return _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=100, num_samples=200)


def _flags_out(diag64, out):
    """The f32 block as the chunked dispatch hands it out: the records rounded,
    flags = valid + 2 * the chain's divergence count."""
    from metadamage_amd import _lib

    d = diag64.astype(np.float32)
    d[:, :, 11] += (2.0 * np.nan_to_num(out[:, _lib.F_DIAG + 7::_lib.DIAG_STRIDE])).astype(np.float32)
    return d


@pytest.fixture(scope="module")
def small_chains(torch_dev):
    """generate(8, seed=21) fitted by one NUTS call (warmup 100, samples 200),
    its diag records and draws, and the reference on those draws."""
    torch = torch_dev
    from metadamage_amd import _lib, engine
    from metadamage_amd.synthetic import generate

    b = generate(8, seed=21)
    opts = _small_opts()
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    res = engine.fit_batch_device(ty, tN, tm, opts)
    diag = engine.nuts_diag_device(res, 8, opts)
    torch.cuda.synchronize()
    out, pred, st = res.out.cpu().numpy(), res.pred.cpu().numpy(), res.status.cpu().numpy()
    draws = engine.samples_view(res, 8, opts).cpu().numpy()
    diag = diag.cpu().numpy()
    want, tr = ref.diag_rows(draws, out[:, _lib.F_DIAG + 6::_lib.DIAG_STRIDE], trace=True)
    for a in (out, pred, st, draws, diag, want):
        a.setflags(write=False)
    return b, out, pred, st, draws, diag, want, tr


def test_real_chains_vs_reference(small_chains):
    b, out, pred, st, draws, diag, want, tr = small_chains
    assert (st == 0).all() and (diag[:, :, 11] == 1.0).all(), (st, diag[:, :, 11])
    assert cases.decision_margin_ok(tr) == []
    _compare(diag, want, "real chains")
    for k in range(6):
        if k in ref.PMD_SUBFITS:
            assert np.isfinite(diag[:, k, :11]).all()
        else:  # null sub-fits store A = c = 0: constant series
            assert (draws[:, k, :, 1:3] == 0.0).all()
            assert np.isnan(diag[:, k][:, [1, 2, 6, 7]]).all()
            assert np.isfinite(diag[:, k][:, [0, 3, 4, 5, 8, 9, 10]]).all()
    assert (diag[:, :, ref.ESS:ref.ESS + 5][np.isfinite(diag[:, :, ref.ESS:ref.ESS + 5])] > 1.0).all()


def test_feature_is_additive_and_chunks_agree(torch_dev, monkeypatch, small_chains):
    from metadamage_amd import _lib, engine, fits

    b, out, pred, st, draws, diag, want, _ = small_chains
    opts = _small_opts()
    p = fits.Packed(b.tax_id, b.tax_id.astype(str), np.full(8, "species"), b.N_alignments, b.y, b.N, b.mm)
    plain = fits.fit_packed(p, opts, shard=False)
    with_diag = fits.fit_packed(p, opts, shard=False, diag=True)
    assert len(plain) == 3 and len(with_diag) == 4
    for a, c in zip(plain, with_diag):
        assert a.dtype == c.dtype and np.array_equal(a.view(np.uint8), c.view(np.uint8))
    assert np.array_equal(plain[0], out[:, :25], equal_nan=True) and np.array_equal(plain[2], st)
    want32 = _flags_out(diag, out)
    assert with_diag[3].dtype == np.float32 and with_diag[3].shape == (8, 6, 12)
    assert np.array_equal(with_diag[3].view(np.int32), want32.view(np.int32))
    # three chunks reuse the one workspace: each chunk's diag runs before the next chunk's fit
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "3")
    assert len(engine.plan_chunks(8, opts)) == 3
    o3, p3, s3, d3 = engine.fit_batch_host(b.y, b.N, b.mm, opts, diag=True)
    assert np.array_equal(d3.view(np.int32), want32.view(np.int32))
    assert np.array_equal(o3, plain[0], equal_nan=True) and np.array_equal(s3, st)
    fitter = engine.ChunkedFitter(3, opts=opts, with_diag=True)
    o4, p4, s4, d4 = fitter.run(b.y, b.N, b.mm, opts)
    assert np.array_equal(d4.view(np.int32), want32.view(np.int32))
    with pytest.raises(ValueError):
        fitter.run(b.y, b.N, b.mm, _lib.default_opts(mode=_lib.MODE_MAP))
    # the frame: divergences are the sum of the six slots
    import types

    df = fits.make_df_fit_results(p, with_diag[0], st == 0, types.SimpleNamespace(shortname="x"), diag=with_diag[3])
    np.testing.assert_array_equal(df["divergences"].to_numpy(),
                                  out[:, _lib.F_DIAG + 7::_lib.DIAG_STRIDE].sum(axis=1).astype(np.uint32))
    assert (df["nuts_diag_valid"] == 1).all()


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
        res = fits.fit_packed(p, opts, shard=True, diag=True)
        q.put((rank, None if res is None else [np.asarray(a) for a in res]))
    except Exception as e:  # surfaced by the parent
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_sharded_diag_equals_single_process(torch_dev):
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
    out, pred, st, diag = got[0]
    b = generate(T, seed=23)
    p = fits.Packed(b.tax_id, b.tax_id.astype(str), np.full(T, "species"), b.N_alignments, b.y, b.N, b.mm)
    opts = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=20, num_samples=40)
    ref_out, ref_pred, ref_st, ref_diag = fits.fit_packed(p, opts, shard=False, diag=True)
    assert diag.shape == (T, 6, 12) and diag.dtype == np.float32
    assert np.array_equal(diag.view(np.int32), ref_diag.view(np.int32))
    assert np.array_equal(st, ref_st) and np.array_equal(pred, ref_pred, equal_nan=True)
    assert np.array_equal(out, round_like_gather(ref_out), equal_nan=True)


# --------------------------------------------------------------------------
# CLI
# --------------------------------------------------------------------------
def test_cli_nuts_diag(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import _lib, engine, fits, io
    from metadamage_amd.cli import cli_app
    from tests.test_nuts_diag import FLOAT_COLUMNS, UINT_COLUMNS, _cfg

    def run(out_dir, inference):
        r = CliRunner().invoke(cli_app, ["fit", "--out-dir", str(out_dir), "--inference", inference, "--max-fits", "10",
                                         str(GOLDEN / "data_ancient.txt")])
        assert r.exit_code == 0, (r.output, r.exception)
        return io.Parquet(out_dir / "fit_results" / "data_ancient.parquet")

    pq = run(tmp_path / "diag", "nuts-diag")
    df = pq.load()
    assert len(df.columns) == 49 and list(df.columns[30:]) == FLOAT_COLUMNS + UINT_COLUMNS
    assert pq.load_metadata()["inference"] == "nuts-diag"
    plain = run(tmp_path / "plain", "nuts").load()
    assert len(plain.columns) == 30
    pd.testing.assert_frame_equal(df[plain.columns], plain)  # value for value
    ok = df["nuts_diag_valid"] == 1
    assert ok.all()
    for c in FLOAT_COLUMNS:
        assert df[c].dtype == np.float32 and np.isfinite(df.loc[ok, c]).all(), c
    assert (df["ess_min"] <= df["ess_D_max"]).all() and (df["rhat_max"] >= df["rhat_D_max"]).all()
    # divergences: the sum of the six diagnostic slots of the same fit
    cfg = _cfg(tmp_path, "nuts-diag")
    p = fits.pack_counts(pd.read_parquet(GOLDEN / "counts_data_ancient.parquet"), cfg)
    out, _, st = engine.fit_batch(p.y, p.N, p.mm, fits.make_opts(cfg, dict(num_warmup=500, num_samples=1000)))
    assert (st == 0).all() and list(p.tax_id) == list(df["tax_id"])
    np.testing.assert_array_equal(out[:, 0].astype(np.float32), df["D_max"].to_numpy())  # the same chains
    np.testing.assert_array_equal(df["divergences"].to_numpy(),
                                  out[:, _lib.F_DIAG + 7::_lib.DIAG_STRIDE].sum(axis=1).astype(np.uint32))
