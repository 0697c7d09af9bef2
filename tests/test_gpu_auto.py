"""GPU tests of the auto inference (MDFIT-AUTO v1):
mdfit_fit_batch_indexed against the rows of the plain call bit for bit,
mdfit_auto_route against tests/auto_ref.py on the crafted records, and
engine.fit_auto_device / fits.fit_packed(auto=True) end to end: every sampled row
is the plain NUTS call's, every other row the MAP call's with the nine
importance-sampled columns, under any chunking."""

from __future__ import annotations

import numpy as np
import pytest

from tests import auto_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    return torch


def _b64(t):
    return t.detach().cpu().contiguous().numpy().view(np.int64)


def _b32(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


# --------------------------------------------------------------------------
# 1. indexed equals full
# --------------------------------------------------------------------------
T1, W1, S1, BASE1 = 48, 50, 64, 1000
# 7 x 6 chains: no multiple of the 4 chain slots of a wave
SUBSETS = {"scattered": [1, 5, 12, 20, 29, 37, 46], "permuted": [29, 1, 46, 12, 37, 5, 20], "single": [23],
           "all": list(range(T1))}


@pytest.fixture(scope="module")
def full_call(torch_dev):
    """One plain mdfit_fit_batch call over 48 synthetic taxa (computed once, read only)."""
    from metadamage_amd import _lib, engine
    from metadamage_amd.synthetic import generate

    torch = torch_dev
    b = generate(T1, seed=7)
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    opts = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=W1, num_samples=S1, index_base=BASE1)
    res = engine.fit_batch_device(ty, tN, tm, opts)
    torch.cuda.synchronize()
    draws = engine.samples_view(res, T1, opts)
    return {"ty": ty, "tN": tN, "tm": tm, "opts": opts, "out": _b64(res.out), "pred": _b32(res.pred),
            "status": res.status.cpu().numpy(), "draws": _b64(draws)}


def _indexed(torch, full, idx, with_index=True):
    from metadamage_amd import engine

    sel = torch.as_tensor(idx, dtype=torch.int64, device=full["ty"].device)
    sy, sN, sm = (full[k].index_select(0, sel) for k in ("ty", "tN", "tm"))
    res = engine.fit_batch_indexed_device(sy, sN, sm, sel if with_index else None, full["opts"])  # its own workspace
    torch.cuda.synchronize()
    draws = engine.samples_view(res, len(idx), full["opts"])
    return _b64(res.out), _b32(res.pred), res.status.cpu().numpy(), _b64(draws)


@pytest.mark.parametrize("name", list(SUBSETS))
def test_indexed_rows_equal_the_full_call(torch_dev, full_call, name):
    idx = SUBSETS[name]
    out, pred, status, draws = _indexed(torch_dev, full_call, idx)
    assert np.array_equal(out, full_call["out"][idx])
    assert np.array_equal(pred, full_call["pred"][idx])
    assert np.array_equal(status, full_call["status"][idx])
    assert np.array_equal(draws, full_call["draws"][idx])
    assert (full_call["status"] == 0).all() and np.isfinite(full_call["draws"].view(np.float64)).all()


def test_null_index_is_the_plain_call_and_the_index_is_used(torch_dev, full_call):
    out, pred, status, draws = _indexed(torch_dev, full_call, SUBSETS["all"], with_index=False)
    assert np.array_equal(out, full_call["out"]) and np.array_equal(pred, full_call["pred"])
    assert np.array_equal(status, full_call["status"]) and np.array_equal(draws, full_call["draws"])
    # the subset without its index draws row t's numbers from stream index_base + t: other draws
    idx = SUBSETS["scattered"]
    _, _, _, plain = _indexed(torch_dev, full_call, idx, with_index=False)
    assert (plain != full_call["draws"][idx]).any()
    # duplicate indices draw the same numbers: the same data under one index twice
    o2, p2, s2, d2 = _indexed(torch_dev, full_call, [12, 12])
    assert np.array_equal(o2[0], o2[1]) and np.array_equal(d2[0], d2[1]) and np.array_equal(p2[0], p2[1])
    assert np.array_equal(o2[0], full_call["out"][12])


def test_map_mode_rejects_an_index(torch_dev, full_call):
    from metadamage_amd import _lib, engine

    sel = torch_dev.arange(4, dtype=torch_dev.int64, device=full_call["ty"].device)
    with pytest.raises(_lib.MdfitError, match="taxon_index"):
        engine.fit_batch_indexed_device(full_call["ty"][:4], full_call["tN"][:4], None, sel,
                                        _lib.default_opts(mode=_lib.MODE_MAP))


# --------------------------------------------------------------------------
# 2. route on the device
# --------------------------------------------------------------------------
def test_route_kernel_equals_reference(torch_dev):
    from metadamage_amd import engine

    torch = torch_dev
    st, psis, waic, out = ref.crafted()
    # 6 copies: 288 taxa, a second block of the one-thread-per-taxon kernel, its tail unfilled
    st, psis, waic, out = (np.concatenate([a] * 6) for a in (st, psis, waic, out))
    want_route, want_out = ref.auto_route(st, psis, waic, out)
    d_out = torch.from_numpy(out).cuda()
    res = engine.FitBatch(d_out, None, torch.from_numpy(st).cuda())
    d_psis, d_waic = torch.from_numpy(psis).cuda(), torch.from_numpy(waic).cuda()
    route = engine.auto_route_device(res, d_psis, d_waic)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(route.cpu().numpy(), want_route)
    np.testing.assert_array_equal(_b64(d_out), want_out.view(np.int64))
    assert np.array_equal(_b64(d_psis), psis.view(np.int64)) and np.array_equal(_b64(d_waic), waic.view(np.int64))
    for want in range(9):
        assert (want_route == want).any()


# --------------------------------------------------------------------------
# 3. end to end
# --------------------------------------------------------------------------
# tools/auto_pick_taxa.py: of generate(400, seed=21), row by row (the draws are
# keyed by index_base + row), classes cycling deep ancient / shallow ancient /
# control-like, the first candidate whose six reference rows (map_waic_ref on the
# oracle's MAP fit, S = 256, seed 0, index_base 500) are valid and whose largest k
# lies >= 0.1 from the threshold min(1 - 1 / log10 256, 0.7) = 0.5848.  The
# reference's k per pick (20 above the threshold: sampled; 44 below: settled):
PICKS = [7, 3, 5, 16, 36, 6, 24, 57, 9, 29, 64, 11, 31, 71, 14, 37, 80, 18, 39, 101, 19, 41, 118, 20, 47, 153, 21, 49,
         200, 22, 53, 207, 25, 58, 224, 28, 59, 235, 33, 65, 267, 35, 73, 311, 38, 77, 319, 42, 79, 326, 43, 89, 331,
         44, 92, 349, 45, 98, 356, 48, 103, 358, 50, 106]
K_REF = [0.48, 0.31, 0.36, 0.80, -0.01, 0.69, 0.17, 0.39, 63.11, 0.39, 0.17, 0.22, 0.40, 0.45, 0.97, 0.37, 0.45, 0.32,
         5.27, 0.12, 5.72, 0.77, 0.30, 0.35, 0.43, 0.39, 0.90, 0.72, 0.34, 0.35, 0.45, 0.08, 0.38, 0.71, 0.37, 0.69,
         0.00, 0.38, 0.75, -0.10, 0.69, 0.81, 0.33, 0.73, 0.31, -0.00, 0.35, 0.85, 0.76, 0.19, 128.50, 0.75, 0.27,
         0.46, 0.25, 0.24, 10.40, 0.26, 0.38, 0.48, 0.40, 0.18, 0.44, 0.26]
S3, W3, N3, BASE3, TAU3 = 256, 100, 100, 500, 0.5848


def _opts3(**kw):
    from metadamage_amd import _lib

    return _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=W3, num_samples=N3, seed=0, index_base=BASE3, **kw)


@pytest.fixture(scope="module")
def batch3(torch_dev):
    """The 64 picked taxa: the auto call, and beside it the MAP call with its
    psis / waic records and the plain NUTS call over all 64 (computed once, read
    only)."""
    from metadamage_amd import _lib, engine
    from metadamage_amd.synthetic import generate

    torch = torch_dev
    b = generate(400, seed=21)
    y, N, mm = b.y[PICKS], b.N[PICKS], b.mm[PICKS]
    ty, tN, tm = engine.to_device_counts(y, N, mm)
    opts = _opts3()
    timings = {}
    res, route, auto = engine.fit_auto_device(ty, tN, tm, opts, S3, timings=timings)
    o_map, o_nuts = engine.auto_opts(opts)
    m = engine.fit_batch_device(ty, tN, tm, o_map)
    psis = engine.map_psis_device(ty, tN, m, S3, 0, BASE3)
    waic = engine.map_waic_device(ty, tN, m, S3, 0, BASE3)
    nuts = engine.fit_batch_device(ty, tN, tm, o_nuts)
    torch.cuda.synchronize()
    host = {"y": y, "N": N, "mm": mm, "timings": timings, "route": route.cpu().numpy(), "auto": auto.cpu().numpy(),
            "out": res.out.cpu().numpy(), "pred": _b32(res.pred), "status": res.status.cpu().numpy(),
            "map_out": m.out.cpu().numpy(), "map_pred": _b32(m.pred), "map_status": m.status.cpu().numpy(),
            "psis": psis.cpu().numpy(), "waic": waic.cpu().numpy(),
            "nuts_out": nuts.out.cpu().numpy(), "nuts_pred": _b32(nuts.pred), "nuts_status": nuts.status.cpu().numpy()}
    for a in host.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return host


def test_auto_end_to_end(batch3):
    from metadamage_amd import _lib

    h = batch3
    route, out = h["route"], h["out"]
    want_route, want_out = ref.auto_route(h["map_status"], h["psis"], h["waic"], h["map_out"])
    np.testing.assert_array_equal(route, want_route)
    assert not ((route & 2) != 0)[(route & 1) == 0].any()  # bit 2 never without bit 1
    sampled = (route & 7) != 0
    print(f"sampled {int(sampled.sum())} of {len(route)}; routes {np.bincount(route, minlength=9).tolist()}; "
          f"stages {h['timings']}")
    assert sampled.sum() >= 4 and (~sampled).sum() >= 4
    # the picks were made for this: the reference's k says which way each taxon goes
    np.testing.assert_array_equal(sampled, np.array(K_REF) > TAU3)
    assert (route[~sampled] == 0).all()  # (no y > N among them)
    assert h["timings"]["n_sampled"] == int(sampled.sum()) and h["timings"]["n_sub_chunks"] >= 1
    # sampled rows: the rows of one plain NUTS call over all 64 taxa, bit for bit
    assert np.array_equal(out[sampled].view(np.int64), h["nuts_out"][sampled].view(np.int64))
    assert np.array_equal(h["pred"][sampled], h["nuts_pred"][sampled])
    assert np.array_equal(h["status"][sampled], h["nuts_status"][sampled])
    # the others: the nine columns from the psis / waic fields, every other column the MAP call's
    u = ~sampled
    psis, waic = h["psis"], h["waic"]
    F, P = _lib.RESULT_FIELDS.index, _lib.MAPPSIS_FIELDS.index
    nine = {F("q_mean"): psis[:, 0, P("q_mean")], F("concentration_mean"): psis[:, 0, P("phi_mean")],
            F("D_max_marginalized_mean"): psis[:, 0, P("D_max_mean")], F("q_mean_forward"): psis[:, 1, P("q_mean")],
            F("q_mean_reverse"): psis[:, 2, P("q_mean")], F("n_sigma"): waic[:, 6, 0],
            F("n_sigma_forward"): waic[:, 6, 1], F("n_sigma_reverse"): waic[:, 6, 2], F("asymmetry"): waic[:, 6, 3]}
    assert sorted(nine) == sorted(F(f) for f in _lib.AUTO_COMPOSED_FIELDS) and len(nine) == 9
    for col, v in nine.items():
        assert np.array_equal(out[u, col].view(np.int64), np.ascontiguousarray(v[u]).view(np.int64)), col
        assert np.isfinite(out[u, col]).all(), col
    rest = [c for c in range(_lib.NOUT) if c not in nine]
    assert np.array_equal(np.ascontiguousarray(out[u][:, rest]).view(np.int64),
                          np.ascontiguousarray(h["map_out"][u][:, rest]).view(np.int64))
    assert np.array_equal(out[u].view(np.int64), want_out[u].view(np.int64))
    assert np.array_equal(h["pred"][u], h["map_pred"][u]) and np.array_equal(h["status"][u], h["map_status"][u])
    # the composed columns are not what MAP left there (the test can tell the copies were made)
    assert (out[u][:, sorted(nine)] != h["map_out"][u][:, sorted(nine)]).any(axis=0).all()
    # the auto block
    a = h["auto"]
    assert a.dtype == np.float32 and a.shape == (64, _lib.NAUTO)
    assert np.array_equal(a[:, 0], route.astype(np.float32)) and np.array_equal(a[:, 1], sampled.astype(np.float32))
    assert np.array_equal(a[:, 2:4].view(np.int32), waic[:, 6, 4:6].astype(np.float32).view(np.int32))


# --------------------------------------------------------------------------
# 4. chunks
# --------------------------------------------------------------------------
def _packed(h):
    from metadamage_amd import fits

    T = len(h["y"])
    names = np.array([f"t{i}" for i in range(T)])
    return fits.Packed(np.arange(T), names, np.array(["species"] * T), np.full(T, 100, np.int64),
                       np.array(h["y"]), np.array(h["N"]), np.array(h["mm"]))


def test_two_chunks_equal_one(batch3, monkeypatch):
    from metadamage_amd import fits

    h = batch3
    monkeypatch.delenv("MDFIT_CHUNK_TAXA", raising=False)
    one = fits.fit_packed(_packed(h), _opts3(), shard=False, auto=True, psis_draws=S3)
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "32")
    two = fits.fit_packed(_packed(h), _opts3(), shard=False, auto=True, psis_draws=S3)
    assert len(one) == len(two) == 4
    for a, b in zip(one, two):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    out, pred, status, auto = one
    # ... and both are the device call of the whole batch
    assert out.shape == (64, 25) and np.array_equal(out.view(np.int64), np.ascontiguousarray(h["out"][:, :25]).view(np.int64))
    assert np.array_equal(pred.view(np.int32), h["pred"]) and np.array_equal(status, h["status"])
    assert np.array_equal(auto.view(np.int32), h["auto"].view(np.int32))


# --------------------------------------------------------------------------
# 5. degenerate splits
# --------------------------------------------------------------------------
def test_all_invalid_launches_no_sampler(torch_dev, batch3):
    from metadamage_amd import engine

    torch = torch_dev
    y, N = np.array(batch3["y"][:8]), np.array(batch3["N"][:8])
    y[:, 3] = N[:, 3] + 1  # some y > N in every row: status 3
    ty, tN, tm = engine.to_device_counts(y, N, np.array(batch3["mm"][:8]))
    timings = {}
    res, route, auto = engine.fit_auto_device(ty, tN, tm, _opts3(), S3, timings=timings)
    m = engine.fit_batch_device(ty, tN, tm, engine.auto_opts(_opts3())[0])
    torch.cuda.synchronize()
    assert (route.cpu().numpy() == 8).all() and (res.status.cpu().numpy() == 3).all()
    assert timings["n_sampled"] == 0 and timings["n_sub_chunks"] == 0 and timings["sampler"] == 0.0
    assert np.array_equal(_b64(res.out), _b64(m.out)) and np.isnan(res.out.cpu().numpy()).all()
    assert np.array_equal(_b32(res.pred), _b32(m.pred)) and np.array_equal(res.status.cpu().numpy(), m.status.cpu().numpy())
    assert (auto[:, 1].cpu().numpy() == 0).all() and (auto[:, 0].cpu().numpy() == 8).all()


def test_all_sampled_equals_the_plain_call(torch_dev, batch3):
    from metadamage_amd import engine

    torch = torch_dev
    T = 12
    ty, tN, tm = engine.to_device_counts(np.array(batch3["y"][:T]), np.array(batch3["N"][:T]), np.array(batch3["mm"][:T]))
    opts = _opts3(max_iter=1)  # no MAP sub-fit converges in one evaluation: status 1, every taxon to the sampler
    timings = {}
    res, route, auto = engine.fit_auto_device(ty, tN, tm, opts, S3, timings=timings)
    nuts = engine.fit_batch_device(ty, tN, tm, engine.auto_opts(opts)[1])
    torch.cuda.synchronize()
    r = route.cpu().numpy()
    assert ((r & 4) != 0).all() and ((r & 7) != 0).all() and timings["n_sampled"] == T
    assert np.array_equal(_b64(res.out), _b64(nuts.out)) and np.array_equal(_b32(res.pred), _b32(nuts.pred))
    assert np.array_equal(res.status.cpu().numpy(), nuts.status.cpu().numpy())
    assert (auto[:, 1].cpu().numpy() == 1).all()
    # ... and they are the rows of the 64-taxon call
    assert np.array_equal(_b64(nuts.out), batch3["nuts_out"][:T].view(np.int64))


# --------------------------------------------------------------------------
# sharded: each rank runs auto on its shard, the auto block travels with the gather
# --------------------------------------------------------------------------
T_SH, S_SH = 61, 64  # ragged shards


def _sharded_inputs():
    from metadamage_amd import _lib, fits
    from metadamage_amd.synthetic import generate

    b = generate(T_SH, seed=23)
    p = fits.Packed(b.tax_id, b.tax_id.astype(str), np.full(T_SH, "species"), b.N_alignments, b.y, b.N, b.mm)
    return p, _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=20, num_samples=40, index_base=7)


def _rank(rank, world, port, q):
    import os

    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)  # both ranks on the one GPU of the box
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from metadamage_amd import fits

        p, opts = _sharded_inputs()
        res = fits.fit_packed(p, opts, shard=True, auto=True, psis_draws=S_SH)
        q.put((rank, None if res is None else [np.asarray(a) for a in res]))
    except Exception as e:  # surfaced by the parent
        q.put((rank, repr(e)))
    finally:
        dist.destroy_process_group()


def test_sharded_auto_equals_single_process(torch_dev):
    import socket

    import torch.multiprocessing as mp

    from metadamage_amd import fits
    from metadamage_amd.distributed import round_like_gather

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    got = dict(q.get(timeout=600) for _ in procs)
    for pr in procs:
        pr.join(timeout=120)
    assert got[1] is None, got[1]
    assert not isinstance(got[0], str), got[0]
    out, pred, st, auto = got[0]
    p, opts = _sharded_inputs()
    ref_out, ref_pred, ref_st, ref_auto = fits.fit_packed(p, opts, shard=False, auto=True, psis_draws=S_SH)
    assert out.shape == (T_SH, 25) and auto.shape == (T_SH, 4) and auto.dtype == np.float32
    assert np.array_equal(st, ref_st)
    assert np.array_equal(out, round_like_gather(ref_out), equal_nan=True)
    assert np.array_equal(pred, ref_pred, equal_nan=True)
    assert np.array_equal(auto, ref_auto, equal_nan=True)
    assert 0 < auto[:, 1].sum() < T_SH  # taxa went both ways


# --------------------------------------------------------------------------
# the CLI path
# --------------------------------------------------------------------------
def test_cli_auto(tmp_path, torch_dev):
    import pandas as pd
    from typer.testing import CliRunner

    from metadamage_amd import _lib, io
    from metadamage_amd.cli import cli_app
    from tests.helpers import GOLDEN
    from tests.test_auto import NEW_COLUMNS

    def run(out_dir, *args):
        r = CliRunner().invoke(cli_app, ["fit", "--out-dir", str(out_dir), *args, str(GOLDEN / "data_ancient.txt")])
        assert r.exit_code == 0, (r.output, r.exception)
        return io.Parquet(out_dir / "fit_results" / "data_ancient.parquet")

    pq = run(tmp_path / "auto", "--inference", "auto")
    df = pq.load()
    assert len(df.columns) == 34 and list(df.columns[30:]) == NEW_COLUMNS
    meta = pq.load_metadata()
    assert meta["inference"] == "auto" and int(meta["psis_draws"]) == 256
    nuts = run(tmp_path / "nuts", "--inference", "nuts").load()
    waic = run(tmp_path / "waic", "--inference", "map-waic").load()
    assert list(df.columns[:30]) == list(nuts.columns) and len(df) == len(nuts) == len(waic)
    s = df["auto_sampled"].to_numpy() == 1
    assert ((df["auto_route"].to_numpy() & 7) != 0).tolist() == s.tolist()
    np.testing.assert_array_equal(df["pareto_k_max"].to_numpy(), waic["pareto_k_waic"].to_numpy())
    np.testing.assert_array_equal(df["psis_ess_min"].to_numpy(), waic["waic_ess_min"].to_numpy())
    # a sampled row is the nuts run's, value for value; a settled one the map run's outside the nine columns,
    # with the WAIC comparisons of the map-waic run in n_sigma x3 and asymmetry
    pd.testing.assert_frame_equal(df.loc[s, nuts.columns].reset_index(drop=True), nuts.loc[s].reset_index(drop=True))
    rest = [c for c in nuts.columns if c not in _lib.AUTO_COMPOSED_FIELDS]
    pd.testing.assert_frame_equal(df.loc[~s, rest].reset_index(drop=True), waic.loc[~s, rest].reset_index(drop=True))
    for name in ("n_sigma", "n_sigma_forward", "n_sigma_reverse"):
        np.testing.assert_array_equal(df.loc[~s, name].to_numpy(), waic.loc[~s, name.replace("n_sigma", "n_sigma_waic")].to_numpy())
    np.testing.assert_array_equal(df.loc[~s, "asymmetry"].to_numpy(), waic.loc[~s, "asymmetry_waic"].to_numpy())
    pa = io.Parquet(tmp_path / "auto" / "fit_predictions" / "data_ancient.parquet").load()
    assert len(pa) == 30 * len(df)
