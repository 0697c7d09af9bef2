"""GPU tests of the auto inference with the posterior predictive (MDFIT-AUTO
v1.1): mdfit_auto_route_pred against tests/auto_pred_ref.py on
the crafted records and on the device's own records, and engine.fit_auto_device
/ fits.fit_packed / the CLI with auto_pred end to end: a sampled row is the plain
NUTS call's, a settled row the MAP call's with the 14 composed columns and the 90
prediction floats, under any chunking; without auto_pred the call is today's."""

from __future__ import annotations

import numpy as np
import pytest

from tests import auto_pred_ref as ref
from tests import auto_ref as v1
from tests.test_gpu_auto import BASE3, N3, S3, W3, _b32, _b64, _opts3, torch_dev  # noqa: F401  (torch_dev: fixture)

pytestmark = pytest.mark.gpu

T3, ADAPT3, RPRED3 = 48, 3, 100


def test_route_pred_kernel_equals_reference(torch_dev):
    from metadamage_amd import engine

    torch = torch_dev
    st, psis, waic, prec, ppred, out, pred = ref.crafted()
    assert len(st) == 288  # a second block of the one-thread-per-taxon kernel, its tail unfilled
    for with_pred in (True, False):
        want_route, want_out, want_pred = ref.auto_route_pred(st, psis, waic, prec, ppred, out,
                                                              pred if with_pred else None)
        d_out = torch.from_numpy(out.copy()).cuda()
        d_pred = torch.from_numpy(pred.copy()).cuda().reshape(-1, 3, 30) if with_pred else None
        res = engine.FitBatch(d_out, d_pred, torch.from_numpy(st).cuda())
        d_in = [torch.from_numpy(a.copy()).cuda() for a in (psis, waic, prec, ppred)]
        route = engine.auto_route_pred_device(res, *d_in)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(route.cpu().numpy(), want_route)
        np.testing.assert_array_equal(_b64(d_out), want_out.view(np.int64))
        if with_pred:
            np.testing.assert_array_equal(_b32(d_pred).reshape(-1, 90), want_pred.view(np.int32))
        for a, d in zip((psis, waic, prec), d_in):  # the records are read only
            assert np.array_equal(_b64(d), a.view(np.int64))
        assert np.array_equal(_b32(d_in[3]), ppred.view(np.int32))
    assert set(want_route) == {a | b | c | d for a in (0, 1) for b in (0, 2) for c in (0, 4) for d in (0, 16)} | {8}


@pytest.fixture(scope="module")
def batch3(torch_dev):
    """The first 48 taxa of generate(300, 21): the auto call with auto_pred, and
    beside it the auto call without, the MAP call with its psis / waic / pred
    records and the plain NUTS call (computed once, read only)."""
    from metadamage_amd import engine
    from metadamage_amd.synthetic import generate

    torch = torch_dev
    b = generate(300, seed=21)
    y, N, mm = b.y[:T3], b.N[:T3], b.mm[:T3]
    ty, tN, tm = engine.to_device_counts(y, N, mm)
    opts = _opts3()
    timings, timings0 = {}, {}
    res, route, auto = engine.fit_auto_device(ty, tN, tm, opts, S3, timings=timings, psis_adapt=ADAPT3,
                                              auto_pred=True, pred_draws=RPRED3)
    res0, route0, auto0 = engine.fit_auto_device(ty, tN, tm, opts, S3, timings=timings0, psis_adapt=ADAPT3)
    o_map, o_nuts = engine.auto_opts(opts)
    m = engine.fit_batch_device(ty, tN, tm, o_map)
    psis, ad = engine.map_psis_device(ty, tN, m, S3, 0, BASE3, adapt_rounds=ADAPT3)
    waic, _ = engine.map_waic_device(ty, tN, m, S3, 0, BASE3, adapt_rounds=ADAPT3)
    ppred, prec, _ = engine.map_pred_device(ty, tN, m, S3, RPRED3, 0, BASE3, adapt_rounds=ADAPT3)
    nuts = engine.fit_batch_device(ty, tN, tm, o_nuts)
    torch.cuda.synchronize()
    host = {"y": y, "N": N, "mm": mm, "timings": timings, "timings0": timings0, "route": route.cpu().numpy(),
            "auto": auto.cpu().numpy(), "auto_pred": res.auto_pred.cpu().numpy(), "adapt": res.adapt.cpu().numpy(),
            "out": res.out.cpu().numpy(), "pred": _b32(res.pred), "status": res.status.cpu().numpy(),
            "route0": route0.cpu().numpy(), "auto0": auto0.cpu().numpy(), "out0": res0.out.cpu().numpy(),
            "pred0": _b32(res0.pred), "status0": res0.status.cpu().numpy(), "has_auto_pred0": res0.auto_pred is not None,
            "map_out": m.out.cpu().numpy(), "map_pred": _b32(m.pred), "map_status": m.status.cpu().numpy(),
            "psis": psis.cpu().numpy(), "waic": waic.cpu().numpy(), "prec": prec.cpu().numpy(),
            "ppred": ppred.cpu().numpy(), "psis_adapt": ad.cpu().numpy(),
            "nuts_out": nuts.out.cpu().numpy(), "nuts_pred": _b32(nuts.pred), "nuts_status": nuts.status.cpu().numpy()}
    for a in host.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return host


def test_auto_pred_end_to_end(batch3):
    from metadamage_amd import _lib, engine

    h = batch3
    route, out = h["route"], h["out"]
    want_route, want_out, want_pred = ref.auto_route_pred(h["map_status"], h["psis"], h["waic"], h["prec"],
                                                          h["ppred"], h["map_out"], h["map_pred"].view(np.float32))
    np.testing.assert_array_equal(route, want_route)
    # by the bit identity of the pred and psis records the flags half of bit 16 needs bit 2
    pf = h["prec"][:, 15].astype(int)
    assert not ((pf & 2) == 0)[(route & (2 | 8)) == 0].any()
    sampled = (route & _lib.ROUTE_SAMPLE_PRED) != 0
    settled = route == 0
    flags = h["psis"][:, :, 15].astype(int)
    adapted = settled & ((flags & _lib.MAPPSIS_ADAPTED) != 0).any(axis=1)
    print(f"sampled {int(sampled.sum())} of {T3}; settled {int(settled.sum())}, {int(adapted.sum())} of them adapted; "
          f"routes {np.bincount(route, minlength=24).tolist()}; stages {h['timings']}")
    assert settled.sum() >= 4 and adapted.sum() >= 1 and np.array_equal(settled | (route == 8), ~sampled)
    assert np.array_equal(adapted, settled & ((pf & _lib.MAPPSIS_ADAPTED) != 0))
    assert h["timings"]["n_sampled"] == int(sampled.sum()) and h["timings"]["pred"] > 0.0
    assert set(h["timings"]) == set(engine.AUTO_STAGES) | {"pred", "n_sampled", "n_sub_chunks", "n_taxa"}
    # sampled rows: the rows of one plain NUTS call over all 48 taxa, bit for bit
    assert np.array_equal(out[sampled].view(np.int64), h["nuts_out"][sampled].view(np.int64))
    assert np.array_equal(h["pred"][sampled], h["nuts_pred"][sampled])
    assert np.array_equal(h["status"][sampled], h["nuts_status"][sampled])
    # settled rows: the 14 columns from the psis / waic / pred fields, every other column the MAP call's
    u = settled
    psis, waic, prec = h["psis"], h["waic"], h["prec"]
    F, P, Q = _lib.RESULT_FIELDS.index, _lib.MAPPSIS_FIELDS.index, _lib.MAPPRED_FIELDS.index
    cols = {F("q_mean"): psis[:, 0, P("q_mean")], F("concentration_mean"): psis[:, 0, P("phi_mean")],
            F("D_max_marginalized_mean"): psis[:, 0, P("D_max_mean")], F("q_mean_forward"): psis[:, 1, P("q_mean")],
            F("q_mean_reverse"): psis[:, 2, P("q_mean")], F("n_sigma"): waic[:, 6, 0],
            F("n_sigma_forward"): waic[:, 6, 1], F("n_sigma_reverse"): waic[:, 6, 2], F("asymmetry"): waic[:, 6, 3]}
    for name in _lib.AUTO_PRED_COMPOSED_FIELDS:
        cols[F(name)] = prec[:, Q(name)]
    assert len(cols) == 14
    for col, v in cols.items():
        assert np.array_equal(out[u, col].view(np.int64), np.ascontiguousarray(v[u]).view(np.int64)), col
    rest = [c for c in range(_lib.NOUT) if c not in cols]
    assert np.array_equal(np.ascontiguousarray(out[u][:, rest]).view(np.int64),
                          np.ascontiguousarray(h["map_out"][u][:, rest]).view(np.int64))
    assert np.array_equal(out[u].view(np.int64), want_out[u].view(np.int64))
    assert np.array_equal(h["pred"][u].reshape(-1, 90), h["ppred"][u].reshape(-1, 90).view(np.int32))
    assert np.array_equal(h["pred"][u].reshape(-1, 90), want_pred[u].view(np.int32))
    assert np.array_equal(h["status"][u], h["map_status"][u])
    assert (out[u][:, sorted(cols)] != h["map_out"][u][:, sorted(cols)]).any(axis=0).all()  # (the copies were made)
    # the window: lower <= D_max <= upper, and not narrower than the mode's on the whole
    live = u & (h["N"][:, 0] > 0)
    lo, mid, hi = out[live, F("D_max_lower_hpdi")], out[live, F("D_max")], out[live, F("D_max_upper_hpdi")]
    assert live.sum() >= 4 and (lo <= mid).all() and (mid <= hi).all()
    w_map = h["map_out"][live, F("D_max_upper_hpdi")] - h["map_out"][live, F("D_max_lower_hpdi")]
    ratio = float(np.median((hi - lo) / w_map))
    print(f"composed window / MAP window over {int(live.sum())} settled taxa: median {ratio:.3f}")
    assert ratio >= 1.0
    # the blocks
    a, ap = h["auto"], h["auto_pred"]
    assert a.dtype == np.float32 and a.shape == (T3, _lib.NAUTO)
    assert np.array_equal(a[:, 0], route.astype(np.float32)) and np.array_equal(a[:, 1], sampled.astype(np.float32))
    assert np.array_equal(a[:, 2:4].view(np.int32), waic[:, 6, 4:6].astype(np.float32).view(np.int32))
    assert ap.dtype == np.float32 and ap.shape == (T3, _lib.NAUTOPRED) and np.isnan(ap[sampled]).all()
    assert np.array_equal(ap[u, 0], prec[u, Q("ess_all"):Q("ess_all") + 3].min(axis=1).astype(np.float32))
    assert np.array_equal(ap[u, 1], prec[u, Q("n_distinct_all"):Q("n_distinct_all") + 3].min(axis=1).astype(np.float32))
    pa = np.where(np.isnan(h["psis_adapt"]), -np.inf, h["psis_adapt"])[:, :, [0, 2]].max(axis=1)
    want_ad = np.where(np.isneginf(pa), np.nan, pa).astype(np.float32)
    assert np.array_equal(h["adapt"], want_ad, equal_nan=True)


def test_without_auto_pred_the_call_is_todays(batch3):
    from metadamage_amd import _lib, engine

    h = batch3
    want_route, want_out = v1.auto_route(h["map_status"], h["psis"], h["waic"], h["map_out"])
    np.testing.assert_array_equal(h["route0"], want_route)
    s0 = (h["route0"] & _lib.ROUTE_SAMPLE) != 0
    assert np.array_equal(h["out0"][s0].view(np.int64), h["nuts_out"][s0].view(np.int64))
    assert np.array_equal(h["out0"][~s0].view(np.int64), want_out[~s0].view(np.int64))
    assert np.array_equal(h["pred0"][s0], h["nuts_pred"][s0]) and np.array_equal(h["pred0"][~s0], h["map_pred"][~s0])
    assert np.array_equal(h["status0"][s0], h["nuts_status"][s0])
    assert not h["has_auto_pred0"] and "pred" not in h["timings0"]
    assert set(h["timings0"]) == set(engine.AUTO_STAGES) | {"n_sampled", "n_sub_chunks", "n_taxa"}
    # the sampled sets differ by MDFIT_ROUTE_PRED only
    np.testing.assert_array_equal(h["route"] & ~np.int32(_lib.ROUTE_PRED), h["route0"])
    s1 = (h["route"] & _lib.ROUTE_SAMPLE_PRED) != 0
    assert np.array_equal(s1 & ~s0, h["route"] == _lib.ROUTE_PRED) and not (s0 & ~s1).any()
    assert np.array_equal(h["auto"][:, 2:].view(np.int32), h["auto0"][:, 2:].view(np.int32))


def _packed(h):
    from metadamage_amd import fits

    T = len(h["y"])
    names = np.array([f"t{i}" for i in range(T)])
    return fits.Packed(np.arange(T), names, np.array(["species"] * T), np.full(T, 100, np.int64),
                       np.array(h["y"]), np.array(h["N"]), np.array(h["mm"]))


def test_two_chunks_equal_one_and_the_gather_carries_the_block(torch_dev, batch3, monkeypatch):
    import torch.distributed as dist

    from metadamage_amd import blocks, distributed as d, fits

    h = batch3
    kw = dict(shard=False, auto=True, psis_draws=S3, psis_adapt=ADAPT3, auto_pred=True, pred_draws=RPRED3)
    monkeypatch.delenv("MDFIT_CHUNK_TAXA", raising=False)
    one = fits.fit_packed(_packed(h), _opts3(), **kw)
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "25")
    two = fits.fit_packed(_packed(h), _opts3(), **kw)
    assert len(one) == len(two) == 6  # out, pred, status, auto, auto_pred, adapt
    for a, b in zip(one, two):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    out, pred, status, auto, apred, adapt = one
    assert np.array_equal(out.view(np.int64), np.ascontiguousarray(h["out"][:, :25]).view(np.int64))
    assert np.array_equal(pred.view(np.int32), h["pred"]) and np.array_equal(status, h["status"])
    assert np.array_equal(auto.view(np.int32), h["auto"].view(np.int32))
    assert np.array_equal(apred.view(np.int32), h["auto_pred"].view(np.int32))
    assert np.array_equal(adapt.view(np.int32), h["adapt"].view(np.int32))
    plain = fits.fit_packed(_packed(h), _opts3(), shard=False, auto=True, psis_draws=S3, psis_adapt=ADAPT3)
    assert len(plain) == 5  # (without auto_pred: today's five arrays)
    assert np.array_equal(plain[0].view(np.int64), np.ascontiguousarray(h["out0"][:, :25]).view(np.int64))
    # the sharded path of a world of one: the gather record carries the block behind the auto block
    monkeypatch.delenv("MDFIT_CHUNK_TAXA", raising=False)
    assert not (dist.is_available() and dist.is_initialized())
    dev = torch_dev.device("cuda", torch_dev.cuda.current_device())
    run = blocks.describe(_opts3(), {"psis_adapt": ADAPT3, "auto_pred": True}, with_auto=True, psis_draws=S3,
                          pred_draws=RPRED3)
    got = fits._fit_sharded(_packed(h), _opts3(), dev, 0, 1, run)
    assert len(got) == 6
    assert np.array_equal(got[0], d.round_like_gather(out), equal_nan=True)
    for a, b in zip(got[1:], one[1:]):
        assert a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                                     np.ascontiguousarray(b).view(np.uint8))


def test_rejections(torch_dev, batch3):
    from metadamage_amd import engine, fits

    ty, tN, tm = engine.to_device_counts(np.array(batch3["y"][:4]), np.array(batch3["N"][:4]), np.array(batch3["mm"][:4]))
    res = engine.alloc_outputs(4, with_pred=False)
    with pytest.raises(ValueError, match="res.pred"):
        engine.fit_auto_device(ty, tN, tm, _opts3(), S3, res=res, auto_pred=True)
    with pytest.raises(ValueError, match="auto_pred"):
        fits.fit_packed(_packed(batch3), _opts3(), shard=False, ppred=True, auto_pred=True)


def test_cli_auto_pred(tmp_path, torch_dev):
    import pandas as pd
    from typer.testing import CliRunner

    from metadamage_amd import fits, io
    from metadamage_amd.cli import cli_app
    from tests.helpers import GOLDEN
    from tests.test_auto import NEW_COLUMNS

    def run(out_dir, *args):
        r = CliRunner().invoke(cli_app, ["fit", "--out-dir", str(out_dir), *args, str(GOLDEN / "data_ancient.txt")])
        assert r.exit_code == 0, (r.output, r.exception)
        return io.Parquet(out_dir / "fit_results" / "data_ancient.parquet")

    args = ("--inference", "auto", "--auto-pred", "--psis-adapt", "3")
    out_dir = tmp_path / "auto-pred"
    pq = run(out_dir, *args)
    df = pq.load()
    assert list(df.columns[30:]) == NEW_COLUMNS + fits.AUTO_PRED_COLUMNS + fits.ADAPT_COLUMNS and len(df.columns) == 38
    meta = pq.load_metadata()
    assert meta["inference"] == "auto" and int(meta["psis_adapt"]) == 3 and int(meta["pred_draws"]) == 1000
    assert meta["auto_pred"] is True
    assert df["pred_ess_min"].dtype == np.float32 and df["pred_distinct_min"].dtype == np.uint32
    s = df["auto_sampled"].to_numpy() == 1
    assert ((df["auto_route"].to_numpy() & 23) != 0).tolist() == s.tolist()
    assert (df.loc[s, "pred_distinct_min"] == 0).all() and np.isnan(df.loc[s, "pred_ess_min"]).all()
    assert (df.loc[~s, "pred_distinct_min"] > 1).all() and (df.loc[~s, "pred_ess_min"] > 1).all()
    plain = run(tmp_path / "auto", "--inference", "auto", "--psis-adapt", "3").load()
    assert list(plain.columns) == [c for c in df.columns if c not in fits.AUTO_PRED_COLUMNS]
    pa = io.Parquet(out_dir / "fit_predictions" / "data_ancient.parquet").load()
    pb = io.Parquet(tmp_path / "auto" / "fit_predictions" / "data_ancient.parquet").load()
    assert list(pa.columns) == list(pb.columns) and len(pa) == 30 * len(df)  # no column is renamed or added
    if (~s).any():
        # a settled taxon: the composed D_max is the first position's composed median
        first = pa["position"].to_numpy() == 1
        np.testing.assert_array_equal(pa.loc[first, "median"].to_numpy()[~s], df.loc[~s, "D_max"].to_numpy())
        both = ~s & (plain["auto_sampled"].to_numpy() == 0)
        keep = [c for c in plain.columns if c not in ("D_max", "D_max_lower_hpdi", "D_max_upper_hpdi",
                                                      "D_max_forward", "D_max_reverse")]
        pd.testing.assert_frame_equal(df.loc[both, keep].reset_index(drop=True),
                                      plain.loc[both, keep].reset_index(drop=True))
    f = out_dir / "fit_results" / "data_ancient.parquet"
    m1 = f.stat().st_mtime_ns
    run(out_dir, *args)  # cache hit: file untouched
    assert f.stat().st_mtime_ns == m1
    pq2 = run(out_dir, *args, "--pred-draws", "100")  # other draws: the cache is not reused
    assert f.stat().st_mtime_ns != m1 and int(pq2.load_metadata()["pred_draws"]) == 100
