"""GPU tests of mdfit_map_quant, mdfit_map_quant_adapt and
mdfit_weighted_order_stats (MDFIT-QUANT v1): the device
function against the Python-integer reference on crafted series bit for bit,
the record's identity with mdfit_map_psis, its fields against the reference run
on its own values tap, the tap against the constrained draws, the ordering of
the statistics, the invariance of the records under every way of calling, the
invalid cases, the rejections and the CLI path."""

from __future__ import annotations

import numpy as np
import pandas as pd
import pytest

from tests import map_psis_ref as pref
from tests import map_quant_ref as ref
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

S_A = 256
SEED = 0
D0 = 0.01
# the values tap against map_psis_ref.constrained(u) in longdouble on generate(300, 21), S = 256: the worst relative
# error measured on the MI355X, asserted at four times it (the margin is for other boxes' contraction paths, as in
# test_gpu_map_psis.py)
E2E_MEASURED = {"values": 3.87e-16}
STAT_FIELDS = list(range(12)) + [14]  # the fields the order statistics fill


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


@pytest.fixture(scope="module")
def batch_a(torch_dev):
    """generate(300, seed=21) fitted by one MAP call, its importance-sampled
    posteriors at S = 256 with the draws, and its order statistics with the
    values tap (computed once, read only)."""
    from metadamage_amd import engine
    from metadamage_amd.synthetic import generate

    torch = torch_dev
    b = generate(300, seed=21)
    ty, tN, res = _map_fit(torch, b.y, b.N, b.mm)
    before = res.out.clone()
    psis, draws = engine.map_psis_device(ty, tN, res, S_A, SEED, 0, draws=True)
    quant, values = engine.map_quant_device(ty, tN, res, S_A, SEED, 0, D0, values=True)
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int64), res.out.view(torch.int64))  # the records are read only
    host = {"b": b, "st": res.status.cpu().numpy(), "psis": psis.cpu().numpy(), "draws": draws.cpu().numpy(),
            "quant": quant.cpu().numpy(), "values": values.cpu().numpy()}
    for a in host.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    host.update(ty=ty, tN=tN, res=res)
    return host


def _valid(batch):
    return (batch["psis"][:, :, pref.FLAGS].astype(np.int64) & pref.VALID) != 0


# --------------------------------------------------------------------------
# the device function on crafted series
# --------------------------------------------------------------------------
@pytest.mark.parametrize("S", (25, 65, 256, 1024))
def test_weighted_order_stats_equals_reference_bitwise(torch_dev, S):
    from metadamage_amd import engine

    v, w, d0, kinds, want = ref.case(S)
    for thr in sorted(set(d0.tolist())):  # (one launch per threshold: d0_on_draw has its own)
        rows = np.flatnonzero(d0 == thr)
        got = engine.weighted_order_stats(v[rows], w[rows], thr)
        for i, g in zip(rows, got):
            assert np.array_equal(ref.bits(g), ref.bits(want[i])), (kinds[i], S, g, want[i])


# --------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------
def test_khat_ess_flags_and_weights_are_map_psis(batch_a):
    psis, quant = batch_a["psis"], batch_a["quant"]
    f = ref.FIELDS.index
    for name in ("khat", "ess", "flags"):
        assert np.array_equal(ref.bits(quant[:, :, f(name)]), ref.bits(psis[:, :, pref.FIELDS.index(name)])), name
    assert np.array_equal(ref.bits(batch_a["values"][..., 5]), ref.bits(batch_a["draws"][..., 5]))
    valid = _valid(batch_a)
    assert np.isnan(quant[~valid][:, STAT_FIELDS]).all() and np.isnan(batch_a["values"][~valid]).all()
    assert np.isfinite(quant[valid][:, STAT_FIELDS]).all()


def test_fields_equal_reference_on_the_tap(batch_a):
    quant, values = batch_a["quant"], batch_a["values"]
    valid = _valid(batch_a)
    n = 0
    for t, r in zip(*np.nonzero(valid)):
        want = ref.record_stats(values[t, r, :, :5], values[t, r, :, 5], D0)
        got = quant[t, r]
        assert np.array_equal(ref.bits(got[STAT_FIELDS]), ref.bits(want[STAT_FIELDS])), (t, r, got, want)
        n += 1
    assert n >= 850


def test_tap_values_vs_constrained_draws(batch_a):
    values, draws = batch_a["values"], batch_a["draws"]
    valid = _valid(batch_a)
    worst = 0.0
    for t, r in zip(*np.nonzero(valid)):
        f = pref.constrained(draws[t, r, :, :4])
        want = np.stack([f[:, 1] + f[:, 2], f[:, 0], f[:, 1], f[:, 2], f[:, 3]], axis=1)
        live = values[t, r, :, 5] > 0  # (an infeasible draw's values are not used)
        got = values[t, r, :, :5].astype(pref.LD)
        den = np.abs(want[live])
        err = np.abs(got[live] - want[live]) / np.where(den > 0, den, 1)
        worst = max(worst, float(err.max()))
    print(f"values tap against constrained(u), {int(valid.sum())} rows: worst relative error {worst:.2e}")
    assert worst <= 4.0 * E2E_MEASURED["values"], worst


def test_ordering_and_not_vacuous(batch_a):
    psis, quant = batch_a["psis"], batch_a["quant"]
    f, pf = ref.FIELDS.index, pref.FIELDS.index
    valid = _valid(batch_a)
    flags = psis[:, :, pref.FLAGS].astype(np.int64)
    q = quant[valid]
    p = psis[valid]
    assert (q[:, f("D_max_lo")] <= q[:, f("D_max_median")]).all()
    assert (q[:, f("D_max_median")] <= q[:, f("D_max_hi")]).all()
    assert (q[:, f("D_max_q05")] <= q[:, f("D_max_median")]).all()
    assert (q[:, f("D_max_median")] <= q[:, f("D_max_q95")]).all()
    assert (q[:, f("q_lo")] <= q[:, f("q_median")]).all() and (q[:, f("q_median")] <= q[:, f("q_hi")]).all()
    assert (np.abs(q[:, f("D_max_median")] - p[:, pf("D_max_mean")]) <= p[:, pf("D_max_std")]).all()
    assert ((q[:, f("D_max_p_above")] >= 0) & (q[:, f("D_max_p_above")] <= 1)).all()
    assert ((q[:, f("n_window")] >= 1) & (q[:, f("n_window")] <= S_A)).all()
    n_taxa, n_rel = int(valid.all(axis=1).sum()), int((valid & ((flags & pref.RELIABLE) != 0)).sum())
    n_wide = int((q[:, f("D_max_hi")] > q[:, f("D_max_lo")]).sum())
    print(f"{n_taxa} taxa with all three rows valid, {int(valid.sum())} valid rows, {n_rel} reliable, "
          f"{n_wide} with hi > lo")
    assert n_taxa >= 285 and n_rel >= 700
    assert n_wide >= int(valid.sum()) - 5  # (a window of one draw: one heavy weight)


# --------------------------------------------------------------------------
# invariance
# --------------------------------------------------------------------------
def test_records_do_not_depend_on_the_call(torch_dev, monkeypatch, batch_a):
    torch = torch_dev
    from metadamage_amd import _lib, distributed as d, engine

    b, ty, tN, res, base = batch_a["b"], batch_a["ty"], batch_a["tN"], batch_a["res"], batch_a["quant"]

    def sub(lo, hi):
        return engine.FitBatch(res.out[lo:hi], None, res.status[lo:hi], None)

    # without the tap
    plain = engine.map_quant_device(ty, tN, res, S_A, SEED, 0, D0)
    # two calls split with index_base
    a = engine.map_quant_device(ty[:130], tN[:130], sub(0, 130), S_A, SEED, 0, D0)
    c = engine.map_quant_device(ty[130:], tN[130:], sub(130, 300), S_A, SEED, 130, D0)
    # another threshold moves the exceedance alone
    other = engine.map_quant_device(ty, tN, res, S_A, SEED, 0, 0.05)
    torch.cuda.synchronize()
    assert np.array_equal(ref.bits(plain.cpu().numpy()), ref.bits(base))
    assert np.array_equal(ref.bits(torch.cat([a, c]).cpu().numpy()), ref.bits(base))
    other = other.cpu().numpy()
    fa = ref.FIELDS.index("D_max_p_above")
    rest = [j for j in range(16) if j != fa]
    assert np.array_equal(ref.bits(other[:, :, rest]), ref.bits(base[:, :, rest]))
    valid = _valid(batch_a)
    assert (other[valid][:, fa] <= base[valid][:, fa]).all() and (other[valid][:, fa] < base[valid][:, fa]).any()
    # through the chunked dispatch in two chunks, and into the gather record of a world of one
    opts = _lib.default_opts(mode=_lib.MODE_MAP)
    base32 = base.astype(np.float32).reshape(300, 48)
    psis32 = batch_a["psis"].astype(np.float32)
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "150")
    assert len(engine.plan_chunks(300, opts, with_psis=True, quantiles=True)) == 2
    got = engine.fit_batch_host(b.y, b.N, b.mm, opts, psis=True, psis_draws=S_A, quantiles=True, dmax_threshold=D0)
    assert len(got) == 5 and got[4].shape == (300, 48) and got[4].dtype == np.float32
    assert np.array_equal(got[4].view(np.int32), base32.view(np.int32))
    assert np.array_equal(got[3].view(np.int32), psis32.view(np.int32))
    today = engine.fit_batch_host(b.y, b.N, b.mm, opts, psis=True, psis_draws=S_A)
    assert len(today) == 4
    for x, z in zip(today, got[:4]):
        assert x.dtype == z.dtype and np.array_equal(x, z, equal_nan=True)
    rec = d.alloc_records(300, torch.device("cuda", torch.cuda.current_device()), with_psis=True, with_quant=True)
    fitter = engine.ChunkedFitter(150, opts=opts, dest_on_device=True, with_psis=True, psis_draws=S_A, quantiles=True,
                                  dmax_threshold=D0)
    fitter.run_into_device(b.y, b.N, b.mm, opts,
                           engine.FitBatch(rec.out, rec.pred, rec.status, psis=rec.psis, quant=rec.quant),
                           chunks=engine.plan_chunks(300, opts, chunk_taxa=150))
    buf = rec.stage()
    torch.cuda.synchronize()
    og, pg, sg, psg, qg = d.unpack_gathered(d.gather_records(buf, 300, 0, 1), 300, 1, with_psis=True, with_quant=True)
    assert np.array_equal(qg.view(np.int32), base32.view(np.int32))
    assert np.array_equal(psg.view(np.int32), psis32.view(np.int32))


def test_adapt_entry(torch_dev, batch_a):
    torch = torch_dev
    from metadamage_amd import engine

    ty, tN, res, base = batch_a["ty"], batch_a["tN"], batch_a["res"], batch_a["quant"]
    q0, v0, a0 = engine.map_quant_device(ty, tN, res, S_A, SEED, 0, D0, values=True, adapt=True)
    q3, v3, a3 = engine.map_quant_device(ty, tN, res, S_A, SEED, 0, D0, values=True, adapt_rounds=3)
    p3, d3, pa3 = engine.map_psis_device(ty, tN, res, S_A, SEED, 0, draws=True, adapt_rounds=3)
    torch.cuda.synchronize()
    # no rounds: the plain entry bit for bit
    assert np.array_equal(ref.bits(q0.cpu().numpy()), ref.bits(base))
    assert np.array_equal(ref.bits(v0.cpu().numpy()), ref.bits(batch_a["values"]))
    # three rounds: khat, ess, flags, the weights and the adapt rows are mdfit_map_psis_adapt's
    q3, v3, a3, p3, d3, pa3 = (x.cpu().numpy() for x in (q3, v3, a3, p3, d3, pa3))
    f = ref.FIELDS.index
    for name in ("khat", "ess", "flags"):
        assert np.array_equal(ref.bits(q3[:, :, f(name)]), ref.bits(p3[:, :, pref.FIELDS.index(name)])), name
    assert np.array_equal(ref.bits(a3), ref.bits(pa3))
    assert np.array_equal(ref.bits(v3[..., 5]), ref.bits(d3[..., 5]))
    adapted = (q3[:, :, f("flags")].astype(np.int64) & 64) != 0
    print(f"{int(adapted.sum())} rows adapted in 3 rounds")
    assert adapted.any()
    # ... and the statistics are those of the best round's draws and weights
    for t, r in list(zip(*np.nonzero(adapted)))[:10]:
        want = ref.record_stats(v3[t, r, :, :5], v3[t, r, :, 5], D0)
        assert np.array_equal(ref.bits(q3[t, r, STAT_FIELDS]), ref.bits(want[STAT_FIELDS])), (t, r)
    same = ~adapted & ((base[:, :, f("flags")].astype(np.int64) & 1) != 0)
    assert np.array_equal(ref.bits(q3[same]), ref.bits(base[same]))  # an untouched row is the plain entry's


# --------------------------------------------------------------------------
# invalid cases and rejections
# --------------------------------------------------------------------------
def test_invalid_cases_and_rejections(torch_dev, batch_a):
    from metadamage_amd import _lib, engine

    torch = torch_dev
    b, ty, tN, res = batch_a["b"], batch_a["ty"], batch_a["tN"], batch_a["res"]
    two = engine.FitBatch(res.out[:2], None, res.status[:2], None)
    for S in (24, 1025):
        with pytest.raises(_lib.MdfitError, match="num_draws"):
            engine.map_quant_device(ty[:2], tN[:2], two, S)
    for d0 in (-0.01, 1.01, float("nan")):
        with pytest.raises(_lib.MdfitError, match="d0 must be in"):
            engine.map_quant_device(ty[:2], tN[:2], two, 64, d0=d0)
        with pytest.raises(_lib.MdfitError, match="d0 must be in"):
            engine.weighted_order_stats(np.zeros((1, 64)), np.full((1, 64), 1 / 64), d0)
    with pytest.raises(_lib.MdfitError, match="adapt_rounds"):
        engine.map_quant_device(ty[:2], tN[:2], two, 64, adapt_rounds=5)
    with pytest.raises(ValueError, match="quantiles needs with_psis"):
        engine.fit_batch_host(b.y[:4], b.N[:4], b.mm[:4], _lib.default_opts(mode=_lib.MODE_MAP), quantiles=True)
    # a taxon with y > N (status 3) and taxa whose fit ran out of iterations (status 1)
    y, N = b.y[:4].copy(), b.N[:4].copy()
    y[1, 7] = N[1, 7] + 1
    ty2, tN2, r2 = _map_fit(torch, y, N, max_iter=1)
    st = r2.status.cpu().numpy()
    assert st[1] == 3 and (st[[0, 2, 3]] == 1).all(), st
    quant, values, adapt = engine.map_quant_device(ty2, tN2, r2, 64, SEED, 0, D0, values=True, adapt_rounds=2)
    torch.cuda.synchronize()
    quant, values, adapt = quant.cpu().numpy(), values.cpu().numpy(), adapt.cpu().numpy()
    assert np.isnan(quant[:, :, :15]).all() and (quant[:, :, 15] == 0).all()
    assert np.isnan(values).all() and np.isnan(adapt).all()
    # a row without a proposal in batch A: NaN with the free bits alone
    flags = batch_a["psis"][:, :, pref.FLAGS].astype(np.int64)
    bad = (batch_a["st"][:, None] == 0) & ((flags & pref.VALID) == 0)
    assert bad.any()
    q = batch_a["quant"][bad]
    assert np.isnan(q[:, :15]).all() and ((q[:, 15].astype(np.int64) & ~60) == 0).all()


# --------------------------------------------------------------------------
# the CLI
# --------------------------------------------------------------------------
def test_cli_map_psis_quantiles(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import fits, io
    from metadamage_amd.cli import cli_app

    def run(out_dir, *args, code=0):
        r = CliRunner().invoke(cli_app, ["fit", "--out-dir", str(out_dir), *args, str(GOLDEN / "data_ancient.txt")])
        assert r.exit_code == code, (r.output, r.exception)
        return io.Parquet(out_dir / "fit_results" / "data_ancient.parquet")

    out_dir = tmp_path / "out"
    pq = run(out_dir, "--inference", "map-psis", "--quantiles")
    df = pq.load()
    new = fits.MAP_QUANT_COLUMNS + fits.MAP_QUANT_UINT_COLUMNS
    assert len(df.columns) == 52 + 16 and list(df.columns[52:]) == new
    meta = pq.load_metadata()
    assert meta["inference"] == "map-psis" and str(meta["quantiles"]) == "True"
    assert float(meta["dmax_threshold"]) == 0.01
    assert (df["map_quant_valid"] == 1).all() and (df["quant_window_min"] >= 1).all()
    assert (df["D_max_posterior_lower_hpdi"] <= df["D_max_posterior_median"]).all()
    assert (df["D_max_posterior_median"] <= df["D_max_posterior_upper_hpdi"]).all()
    assert (np.abs(df["D_max_posterior_median"] - df["D_max_posterior_mean"]) <= df["D_max_std"]).all()
    assert ((df["D_max_prob_above"] >= 0) & (df["D_max_prob_above"] <= 1)).all()
    plain = run(tmp_path / "plain", "--inference", "map-psis").load()
    assert len(plain.columns) == 52
    pd.testing.assert_frame_equal(df[plain.columns], plain)  # map-psis's columns are the run's without the option
    f = out_dir / "fit_results" / "data_ancient.parquet"
    m1 = f.stat().st_mtime_ns
    run(out_dir, "--inference", "map-psis", "--quantiles")  # cache hit: file untouched
    assert f.stat().st_mtime_ns == m1
    pq2 = run(out_dir, "--inference", "map-psis", "--quantiles", "--dmax-threshold", "0.9")  # the cache is not reused
    assert f.stat().st_mtime_ns != m1 and float(pq2.load_metadata()["dmax_threshold"]) == 0.9
    df2 = pq2.load()
    assert (df2["D_max_prob_above"] <= df["D_max_prob_above"]).all()  # (a higher threshold; nothing else moves)
    assert (df2["D_max_prob_above"] < df["D_max_prob_above"]).any()
    pd.testing.assert_frame_equal(df2.drop(columns="D_max_prob_above"), df.drop(columns="D_max_prob_above"))
    run(tmp_path / "bad", "--inference", "map", "--quantiles", code=2)
