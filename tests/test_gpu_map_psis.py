"""GPU tests of mdfit_map_psis and mdfit_psis_weights (MDFIT-PSIS v1, DESIGN.md
§3.8): the smoothing against the reference on crafted series, the held set and
the factorisation's validity against mdfit_map_laplace, the draws, log-weights
and records end to end against tests/map_psis_ref.py, the invariance of the
records under every way of calling, the rejections and the CLI path."""

from __future__ import annotations

import ctypes

import numpy as np
import pandas as pd
import pytest

from tests import laplace_ref
from tests import map_psis_cases as cases
from tests import map_psis_ref as ref
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

S_A = 256
SEED = 0
# mdfit_psis_weights against the reference over ~200 series per S: the worst
# error measured on the MI355X, asserted at ten times it
WEIGHTS_MEASURED = {"w": 8.08e-15, "khat": 2.07e-14}
# end to end on generate(300, 21), S = 256, measured likewise: u against the
# reference's own draws (absolute over max(1, |u|)), the raw log-weight against
# the reference's log p - log g at the kernel's u (absolute over max(1, |lw|)),
# each statistic against the reference fed the kernel's u and lw (relative)
# (khat absolute).  The draws inherit the Laplace factor's agreement with the
# oracle's Hessian -- 6e-12 on phi_std, test_gpu_laplace.py -- times a
# heavy-tailed offset of up to tens of standard deviations
E2E_MEASURED = {"u": 1.52e-10, "lw": 1.03e-11, "mean": 1.16e-15, "std": 2.55e-15, "rho_Ac": 1.20e-12,
                "significance": 2.36e-15, "khat": 1.27e-14, "ess": 7.18e-15}


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


@pytest.fixture(scope="module")
def batch_a(torch_dev):
    """generate(300, seed=21) fitted by one MAP call, its importance-sampled
    posteriors at S = 256 with the draws, and its Laplace records (computed
    once, read only)."""
    from metadamage_amd import engine
    from metadamage_amd.synthetic import generate

    torch = torch_dev
    b = generate(300, seed=21)
    ty, tN, res = _map_fit(torch, b.y, b.N, b.mm)
    before = res.out.clone()
    psis, draws = engine.map_psis_device(ty, tN, res, S_A, SEED, 0, draws=True)
    lap = engine.map_laplace_device(ty, tN, res)
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int64), res.out.view(torch.int64))  # the records are read only
    host = {"b": b, "out": res.out.cpu().numpy(), "st": res.status.cpu().numpy(), "psis": psis.cpu().numpy(),
            "draws": draws.cpu().numpy(), "lap": lap.cpu().numpy()}
    for a in host.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    host.update(ty=ty, tN=tN, res=res)
    return host


@pytest.fixture(scope="module")
def ref_a(batch_a, oracle_lib):
    """The reference's proposals and own draws for batch A from the device's
    records (computed once)."""
    b, out, st = batch_a["b"], batch_a["out"], batch_a["st"]
    return [ref.psis_taxon(oracle_lib, b.y[t, :30], b.N[t, :30], out[t], int(st[t]), S_A, seed=SEED, g=t)
            for t in range(300)]


# --------------------------------------------------------------------------
# the smoothing
# --------------------------------------------------------------------------
@pytest.mark.parametrize("S", (25, 64, 65, 100, 256, 1024))
def test_psis_weights_vs_reference(torch_dev, S):
    from metadamage_amd import engine

    n = 208  # 13 of each kind
    lw, kinds = cases.weights_case(S, n)
    want_w, want_k, want_valid = cases.weights_reference(S, n)
    w, khat = engine.psis_weights(lw)
    worst = cases.weight_errors(w, khat, want_w, want_k, want_valid)
    print(f"S={S} n={n}: worst error " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for i, kind in enumerate(kinds):
        if kind in ("cut_inf", "all_inf", "nan", "posinf"):
            assert np.isnan(khat[i]) and np.isnan(w[i]).all(), kind
            continue
        assert (w[i][np.isneginf(lw[i])] == 0.0).all() and abs(w[i].sum() - 1.0) < 1e-13, kind
        if kind == "const":
            assert khat[i] == 0.0 and (w[i] == 1.0 / S).all()
    for name, v in worst.items():
        assert v <= 10.0 * WEIGHTS_MEASURED[name], (name, v)


# --------------------------------------------------------------------------
# the held set and the factorisation are mdfit_map_laplace's
# --------------------------------------------------------------------------
def _edge_batch(b, ref_golden):
    T = 7
    y = np.zeros((T, 32), np.uint32)
    N = np.zeros((T, 32), np.uint32)
    y[:4, :30], N[:4, :30] = b.y[3, :30], b.N[3, :30]
    y[0, 4] = N[0, 4] + 1  # y > N at one position
    y[1, 15:30] = N[1, 15:30] = 0  # the reverse strand without data
    y[2, :30] = 0  # every y = 0
    N[3, :30] = 1  # N = 1 everywhere
    y[3, :30] = np.arange(30) % 7 == 0
    y[4:, :30], N[4:, :30] = ref_golden["data_ancient__y"], ref_golden["data_ancient__N"]  # N ~ 1e7
    return y, N


def _check_against_laplace(psis, draws, lap, out, st):
    """Per row: the free bits equal; the proposal exists (its draws are finite)
    exactly where the Laplace row is valid and the held set is supported."""
    n_prop = 0
    for t in range(len(st)):
        for r in range(3):
            pf, lf = int(psis[t, r, ref.FLAGS]), int(lap[t, r, 7])
            if st[t] != 0:
                assert pf == 0 and lf == 0 and np.isnan(psis[t, r, :15]).all()
                continue
            mask = lf & 15
            assert (pf >> 2) & 15 == mask, (t, r, pf, lf)
            u = laplace_ref.record_u(out[t], laplace_ref.SUBFITS[r][1])
            c_ok = bool(mask & 4) or u[2] <= laplace_ref.KEPSBIND[2]
            supported = (mask & 11) == 11 and c_ok
            has_proposal = bool(np.isfinite(draws[t, r, :, 3]).all())
            assert has_proposal == (bool(lf & laplace_ref.VALID) and supported), (t, r, pf, lf)
            n_prop += has_proposal
            if not has_proposal:
                assert not pf & ref.VALID and np.isnan(psis[t, r, :15]).all() and np.isnan(draws[t, r]).all()
    return n_prop


def test_free_bits_and_validity_are_laplaces(torch_dev, batch_a, ref_golden):
    from metadamage_amd import engine

    n = _check_against_laplace(batch_a["psis"], batch_a["draws"], batch_a["lap"], batch_a["out"], batch_a["st"])
    print(f"batch A: {n} of 900 rows with a proposal")
    assert n >= 850
    y, N = _edge_batch(batch_a["b"], ref_golden)
    ty, tN, res = _map_fit(torch_dev, y, N)
    psis, draws = engine.map_psis_device(ty, tN, res, 64, SEED, 0, draws=True)
    lap = engine.map_laplace_device(ty, tN, res)
    torch_dev.cuda.synchronize()
    st = res.status.cpu().numpy()
    assert st[0] == 3
    n = _check_against_laplace(psis.cpu().numpy(), draws.cpu().numpy(), lap.cpu().numpy(), res.out.cpu().numpy(), st)
    print(f"edge batch: {n} of 18 rows with a proposal")
    assert n >= 9


# --------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------
def test_end_to_end_vs_reference(batch_a, ref_a, oracle_lib):
    b, st, psis, draws = batch_a["b"], batch_a["st"], batch_a["psis"], batch_a["draws"]
    tau = ref.khat_threshold(S_A)
    worst = dict.fromkeys(E2E_MEASURED, 0.0)
    excluded = compared = 0
    checks = []
    for t in range(300):
        for r in range(3):
            got = psis[t, r]
            res = ref_a[t][r]
            prop = res["prop"]
            if st[t] != 0:
                assert got[ref.FLAGS] == 0 and np.isnan(got[:15]).all()
                continue
            if prop.near:  # a held/free decision within 1e-6 of its threshold: not the data's
                excluded += 1
                continue
            assert (int(got[ref.FLAGS]) >> 2) & 15 == prop.mask, (t, r, got[ref.FLAGS], prop.mask)
            if not prop.valid:
                assert int(got[ref.FLAGS]) == prop.mask << 2 and np.isnan(got[:15]).all(), (t, r)
                continue
            ku, klw, kw = draws[t, r, :, :4], draws[t, r, :, 4], draws[t, r, :, 5]
            # the draws against the reference's own
            worst["u"] = max(worst["u"], float((np.abs(ku - res["u"]) / np.maximum(1, np.abs(res["u"]))).max()))
            # the raw log-weights against log p - log g at the kernel's u
            lw_ref = ref.log_target(oracle_lib, b.y[t, :30], b.N[t, :30], r, ku) - prop.log_g_at(ku)
            inf = np.isneginf(lw_ref.astype(float))
            assert np.array_equal(np.isneginf(klw), inf), (t, r)
            worst["lw"] = max(worst["lw"], float((np.abs(klw[~inf] - lw_ref[~inf])
                                                  / np.maximum(1, np.abs(lw_ref[~inf]))).max()))
            # the infeasible draws against the reference's own
            assert int(inf.sum()) == int(np.isneginf(res["lw"]).sum()), (t, r)
            # the statistics against the reference fed the kernel's u and lw
            want, want_w = ref.record_from(prop, ku, klw, S_A)
            if not int(want[ref.FLAGS]) & ref.VALID:
                assert int(got[ref.FLAGS]) == prop.mask << 2 and np.isnan(got[:15]).all(), (t, r)
                assert np.isnan(kw).all()
                continue
            khat_ref = float(want[ref.KHAT])
            if np.isfinite(khat_ref) and abs(khat_ref - tau) <= 1e-6:
                excluded += 1
                continue
            compared += 1
            assert int(got[ref.FLAGS]) == int(want[ref.FLAGS]), (t, r, got, want)
            assert got[ref.N_INF] == float(want[ref.N_INF]) == inf.sum()
            assert abs(kw.sum() - 1.0) < 1e-12 and (kw[inf] == 0).all()
            for j, name in enumerate(ref.FIELDS[:14]):
                a, w_ = got[j], float(want[j])
                key = "mean" if j < 5 else ("std" if j < 10 else name)
                assert np.isnan(a) == np.isnan(w_), (t, r, name, a, w_)
                if np.isnan(w_) or np.isinf(w_):
                    assert np.isnan(w_) or a == w_
                    continue
                if name == "khat":
                    e = abs(a - want[j])  # absolute: khat crosses 0
                elif w_ == 0.0:
                    e = abs(a)
                else:
                    e = abs(a - want[j]) / abs(want[j])
                worst[key] = max(worst[key], float(e))
                checks.append((key, float(e), t, r, name))
    print(f"batch A, S = {S_A}: {compared} rows compared, {excluded} left out; worst error: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert excluded <= 9  # 1 % of the 900 rows
    assert compared >= 800
    for key, e, t, r, name in checks:
        assert e <= 10.0 * E2E_MEASURED[key], (key, e, t, r, name)
    for key in ("u", "lw"):
        assert worst[key] <= 10.0 * E2E_MEASURED[key], (key, worst[key])
    # a c held on 0 is drawn from its exponential: positive, with a spread
    held = [(t, r) for t in range(300) for r in range(3)
            if int(psis[t, r, ref.FLAGS]) & ref.VALID and not (int(psis[t, r, ref.FLAGS]) >> 2) & 4]
    print(f"c held in {len(held)} valid rows")
    assert len(held) >= 5
    for t, r in held:
        assert (draws[t, r, :, 2] > 0).all() and psis[t, r, 2] > 0 and psis[t, r, 7] > 0


# --------------------------------------------------------------------------
# invariance
# --------------------------------------------------------------------------
def test_records_do_not_depend_on_the_call(torch_dev, monkeypatch, batch_a):
    torch = torch_dev
    from metadamage_amd import _lib, distributed as d, engine

    b, ty, tN, res, base = batch_a["b"], batch_a["ty"], batch_a["tN"], batch_a["res"], batch_a["psis"]

    def sub(lo, hi):
        return engine.FitBatch(res.out[lo:hi], None, res.status[lo:hi], None)

    # without the draws
    plain = engine.map_psis_device(ty, tN, res, S_A, SEED, 0)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(plain.cpu().numpy()), _bits(base))
    # T = 1, 3, 65: the first taxa of the batch
    for T in (1, 3, 65):
        got = engine.map_psis_device(ty[:T], tN[:T], sub(0, T), S_A, SEED, 0)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(base[:T])), T
    # two calls split with index_base
    a = engine.map_psis_device(ty[:130], tN[:130], sub(0, 130), S_A, SEED, 0)
    c = engine.map_psis_device(ty[130:], tN[130:], sub(130, 300), S_A, SEED, 130)
    wrong = engine.map_psis_device(ty[130:], tN[130:], sub(130, 300), S_A, SEED, 0)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(torch.cat([a, c]).cpu().numpy()), _bits(base))
    assert not np.array_equal(_bits(wrong.cpu().numpy()), _bits(base[130:]))  # (the streams are the global taxon's)
    other = engine.map_psis_device(ty, tN, res, S_A, SEED + 1, 0)
    torch.cuda.synchronize()
    assert not np.array_equal(_bits(other.cpu().numpy()), _bits(base))
    # after a poisoning of the LDS
    _lib.check(_lib.load().mdfit_poison_lds(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    got = engine.map_psis_device(ty, tN, res, S_A, SEED, 0)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(base))
    # under graph capture and replay
    s = torch.cuda.Stream()
    dst = torch.zeros((300, 3, _lib.NMAPPSIS), dtype=torch.float64, device=ty.device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        engine.map_psis_device(ty, tN, res, S_A, SEED, 0, psis=dst, stream=torch.cuda.current_stream())
    for _ in range(2):
        dst.fill_(0.0)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(dst.cpu().numpy()), _bits(base))
    # through the chunked dispatch in two chunks, and into the gather record of a world of one
    opts = _lib.default_opts(mode=_lib.MODE_MAP)
    base32 = base.astype(np.float32)
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "150")
    assert len(engine.plan_chunks(300, opts, with_psis=True)) == 2
    o4, p4, s4, ps4 = engine.fit_batch_host(b.y, b.N, b.mm, opts, psis=True, psis_draws=S_A)
    assert ps4.shape == (300, 3, 16) and ps4.dtype == np.float32
    assert np.array_equal(ps4.view(np.int32), base32.view(np.int32))
    plain3 = engine.fit_batch_host(b.y, b.N, b.mm, opts)
    assert len(plain3) == 3
    for x, z in zip(plain3, (o4, p4, s4)):
        assert x.dtype == z.dtype and np.array_equal(x, z, equal_nan=True)
    rec = d.alloc_records(300, torch.device("cuda", torch.cuda.current_device()), with_psis=True)
    assert rec.buf.numel() == 300 * (d.REC_BYTES + d.REC_PSIS)
    fitter = engine.ChunkedFitter(150, opts=opts, dest_on_device=True, with_psis=True, psis_draws=S_A)
    fitter.run_into_device(b.y, b.N, b.mm, opts, engine.FitBatch(rec.out, rec.pred, rec.status, psis=rec.psis),
                           chunks=engine.plan_chunks(300, opts, chunk_taxa=150))
    buf = rec.stage()
    torch.cuda.synchronize()
    og, pg, sg, psg = d.unpack_gathered(d.gather_records(buf, 300, 0, 1), 300, 1, with_psis=True)
    assert np.array_equal(psg.view(np.int32), base32.view(np.int32))
    assert np.array_equal(og, d.round_like_gather(batch_a["out"]), equal_nan=True) and np.array_equal(sg, s4)


# --------------------------------------------------------------------------
# rejections
# --------------------------------------------------------------------------
def test_rejections(torch_dev, batch_a):
    from metadamage_amd import _lib, engine

    torch = torch_dev
    b, ty, tN, res = batch_a["b"], batch_a["ty"], batch_a["tN"], batch_a["res"]
    for S in (24, 1025):
        with pytest.raises(_lib.MdfitError, match="num_draws"):
            engine.map_psis_device(ty[:2], tN[:2], engine.FitBatch(res.out[:2], None, res.status[:2], None), S)
    # a taxon with y > N (status 3) and taxa whose fit ran out of iterations (status 1)
    y, N = b.y[:4].copy(), b.N[:4].copy()
    y[1, 7] = N[1, 7] + 1
    ty2, tN2, r2 = _map_fit(torch, y, N, max_iter=1)
    st = r2.status.cpu().numpy()
    assert st[1] == 3 and (st[[0, 2, 3]] == 1).all(), st
    psis, draws = engine.map_psis_device(ty2, tN2, r2, 64, SEED, 0, draws=True)
    torch.cuda.synchronize()
    psis, draws = psis.cpu().numpy(), draws.cpu().numpy()
    assert np.isnan(psis[:, :, :15]).all() and (psis[:, :, ref.FLAGS] == 0).all() and np.isnan(draws).all()


# --------------------------------------------------------------------------
# the CLI
# --------------------------------------------------------------------------
def test_cli_map_psis(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import io
    from metadamage_amd.cli import cli_app
    from tests.test_map_psis import NEW_COLUMNS

    def run(out_dir, *args):
        r = CliRunner().invoke(cli_app, ["fit", "--out-dir", str(out_dir), *args, str(GOLDEN / "data_ancient.txt")])
        assert r.exit_code == 0, (r.output, r.exception)
        return io.Parquet(out_dir / "fit_results" / "data_ancient.parquet")

    out_dir = tmp_path / "out"
    pq = run(out_dir, "--inference", "map-psis")
    df = pq.load()
    assert len(df.columns) == 52 and list(df.columns[30:]) == NEW_COLUMNS
    meta = pq.load_metadata()
    assert meta["inference"] == "map-psis" and int(meta["psis_draws"]) == 256
    assert (df["map_psis_valid"] == 1).all() and (df["D_max_std"] > 0).all() and (df["psis_ess"] > 1).all()
    np.testing.assert_allclose(df["significance"].to_numpy(),
                               df["D_max_posterior_mean"].to_numpy() / df["D_max_std"].to_numpy(), rtol=1e-6)
    plain = run(tmp_path / "plain", "--inference", "map").load()
    assert len(plain.columns) == 30
    pd.testing.assert_frame_equal(df[plain.columns], plain)  # the 25 result columns (and the names) are the MAP call's
    f = out_dir / "fit_results" / "data_ancient.parquet"
    m1 = f.stat().st_mtime_ns
    run(out_dir, "--inference", "map-psis")  # cache hit: file untouched
    assert f.stat().st_mtime_ns == m1
    pq2 = run(out_dir, "--inference", "map-psis", "--psis-draws", "64")  # other draws: the cache is not reused
    assert f.stat().st_mtime_ns != m1 and int(pq2.load_metadata()["psis_draws"]) == 64
    assert not np.array_equal(pq2.load()["pareto_k"].to_numpy(), df["pareto_k"].to_numpy())
