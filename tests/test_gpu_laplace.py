"""GPU tests of mdfit_map_laplace: the kernel's Hessian against
the fit kernel's own objective entry and the oracle, its held set and 4x4
linear algebra against numpy / mpmath on its own H, the records end to end
against tests/laplace_ref.py, the edge inputs, and the chunked, gathered and
CLI paths."""

from __future__ import annotations

import ctypes

import numpy as np
import pandas as pd
import pytest

from tests import laplace_ref as ref
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

STAT = slice(0, 7)
# End to end against laplace_ref (oracle H, numpy): ten times the worst relative
# error per field measured on the MI355X over batch A and the edge batch
# (DESIGN.md §3.7), never looser than 1e-5.
E2E_MEASURED = {"q_std": 1.83e-13, "A_std": 1.86e-13, "c_std": 2.68e-13, "phi_std": 6.37e-12, "D_max_std": 2.52e-13,
                "rho_Ac": 4.60e-12, "significance": 2.52e-13}
E2E_TOL = {k: min(10.0 * v, 1e-5) for k, v in E2E_MEASURED.items()}


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    return torch


def _fit_and_laplace(torch, y, N, mm=None, poison=False):
    """One MAP call, then mdfit_map_laplace -> host (out, status, lap, gh, u)."""
    from metadamage_amd import _lib, engine

    ty, tN, tm = engine.to_device_counts(y, N, mm)
    T = int(ty.shape[0])
    res = engine.fit_batch_device(ty, tN, tm, _lib.default_opts(mode=_lib.MODE_MAP))
    gh = torch.empty((T, 3, 20), dtype=torch.float64, device=ty.device)
    ku = torch.empty((T, 3, 4), dtype=torch.float64, device=ty.device)
    before = res.out.clone()
    if poison:
        _lib.check(_lib.load().mdfit_poison_lds(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    lap = engine.map_laplace_device(ty, tN, res, gh=gh, u=ku)
    plain = engine.map_laplace_device(ty, tN, res)  # the product call: the same records
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int64), res.out.view(torch.int64))  # the records are read only
    assert torch.equal(plain.view(torch.int64), lap.view(torch.int64))
    return res.out.cpu().numpy(), res.status.cpu().numpy(), lap.cpu().numpy(), gh.cpu().numpy(), ku.cpu().numpy()


@pytest.fixture(scope="module")
def batch_a(torch_dev, oracle_lib):
    """generate(300, seed=21) fitted by one MAP call, its Laplace records, and
    the reference's from the same device records (computed once, read only)."""
    from metadamage_amd.synthetic import generate

    b = generate(300, seed=21)
    out, st, lap, gh, ku = _fit_and_laplace(torch_dev, b.y, b.N, b.mm)
    want, near = ref.laplace_batch(oracle_lib, b.y, b.N, out, st)
    for a in (out, st, lap, gh, ku, want, near):
        a.setflags(write=False)
    return b, out, st, lap, gh, want, near, ku


def _u_all(out):
    return np.array([[ref.record_u(out[t], k) for _, k in ref.SUBFITS] for t in range(out.shape[0])])


def test_gh_equals_the_objective_entry(batch_a):
    """Same code, same numbers: g and H of the kernel against mdfit_objective at
    the rebuilt u -- the kernel's own (at the mode g is ~0 and moves by H du: a
    u rebuilt by numpy's log, an ulp away, shifts it by 1e-11) --; only
    fused-multiply-add contraction can differ.  The kernel's u is numpy's
    rebuild to a few ulp."""
    from metadamage_amd import engine

    b, out, st, lap, gh, _, _, u = batch_a
    ok = np.flatnonzero(st == 0)
    assert np.abs(u[ok] - _u_all(out)[ok]).max() <= 1e-14
    worst_g = worst_h = 0.0
    for r, (subset, _) in enumerate(ref.SUBFITS):
        _, g, H, _ = engine.objective(np.zeros(ok.size, np.int32), np.full(ok.size, subset, np.int32), b.y[ok],
                                      b.N[ok], u[ok, r])
        kg, kH = gh[ok, r, :4], gh[ok, r, 4:].reshape(-1, 4, 4)
        eg = np.abs(kg - g).max(axis=1) / np.maximum(1.0, np.abs(g).max(axis=1))
        eH = np.abs(kH - H).max(axis=(1, 2)) / np.maximum(1.0, np.abs(H).max(axis=(1, 2)))
        worst_g, worst_h = max(worst_g, eg.max()), max(worst_h, eH.max())
        print(f"subset {subset}: max |dg|/scale {eg.max():.2e}, max |dH|/scale {eH.max():.2e}")
        assert (eg <= 1e-13).all() and (eH <= 1e-13).all(), (subset, eg.max(), eH.max())
        assert np.array_equal(kH, kH.transpose(0, 2, 1))


def test_hessian_vs_oracle(batch_a, oracle_lib):
    b, out, st, lap, gh, _, _, _ = batch_a
    u = _u_all(out)
    worst = 0.0
    for t in np.flatnonzero(st == 0):
        for r, (subset, _) in enumerate(ref.SUBFITS):
            _, go, Ho, _ = oracle_lib.objective(0, subset, b.y[t, :30], b.N[t, :30], u[t, r])
            eg = np.abs(gh[t, r, :4] - go).max() / max(1.0, np.abs(go).max())
            eH = np.abs(gh[t, r, 4:].reshape(4, 4) - Ho).max() / max(1.0, np.abs(Ho).max())
            worst = max(worst, eg, eH)
            assert eg <= 1e-8 and eH <= 1e-8, (t, r, eg, eH)
    print(f"kernel g, H vs oracle: worst {worst:.2e} of the largest entry")


def _check_linear_algebra(out, st, lap, gh, items):
    """The kernel's flags and statistics from its OWN g, H and the rebuilt u:
    free bits by free_set's FP64 comparisons, statistics by mpmath."""
    worst = 0.0
    for t, r in items:
        u = ref.record_u(out[t], ref.SUBFITS[r][1])
        g, H = gh[t, r, :4], gh[t, r, 4:].reshape(4, 4)
        free, _ = ref.free_set(u, g, H)
        mask = int(sum(1 << j for j in range(4) if free[j]))
        flags = int(lap[t, r, 7])
        assert flags & 15 == mask, (t, r, flags, mask)
        J, dmax = ref.jacobian(u)
        npy = ref.stats(H, free, J, dmax)
        if not int(npy[7]) & ref.VALID:
            assert not flags & ref.VALID and np.isnan(lap[t, r, STAT]).all(), (t, r)
            continue
        assert flags & ref.VALID, (t, r, lap[t, r])
        want, kap, amp = ref.stats_mp(H, free, J, dmax)
        tol = 1e-14 * kap + 1e-12
        got = lap[t, r]
        for k in range(4):
            if free[k]:
                e = abs(got[k] - want[k]) / abs(want[k])
                worst = max(worst, e / tol)
                assert e <= tol, (t, r, k, kap, got[k], want[k])
            else:
                assert got[k] == 0.0
        if free[1] and free[2]:
            assert abs(got[5] - want[5]) <= tol * abs(want[5]), (t, r, kap, got[5], want[5])
        else:
            assert np.isnan(got[5])
        if want[4] > 0.0:
            assert abs(got[4] - want[4]) <= tol * amp * want[4], (t, r, kap, amp, got[4], want[4])
            assert abs(got[6] - want[6]) <= tol * amp * abs(want[6]), (t, r, kap, amp, got[6], want[6])
        else:
            assert got[4] == 0.0 and np.isnan(got[6])
    return worst


def test_linear_algebra_on_the_device(batch_a):
    b, out, st, lap, gh, _, _, _ = batch_a
    items = [(t, r) for t in np.flatnonzero(st == 0) for r in range(3)]
    worst = _check_linear_algebra(out, st, lap, gh, items)
    print(f"device 4x4 vs mpmath on {len(items)} items: worst error / bound = {worst:.3f}")


def _check_end_to_end(lap, want, near, st, label):
    """Flags equal on every item whose held/free decisions are the data's;
    statistics within E2E_TOL.  Returns the worst relative error per field."""
    T = lap.shape[0]
    skipped = int(near.sum())
    worst = dict.fromkeys(E2E_TOL, 0.0)
    for t in range(T):
        for r in range(3):
            if near[t, r]:
                continue
            assert int(lap[t, r, 7]) == int(want[t, r, 7]), (label, t, r, lap[t, r], want[t, r])
            for k, name in enumerate(ref.FIELDS[:7]):
                a, w = lap[t, r, k], want[t, r, k]
                if np.isnan(w) or w == 0.0:
                    continue
                worst[name] = max(worst[name], abs(a - w) / abs(w))
    print(f"{label}: {skipped} of {3 * T} items left out; worst relative error per field: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for t in range(T):
        for r in range(3):
            if near[t, r]:
                continue
            for k, name in enumerate(ref.FIELDS[:7]):
                a, w = lap[t, r, k], want[t, r, k]
                if np.isnan(w):
                    assert np.isnan(a), (label, t, r, name, a)
                elif w == 0.0:
                    assert a == 0.0, (label, t, r, name, a)
                else:
                    assert abs(a - w) <= E2E_TOL[name] * abs(w), (label, t, r, name, a, w)
            if st[t] != 0:
                assert int(lap[t, r, 7]) == 0 and np.isnan(lap[t, r, STAT]).all()
    return skipped, worst


def _nan_only_where_defined(lap):
    """A valid row holds no NaN but rho_Ac with A or c held and the significance
    of a zero D_max_std (both NaN by definition)."""
    for row in lap.reshape(-1, 8):
        flags = int(row[7])
        if not flags & ref.VALID:
            assert np.isnan(row[STAT]).all()
            continue
        assert np.isfinite(row[:5]).all(), row
        assert np.isnan(row[5]) == (not (flags & 2 and flags & 4)), row
        assert np.isnan(row[6]) == (row[4] == 0.0), row


def test_end_to_end_vs_reference(batch_a):
    b, out, st, lap, gh, want, near, _ = batch_a
    skipped, _ = _check_end_to_end(lap, want, near, st, "batch A")
    assert skipped <= 9  # 1 % of the 900 items
    _nan_only_where_defined(lap)
    # c on its bound: std 0, no correlation, D_max_std from A alone
    held = [t for t in range(300) if st[t] == 0 and int(lap[t, 0, 7]) & ref.VALID and not int(lap[t, 0, 7]) & 4]
    print(f"batch A: c held in {len(held)} PMD-all fits")
    assert len(held) >= 5
    for t in held:
        assert lap[t, 0, 2] == 0.0 and np.isnan(lap[t, 0, 5]) and np.isfinite(lap[t, 0, 4]) and lap[t, 0, 4] > 0.0
        assert out[t, ref.F_DIAG + 2] == 0.0


def test_edges(torch_dev, oracle_lib, ref_golden, batch_a):
    b, _, st_a, lap_a, _, _, _, _ = batch_a
    T = 7
    y = np.zeros((T, 32), np.uint32)
    N = np.zeros((T, 32), np.uint32)
    y[:4, :30], N[:4, :30] = b.y[3, :30], b.N[3, :30]
    y[0, 4] = N[0, 4] + 1  # a: y > N at one position
    y[1, 15:30] = N[1, 15:30] = 0  # b: the reverse strand without data
    y[2, :30] = 0  # c: every y = 0
    N[3, :30] = 1  # d: N = 1 everywhere
    y[3, :30] = np.arange(30) % 7 == 0
    y[4:, :30], N[4:, :30] = ref_golden["data_ancient__y"], ref_golden["data_ancient__N"]  # e: N ~ 1e7
    out, st, lap, gh, _ = _fit_and_laplace(torch_dev, y, N)
    assert st[0] == 3 and np.isnan(lap[0, :, STAT]).all() and (lap[0, :, 7] == 0).all()
    assert np.isnan(gh[0]).all()
    assert (st[[1, 2, 4, 5, 6]] == 0).all(), st
    assert int(lap[1, 2, 7]) & ref.VALID  # prior-only: still a posterior mode with curvature
    assert (lap[4:, :, 7].astype(int) & ref.VALID).all()
    want, near = ref.laplace_batch(oracle_lib, y, N, out, st)
    _check_end_to_end(lap, want, near, st, "edges")
    _nan_only_where_defined(lap)
    _check_linear_algebra(out, st, lap, gh, [(t, r) for t in range(1, T) for r in range(3)])
    # a batch of one taxon, c held
    t1 = next(t for t in range(300) if st_a[t] == 0 and int(lap_a[t, 0, 7]) == 16 + 11)
    o1, s1, l1, _, _ = _fit_and_laplace(torch_dev, b.y[t1:t1 + 1], b.N[t1:t1 + 1], b.mm[t1:t1 + 1])
    assert s1[0] == 0
    assert np.array_equal(l1[0], lap_a[t1], equal_nan=True)
    w1, n1 = ref.laplace_batch(oracle_lib, b.y[t1:t1 + 1], b.N[t1:t1 + 1], o1, s1)
    _check_end_to_end(l1, w1, n1, s1, "one taxon")


def test_poisoned_lds_same_bits(torch_dev, batch_a):
    b, out, st, lap, gh, _, _, _ = batch_a
    o2, s2, l2, g2, _ = _fit_and_laplace(torch_dev, b.y, b.N, b.mm, poison=True)
    assert np.array_equal(o2.view(np.int64), out.view(np.int64))
    assert np.array_equal(l2.view(np.int64), lap.view(np.int64))
    assert np.array_equal(g2.view(np.int64), gh.view(np.int64))


def test_chunked_and_gathered_paths(torch_dev, monkeypatch, batch_a):
    torch = torch_dev
    from metadamage_amd import _lib, distributed as d, engine

    b, out, st, lap, _, _, _, _ = batch_a
    opts = _lib.default_opts(mode=_lib.MODE_MAP)
    lap32 = lap.astype(np.float32)
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "128")
    assert len(engine.plan_chunks(300, opts)) == 3
    o4, p4, s4, l4 = engine.fit_batch_host(b.y, b.N, b.mm, opts, laplace=True)
    assert l4.shape == (300, 3, 8) and l4.dtype == np.float32
    assert np.array_equal(l4.view(np.int32), lap32.view(np.int32))
    plain = engine.fit_batch_host(b.y, b.N, b.mm, opts)
    assert len(plain) == 3
    for a, c in zip(plain, (o4, p4, s4)):
        assert a.dtype == c.dtype and np.array_equal(a, c, equal_nan=True)
    assert np.array_equal(o4, out[:, :25], equal_nan=True) and np.array_equal(s4, st)
    # the buffers of a staging without the flag are what they were
    assert engine.device_bytes(128, opts) + 128 * 3 * 96 == engine.device_bytes(128, opts, with_laplace=True)
    assert engine.device_bytes(128, opts, dest_on_device=True) + 128 * 2 * 96 == \
        engine.device_bytes(128, opts, dest_on_device=True, with_laplace=True)
    # into the gather record of a world of one
    rec = d.alloc_records(300, torch.device("cuda", torch.cuda.current_device()), with_laplace=True)
    assert rec.buf.numel() == 300 * (d.REC_BYTES + d.REC_LAP)
    fitter = engine.ChunkedFitter(128, opts=opts, dest_on_device=True, with_laplace=True)
    fitter.run_into_device(b.y, b.N, b.mm, opts, engine.FitBatch(rec.out, rec.pred, rec.status, lap=rec.lap),
                           chunks=engine.plan_chunks(300, opts, chunk_taxa=128))
    buf = rec.stage()
    torch.cuda.synchronize()
    parts = d.gather_records(buf, 300, 0, 1)
    og, pg, sg, lg = d.unpack_gathered(parts, 300, 1, with_laplace=True)
    assert np.array_equal(lg.view(np.int32), lap32.view(np.int32))
    assert np.array_equal(og, d.round_like_gather(out), equal_nan=True)
    assert np.array_equal(sg, st) and np.array_equal(pg, p4, equal_nan=True)


def test_cli_map_laplace(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import io
    from metadamage_amd.cli import cli_app
    from tests.test_laplace import NEW_COLUMNS

    def run(out_dir, inference):
        r = CliRunner().invoke(cli_app, ["fit", "--out-dir", str(out_dir), "--inference", inference,
                                         str(GOLDEN / "data_ancient.txt")])
        assert r.exit_code == 0, (r.output, r.exception)
        return io.Parquet(out_dir / "fit_results" / "data_ancient.parquet")

    out_dir = tmp_path / "out"
    pq = run(out_dir, "map-laplace")
    df = pq.load()
    assert len(df.columns) == 42 and list(df.columns[30:]) == NEW_COLUMNS
    assert pq.load_metadata()["inference"] == "map-laplace"
    assert (df["laplace_valid"] == 1).all() and (df["D_max_std"] > 0).all()
    np.testing.assert_allclose(df["significance"].to_numpy(),
                               df["D_max_marginalized_mean"].to_numpy() / df["D_max_std"].to_numpy(), rtol=1e-6)
    f = out_dir / "fit_results" / "data_ancient.parquet"
    m1 = f.stat().st_mtime_ns
    run(out_dir, "map-laplace")  # cache hit: file untouched
    assert f.stat().st_mtime_ns == m1
    plain = run(tmp_path / "plain", "map").load()
    assert len(plain.columns) == 30
    pd.testing.assert_frame_equal(df[plain.columns], plain)
    pq2 = run(out_dir, "map")  # another inference: the cache is not reused
    assert f.stat().st_mtime_ns != m1
    assert pq2.load_metadata()["inference"] == "map" and len(pq2.load().columns) == 30
