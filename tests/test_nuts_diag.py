"""CPU tests of the sampling diagnostics (MDFIT-DIAG v1): the
C-ABI entry point without a device, the reference (tests/nuts_diag_ref.py)
against the analytic AR(1) value, the host build of the per-series arithmetic
(csrc/mdfit_nutsdiag.h, under the address and undefined-behaviour sanitizers)
against the reference on the crafted edge shapes, and the frame / options /
chunk-planning / gather-record plumbing."""

from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from tests import nuts_diag_cases as cases
from tests import nuts_diag_ref as ref
from tests.helpers import GOLDEN

ROOT = Path(__file__).resolve().parents[1]

FLOAT_COLUMNS = ["ess_q", "ess_A", "ess_c", "ess_phi", "ess_D_max", "rhat_q", "rhat_A", "rhat_c", "rhat_phi",
                 "rhat_D_max", "mcse_D_max", "ess_q_null", "ess_phi_null", "rhat_q_null", "rhat_phi_null",
                 "ess_min", "rhat_max"]
UINT_COLUMNS = ["divergences", "nuts_diag_valid"]
# host build (sequential sums) against the longdouble reference: S <= 4096 terms
# of FP64 rounding per sum, a handful of sums per statistic -- far below this
HOST_TOL = 1e-11


# --------------------------------------------------------------------------
# ABI
# --------------------------------------------------------------------------
def test_entry_point_declared_exported_and_argument_checked():
    from metadamage_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mdfit.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+mdfit_nuts_diag\s*\(", text)
    assert f"#define MDFIT_NNUTSDIAG {_lib.NNUTSDIAG}" in text
    assert f"#define MDFIT_ABI_VERSION {_lib.ABI_VERSION}" in text and _lib.ABI_VERSION == 3
    assert "mdfit_nuts_diag" in _lib.EXPORTED_SYMBOLS
    assert len(_lib.NUTSDIAG_FIELDS) == _lib.NNUTSDIAG == 12 and _lib.NUTSDIAG_VALID == 1
    assert _lib.NUTSDIAG_FIELDS == FLOAT_COLUMNS[:11] + ["flags"]
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                        check=True).stdout
    assert re.search(r"\bT mdfit_nuts_diag\b", nm)
    nuts = _lib.default_opts(mode=_lib.MODE_NUTS)
    dummy = ctypes.c_void_p(16)
    assert lib.mdfit_nuts_diag(None, None, 0, ctypes.byref(nuts), None, None) == 0
    assert lib.mdfit_nuts_diag(dummy, dummy, -1, ctypes.byref(nuts), dummy, None) == -1
    assert b"n_taxa" in lib.mdfit_last_error()
    assert lib.mdfit_nuts_diag(dummy, dummy, 1, ctypes.byref(_lib.default_opts()), dummy, None) == -1  # MAP options
    assert b"MDFIT_MODE_NUTS" in lib.mdfit_last_error()
    for S in (1, 0, 4097):
        bad = _lib.default_opts(mode=_lib.MODE_NUTS, num_samples=S)
        assert lib.mdfit_nuts_diag(dummy, dummy, 1, ctypes.byref(bad), dummy, None) == -1
        assert b"num_samples" in lib.mdfit_last_error()
    assert lib.mdfit_nuts_diag(dummy, dummy, 1, ctypes.byref(nuts), None, None) == -1  # diag is required
    assert lib.mdfit_nuts_diag(dummy, dummy, (1 << 25) + 1, ctypes.byref(nuts), dummy, None) == -1


# --------------------------------------------------------------------------
# the reference means something: the analytic AR(1) value
# --------------------------------------------------------------------------
N_REPLICATES = 64


@pytest.mark.parametrize("phi", [0.0, 0.5, 0.9])
def test_reference_vs_analytic_ar1(phi):
    """The ESS of a stationary AR(1) series is S (1 - phi) / (1 + phi).  64
    seeded replicates at S = 4096: their mean ESS within 4 standard errors of
    that mean -- the standard error taken from the replicates themselves; at 64
    replicates it is 0.6-1.7 % of the value, so the check resolves a wrong lag
    range, a missing factor 2 or a wrong centring, which move the ESS by tens
    of per cent.  iid series (phi = 0): the mean split R-hat within 4 of its
    standard errors of 1."""
    S = 4096
    rng = np.random.default_rng([7, int(10 * phi)])
    ess, rhat = [], []
    for _ in range(N_REPLICATES):
        x = cases._ar1(rng, S, phi) if phi else rng.standard_normal(S)
        e, r, _ = ref.series_stats(x)
        ess.append(float(e))
        rhat.append(float(r))
    ess, rhat = np.array(ess), np.array(rhat)
    want = S * (1.0 - phi) / (1.0 + phi)
    se = ess.std(ddof=1) / np.sqrt(N_REPLICATES)
    print(f"phi {phi}: mean ESS {ess.mean():.1f}, analytic {want:.1f}, standard error {se:.1f}")
    assert abs(ess.mean() - want) <= 4.0 * se
    if phi == 0.0:
        se_r = rhat.std(ddof=1) / np.sqrt(N_REPLICATES)
        print(f"iid: mean rhat {rhat.mean():.6f}, standard error {se_r:.6f}")
        assert abs(rhat.mean() - 1.0) <= 4.0 * se_r


def test_reference_edge_definitions():
    rng = np.random.default_rng(3)
    e, r, m = ref.series_stats(np.full(50, 0.3))
    assert np.isnan(e) and np.isnan(r) and np.isnan(m)  # gamma_0 == 0
    for S in (2, 3):
        e, r, m = ref.series_stats(rng.standard_normal(S))
        assert np.isfinite(e) and np.isnan(r) and np.isfinite(m)  # h = 1
    S = 1000
    e, _, _ = ref.series_stats(np.where(np.arange(S) % 2 == 0, 1.0, -1.0))
    assert abs(float(e) - S * np.log10(S)) < 1e-9  # the cap
    e, _, _ = ref.series_stats(cases._ar1(rng, 4096, -0.5))
    assert 4096 < float(e) <= 4096 * np.log10(4096)
    _, r, _ = ref.series_stats(np.arange(S) / S)
    assert abs(float(r) - np.sqrt(7.0)) < 0.01  # a line: B / W = 6 up to O(1/S)
    # centring: a large common offset changes nothing
    z = rng.standard_normal(S)
    a = ref.series_stats(1e8 + 1e-3 * z)
    b = ref.series_stats((1e8 + 1e-3 * z) - 1e8)
    assert abs(float(a[0] - b[0])) <= 1e-12 * float(b[0]) and abs(float(a[1] - b[1])) <= 1e-12


# --------------------------------------------------------------------------
# the crafted cases: the stopping decision is not a matter of rounding
# --------------------------------------------------------------------------
@pytest.mark.parametrize("S,T", cases.SHAPES)
def test_crafted_cases_have_a_decision_margin(S, T):
    want, tr = cases.reference(S, T)
    assert cases.decision_margin_ok(tr) == []
    kinds = {cases.kind_of(t, k, j) for t in range(T) for k in range(6) for j in range(4)}
    assert T < 3 or kinds == set(cases.KINDS)
    if S >= 1000 and T >= 3:  # the far-lag path is exercised: a sum that runs past 100 pairs
        assert max(len(raws) for *_, raws, _ in tr) > 100


# --------------------------------------------------------------------------
# the host build of csrc/mdfit_nutsdiag.h under the sanitizers
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("nutsdiag_host") / "nutsdiag_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "nutsdiag_host_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def _hex(v):
    return float(v).hex() if np.isfinite(v) else ("nan" if np.isnan(v) else ("inf" if v > 0 else "-inf"))


def _run_host(exe, rows):
    lines = [str(len(rows))]
    for x, pmd, status in rows:
        lines.append(f"{x.shape[0]} {int(pmd)} {_hex(status)}")
        lines.append(" ".join(_hex(v) for v in x.ravel()))
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return np.array([[float.fromhex(tok) if "nan" not in tok else np.nan for tok in ln.split()]
                     for ln in r.stdout.strip().splitlines()])


def compare_to_reference(got, want, tol):
    """NaN and flag patterns exactly; values within tol[field] (relative).
    Returns the worst relative error per field."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, ref.NFIELD)
    want = np.asarray(want).reshape(-1, ref.NFIELD)
    w64 = want.astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(w64)), np.argwhere(np.isnan(got) != np.isnan(w64))[:8]
    assert np.array_equal(got[:, ref.FLAGS], w64[:, ref.FLAGS])
    worst = {}
    from metadamage_amd import _lib

    for f, name in enumerate(_lib.NUTSDIAG_FIELDS[:11]):
        ok = ~np.isnan(w64[:, f])
        rel = np.abs(got[ok, f].astype(ref.LD) - want[ok, f]) / np.abs(want[ok, f])
        worst[name] = float(rel.max()) if rel.size else 0.0
    print("worst relative error per field: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= (tol[name] if isinstance(tol, dict) else tol), (name, v)
    return worst


@pytest.mark.parametrize("S,T", cases.SHAPES)
def test_host_program_vs_reference(host_program, S, T):
    x, status = cases.case(S, T)
    want, _ = cases.reference(S, T)
    rows = [(x[t, k], k in ref.PMD_SUBFITS, status[t, k]) for t in range(T) for k in range(6)]
    got = _run_host(host_program, rows).reshape(T, 6, ref.NFIELD)
    compare_to_reference(got, want, HOST_TOL)
    (tn, kn), (ts, ks) = cases.faults(T)
    for t, k in ((tn, kn), (ts, ks)):
        assert np.isnan(got[t, k, :11]).all() and got[t, k, 11] == 0.0
    valid = np.ones((T, 6), bool)
    valid[tn, kn] = valid[ts, ks] = False
    assert (got[valid][:, 11] == 1.0).all()
    if S < 4:  # h = 1: no split R-hat, the ESS is defined
        assert np.isnan(got[valid][:, ref.RHAT:ref.RHAT + 5]).all()
    for t in range(T):
        for k in range(6):
            for j in range(4):
                if valid[t, k] and cases.kind_of(t, k, j) == "const":
                    assert np.isnan(got[t, k, ref.ESS + j]) and np.isnan(got[t, k, ref.RHAT + j])


def test_host_program_special_values(host_program):
    rng = np.random.default_rng(9)
    S = 40
    x = rng.standard_normal((S, 4))
    inf = x.copy()
    inf[7, 3] = np.inf
    null = x.copy()
    null[:, 1:3] = 0.0  # a null sub-fit as the chain kernel stores it
    got = _run_host(host_program, [(x, True, 0.0), (inf, True, 0.0), (x, True, np.nan), (null, False, 0.0),
                                   (x, True, 2.0)])
    assert got[0, 11] == 1.0 and np.isfinite(got[0, :11]).all()
    for r in (1, 2, 4):
        assert got[r, 11] == 0.0 and np.isnan(got[r, :11]).all()
    assert got[3, 11] == 1.0
    assert np.isnan(got[3, [1, 2, 6, 7]]).all() and np.isfinite(got[3, [0, 3, 4, 5, 8, 9, 10]]).all()
    assert got[3, 4] == got[3, 0] and got[3, 9] == got[3, 5]  # D_max of a null sub-fit is its q


# --------------------------------------------------------------------------
# frames, options, CLI, chunk planning, gather record
# --------------------------------------------------------------------------
def _cfg(tmp_path, inference="nuts-diag"):
    from metadamage_amd import utils

    cfg = utils.Config(out_dir=tmp_path, max_fits=10, max_cores=1, min_alignments=10, min_y_sum=10,
                       substitution_bases_forward="CT", substitution_bases_reverse="GA", forced=False,
                       version="0.0.0", inference=inference)
    cfg.add_filename(GOLDEN / "data_ancient.txt")
    return cfg


def test_frame_columns_and_dtypes(tmp_path, oracle_lib, ref_meta):
    from metadamage_amd import _lib, fits

    assert fits.NUTS_DIAG_COLUMNS == FLOAT_COLUMNS and fits.NUTS_DIAG_UINT_COLUMNS == UINT_COLUMNS
    cfg = _cfg(tmp_path)
    p = fits.pack_counts(pd.read_parquet(GOLDEN / "counts_data_ancient.parquet"), cfg)
    out, pred, st = oracle_lib.fit_batch(p.y, p.N, p.mm)
    T = len(st)
    keep = st == 0
    plain = fits.make_df_fit_results(p, out, keep, _cfg(tmp_path, "nuts"))
    assert list(plain.columns) == ref_meta["fit_results_columns"] and len(plain.columns) == 30  # today's frame
    pd.testing.assert_frame_equal(plain, fits.make_df_fit_results(p, out, keep, cfg, diag=None))
    rng = np.random.default_rng(4)
    diag = rng.uniform(1.0, 2000.0, (T, 6, 12)).astype(np.float32)
    diag[:, 1::2, 1:3] = np.nan  # (null sub-fits: A, c)
    diag[:, :, 11] = 1.0
    div = rng.integers(0, 7, (T, 6))
    diag[:, :, 11] += 2.0 * div  # the way fit_packed returns the flags
    diag[1, 4, :11] = np.nan
    diag[1, 4, 11] = 0.0
    div[1, 4] = 0
    df = fits.make_df_fit_results(p, out, keep, cfg, diag=diag)
    assert list(df.columns) == ref_meta["fit_results_columns"] + FLOAT_COLUMNS + UINT_COLUMNS
    assert len(df.columns) == 30 + 17 + 2
    pd.testing.assert_frame_equal(df[plain.columns], plain)
    for c in FLOAT_COLUMNS:
        assert df[c].dtype == np.float32, c
    for c in UINT_COLUMNS:
        assert df[c].dtype == np.uint32, c
    f = _lib.NUTSDIAG_FIELDS.index
    for c in FLOAT_COLUMNS[:11]:
        np.testing.assert_array_equal(df[c].to_numpy(), diag[keep, 0, f(c)])
    np.testing.assert_array_equal(df["ess_q_null"].to_numpy(), diag[keep, 1, f("ess_q")])
    np.testing.assert_array_equal(df["ess_phi_null"].to_numpy(), diag[keep, 1, f("ess_phi")])
    np.testing.assert_array_equal(df["rhat_q_null"].to_numpy(), diag[keep, 1, f("rhat_q")])
    np.testing.assert_array_equal(df["rhat_phi_null"].to_numpy(), diag[keep, 1, f("rhat_phi")])
    np.testing.assert_array_equal(df["ess_min"].to_numpy(), np.nanmin(diag[keep][:, :, 0:5].reshape(-1, 30), axis=1))
    np.testing.assert_array_equal(df["rhat_max"].to_numpy(), np.nanmax(diag[keep][:, :, 5:10].reshape(-1, 30), axis=1))
    np.testing.assert_array_equal(df["divergences"].to_numpy(), div[keep].sum(axis=1).astype(np.uint32))
    want_valid = np.ones(T, np.uint32)
    want_valid[1] = 0
    np.testing.assert_array_equal(df["nuts_diag_valid"].to_numpy(), want_valid[keep])
    # a dropped taxon takes its row with it; a taxon whose every row is invalid gives NaN, not a warning
    k2 = np.array([True, False, True])
    d2 = fits.make_df_fit_results(p, out, k2, cfg, diag=diag)
    np.testing.assert_array_equal(d2["ess_q"].to_numpy(), diag[k2, 0, 0])
    allnan = np.full((T, 6, 12), np.nan, np.float32)
    allnan[:, :, 11] = 0.0
    d3 = fits.make_df_fit_results(p, out, keep, cfg, diag=allnan)
    assert d3["ess_min"].isna().all() and (d3["nuts_diag_valid"] == 0).all() and (d3["divergences"] == 0).all()


def test_make_opts_and_cli(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import _lib, fits
    from metadamage_amd.cli import cli_app

    kw = dict(num_warmup=30, num_samples=50)
    o = fits.make_opts(_cfg(tmp_path, "nuts-diag"), kw)
    m = fits.make_opts(_cfg(tmp_path, "nuts"), kw)
    assert o.mode == _lib.MODE_NUTS and bytes(o) == bytes(m) and o.num_samples == 50
    assert fits.mode_of("nuts-diag") == fits.mode_of("nuts") == _lib.MODE_NUTS
    assert fits.mode_of("map") == fits.mode_of("map-laplace") == _lib.MODE_MAP
    assert fits.wants_diag(_cfg(tmp_path, "nuts-diag")) and not fits.wants_diag(_cfg(tmp_path, "nuts"))
    assert not fits.wants_laplace(_cfg(tmp_path, "nuts-diag")) and not fits.wants_diag(_cfg(tmp_path, "map-laplace"))
    with pytest.raises(ValueError):
        fits.mode_of("nuts-foo")
    bad = CliRunner().invoke(cli_app, ["fit", str(GOLDEN / "data_ancient.txt"), "--out-dir", str(tmp_path),
                                       "--inference", "nuts-foo"])
    assert bad.exit_code == 2 and "nuts-diag" in bad.output
    helptext = CliRunner().invoke(cli_app, ["fit", "--help"]).output
    assert "nuts-diag" in helptext


def test_chunk_planning_counts_the_diag_records():
    from metadamage_amd import _lib, engine

    nuts = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=10, num_samples=100)
    assert engine.DIAG_BYTES == 6 * 12 * 4 == 288
    base = engine.device_bytes(128, nuts)
    assert engine.device_bytes(128, nuts, with_diag=True) == base + 128 * (576 + 288)
    base_dev = engine.device_bytes(128, nuts, dest_on_device=True)
    assert engine.device_bytes(128, nuts, dest_on_device=True, with_diag=True) == base_dev + 128 * 576
    # a budget that holds exactly c taxa with the records holds fewer than without
    per = engine.device_bytes(2, nuts, with_diag=True) - engine.device_bytes(1, nuts, with_diag=True)
    budget = engine.N_SETS * (_lib.SAMPLES_OFFSET + 50 * per)
    chunks = engine.plan_chunks(1000, nuts, budget, with_diag=True)
    cap = max(hi - lo for lo, hi in chunks)
    assert cap <= 50 and engine.N_SETS * engine.device_bytes(cap, nuts, with_diag=True) <= budget
    assert engine.N_SETS * engine.device_bytes(51, nuts, with_diag=True) > budget
    assert chunks[0][0] == 0 and chunks[-1][1] == 1000 and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    plain = engine.plan_chunks(1000, nuts, budget)
    assert max(hi - lo for lo, hi in plain) >= cap and len(plain) <= len(chunks)
    # NUTS only: the mirror image of with_laplace
    for opts in (_lib.default_opts(mode=_lib.MODE_MAP), None):
        with pytest.raises(ValueError):
            engine.device_bytes(128, opts, with_diag=True)
        with pytest.raises(ValueError):
            engine.plan_chunks(1000, opts, with_diag=True)
        with pytest.raises(ValueError):
            engine.ChunkedFitter(16, opts=opts, with_diag=True)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_gather_record_with_diag_round_trips(world):
    import torch

    from metadamage_amd import _lib, distributed as d

    assert d.REC_BYTES == 496 and d.REC_DIAG == 288
    T = 13  # uneven shards: 13 = 7 + 6 = 5 + 5 + 3
    n = d.shard_capacity(T, world)
    rng = np.random.default_rng(2)
    parts, want_diag, want_pred, want_st = [], [], [], []
    for r in range(world):
        lo, hi = d.shard_range(T, r, world)
        buf = torch.from_numpy(rng.integers(0, 256, n * (d.REC_BYTES + d.REC_DIAG), dtype=np.uint8))
        pred, status, ints, floats, diag = d.packed_views(buf, n, with_diag=True)
        p0, s0, i0, f0 = d.packed_views(buf[: n * d.REC_BYTES], n)  # the default layout is a prefix
        assert pred.data_ptr() == p0.data_ptr() and status.data_ptr() == s0.data_ptr()
        assert ints.data_ptr() == i0.data_ptr() and floats.data_ptr() == f0.data_ptr()
        assert diag.shape == (n, 6, _lib.NNUTSDIAG) and diag.dtype == torch.float32
        assert diag.data_ptr() == buf.data_ptr() + n * d.REC_BYTES
        w = rng.standard_normal((n, 6, 12)).astype(np.float32)
        w[0, 1, 1] = np.nan
        wp = rng.standard_normal((n, 3, 30)).astype(np.float32)
        ws = rng.integers(0, 4, n).astype(np.int32)
        diag.copy_(torch.from_numpy(w))
        pred.copy_(torch.from_numpy(wp))
        status.copy_(torch.from_numpy(ws))
        ints.copy_(torch.from_numpy(np.rint(rng.standard_normal((n, 8)) * 100)))
        floats.copy_(torch.from_numpy(rng.standard_normal((n, 17)).astype(np.float32)))
        parts.append(buf)
        want_diag.append(w[: hi - lo])
        want_pred.append(wp[: hi - lo])
        want_st.append(ws[: hi - lo])
    out, pr, ss, dg = d.unpack_gathered(parts, T, world, with_diag=True)
    assert out.shape == (T, 25) and dg.shape == (T, 6, 12) and dg.dtype == np.float32
    np.testing.assert_array_equal(dg, np.concatenate(want_diag))
    np.testing.assert_array_equal(pr, np.concatenate(want_pred))
    np.testing.assert_array_equal(ss, np.concatenate(want_st))
    o3 = d.unpack_gathered([b[: n * d.REC_BYTES] for b in parts], T, world)
    assert len(o3) == 3
    np.testing.assert_array_equal(o3[0], out)
    with pytest.raises(ValueError):
        d.packed_views(parts[0], n, with_laplace=True, with_diag=True)
    with pytest.raises(ValueError):
        d.unpack_gathered(parts, T, world, with_laplace=True, with_diag=True)
