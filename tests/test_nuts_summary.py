"""CPU tests of the posterior summary (MDFIT-SUMM v1): the
C-ABI entry point without a device, the host build of the arithmetic
(csrc/mdfit_nutssumm.h, under the address and undefined-behaviour sanitizers)
against the reference (tests/nuts_summary_ref.py) on the crafted shapes, and
the frame / options / chunk-planning / gather-record plumbing."""

from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from tests import nuts_summary_cases as cases
from tests import nuts_summary_ref as ref
from tests.helpers import GOLDEN

ROOT = Path(__file__).resolve().parents[1]

LAPLACE_NAMES = ["D_max_std", "significance", "q_std", "A_std", "c_std", "concentration_std", "rho_Ac",
                 "D_max_std_forward", "q_std_forward", "D_max_std_reverse", "q_std_reverse"]
FLOAT_COLUMNS = LAPLACE_NAMES + ["D_max_posterior_median", "D_max_posterior_lower_hpdi",
                                 "D_max_posterior_upper_hpdi", "q_median", "q_lower_hpdi", "q_upper_hpdi",
                                 "concentration_median"]
UINT_COLUMNS = ["nuts_summary_valid"]
FIELDS = ["q_std", "A_std", "c_std", "phi_std", "D_max_std", "D_max_mean", "D_max_median", "D_max_lo", "D_max_hi",
          "q_median", "q_lo", "q_hi", "phi_median", "rho_Ac", "significance", "flags"]
# The host build (one lane: sequential sums) against nuts_summary_ref
# (longdouble): the worst error per moment field over every crafted shape,
# measured with g++ 11 on x86-64 (relative; rho_Ac absolute).  Asserted at ten
# times that, never looser than 1e-9; the order statistics get no tolerance.
# D_max_mean and significance are largest where a series' mean is nearly 0 and
# its sum cancels (the (65, 67) shape).
MEASURED_HOST = {"q_std": 2.23e-14, "A_std": 6.11e-15, "c_std": 1.20e-14, "phi_std": 7.91e-15, "D_max_std": 2.23e-14,
                 "D_max_mean": 2.88e-12, "rho_Ac": 7.71e-15, "significance": 2.88e-12}
HOST_TOL = {k: min(10.0 * v, 1e-9) for k, v in MEASURED_HOST.items()}


# --------------------------------------------------------------------------
# ABI
# --------------------------------------------------------------------------
def test_entry_point_declared_exported_and_argument_checked():
    from metadamage_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mdfit.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+mdfit_nuts_summary\s*\(", text)
    assert f"#define MDFIT_NNUTSSUMM {_lib.NNUTSSUMM}" in text
    assert f"#define MDFIT_ABI_VERSION {_lib.ABI_VERSION}" in text and _lib.ABI_VERSION == 3
    assert "mdfit_nuts_summary" in _lib.EXPORTED_SYMBOLS
    assert len(_lib.NUTSSUMM_FIELDS) == _lib.NNUTSSUMM == ref.NFIELD == 16 and _lib.NUTSSUMM_VALID == 1
    assert _lib.NUTSSUMM_FIELDS == FIELDS
    header = (ROOT / "metadamage_amd" / "csrc" / "mdfit_nutssumm.h").read_text()
    layout = dict(re.findall(r"\b(k\w+) = (\d+)", header))
    for name, idx in (("kStd", ref.STD), ("kDmaxMean", ref.D_MEAN), ("kDmaxMedian", ref.D_MEDIAN),
                      ("kDmaxLo", ref.D_LO), ("kDmaxHi", ref.D_HI), ("kQMedian", ref.Q_MEDIAN), ("kQLo", ref.Q_LO),
                      ("kQHi", ref.Q_HI), ("kPhiMedian", ref.PHI_MEDIAN), ("kRhoAc", ref.RHO),
                      ("kSignificance", ref.SIGNIFICANCE), ("kFlags", ref.FLAGS)):
        assert int(layout[name]) == idx, name
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                        check=True).stdout
    assert re.search(r"\bT mdfit_nuts_summary\b", nm)
    nuts = _lib.default_opts(mode=_lib.MODE_NUTS)
    dummy = ctypes.c_void_p(16)
    assert lib.mdfit_nuts_summary(None, None, 0, ctypes.byref(nuts), None, None) == 0
    assert lib.mdfit_nuts_summary(dummy, dummy, -1, ctypes.byref(nuts), dummy, None) == -1
    assert b"n_taxa" in lib.mdfit_last_error()
    assert lib.mdfit_nuts_summary(dummy, dummy, 1, ctypes.byref(_lib.default_opts()), dummy, None) == -1  # MAP
    assert b"MDFIT_MODE_NUTS" in lib.mdfit_last_error()
    for S in (1, 0, 4097):
        bad = _lib.default_opts(mode=_lib.MODE_NUTS, num_samples=S)
        assert lib.mdfit_nuts_summary(dummy, dummy, 1, ctypes.byref(bad), dummy, None) == -1
        assert b"num_samples" in lib.mdfit_last_error()
    assert lib.mdfit_nuts_summary(dummy, dummy, 1, ctypes.byref(nuts), None, None) == -1  # summ is required
    assert lib.mdfit_nuts_summary(dummy, dummy, (1 << 25) + 1, ctypes.byref(nuts), dummy, None) == -1


# --------------------------------------------------------------------------
# the reference's own definitions
# --------------------------------------------------------------------------
def test_reference_definitions():
    rng = np.random.default_rng(5)
    x = rng.standard_normal(1000)
    mean, std = ref.mean_std(x)
    assert abs(float(mean) - x.mean()) < 1e-14 and abs(float(std) - x.std(ddof=1)) < 1e-13
    assert ref.mean_std(np.full(50, 0.3))[1] == 0
    y = 0.5 * x + rng.standard_normal(1000)
    assert abs(float(ref.pearson(x, y)) - np.corrcoef(x, y)[0, 1]) < 1e-13
    assert np.isnan(ref.pearson(x, np.zeros(1000)))
    med, lo, hi = ref.order_stats(rng.permutation(1000).astype(float))
    assert (med, lo, hi) == (499.5, 0.0, 680.0)  # every window ties: the first one
    assert ref.order_stats(np.array([3.0, 1.0])) == (2.0, 1.0, 3.0)  # S = 2: one window, [min, max]
    for S in cases.S_VALUES:
        assert 1 <= cases.window(S) < S


# --------------------------------------------------------------------------
# the host build of csrc/mdfit_nutssumm.h under the sanitizers
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("nutssumm_host") / "nutssumm_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "nutssumm_host_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def _hex(v):
    return float(v).hex() if np.isfinite(v) else ("nan" if np.isnan(v) else ("inf" if v > 0 else "-inf"))


def _run_host(exe, rows, tmp_path):
    lines = [str(len(rows))]
    for x, pmd, status in rows:
        lines.append(f"{x.shape[0]} {int(pmd)} {_hex(status)}")
        lines.append(" ".join(_hex(v) for v in x.ravel()))
    src = tmp_path / "draws.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return np.array([[float.fromhex(tok) if "nan" not in tok else np.nan for tok in ln.split()]
                     for ln in r.stdout.strip().splitlines()])


def errors_vs_reference(got, want):
    """NaN and flag patterns and the order statistics exactly (by value);
    returns the worst error per moment field (relative; rho_Ac absolute; a
    reference of exactly 0 -- the std of a constant series -- must be met
    exactly)."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, ref.NFIELD)
    want = np.asarray(want).reshape(-1, ref.NFIELD)
    w64 = want.astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(w64)), np.argwhere(np.isnan(got) != np.isnan(w64))[:8]
    assert np.array_equal(got[:, ref.FLAGS], w64[:, ref.FLAGS])
    for f in ref.ORDER_FIELDS:
        assert np.array_equal(got[:, f], w64[:, f], equal_nan=True), (FIELDS[f], np.argwhere(got[:, f] != w64[:, f])[:8])
    worst = {}
    for f in ref.MOMENT_FIELDS:
        ok = ~np.isnan(w64[:, f])
        zero = ok & (want[:, f] == 0)
        assert (got[zero, f] == 0.0).all(), FIELDS[f]
        ok &= ~zero
        err = np.abs(got[ok, f].astype(ref.LD) - want[ok, f])
        if f != ref.RHO:
            err = err / np.abs(want[ok, f])
        worst[FIELDS[f]] = float(err.max()) if err.size else 0.0
    return worst


def compare_to_reference(got, want, tol):
    worst = errors_vs_reference(got, want)
    print("worst error per field: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= tol[name], (name, v)
    return worst


def check_crafted_properties(got, S, T):
    """What the crafted rows must show whatever computed them: got[T, 6, 16]."""
    x, _ = cases.case(S, T)
    (tn, kn), (ts, ks) = cases.faults(T)
    valid = np.ones((T, 6), bool)
    valid[tn, kn] = valid[ts, ks] = False
    assert np.isnan(got[~valid][:, :15]).all() and (got[~valid][:, 15] == 0.0).all()
    assert (got[valid][:, 15] == 1.0).all()
    L = cases.window(S)
    for t, k in cases.RAMP_ROWS:  # every window ties: the lowest index, [0, L]
        assert tuple(got[t, k, [ref.D_LO, ref.D_HI, ref.Q_LO, ref.Q_HI]]) == (0.0, L, 0.0, L), (t, k)
        assert got[t, k, ref.D_MEDIAN] == got[t, k, ref.Q_MEDIAN] == got[t, k, ref.PHI_MEDIAN] == 0.5 * (S - 1)
        assert got[t, k, ref.STD + 2] == 0.0 and np.isnan(got[t, k, ref.RHO])  # c is constant
    for t in range(T):
        for k in range(6):
            if not valid[t, k]:
                continue
            r = got[t, k]
            assert r[ref.D_LO] <= r[ref.D_MEDIAN] <= r[ref.D_HI] and r[ref.Q_LO] <= r[ref.Q_MEDIAN] <= r[ref.Q_HI]
            if (t, k) in cases.RAMP_ROWS:
                continue
            kinds = [cases.kind_of(t, k, j) for j in range(4)]
            for j in range(4):
                assert (r[ref.STD + j] == 0.0) == (kinds[j] == "const"), (t, k, j)
            if kinds[0] == "const":
                assert r[ref.Q_MEDIAN] == r[ref.Q_LO] == r[ref.Q_HI] == x[t, k, 0, 0]
            if kinds[3] == "const":
                assert r[ref.PHI_MEDIAN] == x[t, k, 0, 3]
            if "const" in kinds[1:3]:
                assert np.isnan(r[ref.RHO])
            else:
                assert abs(r[ref.RHO]) <= 1.0 + 1e-12  # (S = 2 gives +-1 up to a few roundings)
            if k not in ref.PMD_SUBFITS:  # D_max of a null sub-fit is its q
                assert np.array_equal(r[[4, ref.D_MEDIAN, ref.D_LO, ref.D_HI]],
                                      r[[0, ref.Q_MEDIAN, ref.Q_LO, ref.Q_HI]])
                if kinds[0] == "const":
                    assert r[4] == 0.0 and np.isnan(r[ref.SIGNIFICANCE]) and r[ref.D_MEAN] == x[t, k, 0, 0]


@pytest.mark.parametrize("S,T", cases.SHAPES)
def test_host_program_vs_reference(host_program, tmp_path, S, T):
    x, status = cases.case(S, T)
    want = cases.reference(S, T)
    rows = [(x[t, k], k in ref.PMD_SUBFITS, status[t, k]) for t in range(T) for k in range(6)]
    got = _run_host(host_program, rows, tmp_path).reshape(T, 6, ref.NFIELD)
    print(f"S={S} T={T}", end=": ")
    compare_to_reference(got, want, HOST_TOL)
    check_crafted_properties(got, S, T)


def test_host_program_special_values(host_program, tmp_path):
    rng = np.random.default_rng(9)
    S = 40
    x = rng.standard_normal((S, 4))
    inf = x.copy()
    inf[7, 3] = np.inf
    null = x.copy()
    null[:, 1:3] = 0.0  # a null sub-fit as the chain kernel stores it
    const = np.full((S, 4), 0.3)
    got = _run_host(host_program, [(x, True, 0.0), (inf, True, 0.0), (x, True, np.nan), (null, False, 0.0),
                                   (x, True, 2.0), (const, True, 0.0)], tmp_path)
    assert got[0, 15] == 1.0 and np.isfinite(got[0, :15]).all()
    for r in (1, 2, 4):
        assert got[r, 15] == 0.0 and np.isnan(got[r, :15]).all()
    # the null row: A_std = c_std = 0, rho NaN, the D_max fields are q's
    assert got[3, 15] == 1.0 and got[3, 1] == got[3, 2] == 0.0 and np.isnan(got[3, ref.RHO])
    assert np.array_equal(got[3, [4, ref.D_MEDIAN, ref.D_LO, ref.D_HI]], got[3, [0, ref.Q_MEDIAN, ref.Q_LO, ref.Q_HI]])
    assert abs(got[3, ref.D_MEAN] - null[:, 0].mean()) < 1e-14
    assert np.isfinite(got[3, ref.SIGNIFICANCE])
    # the constant row: std 0 (not NaN), significance NaN, median = lo = hi = the constant (D_max: 0.3 + 0.3)
    assert got[5, 15] == 1.0 and (got[5, 0:5] == 0.0).all() and np.isnan(got[5, [ref.RHO, ref.SIGNIFICANCE]]).all()
    assert (got[5, [ref.Q_MEDIAN, ref.Q_LO, ref.Q_HI, ref.PHI_MEDIAN]] == 0.3).all()
    assert (got[5, [ref.D_MEAN, ref.D_MEDIAN, ref.D_LO, ref.D_HI]] == 0.3 + 0.3).all()


# --------------------------------------------------------------------------
# frames, options, CLI, chunk planning, gather record
# --------------------------------------------------------------------------
def _cfg(tmp_path, inference="nuts-summary"):
    from metadamage_amd import utils

    cfg = utils.Config(out_dir=tmp_path, max_fits=10, max_cores=1, min_alignments=10, min_y_sum=10,
                       substitution_bases_forward="CT", substitution_bases_reverse="GA", forced=False,
                       version="0.0.0", inference=inference)
    cfg.add_filename(GOLDEN / "data_ancient.txt")
    return cfg


def test_frame_columns_and_dtypes(tmp_path, oracle_lib, ref_meta):
    from metadamage_amd import _lib, fits

    assert fits.NUTS_SUMMARY_COLUMNS == FLOAT_COLUMNS and fits.NUTS_SUMMARY_UINT_COLUMNS == UINT_COLUMNS
    assert FLOAT_COLUMNS[:11] == [name for name, _, _ in fits.LAPLACE_COLUMNS]  # one set of names downstream
    cfg = _cfg(tmp_path)
    p = fits.pack_counts(pd.read_parquet(GOLDEN / "counts_data_ancient.parquet"), cfg)
    out, pred, st = oracle_lib.fit_batch(p.y, p.N, p.mm)
    T = len(st)
    keep = st == 0
    plain = fits.make_df_fit_results(p, out, keep, _cfg(tmp_path, "nuts"))
    assert list(plain.columns) == ref_meta["fit_results_columns"] and len(plain.columns) == 30  # today's frame
    pd.testing.assert_frame_equal(plain, fits.make_df_fit_results(p, out, keep, cfg, summ=None))
    rng = np.random.default_rng(4)
    summ = rng.uniform(0.01, 2.0, (T, 6, 16)).astype(np.float32)
    summ[:, 1::2, 13] = np.nan  # (null sub-fits: rho)
    summ[:, :, 15] = 1.0
    summ[1, 3, :15] = np.nan  # one PMD row invalid: the taxon is
    summ[1, 3, 15] = 0.0
    summ[2, 4, :15] = np.nan  # a null row invalid: not part of nuts_summary_valid
    summ[2, 4, 15] = 0.0
    df = fits.make_df_fit_results(p, out, keep, cfg, summ=summ)
    assert list(df.columns) == ref_meta["fit_results_columns"] + FLOAT_COLUMNS + UINT_COLUMNS
    assert len(df.columns) == 30 + 18 + 1 == 49
    pd.testing.assert_frame_equal(df[plain.columns], plain)
    for c in FLOAT_COLUMNS:
        assert df[c].dtype == np.float32, c
    assert df["nuts_summary_valid"].dtype == np.uint32
    f = _lib.NUTSSUMM_FIELDS.index
    picks = [("D_max_std", 0, "D_max_std"), ("significance", 0, "significance"), ("q_std", 0, "q_std"),
             ("A_std", 0, "A_std"), ("c_std", 0, "c_std"), ("concentration_std", 0, "phi_std"),
             ("rho_Ac", 0, "rho_Ac"), ("D_max_std_forward", 2, "D_max_std"), ("q_std_forward", 2, "q_std"),
             ("D_max_std_reverse", 3, "D_max_std"), ("q_std_reverse", 3, "q_std"),
             ("D_max_posterior_median", 0, "D_max_median"), ("D_max_posterior_lower_hpdi", 0, "D_max_lo"),
             ("D_max_posterior_upper_hpdi", 0, "D_max_hi"), ("q_median", 0, "q_median"), ("q_lower_hpdi", 0, "q_lo"),
             ("q_upper_hpdi", 0, "q_hi"), ("concentration_median", 0, "phi_median")]
    assert [c for c, _, _ in picks] == FLOAT_COLUMNS
    for c, row, field in picks:
        np.testing.assert_array_equal(df[c].to_numpy(), summ[keep, row, f(field)], err_msg=c)
    want_valid = np.ones(T, np.uint32)
    want_valid[1] = 0
    np.testing.assert_array_equal(df["nuts_summary_valid"].to_numpy(), want_valid[keep])
    # a dropped taxon takes its row with it
    k2 = np.array([True, False, True])
    d2 = fits.make_df_fit_results(p, out, k2, cfg, summ=summ)
    np.testing.assert_array_equal(d2["q_std"].to_numpy(), summ[k2, 0, 0])
    np.testing.assert_array_equal(d2["nuts_summary_valid"].to_numpy(), want_valid[k2])


def test_make_opts_and_cli(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import _lib, fits
    from metadamage_amd.cli import cli_app

    kw = dict(num_warmup=30, num_samples=50)
    o = fits.make_opts(_cfg(tmp_path, "nuts-summary"), kw)
    m = fits.make_opts(_cfg(tmp_path, "nuts"), kw)
    assert o.mode == _lib.MODE_NUTS and bytes(o) == bytes(m) and o.num_samples == 50
    assert fits.mode_of("nuts-summary") == fits.mode_of("nuts-diag") == fits.mode_of("nuts") == _lib.MODE_NUTS
    assert fits.mode_of("map") == fits.mode_of("map-laplace") == _lib.MODE_MAP
    assert fits.wants_summary(_cfg(tmp_path, "nuts-summary"))
    for other in ("nuts", "nuts-diag", "map", "map-laplace"):
        assert not fits.wants_summary(_cfg(tmp_path, other)), other
    assert not fits.wants_diag(_cfg(tmp_path, "nuts-summary")) and not fits.wants_laplace(_cfg(tmp_path, "nuts-summary"))
    with pytest.raises(ValueError, match="nuts-summary"):
        fits.mode_of("nuts-foo")
    bad = CliRunner().invoke(cli_app, ["fit", str(GOLDEN / "data_ancient.txt"), "--out-dir", str(tmp_path),
                                       "--inference", "nuts-foo"])
    assert bad.exit_code == 2
    for name in ("nuts", "map", "map-laplace", "nuts-diag", "nuts-summary"):
        assert name in bad.output, name
    helptext = CliRunner().invoke(cli_app, ["fit", "--help"]).output
    assert "nuts-summary" in helptext and "nuts-diag" in helptext and "map-laplace" in helptext


def test_chunk_planning_counts_the_summary_records():
    from metadamage_amd import _lib, engine

    nuts = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=10, num_samples=100)
    assert engine.SUMM_BYTES == 6 * 16 * 4 == 384
    base = engine.device_bytes(128, nuts)
    assert engine.device_bytes(128, nuts, with_summary=True) == base + 128 * (768 + 384)
    base_dev = engine.device_bytes(128, nuts, dest_on_device=True)
    assert engine.device_bytes(128, nuts, dest_on_device=True, with_summary=True) == base_dev + 128 * 768
    # a budget that holds exactly c taxa with the records holds fewer than without
    per = engine.device_bytes(2, nuts, with_summary=True) - engine.device_bytes(1, nuts, with_summary=True)
    budget = engine.N_SETS * (_lib.SAMPLES_OFFSET + 50 * per)
    chunks = engine.plan_chunks(1000, nuts, budget, with_summary=True)
    cap = max(hi - lo for lo, hi in chunks)
    assert cap <= 50 and engine.N_SETS * engine.device_bytes(cap, nuts, with_summary=True) <= budget
    assert engine.N_SETS * engine.device_bytes(51, nuts, with_summary=True) > budget
    assert chunks[0][0] == 0 and chunks[-1][1] == 1000 and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    plain = engine.plan_chunks(1000, nuts, budget)
    assert max(hi - lo for lo, hi in plain) >= cap and len(plain) <= len(chunks)
    # NUTS only
    for opts in (_lib.default_opts(mode=_lib.MODE_MAP), None):
        with pytest.raises(ValueError):
            engine.device_bytes(128, opts, with_summary=True)
        with pytest.raises(ValueError):
            engine.plan_chunks(1000, opts, with_summary=True)
        with pytest.raises(ValueError):
            engine.ChunkedFitter(16, opts=opts, with_summary=True)
    # one optional extra block per run
    with pytest.raises(ValueError, match="mutually exclusive"):
        engine.device_bytes(128, nuts, with_summary=True, with_diag=True)
    with pytest.raises(ValueError, match="mutually exclusive"):
        engine.plan_chunks(1000, nuts, with_summary=True, with_diag=True)
    with pytest.raises(ValueError, match="mutually exclusive"):
        engine.ChunkedFitter(16, opts=nuts, with_summary=True, with_diag=True)
    with pytest.raises(ValueError):
        engine.ChunkedFitter(16, opts=nuts, with_summary=True, with_laplace=True)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_gather_record_with_summary_round_trips(world):
    import torch

    from metadamage_amd import _lib, distributed as d

    assert d.REC_BYTES == 496 and d.REC_SUMM == 384
    T = 13  # uneven shards: 13 = 7 + 6 = 5 + 5 + 3
    n = d.shard_capacity(T, world)
    rng = np.random.default_rng(2)
    parts, want_summ, want_pred, want_st = [], [], [], []
    for r in range(world):
        lo, hi = d.shard_range(T, r, world)
        buf = torch.from_numpy(rng.integers(0, 256, n * (d.REC_BYTES + d.REC_SUMM), dtype=np.uint8))
        pred, status, ints, floats, summ = d.packed_views(buf, n, with_summary=True)
        p0, s0, i0, f0 = d.packed_views(buf[: n * d.REC_BYTES], n)  # the default layout is a prefix
        assert pred.data_ptr() == p0.data_ptr() and status.data_ptr() == s0.data_ptr()
        assert ints.data_ptr() == i0.data_ptr() and floats.data_ptr() == f0.data_ptr()
        assert summ.shape == (n, 6, _lib.NNUTSSUMM) and summ.dtype == torch.float32
        assert summ.data_ptr() == buf.data_ptr() + n * d.REC_BYTES
        w = rng.standard_normal((n, 6, 16)).astype(np.float32)
        w[0, 1, 13] = np.nan
        wp = rng.standard_normal((n, 3, 30)).astype(np.float32)
        ws = rng.integers(0, 4, n).astype(np.int32)
        summ.copy_(torch.from_numpy(w))
        pred.copy_(torch.from_numpy(wp))
        status.copy_(torch.from_numpy(ws))
        ints.copy_(torch.from_numpy(np.rint(rng.standard_normal((n, 8)) * 100)))
        floats.copy_(torch.from_numpy(rng.standard_normal((n, 17)).astype(np.float32)))
        parts.append(buf)
        want_summ.append(w[: hi - lo])
        want_pred.append(wp[: hi - lo])
        want_st.append(ws[: hi - lo])
    out, pr, ss, sm = d.unpack_gathered(parts, T, world, with_summary=True)
    assert out.shape == (T, 25) and sm.shape == (T, 6, 16) and sm.dtype == np.float32
    np.testing.assert_array_equal(sm, np.concatenate(want_summ))
    np.testing.assert_array_equal(pr, np.concatenate(want_pred))
    np.testing.assert_array_equal(ss, np.concatenate(want_st))
    o3 = d.unpack_gathered([b[: n * d.REC_BYTES] for b in parts], T, world)
    assert len(o3) == 3
    np.testing.assert_array_equal(o3[0], out)
    for other in ("with_laplace", "with_diag"):
        with pytest.raises(ValueError):
            d.packed_views(parts[0], n, with_summary=True, **{other: True})
        with pytest.raises(ValueError):
            d.unpack_gathered(parts, T, world, with_summary=True, **{other: True})
        with pytest.raises(ValueError):
            d.alloc_records(4, "cpu", with_summary=True, **{other: True})
