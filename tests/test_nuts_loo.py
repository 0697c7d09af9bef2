"""CPU tests of PSIS-LOO (MDFIT-LOO v1): the C-ABI entry points
without a device, the reference's own definitions on hand-checkable inputs, the
host build of the arithmetic (csrc/mdfit_nutsloo.h, under the address and
undefined-behaviour sanitizers) against the reference (tests/nuts_loo_ref.py) on
the crafted series, and the frame / options / chunk-planning / gather-record
plumbing."""

from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from tests import nuts_loo_cases as cases
from tests import nuts_loo_ref as ref
from tests.helpers import GOLDEN

ROOT = Path(__file__).resolve().parents[1]

FLOAT_COLUMNS = ["elpd_loo", "p_loo", "elpd_loo_se", "pareto_k_max", "elpd_loo_null", "p_loo_null",
                 "pareto_k_max_null", "n_sigma_loo", "n_sigma_loo_forward", "n_sigma_loo_reverse", "asymmetry_loo"]
UINT_COLUMNS = ["pareto_k_bad", "nuts_loo_valid"]
FIELDS = ["elpd_loo", "p_loo", "elpd_se", "khat_max", "khat_argmax", "n_bad", "lppd", "flags"]
# The host build (one lane: sequential sums, libm) against nuts_loo_ref
# (longdouble) on identical series: the worst error over every crafted series,
# measured with g++ 11 on x86-64 -- elpd relative, khat absolute (it passes
# through the grid's softmax and is O(1), 0 included).  Asserted at ten times
# that, never looser than 1e-9.  Where the reference gives +-inf or exactly 0,
# khat must equal it.
MEASURED_HOST = {"elpd": 1.58e-13, "khat": 9.98e-15}
HOST_TOL = {k: min(10.0 * v, 1e-9) for k, v in MEASURED_HOST.items()}


# --------------------------------------------------------------------------
# ABI
# --------------------------------------------------------------------------
def test_entry_points_declared_exported_and_argument_checked():
    from metadamage_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mdfit.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+mdfit_nuts_loo\s*\(", text) and re.search(r"\bint\s+mdfit_psis\s*\(", text)
    assert f"#define MDFIT_NNUTSLOO {_lib.NNUTSLOO}" in text
    assert f"#define MDFIT_ABI_VERSION {_lib.ABI_VERSION}" in text and _lib.ABI_VERSION == 3
    assert "mdfit_nuts_loo" in _lib.EXPORTED_SYMBOLS and "mdfit_psis" in _lib.EXPORTED_SYMBOLS
    assert len(_lib.NUTSLOO_FIELDS) == len(_lib.NUTSLOO_COMPARE_FIELDS) == _lib.NNUTSLOO == ref.NFIELD == 8
    assert _lib.NUTSLOO_FIELDS == FIELDS and _lib.NLOOROW == 7 and _lib.NUTSLOO_VALID == 1
    assert _lib.NUTSLOO_COMPARE_FIELDS[:4] == ["n_sigma_loo", "n_sigma_loo_forward", "n_sigma_loo_reverse",
                                               "asymmetry_loo"]
    header = (ROOT / "metadamage_amd" / "csrc" / "mdfit_nutsloo.h").read_text()
    layout = dict(re.findall(r"\b(k\w+) = (\d+)", header))
    for name, idx in (("kElpd", ref.ELPD), ("kPLoo", ref.P_LOO), ("kElpdSe", ref.ELPD_SE), ("kKhatMax", ref.KHAT_MAX),
                      ("kKhatArgmax", ref.KHAT_ARGMAX), ("kNBad", ref.N_BAD), ("kLppd", ref.LPPD),
                      ("kFlags", ref.FLAGS), ("kNSigma", ref.N_SIGMA), ("kNSigmaForward", ref.N_SIGMA_FORWARD),
                      ("kNSigmaReverse", ref.N_SIGMA_REVERSE), ("kAsymmetry", ref.ASYMMETRY),
                      ("kAllKhatMax", ref.ALL_KHAT_MAX), ("kAllNBad", ref.ALL_N_BAD)):
        assert int(layout[name]) == idx, name
    # the tail and the grid fit their buffers at every S the entry points accept
    assert max(ref.tail_len(S) for S in range(2, 4097)) <= int(layout["kMaxTail"])
    assert 30 + int(np.sqrt(int(layout["kMaxTail"]))) <= int(layout["kMaxGrid"])
    assert 2 * int(layout["kMaxGrid"]) <= int(layout["kGridBuf"])
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                        check=True).stdout
    assert re.search(r"\bT mdfit_nuts_loo\b", nm) and re.search(r"\bT mdfit_psis\b", nm)
    nuts = _lib.default_opts(mode=_lib.MODE_NUTS)
    dummy = ctypes.c_void_p(16)
    loo = lib.mdfit_nuts_loo
    assert loo(None, None, None, None, 0, ctypes.byref(nuts), None, None, None) == 0
    assert loo(dummy, dummy, dummy, dummy, -1, ctypes.byref(nuts), dummy, None, None) == -1
    assert b"n_taxa" in lib.mdfit_last_error()
    assert loo(dummy, dummy, dummy, dummy, 1, ctypes.byref(_lib.default_opts()), dummy, None, None) == -1  # MAP
    assert b"MDFIT_MODE_NUTS" in lib.mdfit_last_error()
    for S in (1, 0, 4097):
        bad = _lib.default_opts(mode=_lib.MODE_NUTS, num_samples=S)
        assert loo(dummy, dummy, dummy, dummy, 1, ctypes.byref(bad), dummy, None, None) == -1
        assert b"num_samples" in lib.mdfit_last_error()
        assert lib.mdfit_psis(dummy, 1, S, dummy, dummy, None) == -1
        assert b"[2, 4096]" in lib.mdfit_last_error()
    assert loo(dummy, dummy, dummy, dummy, 1, ctypes.byref(nuts), None, None, None) == -1  # loo is required
    assert loo(None, dummy, dummy, dummy, 1, ctypes.byref(nuts), dummy, None, None) == -1  # y is
    assert loo(dummy, dummy, dummy, dummy, (1 << 25) + 1, ctypes.byref(nuts), dummy, None, None) == -1
    assert lib.mdfit_psis(None, 0, 100, None, None, None) == 0
    assert lib.mdfit_psis(dummy, -1, 100, dummy, dummy, None) == -1
    assert lib.mdfit_psis(dummy, 1, 100, None, dummy, None) == -1
    assert lib.mdfit_psis(dummy, (1 << 25) + 1, 100, dummy, dummy, None) == -1


# --------------------------------------------------------------------------
# the reference's own definitions
# --------------------------------------------------------------------------
def test_reference_definitions():
    assert [ref.tail_len(S) for S in (2, 24, 25, 100, 225, 226, 1000, 4096)] == [0, 4, 5, 20, 45, 45, 95, 192]
    tau = ref.khat_threshold(1000)
    assert abs(tau - 2.0 / 3.0) < 1e-15 and ref.khat_threshold(10 ** 6) == 0.7
    # Pareto importance ratios (1 - u)^(-k): l = -log ratio = k log1p(-u)
    u = np.random.default_rng(0).uniform(size=1000)
    khat = [float(ref.psis(k * np.log1p(-u))[1]) for k in (0.2, 0.5, 0.9)]
    print("khat of Pareto ratios, k = 0.2, 0.5, 0.9:", khat)  # 0.191, 0.449, 0.800
    assert khat[0] < khat[1] < khat[2] and khat[0] < tau < khat[2]
    assert abs(khat[0] - 0.2) < 0.15 and abs(khat[1] - 0.5) < 0.15
    # a Gaussian l of sd 0.1 (the crafted one): a thin tail.  (At M = 95 the
    # estimate's own spread is ~0.1 and its prior pulls it 0.05 towards 0.5, so
    # the sign is this series', not every seed's.)
    ll, kinds = cases.psis_case(1000)
    e, k = ref.psis(ll[kinds.index("gauss0.1")])
    assert k < 0 and abs(float(e) + 3.0) < 0.05
    # a constant series: khat 0 and elpd = l, exactly
    e, k = ref.psis(np.full(1000, -2.75))
    assert k == 0 and e == -2.75
    # S = 24: M < 5, khat +inf and the plain importance-sampling (harmonic mean) value
    l24 = np.random.default_rng(1).standard_normal(24) - 3.0
    e, k = ref.psis(l24)
    assert k == np.inf
    plain = -np.log(np.mean(np.exp(-l24.astype(ref.LD))))
    assert abs(float(e - plain)) < 1e-15
    # a value that is not finite: NaN
    bad = l24.copy()
    bad[3] = -np.inf
    assert all(np.isnan(v) for v in ref.psis(bad))
    # smoothing pulls the largest weights in: elpd_psis >= the plain value on a heavy tail
    heavy = 0.9 * np.log1p(-u)
    assert ref.psis(heavy)[0] > -np.log(np.mean(np.exp(-heavy.astype(ref.LD))))
    # the comparison: a better PMD column gives a positive n_sigma
    a = np.arange(30.0)
    assert ref.n_sigma(a, a + 1 + 0.1 * np.sin(a)) > 0 and ref.n_sigma(a + 1 + 0.1 * np.sin(a), a) < 0


# --------------------------------------------------------------------------
# the host build of csrc/mdfit_nutsloo.h under the sanitizers
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("nutsloo_host") / "nutsloo_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "nutsloo_host_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def _hex(v):
    return float(v).hex() if np.isfinite(v) else ("nan" if np.isnan(v) else ("inf" if v > 0 else "-inf"))


def _run_host(exe, series, tmp_path):
    lines = [str(len(series))]
    for l in series:
        lines.append(str(len(l)))
        lines.append(" ".join(_hex(v) for v in l))
    src = tmp_path / "series.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = np.array([[float.fromhex(tok) if "nan" not in tok else np.nan for tok in ln.split()]
                    for ln in r.stdout.strip().splitlines()])
    return got[:, 0], got[:, 1]


def errors_vs_reference(elpd, khat, want_elpd, want_khat, skip=None):
    """NaN patterns and khat's special values (+-inf, exactly 0) by value; returns
    the worst errors {"elpd": relative, "khat": absolute} over the entries not in
    `skip` (a boolean mask)."""
    elpd, khat = np.asarray(elpd, dtype=np.float64).ravel(), np.asarray(khat, dtype=np.float64).ravel()
    we, wk = np.asarray(want_elpd).ravel(), np.asarray(want_khat).ravel()
    use = np.ones(elpd.shape, bool) if skip is None else ~np.asarray(skip).ravel()
    we64, wk64 = we.astype(np.float64), wk.astype(np.float64)
    assert np.array_equal(np.isnan(elpd), np.isnan(we64)) and np.array_equal(np.isnan(khat), np.isnan(wk64))
    special = use & ~np.isnan(wk64) & (np.isinf(wk64) | (wk64 == 0))
    assert np.array_equal(khat[special], wk64[special]), (khat[special], wk64[special])
    ok = use & ~np.isnan(we64)
    err_e = np.abs(elpd[ok].astype(ref.LD) - we[ok]) / np.abs(we[ok])
    okk = use & np.isfinite(wk64) & ~special
    err_k = np.abs(khat[okk].astype(ref.LD) - wk[okk])
    return {"elpd": float(err_e.max()) if err_e.size else 0.0, "khat": float(err_k.max()) if err_k.size else 0.0}


def compare_to_reference(elpd, khat, want_elpd, want_khat, tol, skip=None):
    worst = errors_vs_reference(elpd, khat, want_elpd, want_khat, skip)
    print("worst error: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= tol[name], (name, v)
    return worst


@pytest.mark.parametrize("S,n", cases.PSIS_SHAPES)
def test_host_program_vs_reference(host_program, tmp_path, S, n):
    ll, kinds = cases.psis_case(S, n)
    want_e, want_k = cases.psis_reference(S, n)
    e, k = _run_host(host_program, ll, tmp_path)
    print(f"S={S} n={len(kinds)}", end=": ")
    compare_to_reference(e, k, want_e, want_k, HOST_TOL)
    for i, kind in enumerate(kinds):
        if kind == "const":
            assert k[i] == (0.0 if S >= 25 else np.inf) and e[i] == ll[i, 0]
        if S < 25:
            assert k[i] == np.inf
        if kind == "xstar0" and S >= 25:
            assert k[i] == np.inf


def test_host_program_special_values(host_program, tmp_path):
    sp = cases.special_series()
    e, k = _run_host(host_program, [l for _, l in sp], tmp_path)
    got = {name: (e[i], k[i]) for i, (name, _) in enumerate(sp)}
    want = {name: ref.psis(l) for name, l in sp}
    for name in ("nan", "-inf", "+inf"):
        assert np.isnan(got[name][0]) and np.isnan(got[name][1]), name
    assert got["const"] == (-1.5, 0.0)
    assert got["flat_tail"][1] == 0.0 and want["flat_tail"][1] == 0  # a constant tail under a series that is not
    assert got["xstar0"][1] == np.inf and want["xstar0"][1] == np.inf  # x* = 0, the tail not constant
    assert got["S24"][1] == np.inf and got["S2"][1] == np.inf
    assert np.isfinite(got["ties"][1]) and np.isfinite(want["ties"][1])  # ties across the cutoff rank: M by rank
    names = [name for name, _ in sp]
    compare_to_reference(e, k, [want[n][0] for n in names], [want[n][1] for n in names], HOST_TOL)


# --------------------------------------------------------------------------
# frames, options, CLI, chunk planning, gather record
# --------------------------------------------------------------------------
def _cfg(tmp_path, inference="nuts-loo"):
    from metadamage_amd import utils

    cfg = utils.Config(out_dir=tmp_path, max_fits=10, max_cores=1, min_alignments=10, min_y_sum=10,
                       substitution_bases_forward="CT", substitution_bases_reverse="GA", forced=False,
                       version="0.0.0", inference=inference)
    cfg.add_filename(GOLDEN / "data_ancient.txt")
    return cfg


def test_frame_columns_and_dtypes(tmp_path, oracle_lib, ref_meta):
    from metadamage_amd import fits

    assert fits.NUTS_LOO_COLUMNS == FLOAT_COLUMNS and fits.NUTS_LOO_UINT_COLUMNS == UINT_COLUMNS
    cfg = _cfg(tmp_path)
    p = fits.pack_counts(pd.read_parquet(GOLDEN / "counts_data_ancient.parquet"), cfg)
    out, pred, st = oracle_lib.fit_batch(p.y, p.N, p.mm)
    T = len(st)
    keep = st == 0
    plain = fits.make_df_fit_results(p, out, keep, _cfg(tmp_path, "nuts"))
    assert list(plain.columns) == ref_meta["fit_results_columns"] and len(plain.columns) == 30  # today's frame
    pd.testing.assert_frame_equal(plain, fits.make_df_fit_results(p, out, keep, cfg, loo=None))
    rng = np.random.default_rng(4)
    loo = rng.uniform(0.01, 2.0, (T, 7, 8)).astype(np.float32)
    loo[:, :, 7] = 1.0
    loo[:, 6, 5] = np.arange(T) + 3.0  # the bad count
    loo[1, 3, :7] = np.nan  # one row invalid: the taxon's comparisons are
    loo[1, 3, 7] = 0.0
    loo[1, 6, 7] = 0.0
    loo[1, 6, 1] = np.nan
    df = fits.make_df_fit_results(p, out, keep, cfg, loo=loo)
    assert list(df.columns) == ref_meta["fit_results_columns"] + FLOAT_COLUMNS + UINT_COLUMNS
    assert len(df.columns) == 30 + 11 + 2 == 43
    pd.testing.assert_frame_equal(df[plain.columns], plain)
    for c in FLOAT_COLUMNS:
        assert df[c].dtype == np.float32, c
    for c in UINT_COLUMNS:
        assert df[c].dtype == np.uint32, c
    picks = [("elpd_loo", 0, 0), ("p_loo", 0, 1), ("elpd_loo_se", 0, 2), ("pareto_k_max", 0, 3),
             ("elpd_loo_null", 1, 0), ("p_loo_null", 1, 1), ("pareto_k_max_null", 1, 3), ("n_sigma_loo", 6, 0),
             ("n_sigma_loo_forward", 6, 1), ("n_sigma_loo_reverse", 6, 2), ("asymmetry_loo", 6, 3)]
    assert [c for c, _, _ in picks] == FLOAT_COLUMNS
    for c, row, field in picks:
        np.testing.assert_array_equal(df[c].to_numpy(), loo[keep, row, field], err_msg=c)
    np.testing.assert_array_equal(df["pareto_k_bad"].to_numpy(), (np.arange(T) + 3).astype(np.uint32)[keep])
    want_valid = np.ones(T, np.uint32)
    want_valid[1] = 0
    np.testing.assert_array_equal(df["nuts_loo_valid"].to_numpy(), want_valid[keep])
    # a taxon whose seven rows are NaN (status 3 on the device): count 0, not valid
    nan = loo.copy()
    nan[0] = np.nan
    d3 = fits.make_df_fit_results(p, out, keep, cfg, loo=nan)
    if keep[0]:
        assert d3["pareto_k_bad"].iloc[0] == 0 and d3["nuts_loo_valid"].iloc[0] == 0
    # a dropped taxon takes its row with it
    k2 = np.array([True, False, True])
    d2 = fits.make_df_fit_results(p, out, k2, cfg, loo=loo)
    np.testing.assert_array_equal(d2["elpd_loo"].to_numpy(), loo[k2, 0, 0])
    np.testing.assert_array_equal(d2["nuts_loo_valid"].to_numpy(), want_valid[k2])


def test_make_opts_and_cli(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import _lib, fits
    from metadamage_amd.cli import cli_app

    kw = dict(num_warmup=30, num_samples=50)
    o = fits.make_opts(_cfg(tmp_path, "nuts-loo"), kw)
    m = fits.make_opts(_cfg(tmp_path, "nuts"), kw)
    assert o.mode == _lib.MODE_NUTS and bytes(o) == bytes(m) and o.num_samples == 50
    assert fits.mode_of("nuts-loo") == fits.mode_of("nuts-summary") == fits.mode_of("nuts") == _lib.MODE_NUTS
    assert fits.wants_loo(_cfg(tmp_path, "nuts-loo"))
    for other in ("nuts", "nuts-diag", "nuts-summary", "map", "map-laplace"):
        assert not fits.wants_loo(_cfg(tmp_path, other)), other
    loo_cfg = _cfg(tmp_path, "nuts-loo")
    assert not fits.wants_diag(loo_cfg) and not fits.wants_summary(loo_cfg) and not fits.wants_laplace(loo_cfg)
    with pytest.raises(ValueError, match="nuts-loo"):
        fits.mode_of("nuts-foo")
    bad = CliRunner().invoke(cli_app, ["fit", str(GOLDEN / "data_ancient.txt"), "--out-dir", str(tmp_path),
                                       "--inference", "nuts-foo"])
    assert bad.exit_code == 2
    for name in ("nuts", "map", "map-laplace", "nuts-diag", "nuts-summary", "nuts-loo"):
        assert name in bad.output, name
    helptext = CliRunner().invoke(cli_app, ["fit", "--help"]).output
    assert "nuts-loo" in helptext and "nuts-summary" in helptext


def test_chunk_planning_counts_the_loo_records():
    from metadamage_amd import _lib, engine

    nuts = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=10, num_samples=100)
    assert engine.LOO_BYTES == 7 * 8 * 4 == 224
    base = engine.device_bytes(128, nuts)
    assert engine.device_bytes(128, nuts, with_loo=True) == base + 128 * (448 + 224)
    base_dev = engine.device_bytes(128, nuts, dest_on_device=True)
    assert engine.device_bytes(128, nuts, dest_on_device=True, with_loo=True) == base_dev + 128 * 448
    # a budget that holds exactly c taxa with the records holds fewer than without
    per = engine.device_bytes(2, nuts, with_loo=True) - engine.device_bytes(1, nuts, with_loo=True)
    budget = engine.N_SETS * (_lib.SAMPLES_OFFSET + 50 * per)
    chunks = engine.plan_chunks(1000, nuts, budget, with_loo=True)
    cap = max(hi - lo for lo, hi in chunks)
    assert cap <= 50 and engine.N_SETS * engine.device_bytes(cap, nuts, with_loo=True) <= budget
    assert engine.N_SETS * engine.device_bytes(51, nuts, with_loo=True) > budget
    assert chunks[0][0] == 0 and chunks[-1][1] == 1000 and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    plain = engine.plan_chunks(1000, nuts, budget)
    assert max(hi - lo for lo, hi in plain) >= cap and len(plain) <= len(chunks)
    # NUTS only
    for opts in (_lib.default_opts(mode=_lib.MODE_MAP), None):
        with pytest.raises(ValueError):
            engine.device_bytes(128, opts, with_loo=True)
        with pytest.raises(ValueError):
            engine.plan_chunks(1000, opts, with_loo=True)
        with pytest.raises(ValueError):
            engine.ChunkedFitter(16, opts=opts, with_loo=True)
    # one optional extra block per run
    for other in ("with_diag", "with_summary"):
        with pytest.raises(ValueError, match="mutually exclusive"):
            engine.device_bytes(128, nuts, with_loo=True, **{other: True})
        with pytest.raises(ValueError, match="mutually exclusive"):
            engine.plan_chunks(1000, nuts, with_loo=True, **{other: True})
        with pytest.raises(ValueError, match="mutually exclusive"):
            engine.ChunkedFitter(16, opts=nuts, with_loo=True, **{other: True})
    with pytest.raises(ValueError):
        engine.ChunkedFitter(16, opts=nuts, with_loo=True, with_laplace=True)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_gather_record_with_loo_round_trips(world):
    import torch

    from metadamage_amd import _lib, distributed as d

    assert d.REC_BYTES == 496 and d.REC_LOO == 224
    T = 29  # uneven shards at every world
    n = d.shard_capacity(T, world)
    rng = np.random.default_rng(2)
    parts, want_loo, want_pred, want_st = [], [], [], []
    for r in range(world):
        lo, hi = d.shard_range(T, r, world)
        buf = torch.from_numpy(rng.integers(0, 256, n * (d.REC_BYTES + d.REC_LOO), dtype=np.uint8))
        pred, status, ints, floats, loo = d.packed_views(buf, n, with_loo=True)
        p0, s0, i0, f0 = d.packed_views(buf[: n * d.REC_BYTES], n)  # the default layout is a prefix
        assert pred.data_ptr() == p0.data_ptr() and status.data_ptr() == s0.data_ptr()
        assert ints.data_ptr() == i0.data_ptr() and floats.data_ptr() == f0.data_ptr()
        assert loo.shape == (n, 7, _lib.NNUTSLOO) and loo.dtype == torch.float32
        assert loo.data_ptr() == buf.data_ptr() + n * d.REC_BYTES
        w = rng.standard_normal((n, 7, 8)).astype(np.float32)
        w[0, 1, 3] = np.inf
        w[0, 2, 0] = np.nan
        wp = rng.standard_normal((n, 3, 30)).astype(np.float32)
        ws = rng.integers(0, 4, n).astype(np.int32)
        loo.copy_(torch.from_numpy(w))
        pred.copy_(torch.from_numpy(wp))
        status.copy_(torch.from_numpy(ws))
        ints.copy_(torch.from_numpy(np.rint(rng.standard_normal((n, 8)) * 100)))
        floats.copy_(torch.from_numpy(rng.standard_normal((n, 17)).astype(np.float32)))
        parts.append(buf)
        want_loo.append(w[: hi - lo])
        want_pred.append(wp[: hi - lo])
        want_st.append(ws[: hi - lo])
    out, pr, ss, lo_ = d.unpack_gathered(parts, T, world, with_loo=True)
    assert out.shape == (T, 25) and lo_.shape == (T, 7, 8) and lo_.dtype == np.float32
    np.testing.assert_array_equal(lo_, np.concatenate(want_loo))
    np.testing.assert_array_equal(pr, np.concatenate(want_pred))
    np.testing.assert_array_equal(ss, np.concatenate(want_st))
    o3 = d.unpack_gathered([b[: n * d.REC_BYTES] for b in parts], T, world)
    assert len(o3) == 3
    np.testing.assert_array_equal(o3[0], out)
    for other in ("with_laplace", "with_diag", "with_summary"):
        with pytest.raises(ValueError):
            d.packed_views(parts[0], n, with_loo=True, **{other: True})
        with pytest.raises(ValueError):
            d.unpack_gathered(parts, T, world, with_loo=True, **{other: True})
        with pytest.raises(ValueError):
            d.alloc_records(4, "cpu", with_loo=True, **{other: True})
