"""CPU tests of the importance-weighted WAIC of the MAP fit (MDFIT-WAIC v1,
DESIGN.md §3.9): the C-ABI entry point without a device, the host build of the
pointwise accumulation and the row record (csrc/mdfit_mapwaic.h, one-lane
policy) against the reference (tests/map_waic_ref.py) on crafted series, the
reference against the oracle's NUTS comparisons, and the frames / options / CLI
/ gather-record / chunk-planning plumbing."""

from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from tests import map_psis_ref as pref
from tests import map_waic_cases as cases
from tests import map_waic_ref as ref
from tests.helpers import GOLDEN

ROOT = Path(__file__).resolve().parents[1]

# the host program against the reference over every series of map_waic_cases
# (24 series per S), the worst over the six S (each at S = 1024): lppd_i
# absolute over max(1, |lppd_i|) 1.48e-15, p_i relative 2.73e-14, a record field
# (elpd_waic, p_waic, lppd, ess) relative 4.75e-15 (at S = 100); times ten
HOST_TOL = {"lppd": 1.48e-14, "p": 2.73e-13, "rec": 4.75e-14}


# --------------------------------------------------------------------------
# ABI
# --------------------------------------------------------------------------
def test_entry_point_declared_exported_and_argument_checked():
    from metadamage_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mdfit.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+mdfit_map_waic\s*\(", text)
    assert f"#define MDFIT_NMAPWAIC {_lib.NMAPWAIC}" in text
    assert f"#define MDFIT_ABI_VERSION {_lib.ABI_VERSION}" in text and _lib.ABI_VERSION == 3
    assert "mdfit_map_waic" in _lib.EXPORTED_SYMBOLS
    assert len(_lib.MAPWAIC_FIELDS) == len(_lib.MAPWAIC_COMPARE_FIELDS) == _lib.NMAPWAIC == 8
    assert _lib.MAPWAIC_FIELDS == ref.FIELDS and _lib.MAPWAIC_COMPARE_FIELDS == ref.COMPARE_FIELDS
    assert _lib.NWAICROW == 7
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                        check=True).stdout
    assert re.search(r"\bT mdfit_map_waic\b", nm)
    dummy = ctypes.c_void_p(16)
    assert lib.mdfit_map_waic(None, None, None, None, 0, 256, 0, 0, None, None, None, None) == 0
    assert lib.mdfit_map_waic(None, None, None, None, -1, 256, 0, 0, None, None, None, None) == -1
    assert b"n_taxa" in lib.mdfit_last_error()
    for S in (24, 1025):
        assert lib.mdfit_map_waic(dummy, dummy, dummy, dummy, 1, S, 0, 0, dummy, None, None, None) == -1
        assert b"num_draws" in lib.mdfit_last_error()
    assert lib.mdfit_map_waic(dummy, dummy, dummy, dummy, 1, 256, 0, 0, None, None, None, None) == -1  # waic is required
    assert b"null" in lib.mdfit_last_error()
    assert lib.mdfit_map_waic(dummy, dummy, dummy, dummy, (1 << 25) + 1, 256, 0, 0, dummy, None, None, None) == -1
    assert b"2^25" in lib.mdfit_last_error()


# --------------------------------------------------------------------------
# the host build of csrc/mdfit_mapwaic.h
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mapwaic_host") / "mapwaic_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", str(ROOT / "tests" / "mapwaic_host_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def _hex(v):
    return float(v).hex() if np.isfinite(v) else ("nan" if np.isnan(v) else ("inf" if v > 0 else "-inf"))


def _run_host(exe, items, tmp_path):
    """items: (S, n, khat, w, l, l0) -> per item (lppd[n], p[n], rec[8])."""
    lines = [str(len(items))]
    for S, n, khat, w, l, l0 in items:
        lines += [f"{S} {n} {_hex(khat)}", " ".join(_hex(v) for v in w), " ".join(_hex(v) for v in l.ravel()),
                  " ".join(_hex(v) for v in l0)]
    src = tmp_path / "series.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    out = []
    for (S, n, *_), ln in zip(items, r.stdout.strip().splitlines()):
        v = np.array([float.fromhex(tok) if "nan" not in tok else np.nan for tok in ln.split()])
        out.append((v[:n], v[n:2 * n], v[2 * n:]))
    return out


@pytest.mark.parametrize("S", cases.S_VALUES)
def test_host_program_vs_reference(host_program, tmp_path, S):
    allc = cases.all_series(S)
    got = _run_host(host_program, [(S, l.shape[1], khat, w, l, l0) for _, _, w, l, l0, khat in allc], tmp_path)
    worst = {"lppd": 0.0, "p": 0.0, "rec": 0.0}
    tau = pref.khat_threshold(S)
    for (kind, seed, w, l, l0, khat), (lppd, p, rec) in zip(allc, got):
        n = l.shape[1]
        assert n == (15 if kind.endswith("15") else 30)
        want_l, want_p = cases.reference(w, l)
        assert np.isfinite(lppd).all() and np.isfinite(p).all() and (p >= 0).all(), kind
        e = cases.errors(lppd, p, want_l, want_p)
        for k, v in e.items():
            worst[k] = max(worst[k], v)
        zero = np.asarray(want_p) == 0
        assert (p[zero] == 0.0).all(), kind  # a column that is the same in every draw: exactly
        if kind == "const":
            assert zero[3] and zero[11] and lppd[3] == -7.25 and lppd[11] == 0.0 and p[3] == 0.0 and p[11] == 0.0
        if kind == "one":  # the draw that holds all the weight: its values, no spread
            assert zero.all() and np.array_equal(lppd, l[int(np.argmax(w))])
        if kind.startswith("deep"):
            assert lppd[2] < -800.0 and abs(lppd[7] + 5000.0) < 2.0 and p[7] > 0.0
        want = ref.row_record(want_l, want_p, w, np.longdouble(khat), int((w == 0).sum()), S, 15)
        assert int(rec[ref.FLAGS]) == int(want[ref.FLAGS]) == (1 | (2 if khat <= tau else 0) | 60), (kind, rec)
        assert rec[ref.KHAT] == khat and rec[ref.N_INF] == (w == 0).sum()
        assert rec[ref.PMAX] == p.max()
        for j in (ref.ELPD, ref.PWAIC, ref.LPPD, ref.ESS):
            if want[j] == 0:
                assert rec[j] == 0.0, (kind, j)
            else:
                worst["rec"] = max(worst["rec"], float(abs(rec[j] - want[j]) / abs(want[j])))
    print(f"S={S}: worst error " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= HOST_TOL[name], (name, v)


# --------------------------------------------------------------------------
# the method means something: against the oracle's NUTS comparisons
# --------------------------------------------------------------------------
def _taxa_26():
    """Of generate(400, seed=21): the first 10 ancient taxa with mean N > 3e3,
    the first 8 ancient taxa below that, the first 8 non-ancient taxa."""
    from metadamage_amd.synthetic import generate

    b = generate(400, seed=21)
    anc = b.truth["ancient"]
    deep = b.N[:, :30].mean(axis=1) > 3e3
    taxa = np.concatenate([np.flatnonzero(anc & deep)[:10], np.flatnonzero(anc & ~deep)[:8],
                           np.flatnonzero(~anc)[:8]])
    assert taxa.size == 26
    return b, taxa


def test_reference_vs_nuts_comparisons(oracle_lib):
    """The reference at S = 256 on the Philox stream of seed 0 against two 500 +
    1000 oracle NUTS runs (seeds 0 and 1; "NUTS" below is their mean) and the
    oracle's MAP record, on the 26 taxa of _taxa_26.  Measured: 24 taxa with all
    six rows valid (taxa 10 and 4 have a null-forward / null-reverse delta held
    on its lower bound), 15 of them with all six khat at or below the threshold
    0.585.  Over the 24: median |n_sigma_waic - NUTS| 0.129 (max 0.326) against
    median |MAP - NUTS| 0.639 (max 1.55); the two seeds differ by median 0.079,
    max 0.567.  asymmetry: median |IS - NUTS| 0.248 against MAP's 2.37, and MAP
    has the wrong sign on 21 of the 24.  Over the 15 reliable taxa: n_sigma_waic
    - NUTS in [-0.326, +0.241], asymmetry_waic - NUTS in [-0.759, +0.868] (median
    |.| 0.130), the sign of asymmetry_waic NUTS's on all 15; the seeds differ by
    up to 0.567 (n_sigma) and 0.699 (asymmetry) there.  The one taxon 2.7 off in
    asymmetry (taxon 9) has khat 17 in a row and is flagged.  The bands asserted
    are the measured ranges widened by the seeds' largest difference."""
    b, taxa = _taxa_26()
    S = 256
    y, N = b.y[taxa], b.N[taxa]
    out, _, st = oracle_lib.fit_batch(y, N)
    assert (st == 0).all()
    nuts = []
    for seed in (0, 1):
        no, _, ns = oracle_lib.nuts_batch(y, N, seed=seed, num_warmup=500, num_samples=1000)
        assert (ns == 0).all()
        nuts.append(no)
    rec = np.stack([ref.waic_taxon(oracle_lib, y[i, :30], N[i, :30], out[i], 0, S, seed=0, g=int(t))["rec"]
                    for i, t in enumerate(taxa)]).astype(float)
    flags = rec[:, 6, ref.FLAGS].astype(int)
    valid, reliable = (flags & ref.VALID) != 0, (flags & ref.RELIABLE) != 0
    F_NS, F_ASY = 1, 21  # n_sigma, asymmetry among the result columns
    print("taxon valid rel khat_max | n_sigma: MAP IS NUTS0 NUTS1 | asymmetry: MAP IS NUTS0 NUTS1")
    for i, t in enumerate(taxa):
        print(f"{t:4d} {int(valid[i])} {int(reliable[i])} {rec[i, 6, 4]:6.2f} | {out[i, F_NS]:6.2f} {rec[i, 6, 0]:6.2f} "
              f"{nuts[0][i, F_NS]:6.2f} {nuts[1][i, F_NS]:6.2f} | {out[i, F_ASY]:6.2f} {rec[i, 6, 3]:6.2f} "
              f"{nuts[0][i, F_ASY]:6.2f} {nuts[1][i, F_ASY]:6.2f}")
    assert valid.sum() == 24 and reliable.sum() >= 14, (valid.sum(), reliable.sum())
    assert not (reliable & ~valid).any()
    res = {}
    for name, f, c, lo, hi in (("n_sigma", F_NS, 0, -0.326, 0.241), ("asymmetry", F_ASY, 3, -0.759, 0.868)):
        n0, n1 = nuts[0][:, f], nuts[1][:, f]
        nm = 0.5 * (n0 + n1)
        d_is, d_map = rec[:, 6, c] - nm, out[:, f] - nm
        res[name] = (np.median(np.abs(d_is[valid])), np.median(np.abs(d_map[valid])))
        widen = np.abs(n0 - n1)[reliable].max()
        print(f"{name}: median |IS - NUTS| {res[name][0]:.3f}, |MAP - NUTS| {res[name][1]:.3f} over the valid; reliable: "
              f"IS - NUTS in [{d_is[reliable].min():+.3f}, {d_is[reliable].max():+.3f}], seeds differ by <= {widen:.3f}")
        assert (d_is[reliable] >= lo - widen).all() and (d_is[reliable] <= hi + widen).all(), (name, d_is[reliable])
        if name == "asymmetry":
            agree = reliable & (np.sign(n0) == np.sign(n1))
            assert agree.sum() >= 14
            assert (np.sign(rec[agree, 6, c]) == np.sign(n0[agree])).all()
    assert res["n_sigma"][0] < 0.5 * res["n_sigma"][1], res
    assert res["asymmetry"][0] < 0.5 * res["asymmetry"][1], res
    # what invalidates a taxon here: a null row whose delta is held on its lower bound
    for i in np.flatnonzero(~valid):
        bad = [s for s in range(6) if not int(rec[i, s, ref.FLAGS]) & ref.VALID]
        assert bad and all(s in (4, 5) for s in bad), (taxa[i], bad)
        for s in bad:
            assert (int(rec[i, s, ref.FLAGS]) >> 2) & 8 == 0 and np.isnan(rec[i, s, :7]).all()
            assert np.isnan(rec[i, 6, 1 if s == 4 else 2])
        assert np.isfinite(rec[i, 6, 0]) and np.isfinite(rec[i, 6, 3])


# --------------------------------------------------------------------------
# frames, options, CLI, gather record, chunk planning
# --------------------------------------------------------------------------
def _cfg(tmp_path, inference="map-waic", **kw):
    from metadamage_amd import utils

    cfg = utils.Config(out_dir=tmp_path, max_fits=10, max_cores=1, min_alignments=10, min_y_sum=10,
                       substitution_bases_forward="CT", substitution_bases_reverse="GA", forced=False,
                       version="0.0.0", inference=inference, **kw)
    cfg.add_filename(GOLDEN / "data_ancient.txt")
    return cfg


NEW_COLUMNS = ["n_sigma_waic", "n_sigma_waic_forward", "n_sigma_waic_reverse", "asymmetry_waic", "p_waic",
               "p_waic_null", "elpd_waic", "elpd_waic_null", "pareto_k_waic", "waic_ess_min",
               "map_waic_valid", "map_waic_reliable"]


def test_frame_columns_and_dtypes(tmp_path, oracle_lib, ref_meta):
    from metadamage_amd import fits

    cfg = _cfg(tmp_path)
    p = fits.pack_counts(pd.read_parquet(GOLDEN / "counts_data_ancient.parquet"), cfg)
    out, pred, st = oracle_lib.fit_batch(p.y, p.N, p.mm)
    S = 64
    waic = np.stack([ref.waic_taxon(oracle_lib, p.y[t, :30], p.N[t, :30], out[t], int(st[t]), S, seed=0, g=t)["rec"]
                     for t in range(len(st))]).astype(np.float64)
    assert ((waic[:, 6, ref.FLAGS].astype(int) & 1) != 0).all()
    waic[1, 6, ref.FLAGS] = 1.0  # one taxon over the threshold
    waic32 = waic.astype(np.float32)
    keep = st == 0
    plain = fits.make_df_fit_results(p, out, keep, cfg)
    assert len(plain.columns) == 30
    df = fits.make_df_fit_results(p, out, keep, cfg, waic=waic32)
    assert list(df.columns) == ref_meta["fit_results_columns"] + NEW_COLUMNS and len(df.columns) == 42
    assert NEW_COLUMNS == fits.MAP_WAIC_COLUMNS + fits.MAP_WAIC_UINT_COLUMNS
    pd.testing.assert_frame_equal(df[plain.columns], plain)
    for c in NEW_COLUMNS[:-2]:
        assert df[c].dtype == np.float32, c
    assert df["map_waic_valid"].dtype == np.uint32 and df["map_waic_reliable"].dtype == np.uint32
    for name, row, field in (("n_sigma_waic", 6, 0), ("n_sigma_waic_forward", 6, 1), ("n_sigma_waic_reverse", 6, 2),
                             ("asymmetry_waic", 6, 3), ("p_waic", 0, ref.PWAIC), ("p_waic_null", 1, ref.PWAIC),
                             ("elpd_waic", 0, ref.ELPD), ("elpd_waic_null", 1, ref.ELPD), ("pareto_k_waic", 6, 4),
                             ("waic_ess_min", 6, 5)):
        np.testing.assert_array_equal(df[name].to_numpy(), waic32[keep, row, field], err_msg=name)
    np.testing.assert_array_equal(df["pareto_k_waic"].to_numpy(), waic32[keep][:, :6, ref.KHAT].max(axis=1))
    np.testing.assert_array_equal(df["waic_ess_min"].to_numpy(), waic32[keep][:, :6, ref.ESS].min(axis=1))
    assert (df["map_waic_valid"] == 1).all() and df["map_waic_reliable"].to_numpy()[1] == 0
    assert np.isfinite(df[NEW_COLUMNS[:-2]].to_numpy()).all()
    k2 = np.array([True, False, True])  # a dropped taxon takes its row with it
    d2 = fits.make_df_fit_results(p, out, k2, cfg, waic=waic32)
    np.testing.assert_array_equal(d2["n_sigma_waic"].to_numpy(), waic32[k2, 6, 0])


def test_make_opts_config_and_cli(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import _lib, fits
    from metadamage_amd.cli import cli_app

    o = fits.make_opts(_cfg(tmp_path, "map-waic"))
    m = fits.make_opts(_cfg(tmp_path, "map"))
    assert o.mode == _lib.MODE_MAP and bytes(o) == bytes(m)
    assert fits.wants_waic(_cfg(tmp_path, "map-waic")) and not fits.wants_waic(_cfg(tmp_path, "map"))
    assert not fits.wants_waic(_cfg(tmp_path, "map-psis")) and not fits.wants_psis(_cfg(tmp_path, "map-waic"))
    assert not fits.wants_laplace(_cfg(tmp_path, "map-waic"))
    assert fits.mode_of("map-waic") == _lib.MODE_MAP
    assert fits.psis_draws_of(_cfg(tmp_path, "map-waic")) == 256
    assert fits.psis_draws_of(_cfg(tmp_path, "map-waic", psis_draws=1000)) == 1000
    # the draws are in the metadata (and the cache key) of a map-psis or map-waic run only
    assert _cfg(tmp_path, "map-waic", psis_draws=100).to_dict()["psis_draws"] == 100
    assert _cfg(tmp_path, "map-psis", psis_draws=100).to_dict()["psis_draws"] == 100
    for other in ("map", "map-laplace", "nuts", "nuts-loo"):
        assert "psis_draws" not in _cfg(tmp_path, other).to_dict(), other
    assert "psis_draws" in fits.CACHE_KEYS and "inference" in fits.CACHE_KEYS
    assert _cfg(tmp_path, "map-waic").to_dict()["inference"] == "map-waic"
    runner = CliRunner()
    base = ["fit", str(GOLDEN / "data_ancient.txt"), "--out-dir", str(tmp_path)]
    bad = runner.invoke(cli_app, base + ["--inference", "map-foo"])
    assert bad.exit_code == 2 and "map-waic" in bad.output
    for n in ("24", "1025"):
        bad = runner.invoke(cli_app, base + ["--inference", "map-waic", "--psis-draws", n])
        assert bad.exit_code == 2 and "psis-draws" in bad.output
    assert "map-waic" in runner.invoke(cli_app, ["fit", "--help"], terminal_width=200).output


def test_gather_record_with_waic_round_trips():
    import torch

    from metadamage_amd import _lib, distributed as d

    assert d.REC_BYTES == 496 and d.REC_WAIC == 224 == 7 * 8 * 4
    n = 7
    rng = np.random.default_rng(2)
    buf = torch.from_numpy(rng.integers(0, 256, n * (d.REC_BYTES + d.REC_WAIC), dtype=np.uint8))
    pred, status, ints, floats, wv = d.packed_views(buf, n, with_waic=True)
    p0, s0, i0, f0 = d.packed_views(buf[: n * d.REC_BYTES], n)  # the default layout is a prefix
    assert pred.data_ptr() == p0.data_ptr() and status.data_ptr() == s0.data_ptr()
    assert ints.data_ptr() == i0.data_ptr() and floats.data_ptr() == f0.data_ptr()
    assert wv.shape == (n, _lib.NWAICROW, _lib.NMAPWAIC) and wv.dtype == torch.float32
    assert wv.data_ptr() == buf.data_ptr() + n * d.REC_BYTES
    want = rng.standard_normal((n, 7, 8)).astype(np.float32)
    want[0, 4, 1] = np.nan
    wv.copy_(torch.from_numpy(want))
    st = rng.integers(0, 4, n).astype(np.int32)
    status.copy_(torch.from_numpy(st))
    ints.copy_(torch.from_numpy(np.rint(rng.standard_normal(tuple(ints.shape)) * 100)))
    floats.copy_(torch.from_numpy(rng.standard_normal(tuple(floats.shape)).astype(np.float32)))
    pred.copy_(torch.from_numpy(rng.standard_normal(tuple(pred.shape)).astype(np.float32)))
    out, pr, ss, got = d.unpack_gathered([buf, buf.clone()], 13, 2, with_waic=True)
    assert out.shape == (13, 25) and got.shape == (13, 7, 8) and got.dtype == np.float32
    np.testing.assert_array_equal(got[:7], want)
    np.testing.assert_array_equal(got[7:], want[:6])
    np.testing.assert_array_equal(ss[7:], st[:6])
    rec = d.alloc_records(5, "cpu", with_waic=True)
    assert rec.waic.shape == (5, 7, 8) and rec.psis is None and rec.buf.numel() == 5 * (d.REC_BYTES + d.REC_WAIC)
    for other in ("with_laplace", "with_diag", "with_summary", "with_loo", "with_psis"):
        with pytest.raises(ValueError, match="mutually exclusive"):
            d.packed_views(buf, n, with_waic=True, **{other: True})
        with pytest.raises(ValueError, match="mutually exclusive"):
            d.alloc_records(3, "cpu", with_waic=True, **{other: True})


def test_chunk_planning_with_waic():
    from metadamage_amd import _lib, engine

    assert engine.WAIC_BYTES == 224
    m = _lib.default_opts(mode=_lib.MODE_MAP)
    base = engine.device_bytes(1000, m)
    assert engine.device_bytes(1000, m, with_waic=True) == base + 1000 * 3 * 224
    assert engine.device_bytes(1000, m, dest_on_device=True, with_waic=True) == \
        engine.device_bytes(1000, m, dest_on_device=True) + 1000 * 2 * 224
    assert engine.device_bytes(10, None, with_waic=True) == engine.device_bytes(10, None) + 10 * 3 * 224
    budget = 2 * engine.device_bytes(400, m, with_waic=True)
    chunks = engine.plan_chunks(1000, m, budget, with_waic=True)
    assert chunks[0][0] == 0 and chunks[-1][1] == 1000 and max(hi - lo for lo, hi in chunks) <= 400
    assert len(chunks) >= len(engine.plan_chunks(1000, m, budget))
    n = _lib.default_opts(mode=_lib.MODE_NUTS)
    with pytest.raises(ValueError, match="MODE_MAP"):
        engine.device_bytes(10, n, with_waic=True)
    with pytest.raises(ValueError, match="MODE_MAP"):
        engine.plan_chunks(10, n, with_waic=True)
    for other in ("with_laplace", "with_psis"):
        with pytest.raises(ValueError, match="mutually exclusive"):
            engine.device_bytes(10, m, with_waic=True, **{other: True})
        with pytest.raises(ValueError, match="mutually exclusive"):
            engine.plan_chunks(10, m, with_waic=True, **{other: True})
