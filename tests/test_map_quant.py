"""CPU tests of the weighted order statistics (MDFIT-QUANT v1):
the layout constants against include/mdfit.h, the host build of
csrc/mdfit_mapquant.h against the Python-integer reference
(tests/map_quant_ref.py) bit for bit on crafted series, the equal-weights
reduction to nuts-summary's rules, and the gather-record / frames / options /
CLI plumbing."""

from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from tests import map_quant_ref as ref
from tests.helpers import GOLDEN

ROOT = Path(__file__).resolve().parents[1]


# --------------------------------------------------------------------------
# layout
# --------------------------------------------------------------------------
def test_layout_constants_match_the_header():
    from metadamage_amd import _lib, distributed as d, engine

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mdfit.h").read_text(), flags=re.S)
    assert re.search(r"#define MDFIT_NMAPQUANT\s+16\b", text) and _lib.NMAPQUANT == 16 == ref.NFIELD
    assert _lib.MAPQUANT_FIELDS == ref.FIELDS and len(_lib.MAPQUANT_FIELDS) == _lib.NMAPQUANT
    assert _lib.MAPQUANT_FIELDS.index("khat") == _lib.MAPPSIS_FIELDS.index("khat") == 12
    assert _lib.MAPQUANT_FIELDS.index("ess") == _lib.MAPPSIS_FIELDS.index("ess") == 13
    assert _lib.MAPQUANT_FIELDS.index("flags") == _lib.MAPPSIS_FIELDS.index("flags") == 15
    assert re.search(r"#define MDFIT_ABI_VERSION\s+3\b", text)  # entries are added, none changes
    for sym in ("mdfit_map_quant", "mdfit_map_quant_adapt", "mdfit_weighted_order_stats"):
        assert re.search(rf"\bint\s+{sym}\s*\(", text) and sym in _lib.EXPORTED_SYMBOLS
    assert _lib.NQUANTOUT == 48 and d.REC_QUANT == 192 == engine.QUANT_BYTES and _lib.NQUANTRES == ref.NRES
    lib = _lib.load()
    for fn, n in ((lib.mdfit_map_quant, 12), (lib.mdfit_map_quant_adapt, 14), (lib.mdfit_weighted_order_stats, 7)):
        assert len(fn.argtypes) == n
    # the argument checks need no device
    assert lib.mdfit_map_quant(None, None, None, None, -1, 256, 0, 0, 0.01, None, None, None) == -1
    assert b"n_taxa" in lib.mdfit_last_error()
    for S in (24, 1025):
        assert lib.mdfit_map_quant(None, None, None, None, 0, S, 0, 0, 0.01, None, None, None) == -1
        assert b"num_draws must be in [25, 1024]" in lib.mdfit_last_error()
        assert lib.mdfit_weighted_order_stats(None, None, 0, S, 0.01, None, None) == -1
        assert b"S must be in [25, 1024]" in lib.mdfit_last_error()
    for d0 in (-1e-9, 1.0000001, float("nan"), float("inf"), float("-inf")):
        assert lib.mdfit_map_quant(None, None, None, None, 0, 256, 0, 0, d0, None, None, None) == -1
        assert b"d0 must be in [0, 1]" in lib.mdfit_last_error()
        assert lib.mdfit_map_quant_adapt(None, None, None, None, 0, 256, 0, 0, 0, d0, None, None, None, None) == -1
        assert lib.mdfit_weighted_order_stats(None, None, 0, 256, d0, None, None) == -1
    for R in (-1, 5):
        assert lib.mdfit_map_quant_adapt(None, None, None, None, 0, 256, R, 0, 0, 0.01, None, None, None, None) == -1
        assert b"adapt_rounds" in lib.mdfit_last_error()
    for d0 in (0.0, 1.0):
        assert lib.mdfit_map_quant(None, None, None, None, 0, 256, 0, 0, d0, None, None, None) == 0
    assert lib.mdfit_map_quant(None, None, None, None, 1, 256, 0, 0, 0.01, None, None, None) == -1
    assert b"null" in lib.mdfit_last_error()
    assert lib.mdfit_weighted_order_stats(None, None, 1, 256, 0.01, None, None) == -1
    assert b"null" in lib.mdfit_last_error()


# --------------------------------------------------------------------------
# the reference itself: with equal weights the rules are nuts-summary's
# --------------------------------------------------------------------------
@pytest.mark.parametrize("S", list(range(25, 130)) + [200, 255, 256, 257, 500, 512, 1000, 1023, 1024])
def test_equal_weights_reduce_to_the_sample_rules(S):
    rng = np.random.default_rng([5, S])
    v = rng.uniform(0.0, 0.3, S)
    got = ref.order_stats(v, np.full(S, 1.0 / S), 0.1)
    sv = np.sort(v)
    assert got[ref.OK] == 1.0
    assert got[ref.MEDIAN] == np.median(v)
    n = int(0.68 * S) + 1  # numpyro's hpdi: the narrowest window of int(0.68 S) + 1 sorted draws, the first of equals
    i = int(np.argmin(sv[n - 1:] - sv[: S - n + 1]))
    assert (got[ref.LO], got[ref.HI], got[ref.N_WINDOW]) == (sv[i], sv[i + n - 1], n)
    assert abs(got[ref.P_ABOVE] - (v > 0.1).mean()) < 1e-15  # (m k / (S k) in doubles)
    assert got[ref.Q05] == sv[-(-5 * S // 100) - 1] and got[ref.Q95] == sv[-(-95 * S // 100) - 1]


def test_reference_on_handmade_series():
    S = 25
    v = np.arange(S, dtype=np.float64) / 100.0
    w = np.full(S, 0.1 / (S - 1))
    w[7] = 0.9
    got = ref.order_stats(v, w, 0.07)
    assert got[ref.MEDIAN] == got[ref.LO] == got[ref.HI] == 0.07 and got[ref.N_WINDOW] == 1
    assert got[ref.P_ABOVE] < 0.1  # the comparison is strict: the 0.9 at d0 itself is not above
    assert ref.order_stats(v, w, 0.069)[ref.P_ABOVE] > 0.9
    # half the mass on each of two draws: the median is their mean
    w2 = np.zeros(S)
    w2[[3, 20]] = 0.5
    got = ref.order_stats(v, w2, 0.1)
    assert got[ref.MEDIAN] == 0.5 * (0.03 + 0.20) and (got[ref.LO], got[ref.HI]) == (0.03, 0.20)
    assert got[ref.N_WINDOW] == 2 and got[ref.Q05] == 0.03 and got[ref.Q95] == 0.20 and got[ref.P_ABOVE] == 0.5
    # a draw without mass is never selected, whatever it holds
    v3 = v.copy()
    v3[[0, 24]] = [-np.inf, np.nan]
    w3 = np.full(S, 1.0 / (S - 2))
    w3[[0, 24]] = 0.0
    got = ref.order_stats(v3, w3, 0.1)
    assert got[ref.OK] == 1.0 and got[ref.Q05] >= 0.01 and got[ref.Q95] <= 0.23 and got[ref.MEDIAN] == 0.12
    assert ref.order_stats(v, np.zeros(S), 0.1)[ref.OK] == 0.0
    w4 = w3.copy()
    w4[24] = 1e-3  # the NaN draw has mass
    assert ref.order_stats(v3, w4, 0.1)[ref.OK] == 0.0 and np.isnan(ref.order_stats(v3, w4, 0.1)[:7]).all()


# --------------------------------------------------------------------------
# the host build of csrc/mdfit_mapquant.h
# --------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(tmp_path_factory, request):
    exe = tmp_path_factory.mktemp("mapquant_host") / f"mapquant_host_{request.param}"
    flags = ["-O1", "-g"] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                             if request.param == "sanitized" else [])
    subprocess.run(["g++", "-std=c++17", *flags, str(ROOT / "tests" / "mapquant_host_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def _hex(x) -> str:
    x = float(x)
    if x != x:
        return "nan"
    return ("inf" if x > 0 else "-inf") if np.isinf(x) else x.hex()


def run_host(exe, items, tmp_path):
    """res[n, 8] of the host program on items (v, w, d0)."""
    lines = [str(len(items))]
    for v, w, d0 in items:
        lines += [f"{len(v)} {_hex(d0)}", " ".join(_hex(x) for x in v), " ".join(_hex(x) for x in w)]
    src = tmp_path / "series.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = [[np.nan if "nan" in t else float.fromhex(t) for t in ln.split()] for ln in r.stdout.strip().splitlines()]
    assert len(got) == len(items)
    return np.array(got)


@pytest.mark.parametrize("S", ref.S_VALUES)
def test_host_program_equals_reference_bitwise(host_program, tmp_path, S):
    v, w, d0, kinds, want = ref.case(S)
    got = run_host(host_program, list(zip(v, w, d0)), tmp_path)
    for kind, g, e in zip(kinds, got, want):
        assert np.array_equal(ref.bits(g), ref.bits(e)), (kind, S, g, e)
    ok = dict(zip(kinds, want[:, ref.OK]))
    assert ok["all_zero"] == ok["nan_with_mass"] == ok["bad_weight"] == 0.0
    assert all(ok[k] == 1.0 for k in kinds if k not in ("all_zero", "nan_with_mass", "bad_weight"))
    p = want[kinds.index("point09")]
    assert p[ref.MEDIAN] == p[ref.LO] == p[ref.HI] and p[ref.N_WINDOW] == 1
    e = want[kinds.index("equal")]
    assert e[ref.MEDIAN] == np.median(v[kinds.index("equal")]) and e[ref.N_WINDOW] == int(0.68 * S) + 1
    t = want[kinds.index("two_points")]
    assert (t[ref.LO], t[ref.HI]) == (0.02, 0.29)  # no window of 68 % without both masses


# --------------------------------------------------------------------------
# the gather record
# --------------------------------------------------------------------------
def test_gather_record_carries_the_quant_tail():
    import torch

    from metadamage_amd import distributed as d

    n = 7
    today = d.alloc_records(n, "cpu", with_psis=True, with_adapt=True)
    assert today.quant is None and today.buf.numel() == n * (d.REC_BYTES + d.REC_PSIS + 8)
    rec = d.alloc_records(n, "cpu", with_psis=True, with_quant=True, with_adapt=True)
    assert rec.buf.numel() == today.buf.numel() + n * 192
    assert rec.quant.shape == (n, 48) and rec.quant.dtype == torch.float32 and rec.ppc is None
    p0 = rec.buf.data_ptr()
    assert rec.psis.data_ptr() == p0 + n * d.REC_BYTES
    assert rec.quant.data_ptr() == p0 + n * (d.REC_BYTES + d.REC_PSIS)  # directly behind the psis block ...
    assert rec.adapt.data_ptr() == p0 + n * (d.REC_BYTES + d.REC_PSIS + 192)  # ... and before the adapt tail
    only = d.alloc_records(n, "cpu", with_psis=True, with_quant=True)
    assert only.adapt is None and only.buf.numel() == n * (d.REC_BYTES + d.REC_PSIS + 192)
    for kw in ({}, *({b.switch: True} for b in d.blocks.BLOCKS if b.name != "psis")):
        with pytest.raises(ValueError, match="with_quant goes with with_psis"):
            d.alloc_records(n, "cpu", with_quant=True, **kw)
    rng = np.random.default_rng(11)
    for with_adapt in (True, False):
        r = d.alloc_records(n, "cpu", with_psis=True, with_quant=True, with_adapt=with_adapt)
        r.buf.copy_(torch.from_numpy(rng.integers(0, 256, r.buf.numel(), dtype=np.uint8)))
        r.floats.zero_()  # (random bytes there can be signalling NaN, which numpy's f32 -> f64 cast warns about)
        want_ps = rng.standard_normal((n, *r.psis.shape[1:])).astype(np.float32)
        want_q = rng.standard_normal((n, 48)).astype(np.float32)
        want_q[2] = np.nan
        want_ad = rng.standard_normal((n, 2)).astype(np.float32)
        r.psis.copy_(torch.from_numpy(want_ps))
        r.quant.copy_(torch.from_numpy(want_q))
        if with_adapt:
            r.adapt.copy_(torch.from_numpy(want_ad))
        got = d.unpack_gathered([r.buf, r.buf.clone()], 13, 2, with_psis=True, with_quant=True, with_adapt=with_adapt)
        assert len(got) == (6 if with_adapt else 5)
        np.testing.assert_array_equal(got[3], np.concatenate([want_ps, want_ps[:6]]))
        np.testing.assert_array_equal(got[4], np.concatenate([want_q, want_q[:6]]))
        if with_adapt:
            np.testing.assert_array_equal(got[5], np.concatenate([want_ad, want_ad[:6]]))


def test_plan_counts_the_order_statistics():
    from metadamage_amd import _lib, engine

    opts = _lib.default_opts(mode=_lib.MODE_MAP)
    a = engine.device_bytes(100, opts, with_psis=True)
    assert engine.device_bytes(100, opts, with_psis=True, quantiles=True) - a == 100 * (48 * 8 + 192)
    assert engine.device_bytes(100, opts, with_psis=True, quantiles=True, dest_on_device=True) \
        - engine.device_bytes(100, opts, with_psis=True, dest_on_device=True) == 100 * 48 * 8
    assert engine.device_bytes(100, opts, with_psis=True, quantiles=False) == a
    budget = 2 * engine.device_bytes(50, opts, with_psis=True)
    assert max(hi - lo for lo, hi in engine.plan_chunks(200, opts, budget, with_psis=True)) == 50
    assert max(hi - lo for lo, hi in engine.plan_chunks(200, opts, budget, with_psis=True, quantiles=True)) < 50
    for kw in ({}, {"with_ppred": True}, {"with_waic": True}, {"with_laplace": True}):
        with pytest.raises(ValueError, match="quantiles needs with_psis"):
            engine.device_bytes(10, opts, quantiles=True, **kw)
        with pytest.raises(ValueError, match="quantiles needs with_psis"):
            engine.plan_chunks(10, opts, quantiles=True, **kw)
    for d0 in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="dmax_threshold must be in"):
            engine.plan_chunks(10, opts, with_psis=True, quantiles=True, dmax_threshold=d0)


# --------------------------------------------------------------------------
# options, cache key, CLI
# --------------------------------------------------------------------------
def _cfg(tmp_path, inference="map-psis", **kw):
    from metadamage_amd import utils

    cfg = utils.Config(out_dir=tmp_path, max_fits=10, max_cores=1, min_alignments=10, min_y_sum=10,
                       substitution_bases_forward="CT", substitution_bases_reverse="GA", forced=False,
                       version="0.0.0", inference=inference, **kw)
    cfg.add_filename(GOLDEN / "data_ancient.txt")
    return cfg


def test_config_metadata_cache_key_and_cli(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import fits, utils
    from metadamage_amd.cli import cli_app

    fields = utils.Config.__dataclass_fields__
    assert fields["quantiles"].default is False and fields["dmax_threshold"].default == 0.01
    for inference in ("map-psis", "auto", "map", "nuts", "map-pred"):
        d0 = _cfg(tmp_path, inference).to_dict()
        assert "quantiles" not in d0 and "dmax_threshold" not in d0 and not fits.quantiles_of(_cfg(tmp_path, inference))
        # the metadata of a run without it: today's, whatever the threshold holds
        assert _cfg(tmp_path, inference, quantiles=False, dmax_threshold=0.05).to_dict() == d0
    d0 = _cfg(tmp_path).to_dict()
    d1 = _cfg(tmp_path, quantiles=True).to_dict()
    d2 = _cfg(tmp_path, quantiles=True, dmax_threshold=0.05).to_dict()
    assert d1["quantiles"] is True and d1["dmax_threshold"] == 0.01 and d2["dmax_threshold"] == 0.05
    assert fits.quantiles_of(_cfg(tmp_path, quantiles=True))
    assert fits.dmax_threshold_of(_cfg(tmp_path, quantiles=True, dmax_threshold=0.05)) == 0.05
    assert {k: v for k, v in d1.items() if k not in ("quantiles", "dmax_threshold")} == d0
    assert "quantiles" in fits.CACHE_KEYS and "dmax_threshold" in fits.CACHE_KEYS
    sim = utils.metadata_is_similar
    assert sim(d0, dict(d0), include=fits.CACHE_KEYS) and sim(d1, dict(d1), include=fits.CACHE_KEYS)
    assert not sim(d0, d1, include=fits.CACHE_KEYS) and not sim(d1, d0, include=fits.CACHE_KEYS)
    assert not sim(d1, d2, include=fits.CACHE_KEYS)
    for inference in ("map", "nuts", "auto", "map-pred", "map-waic", "map-evidence", "nuts-summary"):
        with pytest.raises(ValueError, match="quantiles goes with inference 'map-psis'"):
            _cfg(tmp_path, inference, quantiles=True)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="dmax_threshold must be in"):
            _cfg(tmp_path, quantiles=True, dmax_threshold=bad)
    runner = CliRunner()
    base = ["fit", str(GOLDEN / "data_ancient.txt"), "--out-dir", str(tmp_path)]
    for inference in ("map", "nuts", "auto", "map-pred", "map-waic"):
        bad = runner.invoke(cli_app, base + ["--inference", inference, "--quantiles"])
        assert bad.exit_code == 2 and "--quantiles" in bad.output, inference
    for val in ("-0.5", "1.5"):
        bad = runner.invoke(cli_app, base + ["--inference", "map-psis", "--quantiles", "--dmax-threshold", val])
        assert bad.exit_code == 2 and "--dmax-threshold" in bad.output, val
    out = runner.invoke(cli_app, ["fit", "--help"], terminal_width=200).output
    assert "--quantiles" in out and "--dmax-threshold" in out


# --------------------------------------------------------------------------
# frames
# --------------------------------------------------------------------------
def test_frames_from_a_synthetic_tail(tmp_path, oracle_lib, ref_meta):
    from metadamage_amd import _lib, fits

    cfg = _cfg(tmp_path, quantiles=True)
    p = fits.pack_counts(pd.read_parquet(GOLDEN / "counts_data_ancient.parquet"), cfg)
    out, pred, st = oracle_lib.fit_batch(p.y, p.N, p.mm)
    keep = st == 0
    assert keep.all() and len(keep) == 3
    f = _lib.MAPQUANT_FIELDS.index
    quant = np.arange(3 * 48, dtype=np.float32).reshape(3, 3, 16) / 256.0
    quant[:, :, f("n_window")] = [[170, 180, 175], [12, 1, 30], [np.nan, 40, 50]]
    quant[:, :, f("flags")] = [[63, 63, 63], [61, 63 | 64, 61], [60, 63, 63]]
    quant[2, 0, :15] = np.nan
    psis = np.zeros((3, 3, 16), np.float32)
    adapt = np.array([[0.71, 2.0], [0.2, 0.0], [np.nan, np.nan]], dtype=np.float32)
    base = ref_meta["fit_results_columns"]
    today = fits.make_df_fit_results(p, out, keep, cfg, psis=psis)
    df = fits.make_df_fit_results(p, out, keep, cfg, psis=psis, quant=quant.reshape(3, 48))
    assert fits.MAP_QUANT_COLUMNS == [
        "D_max_posterior_median", "D_max_posterior_lower_hpdi", "D_max_posterior_upper_hpdi", "q_median",
        "q_lower_hpdi", "q_upper_hpdi", "concentration_median", "A_median", "c_median", "D_max_posterior_q05",
        "D_max_posterior_q95", "D_max_prob_above", "D_max_posterior_median_forward", "D_max_posterior_median_reverse"]
    assert fits.MAP_QUANT_COLUMNS[:7] == fits.NUTS_SUMMARY_COLUMNS[-7:]  # nuts-summary's names, in its order
    assert fits.MAP_QUANT_UINT_COLUMNS == ["quant_window_min", "map_quant_valid"]
    assert list(df.columns) == (base + fits.MAP_PSIS_COLUMNS + fits.MAP_PSIS_UINT_COLUMNS + fits.MAP_QUANT_COLUMNS
                                + fits.MAP_QUANT_UINT_COLUMNS)
    pd.testing.assert_frame_equal(df[today.columns], today)  # no column is renamed or moved
    for c in fits.MAP_QUANT_COLUMNS:
        assert df[c].dtype == np.float32, c
    for c in fits.MAP_QUANT_UINT_COLUMNS:
        assert df[c].dtype == np.uint32, c
    np.testing.assert_array_equal(df["D_max_posterior_median"].to_numpy(), quant[:, 0, 0])
    np.testing.assert_array_equal(df["D_max_posterior_upper_hpdi"].to_numpy(), quant[:, 0, 2])
    np.testing.assert_array_equal(df["q_lower_hpdi"].to_numpy(), quant[:, 0, 7])
    np.testing.assert_array_equal(df["concentration_median"].to_numpy(), quant[:, 0, 11])
    np.testing.assert_array_equal(df["A_median"].to_numpy(), quant[:, 0, 9])
    np.testing.assert_array_equal(df["D_max_prob_above"].to_numpy(), quant[:, 0, 5])
    np.testing.assert_array_equal(df["D_max_posterior_median_forward"].to_numpy(), quant[:, 1, 0])
    np.testing.assert_array_equal(df["D_max_posterior_median_reverse"].to_numpy(), quant[:, 2, 0])
    assert df["quant_window_min"].tolist() == [170, 1, 0] and df["map_quant_valid"].tolist() == [1, 1, 0]
    both = fits.make_df_fit_results(p, out, keep, cfg, psis=psis, quant=quant.reshape(3, 48), adapt=adapt)
    assert list(both.columns) == list(df.columns) + fits.ADAPT_COLUMNS  # the adapt columns stay last
    d2 = fits.make_df_fit_results(p, out, np.array([True, False, True]), cfg, psis=psis, quant=quant.reshape(3, 48))
    assert d2["quant_window_min"].tolist() == [170, 0] and d2["map_quant_valid"].tolist() == [1, 0]
    # a run without the option: the frame and the cache key are today's
    plain = _cfg(tmp_path)
    assert list(fits.make_df_fit_results(p, out, keep, plain, psis=psis).columns) == list(today.columns)
    assert "quantiles" not in plain.to_dict() and not fits.quantiles_of(plain)
    # the optional arrays behind (out, pred, status): adapt stays last once the quant block is taken out
    x, a = object(), object()
    assert fits._split_rest(_cfg(tmp_path, quantiles=True, psis_adapt=2), [x, a]) == (x, None, a)
