"""CPU tests of the importance-weighted posterior predictive of the MAP fit
(MDFIT-PPRED v1): the C-ABI entry points without a device, the
host build of the resampling and the median / HPDI (csrc/mdfit_mappred.h,
one-lane policy) against the reference (tests/map_pred_ref.py) on crafted
series, the reference against the oracle's post step and against its NUTS
intervals, and the insensitivity of the GPU test's inputs to a last bit."""

from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import oracle as oracle_mod
from tests import map_pred_cases as cases
from tests import map_pred_ref as ref
from tests import map_psis_ref as pref
from tests import nuts_post_cases as post_cases

ROOT = Path(__file__).resolve().parents[1]


# --------------------------------------------------------------------------
# ABI
# --------------------------------------------------------------------------
def test_entry_points_declared_exported_and_argument_checked():
    from metadamage_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mdfit.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+mdfit_map_pred\s*\(", text) and re.search(r"\bint\s+mdfit_resample\s*\(", text)
    assert f"#define MDFIT_NMAPPRED {_lib.NMAPPRED}" in text
    assert f"#define MDFIT_ABI_VERSION {_lib.ABI_VERSION}" in text and _lib.ABI_VERSION == 3
    assert "mdfit_map_pred" in _lib.EXPORTED_SYMBOLS and "mdfit_resample" in _lib.EXPORTED_SYMBOLS
    assert len(_lib.MAPPRED_FIELDS) == _lib.NMAPPRED == 16 and _lib.MAPPRED_FIELDS == ref.FIELDS
    assert _lib.NPREDJOB == ref.NJOB == 32
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                        check=True).stdout
    assert re.search(r"\bT mdfit_map_pred\b", nm) and re.search(r"\bT mdfit_resample\b", nm)
    dummy = ctypes.c_void_p(16)
    none4 = (None, None, None, None)
    assert lib.mdfit_map_pred(*none4, 0, 256, 1000, 0, 0, *none4, None) == 0
    assert lib.mdfit_map_pred(*none4, -1, 256, 1000, 0, 0, *none4, None) == -1
    assert b"n_taxa" in lib.mdfit_last_error()
    d4 = (dummy, dummy, dummy, dummy)
    for S in (24, 1025):
        assert lib.mdfit_map_pred(*d4, 1, S, 1000, 0, 0, dummy, dummy, None, None, None) == -1
        assert b"num_draws" in lib.mdfit_last_error()
    for R in (24, 1025):
        assert lib.mdfit_map_pred(*d4, 1, 256, R, 0, 0, dummy, dummy, None, None, None) == -1
        assert b"num_pred" in lib.mdfit_last_error()
    assert lib.mdfit_map_pred(*d4, 1, 256, 1000, 0, 0, dummy, None, None, None, None) == -1  # rec is required
    assert b"null" in lib.mdfit_last_error()
    assert lib.mdfit_map_pred(*d4, 1, 256, 1000, 0, 0, None, dummy, None, None, None) == -1  # ppred is required
    assert b"null" in lib.mdfit_last_error()
    assert lib.mdfit_map_pred(*d4, (1 << 25) + 1, 256, 1000, 0, 0, dummy, dummy, None, None, None) == -1
    assert b"2^25" in lib.mdfit_last_error()
    assert lib.mdfit_resample(None, 0, 256, 1000, None, None, None) == 0
    for S, R in ((24, 100), (1025, 100), (100, 24), (100, 1025)):
        assert lib.mdfit_resample(dummy, 1, S, R, dummy, dummy, None) == -1
    assert lib.mdfit_resample(dummy, 1, 256, 1000, None, dummy, None) == -1


# --------------------------------------------------------------------------
# the host build of csrc/mdfit_mappred.h
# --------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(tmp_path_factory, request):
    exe = tmp_path_factory.mktemp("mappred_host") / f"mappred_host_{request.param}"
    flags = ["-O1", "-g"] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                             if request.param == "sanitized" else [])
    subprocess.run(["g++", "-std=c++17", *flags, str(ROOT / "tests" / "mappred_host_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def _run_host(exe, lines, tmp_path):
    src = tmp_path / "items.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stdout.strip().splitlines()


def test_host_resampling_equals_reference(host_program, tmp_path):
    items = cases.all_weight_series()
    assert {S for S, *_ in items} == set(cases.S_VALUES) and set(cases.R_VALUES) <= {R for _, R, *_ in items}
    lines = [str(len(items))]
    for S, R, kind, w in items:
        lines += [f"r {S} {R}", " ".join(float(v).hex() for v in w)]
    got = _run_host(host_program, lines, tmp_path)
    assert len(got) == len(items)
    seen = set()
    for (S, R, kind, w), ln in zip(items, got):
        v = np.array(ln.split(), dtype=np.int64)
        idx, nd = v[:R], int(v[R])
        want, want_nd = ref.resample(w, R)
        assert np.array_equal(idx, want) and nd == want_nd, (S, R, kind)
        assert (w[idx] > 0).all(), (S, R, kind)  # a draw of weight 0 is never taken
        assert idx.min() >= 0 and idx.max() < S and (np.diff(idx) >= 0).all()
        if kind == "equal" and R == S:
            assert np.array_equal(idx, np.arange(S)) and nd == S
            seen.add(("identity", S))
        if kind == "one":
            assert (idx == (7 * S) // 11).all() and nd == 1
        if kind == "on_p":  # a cumulative sum that equals p_r belongs to the draws below it
            c = np.cumsum(w)
            hit = np.isin(2.0 * np.arange(R) + 1.0, c)
            assert hit[0] and idx[0] >= 1 and w[idx[0]] > 0
            seen.add(("on_p", int(hit.sum()) > 1))
    assert {("identity", S) for S in cases.S_VALUES} <= seen and ("on_p", True) in seen


def test_host_median_hpdi_equals_numpy(host_program, tmp_path):
    items = cases.count_series()
    lines = [str(len(items))]
    for kind, R, Nn, c in items:
        lines += [f"m {R} {float(Nn).hex()}", " ".join(str(int(v)) for v in c)]
    got = _run_host(host_program, lines, tmp_path)
    assert len(got) == len(items)
    for (kind, R, Nn, c), ln in zip(items, got):
        m3 = np.array([float.fromhex(tok) for tok in ln.split()])
        f = np.sort(c).astype(np.float64) / Nn
        lo, hi = oracle_mod.hpdi(f, 0.68)
        assert m3[0] == np.median(f) and m3[1] == lo and m3[2] == hi, (kind, R, m3, np.median(f), lo, hi)
        assert np.array_equal(m3, ref.summary(oracle_mod, c, Nn))
    assert np.isnan(ref.summary(oracle_mod, items[0][3], 0.0)).all()
    bad = items[0][3].copy()
    bad[3] = ref.NO_COUNT
    assert np.isnan(ref.summary(oracle_mod, bad, 40.0)).all()


# --------------------------------------------------------------------------
# the reference is the oracle's post step when every draw is taken once
# --------------------------------------------------------------------------
def test_reference_with_equal_weights_is_the_oracles_post_step(oracle_lib):
    S = R = 100
    x, status, y, N, names = post_cases.case("rows", S)
    out, pred, st, waic, counts, flags = post_cases.oracle_post("rows", S)
    n = 0
    for t, name in enumerate(names):
        rows = [(True, 0.0, float(S), np.full(S, 1.0 / S), x[t, sub]) for sub in (0, 2, 3)]
        got = ref.assemble(rows, S, R, N[t, :30], oracle_lib, post_cases.POST_SEED, t)
        assert np.array_equal(got["index"], np.tile(np.arange(S), (3, 1))), name
        assert (got["rec"][ref.NDISTINCT:ref.NDISTINCT + 3] == S).all()
        ran = flags[t] <= 1
        assert np.array_equal(got["counts"][ran], counts[t][ran]), name
        assert np.array_equal(got["ppred"].astype(np.float32), pred[t], equal_nan=True), name
        want5 = out[t, [0, 2, 3, 16, 19]]  # D_max, its interval, D_max_forward, D_max_reverse
        assert np.array_equal(got["rec"][:5], want5, equal_nan=True), (name, got["rec"][:5], want5)
        assert int(got["rec"][ref.FLAGS]) == 31
        # np.median and numpyro's hpdi of the counts give the oracle's summary
        for j in np.flatnonzero(ran):
            Nn = float(N[t, ref.JOBS[j][3]])
            want = ref.summary(oracle_mod, got["counts"][j], Nn)
            have = got["ppred"][:, j] if j < 30 else np.array([got["rec"][3 + j - 30]])
            assert np.array_equal(have, want[: have.size], equal_nan=True), (name, j)
            n += 1
    assert n >= 200


# --------------------------------------------------------------------------
# the method means something: against the oracle's NUTS intervals
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


def test_reference_vs_nuts_intervals(oracle_lib):
    """The reference at S = 256, R = 1000 on the Philox stream of seed 0 against
    two 500 + 1000 oracle NUTS runs (seeds 0 and 1; "NUTS" is their mean) and
    the oracle's MAP record, on the 26 taxa of _taxa_26: per taxon the median
    over the 30 positions of (68 % window width) / (NUTS width).  The frame is
    the PMD-all row's, so a taxon counts as reliable here when that row's khat is
    at or under the threshold 0.585.  Measured: 19 reliable taxa; MAP record
    0.892 - 1.000, median 0.950; resampled predictive 0.964 - 1.026, median
    1.002; each NUTS seed against their mean 0.990 - 1.010.  Asserted: at least 18 reliable taxa,
    each ratio in [0.94, 1.05] (the measured range widened by the seeds' own
    +- 0.02), their median within 0.02 of 1, the MAP record's median at most
    0.97."""
    b, taxa = _taxa_26()
    S, R = 256, 1000
    y, N = b.y[taxa], b.N[taxa]
    out, mpred, st = oracle_lib.fit_batch(y, N)
    assert (st == 0).all()
    nuts = []
    for seed in (0, 1):
        no, npred, ns = oracle_lib.nuts_batch(y, N, seed=seed, num_warmup=500, num_samples=1000)
        assert (ns == 0).all()
        nuts.append(np.asarray(npred, float))
    width = lambda p: p[:, 2, :] - p[:, 1, :]  # noqa: E731
    w_nuts = 0.5 * (width(nuts[0]) + width(nuts[1]))
    got = [ref.pred_taxon(oracle_lib, y[i, :30], N[i, :30], out[i], 0, S, R, seed=0, g=int(t))
           for i, t in enumerate(taxa)]
    flags = np.array([int(g["rec"][ref.FLAGS]) for g in got])
    k_all = np.array([g["rec"][ref.KHAT] for g in got])
    reliable = ((flags & 4) != 0) & (k_all <= pref.khat_threshold(S))
    assert not (((flags & ref.RELIABLE) != 0) & ~reliable).any()
    w_is = np.stack([g["ppred"][2] - g["ppred"][1] for g in got])
    w_map = width(np.asarray(mpred, float))
    with np.errstate(invalid="ignore", divide="ignore"):
        r_is = np.nanmedian(w_is / w_nuts, axis=1)
        r_map = np.nanmedian(w_map / w_nuts, axis=1)
        r_s0 = np.nanmedian(width(nuts[0]) / w_nuts, axis=1)
        r_s1 = np.nanmedian(width(nuts[1]) / w_nuts, axis=1)
        z1 = np.stack([w_map[:, 0], w_is[:, 0], width(nuts[0])[:, 0], width(nuts[1])[:, 0]]) / w_nuts[:, 0]
    print("taxon rel khat_all | width / NUTS width, median of 30: MAP IS NUTS0 NUTS1 | at z = +1: MAP IS NUTS0 NUTS1")
    for i, t in enumerate(taxa):
        print(f"{t:4d} {int(reliable[i])} {k_all[i]:6.2f} | {r_map[i]:.3f} {r_is[i]:.3f} {r_s0[i]:.3f} {r_s1[i]:.3f} | "
              + " ".join(f"{v:.3f}" for v in z1[:, i]))
    rr = reliable
    print(f"reliable {rr.sum()} of 26; MAP {r_map[rr].min():.3f} - {r_map[rr].max():.3f} median {np.median(r_map[rr]):.3f}; "
          f"IS {r_is[rr].min():.3f} - {r_is[rr].max():.3f} median {np.median(r_is[rr]):.3f}; "
          f"NUTS seeds {min(r_s0[rr].min(), r_s1[rr].min()):.3f} - {max(r_s0[rr].max(), r_s1[rr].max()):.3f}")
    print(f"z = +1: MAP {z1[0, rr].min():.3f} - {z1[0, rr].max():.3f}; IS {z1[1, rr].min():.3f} - {z1[1, rr].max():.3f}; "
          f"NUTS seeds {z1[2:, rr].min():.3f} - {z1[2:, rr].max():.3f}")
    assert rr.sum() >= 18, rr.sum()
    assert (r_is[rr] >= 0.94).all() and (r_is[rr] <= 1.05).all(), r_is[rr]
    assert abs(np.median(r_is[rr]) - 1.0) <= 0.02, np.median(r_is[rr])
    assert np.median(r_map[rr]) <= 0.97, np.median(r_map[rr])


# --------------------------------------------------------------------------
# the GPU test's inputs do not sit on decision boundaries
# --------------------------------------------------------------------------
def gpu_case_draws(oracle_lib, n_taxa: int, S: int, R: int):
    """(x[T, 6, R, 4], y, N) of the first n_taxa of generate(300, 21): the
    reference's resampled draws of the three PMD rows in the chains 0, 2, 3 of a
    post-step call (NaN in an invalid row's chain), from the oracle's MAP fit."""
    from metadamage_amd.synthetic import generate

    b = generate(300, seed=21)
    y, N = b.y[:n_taxa], b.N[:n_taxa]
    out, _, st = oracle_lib.fit_batch(y, N)
    x = np.full((n_taxa, 6, R, 4), np.nan)
    x[:, [1, 4, 5]] = 0.5
    for t in range(n_taxa):
        if st[t] != 0:
            continue
        for row, r in enumerate(pref.psis_taxon(oracle_lib, y[t, :30], N[t, :30], out[t], 0, S, seed=0, g=t)):
            if int(r["rec"][pref.FLAGS]) & pref.VALID:
                idx, _ = ref.resample(np.asarray(r["w"], np.float64), R)
                th = pref.constrained(np.asarray(r["u"], np.float64)).astype(np.float64)
                x[t, ref.STREAM_SUB[row]] = th[idx]
    return x, y, N


def test_gpu_inputs_are_insensitive_to_a_last_bit_of_theta(oracle_lib):
    """The oracle at theta and at theta (1 +- 2^-52) on the taxa of the GPU
    test: at most 0.5 % of the draws of a regime class and 3 % of a job's
    differ (the caps of tests/test_gpu_nuts_post.py and of the GPU test here)."""
    from tests.test_nuts_post import draw_shares

    x, y, N = gpu_case_draws(oracle_lib, 64, 256, 1000)  # batch A of tests/test_gpu_map_pred.py
    ok = np.isfinite(x).all(axis=(1, 2, 3))
    assert ok.sum() >= 50
    x, y, N = x[ok], y[ok], N[ok]
    base = oracle_lib.nuts_post(y, N, x, seed=0, taps=True)
    tot = {c: [0, 0] for c in post_cases.CLASSES}
    worst_job = 0.0
    for sign in (1.0, -1.0):
        xp = x * (1.0 + sign * 2.0 ** -52)
        got = oracle_lib.nuts_post(y, N, xp, seed=0, taps=True)
        per_class, per_job, _, _ = draw_shares(x, N, base[4], got[4], base[5], got[5])
        worst_job = max(worst_job, float(per_job.max()))
        for c, (d, n) in per_class.items():
            tot[c][0] += d
            tot[c][1] += n
    for c, (d, n) in tot.items():
        print(f"{c}: {d} of {n} draws differ ({100.0 * d / max(n, 1):.4f} %)")
        assert d <= 0.005 * n, (c, d, n)
    print(f"worst job: {100.0 * worst_job:.3f} %")
    assert worst_job <= 0.03
    assert tot["inversion"][1] > 0 and tot["btrs_small"][1] > 0 and tot["boost"][1] > 0


# --------------------------------------------------------------------------
# frames, options, CLI, gather record, chunk planning
# --------------------------------------------------------------------------
def _cfg(tmp_path, inference="map-pred", **kw):
    from metadamage_amd import utils
    from tests.helpers import GOLDEN

    cfg = utils.Config(out_dir=tmp_path, max_fits=10, max_cores=1, min_alignments=10, min_y_sum=10,
                       substitution_bases_forward="CT", substitution_bases_reverse="GA", forced=False,
                       version="0.0.0", inference=inference, **kw)
    cfg.add_filename(GOLDEN / "data_ancient.txt")
    return cfg


NEW_COLUMNS = ["D_max_predictive", "D_max_predictive_lower_hpdi", "D_max_predictive_upper_hpdi",
               "D_max_predictive_forward", "D_max_predictive_reverse", "pareto_k_pred", "pred_ess_min",
               "pred_distinct_min", "map_pred_valid", "map_pred_reliable"]
NEW_PREDICTION_COLUMNS = ["median_posterior", "hdpi_lower_posterior", "hdpi_upper_posterior"]


def test_frame_columns_and_dtypes(tmp_path, oracle_lib, ref_meta):
    import pandas as pd

    from metadamage_amd import engine, fits
    from tests.helpers import GOLDEN

    cfg = _cfg(tmp_path)
    p = fits.pack_counts(pd.read_parquet(GOLDEN / "counts_data_ancient.parquet"), cfg)
    out, pred, st = oracle_lib.fit_batch(p.y, p.N, p.mm)
    S, R = 64, 100
    got = [ref.pred_taxon(oracle_lib, p.y[t, :30], p.N[t, :30], out[t], int(st[t]), S, R, seed=0, g=t)
           for t in range(len(st))]
    rec = np.stack([g["rec"] for g in got])
    assert ((rec[:, ref.FLAGS].astype(int) & 1) != 0).all()
    rec[1, ref.FLAGS] = 29.0  # one taxon over the threshold
    block = np.concatenate([np.stack([g["ppred"] for g in got]).reshape(len(st), 90), rec], axis=1).astype(np.float32)
    assert block.shape == (len(st), engine.PPRED_WORDS)
    pp32, rec32 = engine.split_ppred(block)
    keep = st == 0
    plain = fits.make_df_fit_results(p, out, keep, cfg)
    assert len(plain.columns) == 30
    df = fits.make_df_fit_results(p, out, keep, cfg, ppred=block)
    assert list(df.columns) == ref_meta["fit_results_columns"] + NEW_COLUMNS and len(df.columns) == 40
    assert NEW_COLUMNS == fits.MAP_PRED_COLUMNS + fits.MAP_PRED_UINT_COLUMNS
    pd.testing.assert_frame_equal(df[plain.columns], plain)  # the 25 result columns are the MAP call's
    for c in NEW_COLUMNS[:7]:
        assert df[c].dtype == np.float32, c
    for c in NEW_COLUMNS[7:]:
        assert df[c].dtype == np.uint32, c
    for j, name in enumerate(NEW_COLUMNS[:5]):
        np.testing.assert_array_equal(df[name].to_numpy(), rec32[keep, j], err_msg=name)
    np.testing.assert_array_equal(df["pareto_k_pred"].to_numpy(), rec32[keep, ref.KHAT:ref.KHAT + 3].max(axis=1))
    np.testing.assert_array_equal(df["pred_ess_min"].to_numpy(), rec32[keep, ref.ESS:ref.ESS + 3].min(axis=1))
    np.testing.assert_array_equal(df["pred_distinct_min"].to_numpy(),
                                  rec32[keep, ref.NDISTINCT:ref.NDISTINCT + 3].min(axis=1).astype(np.uint32))
    assert (df["map_pred_valid"] == 1).all() and df["map_pred_reliable"].to_numpy()[1] == 0
    assert np.isfinite(df[NEW_COLUMNS[:7]].to_numpy()).all()
    k2 = np.array([True, False, True])  # a dropped taxon takes its rows with it
    d2 = fits.make_df_fit_results(p, out, k2, cfg, ppred=block)
    np.testing.assert_array_equal(d2["D_max_predictive"].to_numpy(), rec32[k2, 0])
    # the predictions frame
    pred32 = np.asarray(pred, np.float32)
    plain_p = fits.make_df_fit_predictions(p, pred32, keep, cfg)
    dp = fits.make_df_fit_predictions(p, pred32, keep, cfg, ppred=block)
    assert list(dp.columns) == list(plain_p.columns) + NEW_PREDICTION_COLUMNS
    assert NEW_PREDICTION_COLUMNS == fits.MAP_PRED_PREDICTION_COLUMNS
    pd.testing.assert_frame_equal(dp[plain_p.columns], plain_p)  # median, hdpi_lower, hdpi_upper are the MAP call's
    for j, name in enumerate(NEW_PREDICTION_COLUMNS):
        assert dp[name].dtype == np.float32
        np.testing.assert_array_equal(dp[name].to_numpy(), pp32[keep][:, j, :].reshape(-1), err_msg=name)
    dp2 = fits.make_df_fit_predictions(p, pred32, k2, cfg, ppred=block)
    np.testing.assert_array_equal(dp2["median_posterior"].to_numpy(), pp32[k2][:, 0, :].reshape(-1))
    # an invalid taxon's record: NaN columns, zeros in the integer ones
    block[0, 90:105] = np.nan
    block[0, 105] = 0.0
    d3 = fits.make_df_fit_results(p, out, keep, cfg, ppred=block)
    assert np.isnan(d3[NEW_COLUMNS[:7]].to_numpy()[0]).all() and (d3[NEW_COLUMNS[7:]].to_numpy()[0] == 0).all()


def test_make_opts_config_and_cli(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import _lib, fits
    from metadamage_amd.cli import cli_app
    from tests.helpers import GOLDEN

    o = fits.make_opts(_cfg(tmp_path, "map-pred"))
    m = fits.make_opts(_cfg(tmp_path, "map"))
    assert o.mode == _lib.MODE_MAP and bytes(o) == bytes(m)
    assert fits.wants_pred(_cfg(tmp_path, "map-pred")) and not fits.wants_pred(_cfg(tmp_path, "map"))
    for other in ("map-psis", "map-waic", "auto", "nuts"):
        assert not fits.wants_pred(_cfg(tmp_path, other)), other
    c = _cfg(tmp_path, "map-pred")
    assert not (fits.wants_psis(c) or fits.wants_waic(c) or fits.wants_laplace(c) or fits.wants_auto(c))
    assert fits.mode_of("map-pred") == _lib.MODE_MAP
    assert fits.pred_draws_of(c) == 1000 and fits.psis_draws_of(c) == 256
    assert fits.pred_draws_of(_cfg(tmp_path, "map-pred", pred_draws=100)) == 100
    # both draw counts are in the metadata (and the cache key) of a map-pred run, pred_draws of no other
    d = _cfg(tmp_path, "map-pred", psis_draws=100, pred_draws=50).to_dict()
    assert d["psis_draws"] == 100 and d["pred_draws"] == 50 and d["inference"] == "map-pred"
    for other in ("map", "map-laplace", "map-psis", "map-waic", "auto", "nuts", "nuts-loo"):
        assert "pred_draws" not in _cfg(tmp_path, other).to_dict(), other
    for other in ("map", "map-laplace", "nuts", "nuts-loo"):
        assert "psis_draws" not in _cfg(tmp_path, other).to_dict(), other
    assert "pred_draws" in fits.CACHE_KEYS and "psis_draws" in fits.CACHE_KEYS and "inference" in fits.CACHE_KEYS
    runner = CliRunner()
    base = ["fit", str(GOLDEN / "data_ancient.txt"), "--out-dir", str(tmp_path)]
    bad = runner.invoke(cli_app, base + ["--inference", "map-foo"])
    assert bad.exit_code == 2 and "map-pred" in bad.output
    for n in ("24", "1025"):
        bad = runner.invoke(cli_app, base + ["--inference", "map-pred", "--pred-draws", n])
        assert bad.exit_code == 2 and "pred-draws" in bad.output
        bad = runner.invoke(cli_app, base + ["--inference", "map-pred", "--psis-draws", n])
        assert bad.exit_code == 2 and "psis-draws" in bad.output
    text = runner.invoke(cli_app, ["fit", "--help"], terminal_width=200).output
    assert "map-pred" in text and "--pred-draws" in text


def test_gather_record_with_ppred_round_trips():
    import torch

    from metadamage_amd import distributed as d, engine

    assert d.REC_BYTES == 496 and d.REC_PPRED == 424 == 106 * 4 == engine.PPRED_BYTES
    n = 7
    rng = np.random.default_rng(2)
    buf = torch.from_numpy(rng.integers(0, 256, n * (d.REC_BYTES + d.REC_PPRED), dtype=np.uint8))
    pred, status, ints, floats, wv = d.packed_views(buf, n, with_ppred=True)
    p0, s0, i0, f0 = d.packed_views(buf[: n * d.REC_BYTES], n)  # the default layout is a prefix
    assert pred.data_ptr() == p0.data_ptr() and status.data_ptr() == s0.data_ptr()
    assert ints.data_ptr() == i0.data_ptr() and floats.data_ptr() == f0.data_ptr()
    assert wv.shape == (n, 106) and wv.dtype == torch.float32
    assert wv.data_ptr() == buf.data_ptr() + n * d.REC_BYTES
    want = rng.standard_normal((n, 106)).astype(np.float32)
    want[0, 4] = np.nan
    wv.copy_(torch.from_numpy(want))
    st = rng.integers(0, 4, n).astype(np.int32)
    status.copy_(torch.from_numpy(st))
    ints.copy_(torch.from_numpy(np.rint(rng.standard_normal(tuple(ints.shape)) * 100)))
    floats.copy_(torch.from_numpy(rng.standard_normal(tuple(floats.shape)).astype(np.float32)))
    pred.copy_(torch.from_numpy(rng.standard_normal(tuple(pred.shape)).astype(np.float32)))
    out, pr, ss, got = d.unpack_gathered([buf, buf.clone()], 13, 2, with_ppred=True)
    assert out.shape == (13, 25) and got.shape == (13, 106) and got.dtype == np.float32
    np.testing.assert_array_equal(got[:7], want)
    np.testing.assert_array_equal(got[7:], want[:6])
    np.testing.assert_array_equal(ss[7:], st[:6])
    pp, rec = engine.split_ppred(got)
    assert pp.shape == (13, 3, 30) and rec.shape == (13, 16)
    np.testing.assert_array_equal(pp[:7].reshape(7, 90), want[:, :90])
    r = d.alloc_records(5, "cpu", with_ppred=True)
    assert r.ppred.shape == (5, 106) and r.waic is None and r.psis is None
    assert r.buf.numel() == 5 * (d.REC_BYTES + d.REC_PPRED)
    for other in ("with_laplace", "with_diag", "with_summary", "with_loo", "with_psis", "with_waic", "with_auto"):
        with pytest.raises(ValueError, match="mutually exclusive"):
            d.packed_views(buf, n, with_ppred=True, **{other: True})
        with pytest.raises(ValueError, match="mutually exclusive"):
            d.alloc_records(3, "cpu", with_ppred=True, **{other: True})


def test_chunk_planning_with_ppred():
    from metadamage_amd import _lib, engine

    assert engine.PPRED_BYTES == 424 and engine.PPRED_WORDS == 106 and engine.PRED_DRAWS == 1000
    m = _lib.default_opts(mode=_lib.MODE_MAP)
    base = engine.device_bytes(1000, m)
    assert engine.device_bytes(1000, m, with_ppred=True) == base + 1000 * (360 + 128 + 424)
    assert engine.device_bytes(1000, m, dest_on_device=True, with_ppred=True) == \
        engine.device_bytes(1000, m, dest_on_device=True) + 1000 * (360 + 128)
    assert engine.device_bytes(10, None, with_ppred=True) == engine.device_bytes(10, None) + 10 * 912
    budget = 2 * engine.device_bytes(400, m, with_ppred=True)
    chunks = engine.plan_chunks(1000, m, budget, with_ppred=True)
    assert chunks[0][0] == 0 and chunks[-1][1] == 1000 and max(hi - lo for lo, hi in chunks) <= 400
    assert len(chunks) >= len(engine.plan_chunks(1000, m, budget))
    # every other mode's byte counts are what they were
    assert engine.device_bytes(1000, m, with_waic=True) == base + 1000 * 3 * 224
    n = _lib.default_opts(mode=_lib.MODE_NUTS)
    with pytest.raises(ValueError, match="MODE_MAP"):
        engine.device_bytes(10, n, with_ppred=True)
    with pytest.raises(ValueError, match="MODE_MAP"):
        engine.plan_chunks(10, n, with_ppred=True)
    for other in ("with_laplace", "with_psis", "with_waic"):
        with pytest.raises(ValueError, match="mutually exclusive"):
            engine.device_bytes(10, m, with_ppred=True, **{other: True})
        with pytest.raises(ValueError, match="mutually exclusive"):
            engine.plan_chunks(10, m, with_ppred=True, **{other: True})
