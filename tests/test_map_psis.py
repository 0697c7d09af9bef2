"""CPU tests of the importance-sampled posterior of the MAP fit (MDFIT-PSIS v1,
DESIGN.md §3.8): the C-ABI entry points without a device, the reference's
target against the oracle's sampling potential, the host build of the smoothing
and the estimates (csrc/mdfit_mappsis.h, one-lane policy) against the reference
(tests/map_psis_ref.py), the reference against the oracle's NUTS posterior, and
the frames / options / CLI / gather-record / chunk-planning plumbing."""

from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from tests import map_psis_cases as cases
from tests import map_psis_ref as ref
from tests.helpers import GOLDEN

ROOT = Path(__file__).resolve().parents[1]

# the host program against the reference, measured over every series of
# map_psis_cases (w relative to the series' largest weight 3.4e-15, khat 6.5e-15
# absolute, a record field 1.2e-13 relative), times ten
HOST_TOL = {"w": 3.4e-14, "khat": 6.5e-14, "rec": 1.2e-12}


# --------------------------------------------------------------------------
# ABI
# --------------------------------------------------------------------------
def test_entry_points_declared_exported_and_argument_checked():
    from metadamage_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mdfit.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+mdfit_map_psis\s*\(", text) and re.search(r"\bint\s+mdfit_psis_weights\s*\(", text)
    assert f"#define MDFIT_NMAPPSIS {_lib.NMAPPSIS}" in text
    assert f"#define MDFIT_ABI_VERSION {_lib.ABI_VERSION}" in text and _lib.ABI_VERSION == 3
    assert "mdfit_map_psis" in _lib.EXPORTED_SYMBOLS and "mdfit_psis_weights" in _lib.EXPORTED_SYMBOLS
    assert len(_lib.MAPPSIS_FIELDS) == _lib.NMAPPSIS == 16 and _lib.MAPPSIS_FIELDS == ref.FIELDS
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                        check=True).stdout
    assert re.search(r"\bT mdfit_map_psis\b", nm) and re.search(r"\bT mdfit_psis_weights\b", nm)
    dummy = ctypes.c_void_p(16)
    assert lib.mdfit_map_psis(None, None, None, None, 0, 256, 0, 0, None, None, None) == 0
    assert lib.mdfit_map_psis(None, None, None, None, -1, 256, 0, 0, None, None, None) == -1
    assert b"n_taxa" in lib.mdfit_last_error()
    for S in (24, 1025):
        assert lib.mdfit_map_psis(dummy, dummy, dummy, dummy, 1, S, 0, 0, dummy, None, None) == -1
        assert b"num_draws" in lib.mdfit_last_error()
        assert lib.mdfit_psis_weights(dummy, 1, S, dummy, dummy, None) == -1
    assert lib.mdfit_map_psis(dummy, dummy, dummy, dummy, 1, 256, 0, 0, None, None, None) == -1  # psis is required
    assert lib.mdfit_map_psis(dummy, dummy, dummy, dummy, (1 << 25) + 1, 256, 0, 0, dummy, None, None) == -1
    assert lib.mdfit_psis_weights(None, 0, 256, None, None, None) == 0


# --------------------------------------------------------------------------
# the reference's target is the density the sampler draws from
# --------------------------------------------------------------------------
def _deep_taxa():
    from metadamage_amd.synthetic import generate

    b = generate(400, seed=21)
    deep = np.flatnonzero(b.truth["ancient"] & (b.N[:, :30].mean(axis=1) > 3e3))[:16]
    assert deep.size == 16
    return b, deep


def test_target_vs_nuts_potential(oracle_lib):
    """log p(u) + U(v) + log(c(1 - c)) at v = (u0, u1, logit c, u3) is one
    constant per sub-fit over 200 feasible random u.  Measured spread (max -
    min): 6.1e-10, 4.7e-10, 4.3e-10 for the all, forward and reverse rows, at
    constants 2.8e4, 1.3e4, 1.5e4 -- the resolution of the potential's lnGamma
    sums; asserted at ten times the largest."""
    b, deep = _deep_taxa()
    t = deep[0]
    rng = np.random.default_rng(0)
    for row in range(3):
        u = np.column_stack([rng.uniform(-3, 1, 200), rng.uniform(-4, 0, 200), rng.uniform(0.001, 0.2, 200),
                             rng.uniform(2, 9, 200)])
        lp = ref.log_target(oracle_lib, b.y[t, :30], b.N[t, :30], row, u)
        assert np.isfinite(lp.astype(float)).all()
        vals = []
        for i in range(200):
            c = u[i, 2]
            v = np.array([u[i, 0], u[i, 1], np.log(c) - np.log1p(-c), u[i, 3]])
            U, _ = oracle_lib.nuts_potential(0, ref.SUBFITS[row][0], b.y[t, :30], b.N[t, :30], v)
            vals.append(float(lp[i]) + U + np.log(c * (1 - c)))
        spread = max(vals) - min(vals)
        print(f"row {row}: constant {np.mean(vals):.6g}, spread {spread:.2e}")
        assert spread <= 6.2e-9
    # an infeasible draw: -inf
    bad = np.array([[0.0, 0.0, -0.01, 3.0], [0.0, 3.0, 0.2, 3.0], [0.0, 0.0, 0.1, 3.0]])
    lp = ref.log_target(oracle_lib, b.y[t, :30], b.N[t, :30], 0, bad)
    assert lp[0] == -np.inf and lp[1] == -np.inf and np.isfinite(float(lp[2]))


def test_random_numbers_are_the_documented_blocks(oracle_lib):
    """Draw s of stream (seed, g, sub) reads the blocks (g lo, g hi + (sub <<
    24), DOMAIN + s, 0..3) under the key (seed lo, seed hi)."""
    seed, g, sub = 0x1234567890, (5 << 32) + 77, 3
    z, chi2, e = ref.randoms(oracle_lib, seed, g, sub, 3)
    key = [seed & 0xFFFFFFFF, seed >> 32]
    o = oracle_lib.philox([77, 5 + (3 << 24), ref.DOMAIN + 2, 3], key)
    u = ((int(o[0]) >> 5) * 67108864.0 + (int(o[1]) >> 6)) / 9007199254740992.0
    assert abs(float(e[2]) + np.log1p(-u)) < 1e-15
    o = oracle_lib.philox([77, 5 + (3 << 24), ref.DOMAIN + 1, 1], key)
    u1 = 1 - ((int(o[0]) >> 5) * 67108864.0 + (int(o[1]) >> 6)) / 9007199254740992.0
    u2 = ((int(o[2]) >> 5) * 67108864.0 + (int(o[3]) >> 6)) / 9007199254740992.0
    assert abs(float(z[1, 2]) - np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)) < 1e-14
    assert (chi2 > 0).all() and np.isfinite(z.astype(float)).all()


# --------------------------------------------------------------------------
# the host build of csrc/mdfit_mappsis.h
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mappsis_host") / "mappsis_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", str(ROOT / "tests" / "mappsis_host_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def _hex(v):
    return float(v).hex() if np.isfinite(v) else ("nan" if np.isnan(v) else ("inf" if v > 0 else "-inf"))


def _run_host(exe, lw, f, tmp_path):
    n, S = lw.shape
    lines = [str(n)]
    for i in range(n):
        lines += [str(S), " ".join(_hex(v) for v in lw[i]), " ".join(_hex(v) for v in f[i].ravel())]
    src = tmp_path / "series.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = np.array([[float.fromhex(tok) if "nan" not in tok else np.nan for tok in ln.split()]
                    for ln in r.stdout.strip().splitlines()])
    return got[:, 0].astype(bool), got[:, 1], got[:, 2:2 + S], got[:, 2 + S:]


@pytest.mark.parametrize("S", cases.S_VALUES)
def test_host_program_vs_reference(host_program, tmp_path, S):
    lw, kinds = cases.weights_case(S)
    f = cases.draws_case(S, len(kinds))
    want_w, want_k, want_valid = cases.weights_reference(S)
    ok, khat, w, rec = _run_host(host_program, lw, f, tmp_path)
    assert np.array_equal(ok, want_valid)
    worst = cases.weight_errors(w, khat, want_w, want_k, want_valid)
    worst["rec"] = 0.0
    for i, kind in enumerate(kinds):
        if kind in ("cut_inf", "all_inf", "nan", "posinf"):
            assert not ok[i] and np.isnan(rec[i, :15]).all() and rec[i, 15] == 15 << 2, kind
            continue
        assert ok[i], kind
        if kind == "const":  # uniform weights, exactly
            assert khat[i] == 0.0 and (w[i] == 1.0 / S).all()
        if kind == "const_tail":
            assert khat[i] == 0.0
        if kind == "xstar0":
            assert khat[i] == np.inf
        n_inf = int(np.isneginf(lw[i]).sum())
        assert (w[i][np.isneginf(lw[i])] == 0.0).all() and rec[i, ref.N_INF] == n_inf
        assert abs(w[i].sum() - 1.0) < 1e-13
        want = ref.estimates(want_w[i], f[i], want_k[i], n_inf, S, 15)
        assert int(rec[i, ref.FLAGS]) == int(want[ref.FLAGS]), (kind, rec[i, ref.FLAGS], want[ref.FLAGS])
        for j in list(range(12)) + [ref.ESS]:
            assert np.isnan(rec[i, j]) == np.isnan(float(want[j])), (kind, j)
            if not np.isnan(rec[i, j]):
                worst["rec"] = max(worst["rec"], float(abs(rec[i, j] - want[j]) / abs(want[j])))
    print(f"S={S}: worst error " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= HOST_TOL[name], (name, v)


def test_ties_rank_by_draw_index(host_program, tmp_path):
    """Equal raw weights across the cut-off: the later draws of a tie are the
    tail's (a stable sort), so the smoothed weights differ by draw index."""
    S = 100
    M = ref.tail_len(S)
    assert M == 20
    rng = np.random.default_rng(3)
    # 17 distinct larger values, 50 ties at 1.0 -- the last three of them by draw
    # index complete the tail, few enough for its first-quartile excess to be positive -- and 33 at 0
    lw = np.concatenate([1.5 + rng.uniform(size=17) * 2.0, np.full(50, 1.0), np.zeros(33)])[rng.permutation(S)]
    w_ref, k_ref, _, ok_ref = ref.psis_weights(lw)
    assert ok_ref and np.isfinite(float(k_ref))
    ok, khat, w, _ = _run_host(host_program, lw[None, :], cases.draws_case(S, 1), tmp_path)
    assert ok[0]
    err = np.abs(w[0] - w_ref.astype(float)).max() / float(w_ref.max())
    assert err <= HOST_TOL["w"] and abs(khat[0] - float(k_ref)) <= HOST_TOL["khat"]
    ones = np.flatnonzero(lw == 1.0)
    in_tail = M - 17  # the tail's draws among the ties at 1.0: the last of them
    assert len(set(w[0][ones[:-in_tail]])) == 1 and (np.diff(w[0][ones[-in_tail:]]) > 0).all()


# --------------------------------------------------------------------------
# the method means something: against the oracle's NUTS posterior
# --------------------------------------------------------------------------
def test_reference_vs_nuts_posterior(oracle_lib):
    """The 16 deep ancient taxa of test_reference_vs_nuts_posterior_std, the
    reference at S = 1024 on the Philox stream of seed 0, against a 500 + 1000
    oracle chain (PMD-all row).  Measured: 13 of 16 rows with khat at or below
    the threshold 0.668 (taxa 10, 16 and 41 above it: 0.77, 0.74, 0.71); over
    those 13, (mean - NUTS mean) / NUTS std in [-0.088, +0.155] and std / NUTS
    std in [0.891, 1.089]; the MAP modes lie up to 0.40 NUTS std off (taxon
    39), where the importance-sampled mean is 0.04 off.  The bands asserted are
    the measured ranges widened by the chain's own Monte-Carlo error: 0.1 std on
    the mean, 15 % on the std (as test_laplace.py argues)."""
    b, deep = _deep_taxa()
    S = 1024
    tau = ref.khat_threshold(S)
    out, _, st = oracle_lib.fit_batch(b.y[deep], b.N[deep])
    assert (st == 0).all()
    rows = []
    for i, t in enumerate(deep):
        res = ref.psis_taxon(oracle_lib, b.y[t, :30], b.N[t, :30], out[i], 0, S, seed=0, g=int(t), rows=(0,))[0]
        rec = res["rec"].astype(float)
        assert int(rec[ref.FLAGS]) & ref.VALID
        smp, _, rc = oracle_lib.nuts_chain(0, 0, b.y[t, :30], b.N[t, :30], seed=0, g=int(t), sub=0,
                                           num_warmup=500, num_samples=1000)
        assert rc == 0
        D = smp[:, 1] + smp[:, 2]
        mode = out[i, 32 + 1] + out[i, 32 + 2]
        rows.append((rec[ref.KHAT], (rec[4] - D.mean()) / D.std(), rec[9] / D.std(), (mode - D.mean()) / D.std()))
        print(f"taxon {t}: khat {rows[-1][0]:.3f}, mean {rows[-1][1]:+.3f}, std {rows[-1][2]:.3f}, "
              f"mode {rows[-1][3]:+.3f} (NUTS std)")
    rows = np.array(rows)
    good = rows[:, 0] <= tau
    print(f"{good.sum()} of 16 rows with khat <= {tau:.3f}")
    assert good.sum() >= 12
    assert (rows[good, 1] >= -0.088 - 0.1).all() and (rows[good, 1] <= 0.155 + 0.1).all(), rows[good, 1]
    assert (rows[good, 2] >= 0.891 * 0.85).all() and (rows[good, 2] <= 1.089 * 1.15).all(), rows[good, 2]
    far = int(np.argmax(np.abs(rows[:, 3])))
    assert abs(rows[far, 1]) < abs(rows[far, 3]), rows[far]


# --------------------------------------------------------------------------
# frames, options, CLI, gather record, chunk planning
# --------------------------------------------------------------------------
def _cfg(tmp_path, inference="map-psis", **kw):
    from metadamage_amd import utils

    cfg = utils.Config(out_dir=tmp_path, max_fits=10, max_cores=1, min_alignments=10, min_y_sum=10,
                       substitution_bases_forward="CT", substitution_bases_reverse="GA", forced=False,
                       version="0.0.0", inference=inference, **kw)
    cfg.add_filename(GOLDEN / "data_ancient.txt")
    return cfg


NEW_COLUMNS = ["D_max_std", "significance", "q_std", "A_std", "c_std", "concentration_std", "rho_Ac",
               "D_max_std_forward", "q_std_forward", "D_max_std_reverse", "q_std_reverse",
               "D_max_posterior_mean", "q_posterior_mean", "concentration_posterior_mean",
               "D_max_posterior_mean_forward", "D_max_posterior_mean_reverse",
               "pareto_k", "pareto_k_forward", "pareto_k_reverse", "psis_ess",
               "map_psis_valid", "map_psis_reliable"]


def test_frame_columns_and_dtypes(tmp_path, oracle_lib, ref_meta):
    from metadamage_amd import _lib, fits

    cfg = _cfg(tmp_path)
    p = fits.pack_counts(pd.read_parquet(GOLDEN / "counts_data_ancient.parquet"), cfg)
    out, pred, st = oracle_lib.fit_batch(p.y, p.N, p.mm)
    S = 64
    psis = np.stack([np.stack([r["rec"] for r in ref.psis_taxon(oracle_lib, p.y[t, :30], p.N[t, :30], out[t],
                                                                int(st[t]), S, seed=0, g=t)])
                     for t in range(len(st))]).astype(np.float64)
    psis[1, 2, ref.FLAGS] = float(int(psis[1, 2, ref.FLAGS]) & ~ref.RELIABLE)  # one row over the threshold
    psis32 = psis.astype(np.float32)
    keep = st == 0
    plain = fits.make_df_fit_results(p, out, keep, cfg)
    assert len(plain.columns) == 30
    df = fits.make_df_fit_results(p, out, keep, cfg, psis=psis32)
    assert list(df.columns) == ref_meta["fit_results_columns"] + NEW_COLUMNS and len(df.columns) == 52
    assert NEW_COLUMNS[:11] == [name for name, _, _ in fits.LAPLACE_COLUMNS]
    pd.testing.assert_frame_equal(df[plain.columns], plain)
    for c in NEW_COLUMNS[:-2]:
        assert df[c].dtype == np.float32, c
    assert df["map_psis_valid"].dtype == np.uint32 and df["map_psis_reliable"].dtype == np.uint32
    f = _lib.MAPPSIS_FIELDS.index
    for name, row, field in (("D_max_std", 0, "D_max_std"), ("significance", 0, "significance"),
                             ("concentration_std", 0, "phi_std"), ("rho_Ac", 0, "rho_Ac"),
                             ("q_std_forward", 1, "q_std"), ("D_max_std_reverse", 2, "D_max_std"),
                             ("D_max_posterior_mean", 0, "D_max_mean"), ("q_posterior_mean", 0, "q_mean"),
                             ("concentration_posterior_mean", 0, "phi_mean"),
                             ("D_max_posterior_mean_forward", 1, "D_max_mean"),
                             ("D_max_posterior_mean_reverse", 2, "D_max_mean"), ("pareto_k", 0, "khat"),
                             ("pareto_k_forward", 1, "khat"), ("pareto_k_reverse", 2, "khat"), ("psis_ess", 0, "ess")):
        np.testing.assert_array_equal(df[name].to_numpy(), psis32[keep, row, f(field)], err_msg=name)
    flags = psis[keep][:, :, ref.FLAGS].astype(int)
    valid = ((flags & 1) != 0).all(axis=1)
    np.testing.assert_array_equal(df["map_psis_valid"].to_numpy(), valid.astype(np.uint32))
    np.testing.assert_array_equal(df["map_psis_reliable"].to_numpy(),
                                  (valid & ((flags & 2) != 0).all(axis=1)).astype(np.uint32))
    assert (df["map_psis_valid"] == 1).all() and df["map_psis_reliable"].to_numpy()[1] == 0
    assert (df["D_max_std"] > 0).all()
    k2 = np.array([True, False, True])  # a dropped taxon takes its row with it
    d2 = fits.make_df_fit_results(p, out, k2, cfg, psis=psis32)
    np.testing.assert_array_equal(d2["pareto_k"].to_numpy(), psis32[k2, 0, f("khat")])


def test_make_opts_config_and_cli(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import _lib, fits
    from metadamage_amd.cli import cli_app

    o = fits.make_opts(_cfg(tmp_path, "map-psis"))
    m = fits.make_opts(_cfg(tmp_path, "map"))
    assert o.mode == _lib.MODE_MAP and bytes(o) == bytes(m)
    assert fits.wants_psis(_cfg(tmp_path, "map-psis")) and not fits.wants_psis(_cfg(tmp_path, "map"))
    assert not fits.wants_laplace(_cfg(tmp_path, "map-psis"))
    assert fits.mode_of("map-psis") == _lib.MODE_MAP
    assert fits.psis_draws_of(_cfg(tmp_path, "map-psis")) == 256
    assert fits.psis_draws_of(_cfg(tmp_path, "map-psis", psis_draws=1000)) == 1000
    # the draws are in the metadata (and the cache key) of a map-psis run only
    assert _cfg(tmp_path, "map-psis", psis_draws=100).to_dict()["psis_draws"] == 100
    assert "psis_draws" not in _cfg(tmp_path, "map").to_dict() and "psis_draws" in fits.CACHE_KEYS
    runner = CliRunner()
    base = ["fit", str(GOLDEN / "data_ancient.txt"), "--out-dir", str(tmp_path)]
    bad = runner.invoke(cli_app, base + ["--inference", "map-foo"])
    assert bad.exit_code == 2 and "map-psis" in bad.output
    for n in ("24", "1025"):
        bad = runner.invoke(cli_app, base + ["--inference", "map-psis", "--psis-draws", n])
        assert bad.exit_code == 2 and "psis-draws" in bad.output
    assert "--psis-draws" in runner.invoke(cli_app, ["fit", "--help"], terminal_width=200).output


def test_gather_record_with_psis_round_trips():
    import torch

    from metadamage_amd import _lib, distributed as d

    assert d.REC_BYTES == 496 and d.REC_PSIS == 192
    n = 7
    rng = np.random.default_rng(2)
    buf = torch.from_numpy(rng.integers(0, 256, n * (d.REC_BYTES + d.REC_PSIS), dtype=np.uint8))
    pred, status, ints, floats, ps = d.packed_views(buf, n, with_psis=True)
    p0, s0, i0, f0 = d.packed_views(buf[: n * d.REC_BYTES], n)  # the default layout is a prefix
    assert pred.data_ptr() == p0.data_ptr() and status.data_ptr() == s0.data_ptr()
    assert ints.data_ptr() == i0.data_ptr() and floats.data_ptr() == f0.data_ptr()
    assert ps.shape == (n, 3, _lib.NMAPPSIS) and ps.dtype == torch.float32
    assert ps.data_ptr() == buf.data_ptr() + n * d.REC_BYTES
    want = rng.standard_normal((n, 3, 16)).astype(np.float32)
    want[0, 1, 5] = np.nan
    ps.copy_(torch.from_numpy(want))
    st = rng.integers(0, 4, n).astype(np.int32)
    status.copy_(torch.from_numpy(st))
    ints.copy_(torch.from_numpy(np.rint(rng.standard_normal(tuple(ints.shape)) * 100)))
    floats.copy_(torch.from_numpy(rng.standard_normal(tuple(floats.shape)).astype(np.float32)))
    pred.copy_(torch.from_numpy(rng.standard_normal(tuple(pred.shape)).astype(np.float32)))
    out, pr, ss, got = d.unpack_gathered([buf, buf.clone()], 13, 2, with_psis=True)
    assert out.shape == (13, 25) and got.shape == (13, 3, 16) and got.dtype == np.float32
    np.testing.assert_array_equal(got[:7], want)
    np.testing.assert_array_equal(got[7:], want[:6])
    np.testing.assert_array_equal(ss[7:], st[:6])
    for other in ("with_laplace", "with_diag", "with_summary", "with_loo"):
        with pytest.raises(ValueError, match="mutually exclusive"):
            d.packed_views(buf, n, with_psis=True, **{other: True})


def test_chunk_planning_with_psis():
    from metadamage_amd import _lib, engine

    assert engine.PSIS_BYTES == 192 and engine.PSIS_DRAWS == 256
    m = _lib.default_opts(mode=_lib.MODE_MAP)
    base = engine.device_bytes(1000, m)
    assert engine.device_bytes(1000, m, with_psis=True) == base + 1000 * 3 * 192
    assert engine.device_bytes(1000, m, dest_on_device=True, with_psis=True) == \
        engine.device_bytes(1000, m, dest_on_device=True) + 1000 * 2 * 192
    assert engine.device_bytes(10, None, with_psis=True) == engine.device_bytes(10, None) + 10 * 3 * 192
    budget = 2 * engine.device_bytes(400, m, with_psis=True)
    chunks = engine.plan_chunks(1000, m, budget, with_psis=True)
    assert chunks[0][0] == 0 and chunks[-1][1] == 1000 and max(hi - lo for lo, hi in chunks) <= 400
    assert len(chunks) >= len(engine.plan_chunks(1000, m, budget))
    n = _lib.default_opts(mode=_lib.MODE_NUTS)
    with pytest.raises(ValueError, match="MODE_MAP"):
        engine.device_bytes(10, n, with_psis=True)
    with pytest.raises(ValueError, match="MODE_MAP"):
        engine.plan_chunks(10, n, with_psis=True)
    with pytest.raises(ValueError, match="mutually exclusive"):
        engine.device_bytes(10, m, with_laplace=True, with_psis=True)
    with pytest.raises(ValueError, match="mutually exclusive"):
        engine.plan_chunks(10, m, with_laplace=True, with_psis=True)
