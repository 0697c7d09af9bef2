"""CPU tests of the Laplace standard errors of the MAP fit: the
C-ABI entry point without a device, the host build of the 4x4 routine against
mpmath, the reference (tests/laplace_ref.py) against the oracle's NUTS spread,
and the frames / CLI / gather-record plumbing."""

from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from tests import laplace_ref as ref
from tests.helpers import GOLDEN

ROOT = Path(__file__).resolve().parents[1]


# --------------------------------------------------------------------------
# ABI
# --------------------------------------------------------------------------
def test_entry_point_declared_exported_and_argument_checked():
    from metadamage_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mdfit.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+mdfit_map_laplace\s*\(", text)
    assert f"#define MDFIT_NLAPLACE {_lib.NLAPLACE}" in text
    assert f"#define MDFIT_ABI_VERSION {_lib.ABI_VERSION}" in text and _lib.ABI_VERSION == 3
    assert "mdfit_map_laplace" in _lib.EXPORTED_SYMBOLS
    assert len(_lib.LAPLACE_FIELDS) == _lib.NLAPLACE == 8
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                        check=True).stdout
    assert re.search(r"\bT mdfit_map_laplace\b", nm)
    assert lib.mdfit_map_laplace(None, None, None, None, 0, None, None, None) == 0
    assert lib.mdfit_map_laplace(None, None, None, None, -1, None, None, None) == -1
    assert b"n_taxa" in lib.mdfit_last_error()
    dummy = ctypes.c_void_p(16)
    assert lib.mdfit_map_laplace(dummy, dummy, dummy, dummy, 1, None, None, None) == -1  # lap is required


# --------------------------------------------------------------------------
# host linear algebra vs mpmath
# --------------------------------------------------------------------------
def _pack(H):
    return [H[j][m] for j in range(4) for m in range(j, 4)]


def _spd_case(rng, mask, kappa):
    """A 4x4 symmetric H whose free block is SPD with a Jacobi-scaled condition
    number near kappa and raw diagonals 10^U(-12, 7); held rows hold junk."""
    idx = [j for j in range(4) if mask >> j & 1]
    n = len(idx)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0.0, -np.log10(kappa), n) if n > 1 else np.ones(1)
    R = (Q * lam) @ Q.T
    R = (R + R.T) / 2
    s = 1.0 / np.sqrt(np.diag(R))
    R = R * np.outer(s, s)
    d = 10.0 ** rng.uniform(-12.0, 7.0, n)
    Hf = R * np.sqrt(np.outer(d, d))
    H = rng.standard_normal((4, 4)) * 1e3
    H = (H + H.T) / 2
    for j in range(4):
        if not mask >> j & 1:
            H[j, j] = -abs(H[j, j])  # a held coordinate's curvature is never read
    H[np.ix_(idx, idx)] = (Hf + Hf.T) / 2
    return H


def _mp_pivots(H, mask):
    import mpmath as mp

    idx = [j for j in range(4) if mask >> j & 1]
    with mp.workdps(50):
        n = len(idx)
        R = mp.matrix(n, n)
        for a, j in enumerate(idx):
            for b, m in enumerate(idx):
                R[a, b] = mp.mpf(float(H[j, m])) / mp.sqrt(mp.mpf(float(H[j, j])) * mp.mpf(float(H[m, m])))
        piv = []
        for k in range(n):  # Schur-complement diagonals = L_kk^2
            piv.append(float(R[k, k]))
            for a in range(k + 1, n):
                f = R[a, k] / R[k, k]
                for b in range(k + 1, n):
                    R[a, b] -= f * R[k, b]
        return piv


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("laplace_host") / "laplace_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "laplace_host_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def _run_host(exe, cases):
    lines = [str(len(cases))]
    for H, mask, J, dmax in cases:
        lines.append(" ".join([str(mask)] + [float(v).hex() for v in (*_pack(H), *J, dmax)]))
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [[float.fromhex(tok) if "nan" not in tok else np.nan for tok in ln.split()]
            for ln in r.stdout.strip().splitlines()]
    return np.array(rows)


def test_host_linear_algebra_vs_mpmath(host_program):
    rng = np.random.default_rng(5)
    cases = []
    masks = list(range(1, 16))  # every free set of 1-4 coordinates
    for kappa in (1.0, 1e2, 1e4, 1e6, 1e7):
        for mask in masks:
            H = _spd_case(rng, mask, kappa)
            J = np.array([rng.uniform(0.01, 0.25), rng.uniform(0.01, 0.25), 1.0, 10.0 ** rng.uniform(-3, 4)])
            cases.append((H, mask, J, rng.uniform(0.01, 0.6)))
    got = _run_host(host_program, cases)
    n_valid = 0
    worst = 0.0
    for (H, mask, J, dmax), rec in zip(cases, got):
        piv = _mp_pivots(H, mask)
        if min(piv) <= ref.PIV_MIN * (1 + 1e-6):  # (kappa 1e7: a pivot may sit at the limit)
            if min(piv) < ref.PIV_MIN * (1 - 1e-6):
                assert int(rec[7]) == mask and np.isnan(rec[:7]).all()
            continue
        free = np.array([bool(mask >> j & 1) for j in range(4)])
        want, kap, amp = ref.stats_mp(H, free, J, dmax)
        assert int(rec[7]) == (mask | ref.VALID), (mask, rec)
        n_valid += 1
        tol = 1e-14 * kap + 1e-12
        for k in range(4):
            if free[k]:
                err = abs(rec[k] - want[k]) / abs(want[k])
                worst = max(worst, err / tol)
                assert err <= tol, (mask, kap, k, rec[k], want[k])
            else:
                assert rec[k] == 0.0
        if free[1] and free[2]:
            assert abs(rec[5] - want[5]) <= tol * abs(want[5]), (mask, kap, rec[5], want[5])
        else:
            assert np.isnan(rec[5])
        if want[4] > 0:
            # the variance of A + c cancels between its three terms by the factor amp
            assert abs(rec[4] - want[4]) <= tol * amp * want[4], (mask, kap, amp, rec[4], want[4])
            assert abs(rec[6] - want[6]) <= tol * amp * abs(want[6])
        else:
            assert rec[4] == 0.0 and np.isnan(rec[6])
    assert n_valid >= 60
    print(f"host 4x4 vs mpmath: {n_valid} valid cases, worst error / bound = {worst:.3f}")


def test_host_small_pivot_is_invalid(host_program):
    # scaled free block [[1, r], [r, 1]]: second pivot 1 - r^2 = 2e-9 < 1e-8
    r = 1.0 - 1e-9
    H = np.diag([3.0, 2e5, 4e-7, 9.0])
    H[1, 2] = H[2, 1] = r * np.sqrt(H[1, 1] * H[2, 2])
    J = np.array([0.2, 0.1, 1.0, 5.0])
    ok = H.copy()
    ok[1, 2] = ok[2, 1] = 0.5 * np.sqrt(H[1, 1] * H[2, 2])
    neg = ok.copy()
    neg[3, 3] = -1.0
    got = _run_host(host_program, [(H, 15, J, 0.3), (ok, 15, J, 0.3), (neg, 15, J, 0.3), (neg, 7, J, 0.3),
                                   (ok, 0, J, 0.3)])
    assert int(got[0, 7]) == 15 and np.isnan(got[0, :7]).all()  # pivot below the limit
    assert int(got[1, 7]) == 31 and np.isfinite(got[1, :7]).all()
    assert int(got[2, 7]) == 15 and np.isnan(got[2, :7]).all()  # a free H_jj <= 0
    assert int(got[3, 7]) == 7 + 16 and got[3, 3] == 0.0  # ... not when that coordinate is held
    assert int(got[4, 7]) == 0 and np.isnan(got[4, :7]).all()  # nothing free


# --------------------------------------------------------------------------
# the reference means something: Laplace std vs the oracle's NUTS spread
# --------------------------------------------------------------------------
def test_reference_vs_nuts_posterior_std(oracle_lib):
    """16 deep ancient taxa: the Laplace D_max and phi standard errors over the
    std of a 500 + 1000 oracle chain lie in [0.7, 1.3] (measured 0.83-1.03 and
    0.93-1.09; the band leaves ~15 % for the Monte-Carlo error of a 1000-draw std)."""
    from metadamage_amd.synthetic import generate

    b = generate(400, seed=21)
    deep = np.flatnonzero(b.truth["ancient"] & (b.N[:, :30].mean(axis=1) > 3e3))[:16]
    assert deep.size == 16
    out, _, st = oracle_lib.fit_batch(b.y[deep], b.N[deep])
    assert (st == 0).all()
    ratios = []
    for i, t in enumerate(deep):
        lap, _, _ = ref.laplace_taxon(oracle_lib, b.y[t, :30], b.N[t, :30], out[i], 0)
        assert int(lap[0, 7]) & ref.VALID
        smp, _, rc = oracle_lib.nuts_chain(0, 0, b.y[t, :30], b.N[t, :30], seed=0, g=int(t), sub=0,
                                           num_warmup=500, num_samples=1000)
        assert rc == 0
        ratios.append((lap[0, 4] / np.std(smp[:, 1] + smp[:, 2]), lap[0, 3] / np.std(smp[:, 3])))
    ratios = np.array(ratios)
    print("Laplace / NUTS std: D_max %.2f-%.2f, phi %.2f-%.2f" % (ratios[:, 0].min(), ratios[:, 0].max(),
                                                                   ratios[:, 1].min(), ratios[:, 1].max()))
    assert (ratios >= 0.7).all() and (ratios <= 1.3).all(), ratios


# --------------------------------------------------------------------------
# frames, options, CLI, gather record
# --------------------------------------------------------------------------
NEW_COLUMNS = ["D_max_std", "significance", "q_std", "A_std", "c_std", "concentration_std", "rho_Ac",
               "D_max_std_forward", "q_std_forward", "D_max_std_reverse", "q_std_reverse", "laplace_valid"]


def _cfg(tmp_path, inference="map-laplace"):
    from metadamage_amd import utils

    cfg = utils.Config(out_dir=tmp_path, max_fits=10, max_cores=1, min_alignments=10, min_y_sum=10,
                       substitution_bases_forward="CT", substitution_bases_reverse="GA", forced=False,
                       version="0.0.0", inference=inference)
    cfg.add_filename(GOLDEN / "data_ancient.txt")
    return cfg


def test_frame_columns_and_dtypes(tmp_path, oracle_lib, ref_meta):
    from metadamage_amd import _lib, fits

    cfg = _cfg(tmp_path)
    p = fits.pack_counts(pd.read_parquet(GOLDEN / "counts_data_ancient.parquet"), cfg)
    out, pred, st = oracle_lib.fit_batch(p.y, p.N, p.mm)
    lap, _ = ref.laplace_batch(oracle_lib, p.y, p.N, out, st)
    lap32 = lap.astype(np.float32)
    keep = st == 0
    plain = fits.make_df_fit_results(p, out, keep, cfg)
    plain_none = fits.make_df_fit_results(p, out, keep, cfg, lap=None)
    pd.testing.assert_frame_equal(plain, plain_none)
    assert list(plain.columns) == ref_meta["fit_results_columns"] and len(plain.columns) == 30
    df = fits.make_df_fit_results(p, out, keep, cfg, lap=lap32)
    assert list(df.columns) == ref_meta["fit_results_columns"] + NEW_COLUMNS and len(df.columns) == 42
    pd.testing.assert_frame_equal(df[plain.columns], plain)
    for c in NEW_COLUMNS[:-1]:
        assert df[c].dtype == np.float32, c
    assert df["laplace_valid"].dtype == np.uint32
    f = _lib.LAPLACE_FIELDS.index
    np.testing.assert_array_equal(df["D_max_std"].to_numpy(), lap32[keep, 0, f("D_max_std")])
    np.testing.assert_array_equal(df["significance"].to_numpy(), lap32[keep, 0, f("significance")])
    np.testing.assert_array_equal(df["concentration_std"].to_numpy(), lap32[keep, 0, f("phi_std")])
    np.testing.assert_array_equal(df["rho_Ac"].to_numpy(), lap32[keep, 0, f("rho_Ac")])
    np.testing.assert_array_equal(df["q_std_forward"].to_numpy(), lap32[keep, 1, f("q_std")])
    np.testing.assert_array_equal(df["D_max_std_reverse"].to_numpy(), lap32[keep, 2, f("D_max_std")])
    np.testing.assert_array_equal(df["laplace_valid"].to_numpy(),
                                  ((lap[keep, 0, 7].astype(int) & 16) != 0).astype(np.uint32))
    assert (df["laplace_valid"] == 1).all() and (df["D_max_std"] > 0).all()
    # a dropped taxon takes its Laplace row with it
    k2 = np.array([True, False, True])
    d2 = fits.make_df_fit_results(p, out, k2, cfg, lap=lap32)
    np.testing.assert_array_equal(d2["q_std"].to_numpy(), lap32[k2, 0, 0])


def test_make_opts_and_cli(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import _lib, fits
    from metadamage_amd.cli import cli_app

    o = fits.make_opts(_cfg(tmp_path, "map-laplace"))
    m = fits.make_opts(_cfg(tmp_path, "map"))
    assert o.mode == _lib.MODE_MAP and bytes(o) == bytes(m)
    assert fits.wants_laplace(_cfg(tmp_path, "map-laplace")) and not fits.wants_laplace(_cfg(tmp_path, "map"))
    with pytest.raises(ValueError):
        fits.make_opts(_cfg(tmp_path, "map-foo"))
    assert "inference" in fits.CACHE_KEYS
    bad = CliRunner().invoke(cli_app, ["fit", str(GOLDEN / "data_ancient.txt"), "--out-dir", str(tmp_path),
                                       "--inference", "map-foo"])
    assert bad.exit_code == 2 and "map-laplace" in bad.output


def test_gather_record_with_laplace_round_trips():
    import torch

    from metadamage_amd import _lib, distributed as d

    assert d.REC_BYTES == 8 * 8 + 17 * 4 + 360 + 4 == 496  # unchanged
    assert d.REC_LAP == 96
    n = 7
    rng = np.random.default_rng(2)
    buf = torch.from_numpy(rng.integers(0, 256, n * (d.REC_BYTES + d.REC_LAP), dtype=np.uint8))
    pred, status, ints, floats, lap = d.packed_views(buf, n, with_laplace=True)
    p0, s0, i0, f0 = d.packed_views(buf[: n * d.REC_BYTES], n)  # the default layout is a prefix
    assert pred.data_ptr() == p0.data_ptr() and status.data_ptr() == s0.data_ptr()
    assert ints.data_ptr() == i0.data_ptr() and floats.data_ptr() == f0.data_ptr()
    assert lap.shape == (n, 3, _lib.NLAPLACE) and lap.dtype == torch.float32
    assert lap.data_ptr() == buf.data_ptr() + n * d.REC_BYTES
    want = {k: rng.standard_normal(tuple(v.shape)).astype(v.numpy().dtype) for k, v in
            (("pred", pred), ("ints", ints), ("floats", floats), ("lap", lap))}
    want["lap"][0, 1, 5] = np.nan
    want["ints"] = np.rint(want["ints"] * 100)
    st = rng.integers(0, 4, n).astype(np.int32)
    pred.copy_(torch.from_numpy(want["pred"]))
    ints.copy_(torch.from_numpy(want["ints"]))
    floats.copy_(torch.from_numpy(want["floats"]))
    lap.copy_(torch.from_numpy(want["lap"]))
    status.copy_(torch.from_numpy(st))
    # two ranks, 7 + 6 taxa: the second part's last record is padding
    out, pr, ss, lp = d.unpack_gathered([buf, buf.clone()], 13, 2, with_laplace=True)
    assert out.shape == (13, 25) and lp.shape == (13, 3, 8) and lp.dtype == np.float32
    np.testing.assert_array_equal(lp[:7], want["lap"])
    np.testing.assert_array_equal(lp[7:], want["lap"][:6])
    np.testing.assert_array_equal(pr[:7], want["pred"])
    np.testing.assert_array_equal(ss[7:], st[:6])
    np.testing.assert_array_equal(out[:7, d.INT_LO:d.INT_HI], want["ints"])
    np.testing.assert_array_equal(out[:7][:, d.FLOAT_COLS], want["floats"].astype(np.float64))
    o3 = d.unpack_gathered([buf[: n * d.REC_BYTES]], 7, 1)
    assert len(o3) == 3
    np.testing.assert_array_equal(o3[0], out[:7])
