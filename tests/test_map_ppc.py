"""CPU tests of the posterior predictive check (MDFIT-PPC v1):
the layout constants against include/mdfit.h, the record on hand-made counts,
the calibration and the power of the specification on the numpy reference
(tests/map_ppc_ref.py), and the gather-record / frames / options / CLI
plumbing."""

from __future__ import annotations

import re
import subprocess
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from tests import map_ppc_ref as ref
from tests.helpers import GOLDEN

ROOT = Path(__file__).resolve().parents[1]


# --------------------------------------------------------------------------
# layout
# --------------------------------------------------------------------------
def test_layout_constants_match_the_header():
    from metadamage_amd import _lib, distributed as d, engine

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mdfit.h").read_text(), flags=re.S)
    assert re.search(r"#define MDFIT_NMAPPPC\s+12\b", text) and _lib.NMAPPPC == 12 == ref.NFIELD
    for name, val in (("VALID", 1), ("RELIABLE", 2), ("NONCOUNT", 8)):
        assert re.search(rf"#define MDFIT_PPC_{name}\s+{val}\b", text), name
    assert (_lib.MAPPPC_VALID, _lib.MAPPPC_RELIABLE, _lib.MAPPPC_NONCOUNT) == (ref.VALID, ref.RELIABLE, ref.NONCOUNT)
    assert _lib.MAPPSIS_ADAPTED == ref.ADAPTED
    assert _lib.MAPPPC_FIELDS == ref.FIELDS and len(_lib.MAPPPC_FIELDS) == _lib.NMAPPPC
    assert re.search(r"#define MDFIT_ABI_VERSION\s+3\b", text)  # entries are added, none changes
    for sym in ("mdfit_map_ppc", "mdfit_map_ppc_adapt"):
        assert re.search(rf"\bint\s+{sym}\s*\(", text) and sym in _lib.EXPORTED_SYMBOLS
    assert _lib.NPPCOUT == 42 and d.REC_PPC == 168 == engine.PPC_BYTES
    lib = _lib.load()
    for fn, n in ((lib.mdfit_map_ppc, 15), (lib.mdfit_map_ppc_adapt, 17)):
        assert len(fn.argtypes) == n
    # the argument checks need no device
    none = [None] * 6
    assert lib.mdfit_map_ppc(None, None, None, None, -1, 256, 1000, 0, 0, *none) == -1
    assert b"n_taxa" in lib.mdfit_last_error()
    for S in (24, 1025):
        assert lib.mdfit_map_ppc(None, None, None, None, 0, S, 1000, 0, 0, *none) == -1
        assert b"num_draws must be in [25, 1024]" in lib.mdfit_last_error()
    for R in (24, 1025):
        assert lib.mdfit_map_ppc_adapt(None, None, None, None, 0, 256, R, 0, 0, 0, None, *none) == -1
        assert b"num_pred must be in [25, 1024]" in lib.mdfit_last_error()
    assert lib.mdfit_map_ppc_adapt(None, None, None, None, 0, 256, 1000, 5, 0, 0, None, *none) == -1
    assert b"adapt_rounds" in lib.mdfit_last_error()
    assert lib.mdfit_map_ppc(None, None, None, None, 0, 256, 1000, 0, 0, *none) == 0
    assert lib.mdfit_map_ppc(None, None, None, None, 1, 256, 1000, 0, 0, *none) == -1
    assert b"null" in lib.mdfit_last_error()


# --------------------------------------------------------------------------
# the record on hand-made counts
# --------------------------------------------------------------------------
def _theta(R, q=0.3, A=0.2, c=0.01, phi=500.0):
    return np.tile(np.array([q, A, c, phi]), (R, 1))


def _record(y, N, counts, R, theta=None, khat=0.3, S=256):
    from tests import map_psis_ref as pref

    theta = _theta(R) if theta is None else theta
    disc, _ = ref.discrepancies(theta, y, N, counts)
    gt, eq, live, nonc = ref.column_counts(y, N, counts)
    rec, ppos = ref.record_from(disc, gt, eq, live, nonc, R, khat, 100.0, 50, pref.khat_threshold(S))
    return rec, ppos, disc


def test_handmade_records():
    R = 40
    N = np.full(30, 1000, np.int64)
    y = (N * (0.2 * 0.7 ** (np.arange(30) % 15) + 0.01)).astype(np.int64)
    # every replicate equals the data: mid-p 0.5 everywhere, the replicated discrepancy ties the observed one
    same = np.tile(y[:, None], (1, R)).astype(np.uint32)
    rec, ppos, disc = _record(y, N, same, R)
    assert (ppos == 0.5).all() and rec[ref.P_OUT] == 1.0 and rec[ref.P_STR] == 1.0
    assert np.array_equal(disc[:, 0], disc[:, 1]) and np.array_equal(disc[:, 2], disc[:, 3])
    assert rec[ref.P_WORST] == 1.0 and rec[ref.WORST] == 0 and rec[ref.N_LOW] == 0 and rec[ref.N_POINTS] == 30
    assert int(rec[ref.FLAGS]) == ref.VALID | ref.RELIABLE
    assert rec[ref.T_OUT] == disc[0, 0] and rec[ref.T_STR] == disc[0, 2]
    # a strand without a column: p_strand is NaN, everything else stands
    N1 = N.copy()
    N1[15:] = 0
    rec1, ppos1, _ = _record(y, N1, same, R)
    assert np.isnan(rec1[ref.P_STR]) and rec1[ref.P_OUT] == 1.0 and rec1[ref.N_POINTS] == 15
    assert (ppos1[:15] == 0.5).all() and np.isnan(ppos1[15:]).all() and int(rec1[ref.FLAGS]) & ref.VALID
    # one column without reads
    N2 = N.copy()
    N2[7] = 0
    rec2, ppos2, _ = _record(y, N2, same, R)
    assert np.isnan(ppos2[7]) and rec2[ref.N_POINTS] == 29 and np.isfinite(rec2[ref.P_STR])
    # the upper mid-p and the tie rule of worst_pos: columns 3 and 20 equally far out, on opposite sides
    c = same.copy()
    c[3] = y[3] + 5  # every replicate above: p = 1, two-sided 0
    c[20] = y[20] - 5  # every replicate below: p = 0, two-sided 0
    c[9, : R // 4] = y[9] + 1  # a quarter above, the rest equal: p = (2 * 10 + 30) / 80
    rec3, ppos3, _ = _record(y, N, c, R)
    assert ppos3[3] == 1.0 and ppos3[20] == 0.0 and ppos3[9] == np.float32(50.0 / 80.0)
    assert rec3[ref.WORST] == 3 and rec3[ref.P_WORST] == 0.0 and rec3[ref.N_LOW] == 2
    c[3] = same[3]
    rec4, _, _ = _record(y, N, c, R)
    assert rec4[ref.WORST] == 20 and rec4[ref.N_LOW] == 1
    # p_outlier and p_strand are counts over R: half the replicates carry a spike, a quarter a strand shift
    c = same.copy()
    c[5, : R // 2] += 200
    rec5, _, disc5 = _record(y, N, c, R)
    assert rec5[ref.P_OUT] == 1.0  # (a spike only raises the replicated maximum)
    ys = y.copy()
    ys[5] += 200
    rec6, _, _ = _record(ys, N, c, R)
    assert rec6[ref.P_OUT] == 0.5 and rec6[ref.T_OUT] > 10
    c = same.copy()
    c[:15, : R // 4] += 30
    ysh = y.copy()
    ysh[:15] += 30
    rec7, _, _ = _record(ysh, N, c, R)
    assert rec7[ref.P_STR] == 0.25 and rec7[ref.T_STR] > 0
    ysh[:15] -= 60
    assert _record(ysh, N, c, R)[0][ref.T_STR] < 0  # t_strand is signed, p_strand two-sided
    # a replicated draw that is no count: the p-values are NaN, the valid bit is clear, bit 3 is set
    c = same.copy()
    c[4, 2] = ref.NO_COUNT
    rec8, ppos8, _ = _record(y, N, c, R)
    assert int(rec8[ref.FLAGS]) == ref.RELIABLE | ref.NONCOUNT and np.isnan(ppos8).all()
    assert np.isnan(rec8[[ref.P_OUT, ref.P_STR, ref.WORST, ref.P_WORST, ref.N_LOW]]).all()
    assert np.isfinite(rec8[[ref.T_OUT, ref.T_STR, ref.N_POINTS]]).all()
    # khat over the threshold: valid, not reliable
    assert int(_record(y, N, same, R, khat=0.9)[0][ref.FLAGS]) == ref.VALID
    # a column whose variance is not positive (D clamps to 0) is skipped on both sides
    th = _theta(R, A=0.0, c=0.0)
    assert (ref.discrepancies(th, y, N, same)[0] == 0).all()
    inv = ref.invalid_taxon(R)
    assert inv["rec"][ref.FLAGS] == 0 and np.isnan(inv["rec"][:11]).all() and (inv["index"] == -1).all()


# --------------------------------------------------------------------------
# the host build of the per-column part (csrc/mdfit_mapppc.h: mid_p, worst_position)
# --------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(tmp_path_factory, request):
    exe = tmp_path_factory.mktemp("mapppc_host") / f"mapppc_host_{request.param}"
    flags = ["-O1", "-g"] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                             if request.param == "sanitized" else [])
    subprocess.run(["g++", "-std=c++17", *flags, str(ROOT / "tests" / "mapppc_host_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def test_host_worst_position_equals_reference(host_program, tmp_path):
    rng = np.random.default_rng(3)
    items = []
    for R in (25, 100, 1000, 1024):
        for kind in range(6):
            live = np.ones(30, bool)
            gt = rng.integers(0, R + 1, 30)
            if kind == 1:  # columns without reads, the first among them
                live[[0, 7, 29]] = False
            if kind == 2:  # no column at all
                live[:] = False
            if kind == 3:  # ties at the smallest value, on both sides
                gt[:] = R // 2
                gt[[5, 12]] = 0
                gt[21] = R
            if kind == 4:  # every replicate equal to the data
                gt[:] = 0
            eq = rng.integers(0, R - gt + 1) if kind not in (3, 4) else np.where(gt == R // 2, R - 2 * (R // 2), 0)
            if kind == 4:
                eq = np.full(30, R)
            if kind == 5:  # values on both sides of the 0.05 bar
                gt = rng.integers(0, max(R // 20, 2), 30)
                eq = rng.integers(0, 3, 30)
            items.append((R, live, gt.astype(np.int64), np.asarray(eq, np.int64)))
    lines = [str(len(items))]
    for R, live, gt, eq in items:
        lines += [str(R), " ".join(f"{int(h)} {int(g)} {int(e)}" for h, g, e in zip(live, gt, eq))]
    src = tmp_path / "items.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(host_program), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = r.stdout.strip().splitlines()
    assert len(got) == len(items)
    disc = np.zeros((1, 4))
    for (R, live, gt, eq), ln in zip(items, got):
        tok = ln.split()
        p = np.array([float.fromhex(t) if t not in ("nan", "-nan") else np.nan for t in tok[:30]])
        worst, p_worst, n_low, n_points = int(tok[30]), *(float.fromhex(t) if "nan" not in t else np.nan
                                                          for t in tok[31:])
        want, wpos = ref.record_from(disc, gt, eq, live, False, R, 0.1, 1.0, 1, 0.7)
        assert np.array_equal(p.astype(np.float32), wpos, equal_nan=True), (R, p, wpos)
        assert n_points == want[ref.N_POINTS] and n_low == want[ref.N_LOW]
        if live.any():
            assert worst == want[ref.WORST] and p_worst == want[ref.P_WORST], (R, worst, want)
        else:
            assert worst == -1 and np.isnan(p_worst) and np.isnan(want[ref.WORST])


# --------------------------------------------------------------------------
# calibration and power of the specification (on the reference alone)
# --------------------------------------------------------------------------
S_CAL, R_CAL, T_CAL = 256, 1000, 60


def _reference_batch(oracle_lib, y, N, mm):
    out, _pred, st = oracle_lib.fit_batch(y, N, mm)
    res = [ref.ppc_taxon(oracle_lib, y[t, :30], N[t, :30], out[t], int(st[t]), S_CAL, R_CAL, seed=0, g=t)
           for t in range(len(y))]
    rec = np.stack([r["rec"] for r in res])
    ppos = np.stack([r["ppos"] for r in res])
    return rec, ppos, (rec[:, ref.FLAGS].astype(int) & ref.VALID) != 0


def test_calibration_and_power_of_the_specification(oracle_lib):
    from metadamage_amd.synthetic import generate

    b = generate(300, seed=21)
    y0, N, mm = b.y[:T_CAL].copy(), b.N[:T_CAL].copy(), b.mm[:T_CAL].copy()
    rec, _, valid = _reference_batch(oracle_lib, y0, N, mm)
    print(f"clean: {int(valid.sum())} valid of {T_CAL}; min p_outlier {np.nanmin(rec[valid, ref.P_OUT]):.4f}, "
          f"min p_strand {np.nanmin(rec[valid, ref.P_STR]):.4f}")
    assert valid.sum() >= 50
    assert not (rec[valid, ref.P_OUT] < 0.01).any()
    assert not (rec[valid, ref.P_STR] < 0.01).any()
    # a tripled count at one position
    y = y0.copy()
    y[:, 4] = np.minimum(N[:, 4].astype(np.int64), 3 * y[:, 4].astype(np.int64) + 30).astype(np.uint32)
    rec, ppos, valid = _reference_batch(oracle_lib, y, N, mm)
    n_out = int((rec[valid, ref.P_OUT] < 0.01).sum())
    med = float(np.nanmedian(ppos[valid, 4]))
    print(f"spike at column 4: {int(valid.sum())} valid; p_outlier < 0.01 on {n_out}, median ppc_p there {med:.4f}, "
          f"worst_pos == 4 on {int((rec[valid, ref.WORST] == 4).sum())}; "
          f"(diagnostic) p_strand < 0.01 on {int((rec[valid, ref.P_STR] < 0.01).sum())}")
    assert n_out >= 15
    assert med < 0.02
    # the reverse strand's counts cut to a third
    y = y0.copy()
    y[:, 15:30] //= 3
    rec, _, valid = _reference_batch(oracle_lib, y, N, mm)
    n_str = int((rec[valid, ref.P_STR] < 0.01).sum())
    print(f"reverse strand // 3: {int(valid.sum())} valid; p_strand < 0.01 on {n_str}; "
          f"(diagnostic) p_outlier < 0.01 on {int((rec[valid, ref.P_OUT] < 0.01).sum())}")
    assert n_str >= 30


# --------------------------------------------------------------------------
# the gather record
# --------------------------------------------------------------------------
def test_gather_record_carries_the_ppc_tail():
    import torch

    from metadamage_amd import distributed as d

    n = 7
    today = d.alloc_records(n, "cpu", with_ppred=True, with_ppred_adapt=True)
    assert today.ppc is None and today.buf.numel() == n * (d.REC_BYTES + 424 + 8) and d.REC_PPRED == 424
    rec = d.alloc_records(n, "cpu", with_ppred=True, with_ppc=True, with_ppred_adapt=True)
    assert rec.buf.numel() == today.buf.numel() + n * 168
    assert rec.ppc.shape == (n, 42) and rec.ppc.dtype == torch.float32
    p0 = rec.buf.data_ptr()
    assert rec.ppred.data_ptr() == p0 + n * d.REC_BYTES
    assert rec.ppc.data_ptr() == p0 + n * (d.REC_BYTES + 424)  # directly behind the ppred block ...
    assert rec.adapt.data_ptr() == p0 + n * (d.REC_BYTES + 424 + 168)  # ... and before the adapt tail
    only = d.alloc_records(n, "cpu", with_ppred=True, with_ppc=True)
    assert only.adapt is None and only.buf.numel() == n * (d.REC_BYTES + 424 + 168)
    for kw in ({}, *({b.switch: True} for b in d.blocks.BLOCKS if b.name != "ppred")):
        with pytest.raises(ValueError, match="with_ppc goes with with_ppred"):
            d.alloc_records(n, "cpu", with_ppc=True, **kw)
    rng = np.random.default_rng(11)
    for with_adapt in (True, False):
        r = d.alloc_records(n, "cpu", with_ppred=True, with_ppc=True, with_ppred_adapt=with_adapt)
        r.buf.copy_(torch.from_numpy(rng.integers(0, 256, r.buf.numel(), dtype=np.uint8)))
        r.floats.zero_()  # (random bytes there can be signalling NaN, which numpy's f32 -> f64 cast warns about)
        want_pp = rng.standard_normal((n, 106)).astype(np.float32)
        want_pc = rng.standard_normal((n, 42)).astype(np.float32)
        want_pc[2] = np.nan
        want_ad = rng.standard_normal((n, 2)).astype(np.float32)
        r.ppred.copy_(torch.from_numpy(want_pp))
        r.ppc.copy_(torch.from_numpy(want_pc))
        if with_adapt:
            r.adapt.copy_(torch.from_numpy(want_ad))
        got = d.unpack_gathered([r.buf, r.buf.clone()], 13, 2, with_ppred=True, with_ppc=True,
                                with_ppred_adapt=with_adapt)
        assert len(got) == (6 if with_adapt else 5)
        np.testing.assert_array_equal(got[3], np.concatenate([want_pp, want_pp[:6]]))
        np.testing.assert_array_equal(got[4], np.concatenate([want_pc, want_pc[:6]]))
        if with_adapt:
            np.testing.assert_array_equal(got[5], np.concatenate([want_ad, want_ad[:6]]))


def test_plan_counts_the_check():
    from metadamage_amd import _lib, engine

    opts = _lib.default_opts(mode=_lib.MODE_MAP)
    a = engine.device_bytes(100, opts, with_ppred=True)
    assert engine.device_bytes(100, opts, with_ppred=True, ppc=True) - a == 100 * (30 * 4 + 12 * 8 + 168)
    assert engine.device_bytes(100, opts, with_ppred=True, ppc=True, dest_on_device=True) \
        - engine.device_bytes(100, opts, with_ppred=True, dest_on_device=True) == 100 * (30 * 4 + 12 * 8)
    assert engine.device_bytes(100, opts, with_ppred=True, ppc=False) == a
    budget = 2 * engine.device_bytes(50, opts, with_ppred=True)
    assert max(hi - lo for lo, hi in engine.plan_chunks(200, opts, budget, with_ppred=True)) == 50
    assert max(hi - lo for lo, hi in engine.plan_chunks(200, opts, budget, with_ppred=True, ppc=True)) < 50
    for kw in ({}, {"with_psis": True}, {"with_laplace": True}):
        with pytest.raises(ValueError, match="ppc needs with_ppred"):
            engine.device_bytes(10, opts, ppc=True, **kw)
        with pytest.raises(ValueError, match="ppc needs with_ppred"):
            engine.plan_chunks(10, opts, ppc=True, **kw)
    blk = np.arange(3 * 42, dtype=np.float32).reshape(3, 42)
    ppos, rec = engine.split_ppc(blk)
    assert ppos.shape == (3, 30) and rec.shape == (3, 12) and rec[0, 0] == 30


# --------------------------------------------------------------------------
# options, cache key, CLI
# --------------------------------------------------------------------------
def _cfg(tmp_path, inference="map-pred", **kw):
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

    assert utils.Config.__dataclass_fields__["ppc"].default is False
    for inference in ("map-pred", "auto", "map", "nuts"):
        d0 = _cfg(tmp_path, inference).to_dict()
        assert "ppc" not in d0 and not fits.ppc_of(_cfg(tmp_path, inference))
        assert _cfg(tmp_path, inference, ppc=False).to_dict() == d0  # the metadata of a run without it: today's
    d0 = _cfg(tmp_path).to_dict()
    d1 = _cfg(tmp_path, ppc=True).to_dict()
    assert d1["ppc"] is True and fits.ppc_of(_cfg(tmp_path, ppc=True))
    assert {k: v for k, v in d1.items() if k != "ppc"} == d0
    assert "ppc" in fits.CACHE_KEYS
    sim = utils.metadata_is_similar
    assert sim(d0, dict(d0), include=fits.CACHE_KEYS) and sim(d1, dict(d1), include=fits.CACHE_KEYS)
    assert not sim(d0, d1, include=fits.CACHE_KEYS) and not sim(d1, d0, include=fits.CACHE_KEYS)
    for inference in ("map", "nuts", "auto", "map-psis", "map-waic", "map-evidence"):
        with pytest.raises(ValueError, match="ppc goes with inference 'map-pred'"):
            _cfg(tmp_path, inference, ppc=True)
    runner = CliRunner()
    base = ["fit", str(GOLDEN / "data_ancient.txt"), "--out-dir", str(tmp_path)]
    for inference in ("map", "nuts", "auto", "map-psis", "map-waic"):
        bad = runner.invoke(cli_app, base + ["--inference", inference, "--ppc"])
        assert bad.exit_code == 2 and "--ppc" in bad.output, inference
    assert "--ppc" in runner.invoke(cli_app, ["fit", "--help"], terminal_width=200).output


# --------------------------------------------------------------------------
# frames
# --------------------------------------------------------------------------
def test_frames_from_a_synthetic_tail(tmp_path, oracle_lib, ref_meta):
    from metadamage_amd import _lib, fits

    cfg = _cfg(tmp_path, ppc=True)
    p = fits.pack_counts(pd.read_parquet(GOLDEN / "counts_data_ancient.parquet"), cfg)
    out, pred, st = oracle_lib.fit_batch(p.y, p.N, p.mm)
    keep = st == 0
    assert keep.all() and len(keep) == 3
    f = _lib.MAPPPC_FIELDS.index
    ppc = np.zeros((3, 42), np.float32)
    ppc[:, :30] = np.linspace(0.0, 1.0, 90, dtype=np.float32).reshape(3, 30)
    ppc[0, 30:] = [0.25, 0.5, 3.5, -1.25, 0, 0.125, 2, 30, 0.3, 120.0, 80, 3]
    ppc[1, 30:] = [0.001, 0.75, 40.0, 2.5, 19, 0.002, 1, 29, 0.8, 30.0, 12, 1 | 64]
    ppc[2, 30:] = np.nan
    ppc[2, 30 + f("flags")] = 0
    ppc[2, :30] = np.nan
    ppred = np.zeros((3, 106), np.float32)
    adapt = np.array([[0.71, 2.0], [0.2, 0.0], [np.nan, np.nan]], dtype=np.float32)
    base = ref_meta["fit_results_columns"]
    today = fits.make_df_fit_results(p, out, keep, cfg, ppred=ppred)
    df = fits.make_df_fit_results(p, out, keep, cfg, ppred=ppred, ppc=ppc)
    assert fits.PPC_COLUMNS == ["ppc_p_outlier", "ppc_p_strand", "ppc_t_outlier", "ppc_t_strand", "ppc_worst_position",
                                "ppc_p_worst", "ppc_n_low", "ppc_valid"]
    assert list(df.columns) == base + fits.MAP_PRED_COLUMNS + fits.MAP_PRED_UINT_COLUMNS + fits.PPC_COLUMNS
    pd.testing.assert_frame_equal(df[today.columns], today)  # no column is renamed or moved
    for c in ("ppc_p_outlier", "ppc_p_strand", "ppc_t_outlier", "ppc_t_strand", "ppc_p_worst"):
        assert df[c].dtype == np.float32, c
    assert df["ppc_worst_position"].dtype == np.int8 and df["ppc_n_low"].dtype == np.uint8
    assert df["ppc_valid"].dtype == bool
    np.testing.assert_array_equal(df["ppc_p_outlier"].to_numpy(), ppc[:, 30])
    np.testing.assert_array_equal(df["ppc_t_strand"].to_numpy(), ppc[:, 33])
    assert df["ppc_worst_position"].tolist() == [1, -5, 0]  # column 0: z = +1; column 19: z = -5; none: 0
    assert df["ppc_n_low"].tolist() == [2, 1, 0] and df["ppc_valid"].tolist() == [True, True, False]
    both = fits.make_df_fit_results(p, out, keep, cfg, ppred=ppred, ppc=ppc, adapt=adapt)
    assert list(both.columns) == list(df.columns) + fits.ADAPT_COLUMNS  # the adapt columns stay last
    d2 = fits.make_df_fit_results(p, out, np.array([True, False, True]), cfg, ppred=ppred, ppc=ppc)
    assert d2["ppc_worst_position"].tolist() == [1, 0] and d2["ppc_valid"].tolist() == [True, False]
    pa = fits.make_df_fit_predictions(p, pred, keep, cfg, ppred=ppred)
    pb = fits.make_df_fit_predictions(p, pred, keep, cfg, ppred=ppred, ppc=ppc)
    assert list(pb.columns) == list(pa.columns) + fits.PPC_PREDICTION_COLUMNS == list(pa.columns) + ["ppc_p"]
    pd.testing.assert_frame_equal(pb[pa.columns], pa)
    assert pb["ppc_p"].dtype == np.float32
    np.testing.assert_array_equal(pb["ppc_p"].to_numpy(), ppc[:, :30].reshape(-1))
    assert pb["position"].tolist()[:30] == list(range(1, 16)) + list(range(-1, -16, -1))
    pc = fits.make_df_fit_predictions(p, pred, np.array([False, True, True]), cfg, ppred=ppred, ppc=ppc)
    np.testing.assert_array_equal(pc["ppc_p"].to_numpy(), ppc[1:, :30].reshape(-1))
    # the optional arrays behind (out, pred, status): the check rides directly behind the ppred block
    x, a = object(), object()
    assert fits._split_rest(_cfg(tmp_path, ppc=True, psis_adapt=2), [x, a]) == (x, None, a)
