"""CPU tests of the moment-matched proposal rounds of the MAP importance
sampling (MDFIT-ADAPT v1): the C-ABI entry points without a
device, the rule's effect on generate(300, 21) and its accuracy against the
oracle's NUTS posterior through the reference (tests/map_adapt_ref.py), the
host build of the refit (csrc/mdfit_mapadapt.h, one-lane policy) on crafted
series, and the frames / options / CLI / gather-record plumbing."""

from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import map_adapt_cases as cases
from tests import map_adapt_ref as ad
from tests import map_psis_ref as ref

ROOT = Path(__file__).resolve().parents[1]

S_A, R_A, SEED = 256, 3, 0
# the host program against the reference over every series of map_adapt_cases,
# measured (m absolute over max(1, |m|) 1.9e-15, d relative 1.1e-15, F absolute
# 4.7e-13 -- a correlation matrix of condition ~1e3 at S = 1024 --, the rate
# relative 1.5e-15), times ten
HOST_TOL = {"m": 1.9e-14, "d": 1.1e-14, "F": 4.7e-12, "gc": 1.5e-14}


# --------------------------------------------------------------------------
# ABI
# --------------------------------------------------------------------------
def test_entry_points_declared_exported_and_argument_checked():
    from metadamage_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mdfit.h").read_text(), flags=re.S)
    names = ("mdfit_map_psis_adapt", "mdfit_map_waic_adapt", "mdfit_adapt_proposal")
    for name in names:
        assert re.search(rf"\bint\s+{name}\s*\(", text) and name in _lib.EXPORTED_SYMBOLS
    assert f"#define MDFIT_NMAPADAPT {_lib.NMAPADAPT}" in text and len(_lib.MAPADAPT_FIELDS) == _lib.NMAPADAPT == 4
    assert f"#define MDFIT_FLAG_ADAPTED {_lib.MAPPSIS_ADAPTED}" in text and _lib.MAPPSIS_ADAPTED == ad.ADAPTED == 64
    assert f"#define MDFIT_ADAPT_MAX_ROUNDS {_lib.ADAPT_MAX_ROUNDS}" in text and _lib.ADAPT_MAX_ROUNDS == ad.MAX_ROUNDS
    assert f"#define MDFIT_ABI_VERSION {_lib.ABI_VERSION}" in text and _lib.ABI_VERSION == 3
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                        check=True).stdout
    for name in names:
        assert re.search(rf"\bT {name}\b", nm)
    dummy = ctypes.c_void_p(16)
    assert lib.mdfit_map_psis_adapt(None, None, None, None, 0, 256, 3, 0, 0, None, None, None, None) == 0
    assert lib.mdfit_map_waic_adapt(None, None, None, None, 0, 256, 3, 0, 0, None, None, None, None, None) == 0
    for R in (-1, 5):
        assert lib.mdfit_map_psis_adapt(dummy, dummy, dummy, dummy, 1, 256, R, 0, 0, dummy, None, None, None) == -1
        assert b"adapt_rounds" in lib.mdfit_last_error()
        assert lib.mdfit_map_waic_adapt(dummy, dummy, dummy, dummy, 1, 256, R, 0, 0, dummy, None, None, None,
                                        None) == -1
        assert b"adapt_rounds" in lib.mdfit_last_error()
    for S in (24, 1025):
        assert lib.mdfit_map_psis_adapt(dummy, dummy, dummy, dummy, 1, S, 3, 0, 0, dummy, None, None, None) == -1
        assert b"num_draws" in lib.mdfit_last_error()
        assert lib.mdfit_adapt_proposal(dummy, dummy, dummy, dummy, dummy, 1, S, dummy, dummy, None) == -1
    assert lib.mdfit_map_psis_adapt(dummy, dummy, dummy, dummy, 1, 256, 3, 0, 0, None, None, None, None) == -1
    assert lib.mdfit_map_waic_adapt(dummy, dummy, dummy, dummy, 1, 256, 3, 0, 0, None, None, None, None, None) == -1
    assert lib.mdfit_adapt_proposal(None, None, None, None, None, 0, 256, None, None, None) == 0
    assert lib.mdfit_adapt_proposal(dummy, dummy, dummy, dummy, dummy, 1, 256, None, dummy, None) == -1


# --------------------------------------------------------------------------
# the rule, through the reference
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch_ref(oracle_lib):
    """generate(300, 21) fitted by the oracle, every PMD row through the
    reference's rounds at S = 256, R = 3, seed 0 (computed once, read only)."""
    from metadamage_amd.synthetic import generate

    b = generate(300, seed=21)
    out, _, st = oracle_lib.fit_batch(b.y, b.N)
    rows = [ad.adapt_taxon(oracle_lib, b.y[t, :30], b.N[t, :30], out[t], int(st[t]), S_A, R_A, seed=SEED, g=t)
            for t in range(300)]
    return b, out, st, rows


def test_effect_on_the_rows_over_the_threshold(batch_ref, oracle_lib):
    """Measured on generate(300, 21), S = 256, R = 3, seed 0: 894 valid PMD rows,
    153 over tau = 0.585 in round 0, 23 after the rounds (c free 114 -> 7, c held
    39 -> 16); best round 0 / 1 / 2 / 3 in 755 / 115 / 17 / 7 rows; taxa with all
    three rows reliable 185 -> 275 of 294.  Asserted: at most a third of round
    0's count stays over tau, no reliable row is touched, round 0 is
    map_psis_ref.psis_taxon's exactly."""
    b, out, st, rows = batch_ref
    tau = ref.khat_threshold(S_A)
    n_valid = over0 = over1 = 0
    by_round = [0, 0, 0, 0]
    by_c = {True: [0, 0], False: [0, 0]}
    taxa0 = taxa1 = taxa_all = 0
    for t in range(300):
        v1 = ref.psis_taxon(oracle_lib, b.y[t, :30], b.N[t, :30], out[t], int(st[t]), S_A, seed=SEED, g=t) \
            if t < 40 else None
        rel0 = rel1 = full = 0
        for r, res in enumerate(rows[t]):
            if "rounds" not in res:
                continue
            r0 = res["rounds"][0]
            if v1 is not None:  # round 0 is MDFIT-PSIS v1
                assert np.array_equal(r0["u"], v1[r]["u"]) and np.array_equal(r0["lw"], v1[r]["lw"])
                if r0["ok"]:
                    rec0 = ref.estimates(r0["w"], ref.constrained(r0["u64"]), r0["khat"], r0["n_inf"], S_A,
                                         res["prop"].mask)
                    assert np.array_equal(rec0, v1[r]["rec"], equal_nan=True)
            if not r0["ok"]:
                assert res["best_round"] == 0 and res["tried"] == 0 and np.isnan(res["adapt"]).all()
                continue
            full += 1
            n_valid += 1
            k0, kb = float(r0["khat"]), float(res["best"]["khat"])
            assert kb <= k0 and res["adapt"][0] == k0
            assert (int(res["rec"][ref.FLAGS]) & ad.ADAPTED != 0) == (res["best_round"] > 0)
            if k0 <= tau:  # a reliable row is never touched
                assert res["tried"] == 0 and res["best_round"] == 0 and len(res["rounds"]) == 1
                assert np.array_equal(res["rec"], ref.estimates(r0["w"], ref.constrained(r0["u64"]), r0["khat"],
                                                                r0["n_inf"], S_A, res["prop"].mask), equal_nan=True)
            over0 += k0 > tau
            over1 += kb > tau
            by_c[res["prop"].cheld][0] += k0 > tau
            by_c[res["prop"].cheld][1] += kb > tau
            by_round[res["best_round"]] += 1
            rel0 += k0 <= tau
            rel1 += kb <= tau
        taxa_all += full == 3
        taxa0 += rel0 == 3
        taxa1 += rel1 == 3
    print(f"{n_valid} valid rows; over tau {over0} -> {over1} (c free {by_c[False][0]} -> {by_c[False][1]}, c held "
          f"{by_c[True][0]} -> {by_c[True][1]}); best round {by_round}; taxa with three reliable rows {taxa0} -> "
          f"{taxa1} of {taxa_all}")
    assert n_valid == 894 and over0 == 153
    assert 3 * over1 <= over0, (over0, over1)
    assert taxa1 > taxa0


def test_adapted_rows_vs_nuts_posterior(batch_ref, oracle_lib):
    """The first 12 rescued PMD-all rows (khat of round 0 over tau, the best
    round's at or under it) -- taxa 6, 9, 15, 18, 35, 46, 51, 55, 58, 60, 63,
    76, khat 0.61-0.95 -> -0.14-0.48 -- against a 500 + 1000 oracle chain.
    Measured: (D_max mean - NUTS mean) / NUTS std in [-0.171, +0.097], D_max std /
    NUTS std in [0.796, 1.132] (round 0 on the same rows: [-0.413, +0.160] and
    [0.645, 1.244]).  The bands asserted are the measured ranges widened by the
    chain's own Monte-Carlo error, 0.1 std on the mean and 15 % on the std, as
    test_map_psis.py argues."""
    b, out, st, rows = batch_ref
    tau = ref.khat_threshold(S_A)
    rescued = [t for t in range(300) if "rounds" in rows[t][0] and rows[t][0]["rounds"][0]["ok"]
               and float(rows[t][0]["rounds"][0]["khat"]) > tau >= float(rows[t][0]["best"]["khat"])][:12]
    assert len(rescued) == 12
    stats = []
    for t in rescued:
        rec = rows[t][0]["rec"].astype(float)
        smp, _, rc = oracle_lib.nuts_chain(0, 0, b.y[t, :30], b.N[t, :30], seed=0, g=int(t), sub=0, num_warmup=500,
                                           num_samples=1000)
        assert rc == 0
        D = smp[:, 1] + smp[:, 2]
        stats.append(((rec[4] - D.mean()) / D.std(), rec[9] / D.std()))
        print(f"taxon {t}: khat {rows[t][0]['adapt'][0]:.3f} -> {rec[ref.KHAT]:.3f}, mean {stats[-1][0]:+.3f}, "
              f"std {stats[-1][1]:.3f} (NUTS std)")
    stats = np.array(stats)
    print(f"mean in [{stats[:, 0].min():+.3f}, {stats[:, 0].max():+.3f}], std in [{stats[:, 1].min():.3f}, "
          f"{stats[:, 1].max():.3f}]")
    assert (stats[:, 0] >= -0.171 - 0.1).all() and (stats[:, 0] <= 0.097 + 0.1).all(), stats[:, 0]
    assert (stats[:, 1] >= 0.796 * 0.85).all() and (stats[:, 1] <= 1.132 * 1.15).all(), stats[:, 1]


# --------------------------------------------------------------------------
# the host build of csrc/mdfit_mapadapt.h
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("adapt_host") / "adapt_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", str(ROOT / "tests" / "adapt_host_main.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def _hex(v):
    return float(v).hex() if np.isfinite(v) else ("nan" if np.isnan(v) else ("inf" if v > 0 else "-inf"))


def _run_host(exe, u, w, mask, cheld, K, tmp_path):
    n, S = w.shape
    lines = [str(n)]
    for i in range(n):
        lines += [f"{S} {mask[i]} {cheld[i]} " + " ".join(_hex(v) for v in K[i]), " ".join(_hex(v) for v in w[i]),
                  " ".join(_hex(v) for v in u[i].ravel())]
    src = tmp_path / "series.txt"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = np.array([[float.fromhex(tok) if "nan" not in tok else np.nan for tok in ln.split()]
                    for ln in r.stdout.strip().splitlines()])
    return got[:, 0].astype(bool), (got[:, 1:5], got[:, 5:9], got[:, 9:25].reshape(n, 4, 4), got[:, 25])


@pytest.mark.parametrize("S", cases.S_VALUES)
def test_host_program_vs_reference(host_program, tmp_path, S):
    u, w, mask, cheld, K, kinds = cases.series(S)
    want = cases.reference(u, w, mask, cheld, K)
    ok, got = _run_host(host_program, u, w, mask, cheld, K, tmp_path)
    for i, kind in enumerate(kinds):  # the stop flag, everywhere
        assert ok[i] == (want[i] is not None) == (kind not in cases.STOPS), (kind, ok[i])
        if not ok[i]:
            assert all(np.isnan(g[i]).all() for g in got)
    worst = cases.errors(got, want)
    print(f"S={S}: worst error " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, v in worst.items():
        assert v <= HOST_TOL[name], (name, v)
    m, d, F, gc = got
    for i in np.flatnonzero(ok):  # the form psis_draw reads: upper triangular, unit rows, positive diagonal
        assert (np.tril(F[i], -1) == 0).all() and (np.diag(F[i]) > 0).all()
        assert np.abs((F[i] * F[i]).sum(axis=1) - 1).max() < 1e-12
        if cheld[i]:
            assert m[i, 2] == 0 and d[i, 2] == 1 and F[i, 2, 2] == 1 and gc[i] > 0


# --------------------------------------------------------------------------
# frames, options, CLI, gather record
# --------------------------------------------------------------------------
def _cfg(tmp_path, inference="map-psis", **kw):
    from metadamage_amd import utils
    from tests.helpers import GOLDEN

    cfg = utils.Config(out_dir=tmp_path, max_fits=10, max_cores=1, min_alignments=10, min_y_sum=10,
                       substitution_bases_forward="CT", substitution_bases_reverse="GA", forced=False,
                       version="0.0.0", inference=inference, **kw)
    cfg.add_filename(GOLDEN / "data_ancient.txt")
    return cfg


def test_frames_carry_the_two_columns_only_when_asked(tmp_path, oracle_lib):
    import pandas as pd

    from metadamage_amd import _lib, fits
    from tests.helpers import GOLDEN

    p = fits.pack_counts(pd.read_parquet(GOLDEN / "counts_data_ancient.parquet"), _cfg(tmp_path))
    out, pred, st = oracle_lib.fit_batch(p.y, p.N, p.mm)
    T = len(st)
    rows = [ad.adapt_taxon(oracle_lib, p.y[t, :30], p.N[t, :30], out[t], int(st[t]), 64, 3, seed=0, g=t)
            for t in range(T)]
    psis32 = np.array([[r["rec"] for r in taxon] for taxon in rows]).astype(np.float64).astype(np.float32)
    full = np.array([[r["adapt"] for r in taxon] for taxon in rows])
    adapt32 = np.stack([full[:, :, 0].max(axis=1), full[:, :, 2].max(axis=1)], axis=1).astype(np.float32)
    adapt32[1] = np.nan  # (a taxon without a valid row)
    waic32 = np.zeros((T, _lib.NWAICROW, _lib.NMAPWAIC), np.float32)
    auto32 = np.zeros((T, _lib.NAUTO), np.float32)
    keep = st == 0
    for kw, cfg in (({"psis": psis32}, _cfg(tmp_path)), ({"waic": waic32}, _cfg(tmp_path, "map-waic")),
                    ({"auto": auto32}, _cfg(tmp_path, "auto"))):
        today = fits.make_df_fit_results(p, out, keep, cfg, **kw)
        assert "pareto_k_initial" not in today.columns and "psis_adapt_rounds" not in today.columns
        pd.testing.assert_frame_equal(fits.make_df_fit_results(p, out, keep, cfg, adapt=None, **kw), today)
        df = fits.make_df_fit_results(p, out, keep, cfg, adapt=adapt32, **kw)
        assert list(df.columns) == list(today.columns) + fits.ADAPT_COLUMNS
        assert list(df.columns[-2:]) == ["pareto_k_initial", "psis_adapt_rounds"]
        pd.testing.assert_frame_equal(df[today.columns], today)
        assert df["pareto_k_initial"].dtype == np.float32 and df["psis_adapt_rounds"].dtype == np.uint32
        np.testing.assert_array_equal(df["pareto_k_initial"].to_numpy(), adapt32[keep, 0])
        np.testing.assert_array_equal(df["psis_adapt_rounds"].to_numpy(),
                                      np.nan_to_num(adapt32[keep, 1]).astype(np.uint32))
    k2 = np.array([True, False, True])  # a dropped taxon takes its row with it
    d2 = fits.make_df_fit_results(p, out, k2, _cfg(tmp_path), psis=psis32, adapt=adapt32)
    np.testing.assert_array_equal(d2["pareto_k_initial"].to_numpy(), adapt32[k2, 0])


def test_config_metadata_cache_key_and_cli(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import fits, utils
    from metadamage_amd.cli import cli_app
    from tests.helpers import GOLDEN

    assert utils.Config.__dataclass_fields__["psis_adapt"].default == 0
    for inference in ("map-psis", "map-waic", "auto", "map", "nuts"):
        d0 = _cfg(tmp_path, inference).to_dict()
        assert "psis_adapt" not in d0 and fits.psis_adapt_of(_cfg(tmp_path, inference)) == 0
        assert _cfg(tmp_path, inference, psis_adapt=0).to_dict() == d0  # the metadata of a run without it: today's
    d3 = _cfg(tmp_path, "map-psis", psis_adapt=3).to_dict()
    assert d3["psis_adapt"] == 3 and fits.psis_adapt_of(_cfg(tmp_path, "auto", psis_adapt=2)) == 2
    assert {k: v for k, v in d3.items() if k != "psis_adapt"} == _cfg(tmp_path, "map-psis").to_dict()
    # the cache key: a run with rounds does not reuse a run without, nor the other way round
    assert "psis_adapt" in fits.CACHE_KEYS
    d0 = _cfg(tmp_path, "map-psis").to_dict()
    assert utils.metadata_is_similar(d0, dict(d0), include=fits.CACHE_KEYS)
    assert utils.metadata_is_similar(d3, dict(d3), include=fits.CACHE_KEYS)
    assert not utils.metadata_is_similar(d0, d3, include=fits.CACHE_KEYS)
    assert not utils.metadata_is_similar(d3, d0, include=fits.CACHE_KEYS)
    assert not utils.metadata_is_similar(d3, _cfg(tmp_path, "map-psis", psis_adapt=2).to_dict(),
                                         include=fits.CACHE_KEYS)
    runner = CliRunner()
    base = ["fit", str(GOLDEN / "data_ancient.txt"), "--out-dir", str(tmp_path)]
    for n in ("-1", "5"):
        bad = runner.invoke(cli_app, base + ["--inference", "map-psis", "--psis-adapt", n])
        assert bad.exit_code == 2 and "psis-adapt" in bad.output
    for inference in ("map-pred", "map", "nuts"):
        bad = runner.invoke(cli_app, base + ["--inference", inference, "--psis-adapt", "3"])
        assert bad.exit_code == 2 and "psis-adapt" in bad.output, inference
    assert "--psis-adapt" in runner.invoke(cli_app, ["fit", "--help"], terminal_width=200).output


def test_engine_argument_checks():
    from metadamage_amd import engine

    assert engine._check_psis_adapt(0, False) == 0 and engine._check_psis_adapt(4, True) == 4
    for R in (-1, 5):
        with pytest.raises(ValueError, match="psis_adapt"):
            engine._check_psis_adapt(R, True)
    with pytest.raises(ValueError, match="psis_adapt"):
        engine._check_psis_adapt(2, False)


def _fill(lo, hi, shape):
    """Deterministic f32 rows of the global taxa lo .. hi - 1."""
    t = np.arange(lo, hi, dtype=np.float64).reshape((-1,) + (1,) * len(shape))
    return (t * 1000 + np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)).astype(np.float32)


def _gather_worker(rank, world, port, T, kind, q):
    import os

    import torch
    import torch.distributed as dist

    from metadamage_amd import distributed as d

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lo, hi = d.shard_range(T, rank, world)
        cap = d.shard_capacity(T, world)
        rec = d.alloc_records(cap, "cpu", with_adapt=True, **{kind: True})
        rec.buf.zero_()
        rec.out.zero_()
        block = {"with_psis": rec.psis, "with_waic": rec.waic, "with_auto": rec.auto}[kind]
        block[: hi - lo] = torch.from_numpy(_fill(lo, hi, tuple(block.shape[1:])))
        ad32 = _fill(lo, hi, (2,)) + 0.5
        if lo == 0:
            ad32[0, 0] = np.nan
        rec.adapt[: hi - lo] = torch.from_numpy(ad32)
        rec.status[: hi - lo] = torch.arange(lo, hi, dtype=torch.int32)
        parts = d.gather_records(rec.stage(), cap, rank, world)
        if rank == 0:
            q.put(d.unpack_gathered(parts, T, world, with_adapt=True, **{kind: True}))
        else:
            assert parts is None
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,T,kind", [(2, 13, "with_psis"), (3, 7, "with_waic"), (2, 5, "with_auto")])
def test_gloo_gather_round_trips_the_adapt_block(world, T, kind):
    import socket

    import torch.multiprocessing as mp

    from metadamage_amd import _lib

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, T, kind, q)) for r in range(world)]
    for p in procs:
        p.start()
    out, pred, st, block, adapt = q.get(timeout=120)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    shape = {"with_psis": (3, _lib.NMAPPSIS), "with_waic": (_lib.NWAICROW, _lib.NMAPWAIC),
             "with_auto": (_lib.NAUTO,)}[kind]
    np.testing.assert_array_equal(st, np.arange(T))
    np.testing.assert_array_equal(block, _fill(0, T, shape))
    want = _fill(0, T, (2,)) + 0.5
    want[0, 0] = np.nan
    assert adapt.dtype == np.float32 and adapt.shape == (T, _lib.NADAPTOUT)
    np.testing.assert_array_equal(adapt, want)


def test_gather_record_layout_with_the_adapt_block():
    import torch

    from metadamage_amd import _lib, distributed as d

    assert d.REC_ADAPT == 8
    n = 7
    plain = d.alloc_records(n, "cpu", with_psis=True)
    rec = d.alloc_records(n, "cpu", with_psis=True, with_adapt=True)
    assert plain.adapt is None and plain.buf.numel() == n * (d.REC_BYTES + d.REC_PSIS)  # (today's record)
    assert rec.buf.numel() == plain.buf.numel() + n * d.REC_ADAPT
    assert rec.adapt.shape == (n, _lib.NADAPTOUT) and rec.adapt.dtype == torch.float32
    assert rec.adapt.data_ptr() == rec.buf.data_ptr() + n * (d.REC_BYTES + d.REC_PSIS)  # behind the psis block
    assert rec.psis.data_ptr() == rec.buf.data_ptr() + n * d.REC_BYTES
    for kw in ({}, {"with_laplace": True}, {"with_ppred": True}, {"with_loo": True}):
        with pytest.raises(ValueError, match="with_adapt"):
            d.alloc_records(n, "cpu", with_adapt=True, **kw)
