"""CPU tests of the auto inference with the posterior predictive (MDFIT-AUTO
v1.1): the C-ABI entry point without a device, the host build
of the routing rule and the composition (csrc/mdfit_auto.h) against the numpy
restatement (tests/auto_pred_ref.py) on crafted records, bit for bit and under
the address and undefined-behaviour sanitizers, and the frames / options / CLI
/ gather-record plumbing."""

from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from tests import auto_pred_ref as ref
from tests import auto_ref as v1
from tests.helpers import GOLDEN

ROOT = Path(__file__).resolve().parents[1]


# --------------------------------------------------------------------------
# ABI
# --------------------------------------------------------------------------
def test_entry_point_declared_exported_and_argument_checked():
    from metadamage_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mdfit.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+mdfit_auto_route_pred\s*\(", text) and re.search(r"\bint\s+mdfit_auto_route\s*\(", text)
    assert re.search(r"#define MDFIT_ROUTE_PRED\s+16\b", text) and re.search(r"#define MDFIT_ROUTE_SAMPLE_PRED\s+23\b", text)
    assert (_lib.ROUTE_PRED, _lib.ROUTE_SAMPLE_PRED) == (ref.R_PRED, ref.R_SAMPLE_PRED)
    assert _lib.ROUTE_SAMPLE_PRED == _lib.ROUTE_SAMPLE | _lib.ROUTE_PRED
    assert "mdfit_auto_route_pred" in _lib.EXPORTED_SYMBOLS
    fields = _lib.AUTO_COMPOSED_FIELDS + _lib.AUTO_PRED_COMPOSED_FIELDS
    assert sorted(_lib.RESULT_FIELDS.index(f) for f in fields) == ref.COMPOSED and len(ref.COMPOSED) == 14
    assert all(_lib.RESULT_FIELDS[c] == name for name, c in ref.F_PRED.items())
    assert [_lib.MAPPRED_FIELDS[k] for _, k in ref.PRED_COPIES] == _lib.AUTO_PRED_COMPOSED_FIELDS
    assert _lib.MAPPRED_FIELDS[ref.PRED_FLAGS] == "flags" and _lib.MAPPRED_FIELDS[ref.PRED_NNONCOUNT] == "n_noncount_jobs"
    assert _lib.NPRED * _lib.NPOS == ref.NPRED_FLOATS
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                        check=True).stdout
    assert re.search(r"\bT mdfit_auto_route_pred\b", nm)
    dummy = ctypes.c_void_p(16)
    ar = lib.mdfit_auto_route_pred
    assert ar(None, None, None, None, None, -1, None, None, None, None) == -1 and b"n_taxa" in lib.mdfit_last_error()
    assert ar(None, None, None, None, None, 0, None, None, None, None) == 0
    for missing in range(5):  # status, psis, waic, prec, ppred are required; pred is not
        a = [dummy] * 5
        a[missing] = None
        assert ar(*a, 1, dummy, None, dummy, None) == -1 and b"null" in lib.mdfit_last_error(), missing
    assert ar(dummy, dummy, dummy, dummy, dummy, 1, None, None, dummy, None) == -1
    assert ar(dummy, dummy, dummy, dummy, dummy, 1, dummy, None, None, None) == -1
    assert ar(dummy, dummy, dummy, dummy, dummy, (1 << 25) + 1, dummy, dummy, dummy, None) == -1
    assert b"2^25" in lib.mdfit_last_error()


# --------------------------------------------------------------------------
# the host build of csrc/mdfit_auto.h
# --------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["plain", "sanitized"])
def host_program(tmp_path_factory, request):
    exe = tmp_path_factory.mktemp("auto_pred_host") / f"auto_pred_host_{request.param}"
    flags = ["-O1", "-g"] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
                             if request.param == "sanitized" else [])
    subprocess.run(["g++", "-std=c++17", *flags, "-I", str(ROOT / "tests" / "host_shim"),
                    str(ROOT / "tests" / "auto_pred_host_main.cpp"), "-o", str(exe)], check=True)
    return exe


def run_host(exe, tmp_path, st, psis, waic, prec, ppred, out, pred):
    T = len(st)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int64(T).tobytes())
        f.write(np.int64(pred is not None).tobytes())
        for a, dt in ((st, np.int32), (psis, np.float64), (waic, np.float64), (prec, np.float64),
                      (ppred, np.float32), (out, np.float64)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
        if pred is not None:
            f.write(np.ascontiguousarray(pred, dtype=np.float32).tobytes())
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = dst.read_bytes()
    route = np.frombuffer(raw[: 4 * T], dtype=np.int32)
    o_end = 4 * T + 8 * T * ref.NOUT
    got_out = np.frombuffer(raw[4 * T:o_end], dtype=np.float64).reshape(T, ref.NOUT)
    got_pred = np.frombuffer(raw[o_end:], dtype=np.float32).reshape(T, ref.NPRED_FLOATS) if pred is not None else None
    assert len(raw) == o_end + (4 * T * ref.NPRED_FLOATS if pred is not None else 0)
    return route, got_out, got_pred


def test_crafted_records_cover_every_route():
    st, psis, waic, prec, ppred, out, pred = ref.crafted()
    route, comp, cpred = ref.auto_route_pred(st, psis, waic, prec, ppred, out, pred)
    # every combination of the five causes: the four sampling bits in all 16 ways, and the invalid taxon alone
    assert set(route[st != v1.INVALID]) == {a | b | c | d for a in (0, 1) for b in (0, 2) for c in (0, 4)
                                            for d in (0, 16)}
    assert set(route[st == v1.INVALID]) == {8}
    assert ((route & 4) != 0).tolist() == [s in (1, 2) for s in st]
    # v1's bits are v1's; the new bit is the pred record's alone
    r1, _ = v1.auto_route(st, psis, waic, out)
    np.testing.assert_array_equal(route & ~np.int32(16), r1)
    ok = st != v1.INVALID
    fl, nn = prec[:, ref.PRED_FLAGS], prec[:, ref.PRED_NNONCOUNT]
    want16 = ok & ~(np.isin(fl, (3.0, 67.0)) & (nn == 0.0))  # (NaN, negative, 2^32 + 3 and 1 have no bit 1)
    np.testing.assert_array_equal((route & 16) != 0, want16)
    # only route-0 rows change, and only in the 14 columns and the 90 floats
    changed = comp.view(np.int64) != out.view(np.int64)
    pchanged = cpred.view(np.int32) != pred.view(np.int32)
    assert (route == 0).sum() >= 2 and not changed[route != 0].any() and not pchanged[route != 0].any()
    assert not changed[:, [c for c in range(ref.NOUT) if c not in ref.COMPOSED]].any()
    assert changed[route == 0][:, ref.COMPOSED].all() and pchanged[route == 0].all()
    np.testing.assert_array_equal(cpred[route == 0].view(np.int32), ppred[route == 0].view(np.int32))
    assert np.isnan(comp[st == v1.INVALID]).all() and np.isnan(cpred[st == v1.INVALID]).all()


def test_host_program_equals_reference(host_program, tmp_path):
    st, psis, waic, prec, ppred, out, pred = ref.crafted()
    for with_pred in (True, False):
        p_in = pred if with_pred else None
        want_route, want_out, want_pred = ref.auto_route_pred(st, psis, waic, prec, ppred, out, p_in)
        route, got, gpred = run_host(host_program, tmp_path, st, psis, waic, prec, ppred, out, p_in)
        np.testing.assert_array_equal(route, want_route)
        np.testing.assert_array_equal(got.view(np.int64), want_out.view(np.int64))  # bit patterns: NaN, -0.0, subnormal
        if with_pred:
            np.testing.assert_array_equal(gpred.view(np.int32), want_pred.view(np.int32))
        else:
            assert gpred is None and want_pred is None
    e = slice(0, 0)
    assert run_host(host_program, tmp_path, st[e], psis[e], waic[e], prec[e], ppred[e], out[e], pred[e])[0].size == 0


# --------------------------------------------------------------------------
# frames, options, CLI, gather record
# --------------------------------------------------------------------------
def _cfg(tmp_path, inference="auto", **kw):
    from metadamage_amd import utils

    cfg = utils.Config(out_dir=tmp_path, max_fits=10, max_cores=1, min_alignments=10, min_y_sum=10,
                       substitution_bases_forward="CT", substitution_bases_reverse="GA", forced=False,
                       version="0.0.0", inference=inference, **kw)
    cfg.add_filename(GOLDEN / "data_ancient.txt")
    return cfg


def test_frame_columns_and_dtypes(tmp_path, oracle_lib, ref_meta):
    from metadamage_amd import _lib, fits

    cfg = _cfg(tmp_path, auto_pred=True)
    p = fits.pack_counts(pd.read_parquet(GOLDEN / "counts_data_ancient.parquet"), cfg)
    out, pred, st = oracle_lib.fit_batch(p.y, p.N, p.mm)
    keep = st == 0
    assert keep.all() and len(keep) == 3
    auto = np.array([[0, 0, 0.25, 200.5], [16, 1, 0.3, 150.0], [5, 1, np.nan, np.nan]], dtype=np.float32)
    apred = np.array([[180.25, 97.0], [np.nan, np.nan], [np.nan, np.nan]], dtype=np.float32)
    adapt = np.array([[0.71, 2.0], [0.2, 0.0], [np.nan, np.nan]], dtype=np.float32)
    base = ref_meta["fit_results_columns"]
    today = fits.make_df_fit_results(p, out, keep, cfg, auto=auto)
    df = fits.make_df_fit_results(p, out, keep, cfg, auto=auto, auto_pred=apred)
    assert fits.AUTO_PRED_COLUMNS == ["pred_ess_min", "pred_distinct_min"] == _lib.AUTOPRED_FIELDS
    assert list(df.columns) == base + fits.AUTO_UINT_COLUMNS + fits.AUTO_COLUMNS + fits.AUTO_PRED_COLUMNS
    pd.testing.assert_frame_equal(df[today.columns], today)  # no column is renamed or moved
    assert df["pred_ess_min"].dtype == np.float32 and df["pred_distinct_min"].dtype == np.uint32
    np.testing.assert_array_equal(df["pred_ess_min"].to_numpy(), apred[:, 0])
    assert df["pred_distinct_min"].tolist() == [97, 0, 0]  # 0 where the taxon is sampled
    both = fits.make_df_fit_results(p, out, keep, cfg, auto=auto, auto_pred=apred, adapt=adapt)
    assert list(both.columns) == list(df.columns) + fits.ADAPT_COLUMNS  # the adapt columns stay last
    pd.testing.assert_frame_equal(both[df.columns], df)
    d2 = fits.make_df_fit_results(p, out, np.array([True, False, True]), cfg, auto=auto, auto_pred=apred)
    assert d2["pred_distinct_min"].tolist() == [97, 0]
    # "map-pred" with the rounds: the two adapt columns behind the map-pred columns
    ppred = np.zeros((3, 106), np.float32)
    mp = fits.make_df_fit_results(p, out, keep, _cfg(tmp_path, "map-pred", psis_adapt=3), ppred=ppred, adapt=adapt)
    assert list(mp.columns) == base + fits.MAP_PRED_COLUMNS + fits.MAP_PRED_UINT_COLUMNS + fits.ADAPT_COLUMNS
    # the optional arrays behind (out, pred, status): extra, then auto_pred, then adapt
    x, q, a = object(), object(), object()
    assert fits._split_rest(_cfg(tmp_path, auto_pred=True, psis_adapt=3), [x, q, a]) == (x, q, a)
    assert fits._split_rest(_cfg(tmp_path, auto_pred=True), [x, q]) == (x, q, None)
    assert fits._split_rest(_cfg(tmp_path, psis_adapt=2), [x, a]) == (x, None, a)
    assert fits._split_rest(_cfg(tmp_path), [x]) == (x, None, None)
    assert fits._split_rest(_cfg(tmp_path, "map-pred", psis_adapt=1), [x, a]) == (x, None, a)
    assert fits._split_rest(_cfg(tmp_path, "map"), []) == (None, None, None)


def test_config_metadata_cache_key_and_cli(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import engine, fits, utils
    from metadamage_amd.cli import cli_app

    assert utils.Config.__dataclass_fields__["auto_pred"].default is False
    for inference in ("auto", "map-pred", "map", "nuts"):
        d0 = _cfg(tmp_path, inference).to_dict()
        assert "auto_pred" not in d0 and not fits.auto_pred_of(_cfg(tmp_path, inference))
        assert _cfg(tmp_path, inference, auto_pred=False).to_dict() == d0  # the metadata of a run without it: today's
    assert "pred_draws" not in _cfg(tmp_path, "auto").to_dict()
    d1 = _cfg(tmp_path, "auto", auto_pred=True, pred_draws=100).to_dict()
    assert d1["auto_pred"] is True and d1["pred_draws"] == 100 and fits.auto_pred_of(_cfg(tmp_path, auto_pred=True))
    assert {k: v for k, v in d1.items() if k not in ("auto_pred", "pred_draws")} == _cfg(tmp_path, "auto").to_dict()
    assert "auto_pred" in fits.CACHE_KEYS and "pred_draws" in fits.CACHE_KEYS
    d0 = _cfg(tmp_path, "auto").to_dict()
    sim = utils.metadata_is_similar
    assert sim(d0, dict(d0), include=fits.CACHE_KEYS) and sim(d1, dict(d1), include=fits.CACHE_KEYS)
    assert not sim(d0, d1, include=fits.CACHE_KEYS) and not sim(d1, d0, include=fits.CACHE_KEYS)
    assert not sim(d1, _cfg(tmp_path, "auto", auto_pred=True, pred_draws=200).to_dict(), include=fits.CACHE_KEYS)
    # map-pred takes the rounds (Config and the engine; the CLI keeps --psis-adapt to map-psis, map-waic and auto)
    assert _cfg(tmp_path, "map-pred", psis_adapt=3).to_dict()["psis_adapt"] == 3
    assert engine._check_psis_adapt(3, True) == 3
    # the rejections
    for inference in ("map", "nuts", "map-pred", "map-waic"):
        with pytest.raises(ValueError, match="auto_pred"):
            fits.auto_pred_of(_cfg(tmp_path, inference, auto_pred=True))
    runner = CliRunner()
    base = ["fit", str(GOLDEN / "data_ancient.txt"), "--out-dir", str(tmp_path)]
    for inference in ("map", "nuts", "map-pred", "map-psis", "map-waic"):
        bad = runner.invoke(cli_app, base + ["--inference", inference, "--auto-pred"])
        assert bad.exit_code == 2 and "auto-pred" in bad.output, inference
    for n in ("24", "1025"):  # --pred-draws applies
        bad = runner.invoke(cli_app, base + ["--inference", "auto", "--auto-pred", "--pred-draws", n])
        assert bad.exit_code == 2 and "pred-draws" in bad.output
    for inference in ("map", "nuts", "map-laplace"):
        bad = runner.invoke(cli_app, base + ["--inference", inference, "--psis-adapt", "3"])
        assert bad.exit_code == 2 and "psis-adapt" in bad.output, inference
    assert "--auto-pred" in runner.invoke(cli_app, ["fit", "--help"], terminal_width=200).output


def test_gather_record_carries_the_blocks():
    import torch

    from metadamage_amd import _lib, distributed as d

    assert d.REC_AUTO_PRED == 8 == _lib.NAUTOPRED * 4
    n = 7
    plain = d.alloc_records(n, "cpu", with_auto=True, with_adapt=True)
    assert plain.auto_pred is None and plain.buf.numel() == n * (d.REC_BYTES + d.REC_AUTO + d.REC_ADAPT)  # today's
    rec = d.alloc_records(n, "cpu", with_auto=True, with_adapt=True, with_auto_pred=True)
    assert rec.buf.numel() == plain.buf.numel() + n * d.REC_AUTO_PRED
    assert rec.auto_pred.shape == (n, 2) and rec.auto_pred.dtype == torch.float32
    base = rec.buf.data_ptr() + n * (d.REC_BYTES + d.REC_AUTO)
    assert rec.auto.data_ptr() == rec.buf.data_ptr() + n * d.REC_BYTES
    assert rec.auto_pred.data_ptr() == base and rec.adapt.data_ptr() == base + n * d.REC_AUTO_PRED  # before the adapt block
    only = d.alloc_records(n, "cpu", with_auto=True, with_auto_pred=True)
    assert only.adapt is None and only.buf.numel() == n * (d.REC_BYTES + d.REC_AUTO + d.REC_AUTO_PRED)
    for kw in ({}, {"with_psis": True}, {"with_ppred": True}):
        with pytest.raises(ValueError, match="with_auto_pred"):
            d.alloc_records(n, "cpu", with_auto_pred=True, **kw)
    # map-pred with the rounds: the adapt block behind the ppred block, by a switch of its own
    for kw in ({}, {"with_psis": True}, {"with_auto": True}):
        with pytest.raises(ValueError, match="with_ppred_adapt"):
            d.alloc_records(n, "cpu", with_ppred_adapt=True, **kw)
    pp = d.alloc_records(n, "cpu", with_ppred=True, with_ppred_adapt=True)
    assert pp.buf.numel() == n * (d.REC_BYTES + d.REC_PPRED + d.REC_ADAPT)
    assert pp.adapt.data_ptr() == pp.buf.data_ptr() + n * (d.REC_BYTES + d.REC_PPRED)
    # round trip through two parts of a world of two
    rng = np.random.default_rng(5)
    for with_adapt in (True, False):
        r = d.alloc_records(n, "cpu", with_auto=True, with_adapt=with_adapt, with_auto_pred=True)
        r.buf.copy_(torch.from_numpy(rng.integers(0, 256, r.buf.numel(), dtype=np.uint8)))
        want_auto = rng.standard_normal((n, 4)).astype(np.float32)
        want_ap = rng.standard_normal((n, 2)).astype(np.float32)
        want_ap[1] = np.nan
        want_ad = rng.standard_normal((n, 2)).astype(np.float32)
        r.auto.copy_(torch.from_numpy(want_auto))
        r.auto_pred.copy_(torch.from_numpy(want_ap))
        if with_adapt:
            r.adapt.copy_(torch.from_numpy(want_ad))
        got = d.unpack_gathered([r.buf, r.buf.clone()], 13, 2, with_auto=True, with_adapt=with_adapt,
                                with_auto_pred=True)
        assert len(got) == (6 if with_adapt else 5)
        np.testing.assert_array_equal(got[3], np.concatenate([want_auto, want_auto[:6]]))
        np.testing.assert_array_equal(got[4], np.concatenate([want_ap, want_ap[:6]]))
        if with_adapt:
            np.testing.assert_array_equal(got[5], np.concatenate([want_ad, want_ad[:6]]))
    got = d.unpack_gathered([pp.buf, pp.buf.clone()], 13, 2, with_ppred=True, with_ppred_adapt=True)
    assert len(got) == 5 and got[3].shape == (13, 106) and got[4].shape == (13, 2)
