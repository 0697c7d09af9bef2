"""CPU tests of the auto inference (MDFIT-AUTO v1): the C-ABI
entry points without a device, the host build of the routing rule and the
composition (csrc/mdfit_auto.h) against the numpy restatement
(tests/auto_ref.py) on crafted records, bit for bit, and the frames / options /
CLI / gather-record plumbing."""

from __future__ import annotations

import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pandas as pd
import pytest

from tests import auto_ref as ref
from tests.helpers import GOLDEN

ROOT = Path(__file__).resolve().parents[1]


# --------------------------------------------------------------------------
# ABI
# --------------------------------------------------------------------------
def test_entry_points_declared_exported_and_argument_checked():
    from metadamage_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mdfit.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+mdfit_fit_batch_indexed\s*\(", text)
    assert re.search(r"\bint\s+mdfit_auto_route\s*\(", text)
    assert f"#define MDFIT_ABI_VERSION {_lib.ABI_VERSION}" in text and _lib.ABI_VERSION == 3
    for name, v in (("WAIC", _lib.ROUTE_WAIC), ("PSIS", _lib.ROUTE_PSIS), ("STATUS", _lib.ROUTE_STATUS),
                    ("INVALID", _lib.ROUTE_INVALID), ("SAMPLE", _lib.ROUTE_SAMPLE)):
        assert re.search(rf"#define MDFIT_ROUTE_{name}\s+{v}\b", text), name
    assert (_lib.ROUTE_WAIC, _lib.ROUTE_PSIS, _lib.ROUTE_STATUS, _lib.ROUTE_INVALID, _lib.ROUTE_SAMPLE) == \
        (ref.R_WAIC, ref.R_PSIS, ref.R_STATUS, ref.R_INVALID, ref.R_SAMPLE)
    assert "mdfit_fit_batch_indexed" in _lib.EXPORTED_SYMBOLS and "mdfit_auto_route" in _lib.EXPORTED_SYMBOLS
    assert sorted(_lib.RESULT_FIELDS.index(f) for f in _lib.AUTO_COMPOSED_FIELDS) == ref.COMPOSED
    assert {_lib.RESULT_FIELDS[c] for c in ref.COMPOSED} == set(ref.F)
    assert all(_lib.RESULT_FIELDS[c] == name for name, c in ref.F.items())
    lib = _lib.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True,
                        check=True).stdout
    assert re.search(r"\bT mdfit_fit_batch_indexed\b", nm) and re.search(r"\bT mdfit_auto_route\b", nm)
    dummy = ctypes.c_void_p(16)
    nuts = _lib.default_opts(mode=_lib.MODE_NUTS)
    mapo = _lib.default_opts(mode=_lib.MODE_MAP)
    fb = lib.mdfit_fit_batch_indexed
    assert fb(None, None, None, -1, None, ctypes.byref(nuts), None, None, None, None, None) == -1
    assert b"n_taxa" in lib.mdfit_last_error()
    assert fb(None, None, None, 0, None, ctypes.byref(nuts), None, None, None, None, None) == 0
    assert fb(None, None, None, 0, dummy, ctypes.byref(nuts), None, None, None, None, None) == 0
    # the MAP fit draws nothing: an index with it is an argument error, whatever else is given
    assert fb(dummy, dummy, None, 1, dummy, ctypes.byref(mapo), dummy, None, dummy, dummy, None) == -1
    assert b"taxon_index" in lib.mdfit_last_error()
    assert fb(dummy, dummy, None, 1, dummy, None, dummy, None, dummy, dummy, None) == -1  # (default opts: MAP)
    assert b"taxon_index" in lib.mdfit_last_error()
    assert fb(None, None, None, 0, dummy, ctypes.byref(mapo), None, None, None, None, None) == -1
    # ... and the plain entry's argument checks are the indexed one's with a null index
    assert fb(dummy, dummy, None, 1, None, ctypes.byref(nuts), None, None, dummy, dummy, None) == -1
    assert b"null" in lib.mdfit_last_error()
    ar = lib.mdfit_auto_route
    assert ar(None, None, None, -1, None, None, None) == -1 and b"n_taxa" in lib.mdfit_last_error()
    assert ar(None, None, None, 0, None, None, None) == 0
    assert ar(dummy, dummy, dummy, 1, dummy, None, None) == -1 and b"null" in lib.mdfit_last_error()
    assert ar(dummy, dummy, dummy, (1 << 25) + 1, dummy, dummy, None) == -1 and b"2^25" in lib.mdfit_last_error()


# --------------------------------------------------------------------------
# the host build of csrc/mdfit_auto.h
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("auto_host") / "auto_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-I", str(ROOT / "tests" / "host_shim"),
                    str(ROOT / "tests" / "auto_host_main.cpp"), "-o", str(exe)], check=True)
    return exe


def run_host(exe, tmp_path, st, psis, waic, out):
    T = len(st)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int64(T).tobytes())
        for a, dt in ((st, np.int32), (psis, np.float64), (waic, np.float64), (out, np.float64)):
            f.write(np.ascontiguousarray(a, dtype=dt).tobytes())
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    raw = dst.read_bytes()
    route = np.frombuffer(raw[: 4 * T], dtype=np.int32)
    return route, np.frombuffer(raw[4 * T:], dtype=np.float64).reshape(T, ref.NOUT)


def test_crafted_records_cover_every_route():
    st, psis, waic, out = ref.crafted()
    route, comp = ref.auto_route(st, psis, waic, out)
    # every bit alone, the combinations, and taxa that go each way
    for want in (0, 1, 2, 3, 4, 5, 6, 7, 8):
        assert (route == want).any(), want
    assert set(route[st == ref.INVALID]) == {8} and (route[st != ref.INVALID] < 8).all()
    assert ((route & 4) != 0).tolist() == [s in (1, 2) for s in st]
    # only route-0 rows change, and only in the nine columns
    changed = comp.view(np.int64) != out.view(np.int64)
    assert not changed[route != 0].any()
    assert not changed[:, [c for c in range(ref.NOUT) if c not in ref.COMPOSED]].any()
    assert changed[route == 0][:, ref.COMPOSED].all()
    assert np.isnan(out[st == ref.INVALID]).all() and np.isnan(comp[st == ref.INVALID]).all()


def test_host_program_equals_reference(host_program, tmp_path):
    st, psis, waic, out = ref.crafted()
    want_route, want_out = ref.auto_route(st, psis, waic, out)
    route, got = run_host(host_program, tmp_path, st, psis, waic, out)
    np.testing.assert_array_equal(route, want_route)
    np.testing.assert_array_equal(got.view(np.int64), want_out.view(np.int64))  # bit patterns: NaN, -0.0, subnormal
    # flags that are no integer (NaN, negative, huge) have no bit: routed to the sampler
    st2 = np.zeros(3, np.int32)
    p2, w2, o2 = psis[:3].copy(), waic[:3].copy(), out[:3].copy()
    p2[:, :, -1], w2[:, :, -1] = 63.0, 63.0
    w2[0, 6, -1], w2[1, 6, -1], p2[2, 1, -1] = -2.0, 1e300, -3.0
    r2, g2 = run_host(host_program, tmp_path, st2, p2, w2, o2)
    w_r2, w_o2 = ref.auto_route(st2, p2, w2, o2)
    assert r2.tolist() == w_r2.tolist() == [1, 1, 2]
    np.testing.assert_array_equal(g2.view(np.int64), w_o2.view(np.int64))
    assert run_host(host_program, tmp_path, st[:0], psis[:0], waic[:0], out[:0])[0].size == 0


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


NEW_COLUMNS = ["auto_route", "auto_sampled", "pareto_k_max", "psis_ess_min"]


def test_frame_columns_and_dtypes(tmp_path, oracle_lib, ref_meta):
    from metadamage_amd import fits

    cfg = _cfg(tmp_path)
    p = fits.pack_counts(pd.read_parquet(GOLDEN / "counts_data_ancient.parquet"), cfg)
    out, pred, st = oracle_lib.fit_batch(p.y, p.N, p.mm)
    auto = np.array([[0, 0, 0.25, 200.5], [1, 1, 0.9, 12.0], [5, 1, np.nan, np.nan]], dtype=np.float32)
    keep = st == 0
    assert keep.all() and len(keep) == 3
    plain = fits.make_df_fit_results(p, out, keep, cfg)
    df = fits.make_df_fit_results(p, out, keep, cfg, auto=auto)
    assert list(df.columns) == ref_meta["fit_results_columns"] + NEW_COLUMNS and len(df.columns) == 34
    assert NEW_COLUMNS == fits.AUTO_UINT_COLUMNS + fits.AUTO_COLUMNS
    pd.testing.assert_frame_equal(df[plain.columns], plain)  # the 25 columns (and the names) stay as they are
    assert df["auto_route"].dtype == np.uint32 and df["auto_sampled"].dtype == np.uint32
    assert df["pareto_k_max"].dtype == np.float32 and df["psis_ess_min"].dtype == np.float32
    assert df["auto_route"].tolist() == [0, 1, 5] and df["auto_sampled"].tolist() == [0, 1, 1]
    np.testing.assert_array_equal(df["pareto_k_max"].to_numpy(), auto[:, 2])
    np.testing.assert_array_equal(df["psis_ess_min"].to_numpy(), auto[:, 3])
    k2 = np.array([True, False, True])  # a dropped taxon takes its row with it
    d2 = fits.make_df_fit_results(p, out, k2, cfg, auto=auto)
    assert d2["auto_route"].tolist() == [0, 5]


def test_make_opts_config_and_cli(tmp_path):
    from typer.testing import CliRunner

    from metadamage_amd import _lib, engine, fits
    from metadamage_amd.cli import cli_app

    o = fits.make_opts(_cfg(tmp_path, "auto"), dict(num_warmup=70, num_samples=90))
    n = fits.make_opts(_cfg(tmp_path, "nuts"), dict(num_warmup=70, num_samples=90))
    assert bytes(o) == bytes(n) and o.mode == _lib.MODE_NUTS
    # the two option sets of the call are copies of one: only the mode differs
    o.seed, o.index_base = 11, 1000
    om, on = engine.auto_opts(o)
    assert (om.mode, on.mode) == (_lib.MODE_MAP, _lib.MODE_NUTS)
    om.mode = on.mode
    assert bytes(om) == bytes(on) == bytes(o)
    dm, dn = engine.auto_opts(None)
    assert (dm.mode, dn.mode, dn.num_warmup, dn.num_samples, dm.max_iter) == (0, 1, 500, 1000, 200)
    assert fits.wants_auto(_cfg(tmp_path, "auto"))
    for other in ("map", "map-waic", "map-psis", "nuts", "nuts-loo"):
        assert not fits.wants_auto(_cfg(tmp_path, other)), other
    for w in (fits.wants_waic, fits.wants_psis, fits.wants_laplace, fits.wants_loo, fits.wants_diag,
              fits.wants_summary):
        assert not w(_cfg(tmp_path, "auto"))
    assert fits.psis_draws_of(_cfg(tmp_path, "auto")) == 256
    assert fits.psis_draws_of(_cfg(tmp_path, "auto", psis_draws=100)) == 100
    # the metadata records the inference and keeps the draws (the cache key)
    d = _cfg(tmp_path, "auto", psis_draws=100).to_dict()
    assert d["inference"] == "auto" and d["psis_draws"] == 100
    for other in ("map", "nuts"):
        assert "psis_draws" not in _cfg(tmp_path, other).to_dict(), other
    with pytest.raises(ValueError, match="auto"):
        fits.mode_of("automatic")
    runner = CliRunner()
    base = ["fit", str(GOLDEN / "data_ancient.txt"), "--out-dir", str(tmp_path)]
    bad = runner.invoke(cli_app, base + ["--inference", "auto-foo"])
    assert bad.exit_code == 2 and "auto" in bad.output
    # accepted: the option check passes and the draws are validated for it
    for k in ("24", "1025"):
        bad = runner.invoke(cli_app, base + ["--inference", "auto", "--psis-draws", k])
        assert bad.exit_code == 2 and "psis-draws" in bad.output
    assert "auto:" in runner.invoke(cli_app, ["fit", "--help"], terminal_width=200).output


def test_gather_record_with_auto_round_trips():
    import torch

    from metadamage_amd import _lib, distributed as d

    assert d.REC_BYTES == 496 and d.REC_AUTO == 16 == _lib.NAUTO * 4
    n = 7
    rng = np.random.default_rng(3)
    buf = torch.from_numpy(rng.integers(0, 256, n * (d.REC_BYTES + d.REC_AUTO), dtype=np.uint8))
    pred, status, ints, floats, av = d.packed_views(buf, n, with_auto=True)
    p0, s0, i0, f0 = d.packed_views(buf[: n * d.REC_BYTES], n)  # the default layout is a prefix
    assert pred.data_ptr() == p0.data_ptr() and status.data_ptr() == s0.data_ptr()
    assert ints.data_ptr() == i0.data_ptr() and floats.data_ptr() == f0.data_ptr()
    assert av.shape == (n, _lib.NAUTO) and av.dtype == torch.float32
    assert av.data_ptr() == buf.data_ptr() + n * d.REC_BYTES
    want = rng.standard_normal((n, 4)).astype(np.float32)
    want[0, 2] = np.nan
    av.copy_(torch.from_numpy(want))
    st = rng.integers(0, 4, n).astype(np.int32)
    status.copy_(torch.from_numpy(st))
    ints.copy_(torch.from_numpy(np.rint(rng.standard_normal(tuple(ints.shape)) * 100)))
    floats.copy_(torch.from_numpy(rng.standard_normal(tuple(floats.shape)).astype(np.float32)))
    pred.copy_(torch.from_numpy(rng.standard_normal(tuple(pred.shape)).astype(np.float32)))
    out, pr, ss, got = d.unpack_gathered([buf, buf.clone()], 13, 2, with_auto=True)
    assert out.shape == (13, 25) and got.shape == (13, 4) and got.dtype == np.float32
    np.testing.assert_array_equal(got[:7], want)
    np.testing.assert_array_equal(got[7:], want[:6])
    np.testing.assert_array_equal(ss[7:], st[:6])
    rec = d.alloc_records(5, "cpu", with_auto=True)
    assert rec.auto.shape == (5, 4) and rec.waic is None and rec.buf.numel() == 5 * (d.REC_BYTES + d.REC_AUTO)
    for other in ("with_laplace", "with_diag", "with_summary", "with_loo", "with_psis", "with_waic"):
        with pytest.raises(ValueError, match="mutually exclusive"):
            d.packed_views(buf, n, with_auto=True, **{other: True})
        with pytest.raises(ValueError, match="mutually exclusive"):
            d.alloc_records(3, "cpu", with_auto=True, **{other: True})
