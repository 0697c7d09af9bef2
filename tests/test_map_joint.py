"""map-waic --joint without a device: the two C-ABI entries and their argument
checks, the memory plan, the gather record's joint tail, the frame's columns
and the option's way through Config, the metadata and the CLI (DESIGN.md
§3.18)."""

from __future__ import annotations

import ctypes

import numpy as np
import pandas as pd
import pytest

from tests.helpers import GOLDEN

D = ctypes.c_void_p(16)
D4 = (D, D, D, D)
E_ARG = -1


@pytest.fixture(scope="module")
def lib():
    from metadamage_amd import _lib

    return _lib.load()


# --------------------------------------------------------------------------
# the C-ABI
# --------------------------------------------------------------------------
def test_symbols_resolve(lib):
    from metadamage_amd import _lib

    for name in ("mdfit_map_joint", "mdfit_map_joint_adapt"):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert _lib.NJOINTOUT == 7 * _lib.NMAPEVID + 3 * _lib.NMAPPSIS == 104


@pytest.mark.parametrize("S", [24, 1025])
def test_num_draws_out_of_range_is_an_argument_error(lib, S):
    assert lib.mdfit_map_joint(*D4, 1, S, 0, 0, D, D, D, None, None, None) == E_ARG
    assert lib.mdfit_last_error() == b"num_draws must be in [25, 1024]"
    assert lib.mdfit_map_joint_adapt(*D4, 1, S, 2, 0, 0, D, D, D, None, None, None, None) == E_ARG
    assert lib.mdfit_last_error() == b"num_draws must be in [25, 1024]"


@pytest.mark.parametrize("rounds", [-1, 5])
def test_adapt_rounds_out_of_range_is_an_argument_error(lib, rounds):
    assert lib.mdfit_map_joint_adapt(*D4, 1, 256, rounds, 0, 0, D, D, D, None, None, None, None) == E_ARG
    assert lib.mdfit_last_error() == b"adapt_rounds must be in [0, 4]"


@pytest.mark.parametrize("missing", [0, 1, 2])
def test_null_record_is_an_argument_error(lib, missing):
    recs = [D, D, D]
    recs[missing] = None  # waic, evid, psis
    assert lib.mdfit_map_joint(*D4, 1, 256, 0, 0, *recs, None, None, None) == E_ARG
    assert lib.mdfit_last_error() == b"null required pointer"
    assert lib.mdfit_map_joint_adapt(*D4, 1, 256, 2, 0, 0, *recs, None, None, None, None) == E_ARG
    assert lib.mdfit_last_error() == b"null required pointer"
    # no taxa: nothing to do, whatever the pointers
    assert lib.mdfit_map_joint(*D4, 0, 256, 0, 0, *recs, None, None, None) == 0


# --------------------------------------------------------------------------
# the memory plan
# --------------------------------------------------------------------------
def test_plan_counts_the_joint_records():
    from metadamage_amd import _lib, engine

    o = _lib.default_opts(mode=_lib.MODE_MAP)
    a = engine.device_bytes(1000, o, with_waic=True)
    assert engine.device_bytes(1000, o, with_waic=True, joint=True) - a == 1000 * (832 + 416)
    assert engine.device_bytes(1000, o, with_waic=True, joint=True, dest_on_device=True) \
        - engine.device_bytes(1000, o, with_waic=True, dest_on_device=True) == 1000 * 832
    assert engine.device_bytes(1000, o, with_waic=True, joint=False) == a
    budget = 2 * engine.device_bytes(50, o, with_waic=True)
    assert max(hi - lo for lo, hi in engine.plan_chunks(200, o, budget, with_waic=True)) == 50
    assert max(hi - lo for lo, hi in engine.plan_chunks(200, o, budget, with_waic=True, joint=True)) < 50
    for kw in ({}, {"with_psis": True}, {"with_evidence": True}, {"with_ppred": True}, {"with_laplace": True}):
        with pytest.raises(ValueError, match="joint needs with_waic"):
            engine.device_bytes(10, o, joint=True, **kw)
        with pytest.raises(ValueError, match="joint needs with_waic"):
            engine.plan_chunks(10, o, joint=True, **kw)


def test_split_joint():
    from metadamage_amd import engine

    block = np.arange(5 * 104, dtype=np.float32).reshape(5, 104)
    evid, psis = engine.split_joint(block)
    assert evid.shape == (5, 7, 8) and psis.shape == (5, 3, 16)
    assert np.array_equal(evid.reshape(5, -1), block[:, :56]) and np.array_equal(psis.reshape(5, -1), block[:, 56:])


# --------------------------------------------------------------------------
# the gather record
# --------------------------------------------------------------------------
def test_gather_record_carries_the_joint_tail():
    import torch

    from metadamage_amd import distributed as d

    n = 5
    assert (d.REC_BYTES, d.REC_WAIC, d.REC_JOINT) == (496, 224, 416)
    rec = d.alloc_records(n, "cpu", with_waic=True, with_joint=True)
    assert rec.buf.numel() == n * (496 + 224 + 416)
    assert rec.joint.shape == (n, 104) and rec.joint.dtype == torch.float32 and rec.quant is None and rec.adapt is None
    p0 = rec.buf.data_ptr()
    assert rec.waic.data_ptr() == p0 + n * d.REC_BYTES
    assert rec.joint.data_ptr() == p0 + n * (d.REC_BYTES + d.REC_WAIC)  # right behind the waic block ...
    with_ad = d.alloc_records(n, "cpu", with_waic=True, with_joint=True, with_adapt=True)
    assert with_ad.adapt.data_ptr() == with_ad.buf.data_ptr() + n * (496 + 224 + 416)  # ... and before the adapt tail
    today = d.alloc_records(n, "cpu", with_waic=True, with_adapt=True)
    assert today.joint is None and today.buf.numel() == n * (496 + 224 + 8)
    for kw in ({}, *({b.switch: True} for b in d.blocks.BLOCKS if b.name != "waic")):
        with pytest.raises(ValueError, match="with_joint goes with with_waic"):
            d.alloc_records(n, "cpu", with_joint=True, **kw)
    # a two-part round trip over random bytes
    rng = np.random.default_rng(5)
    for with_adapt in (True, False):
        r = d.alloc_records(n, "cpu", with_waic=True, with_joint=True, with_adapt=with_adapt)
        r.buf.copy_(torch.from_numpy(rng.integers(0, 256, r.buf.numel(), dtype=np.uint8)))
        r.floats.zero_()  # (random bytes there can be signalling NaN, which numpy's f32 -> f64 cast warns about)
        want_j = rng.integers(0, 1 << 32, (n, 104), dtype=np.uint32).view(np.float32)
        want_w = rng.standard_normal((n, 7, 8)).astype(np.float32)
        r.joint.copy_(torch.from_numpy(want_j))
        r.waic.copy_(torch.from_numpy(want_w))
        got = d.unpack_gathered([r.buf, r.buf.clone()], 2 * n - 1, 2, with_waic=True, with_joint=True,
                                with_adapt=with_adapt)
        assert len(got) == (6 if with_adapt else 5)
        assert np.array_equal(got[3], np.concatenate([want_w, want_w[: n - 1]]))
        assert np.array_equal(got[4].view(np.uint32), np.concatenate([want_j, want_j[: n - 1]]).view(np.uint32))
        if with_adapt:
            assert np.array_equal(got[5].view(np.uint32),
                                  np.concatenate([r.adapt.numpy(), r.adapt.numpy()[: n - 1]]).view(np.uint32))


# --------------------------------------------------------------------------
# options, cache key, CLI
# --------------------------------------------------------------------------
def _cfg(tmp_path, inference="map-waic", **kw):
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

    assert utils.Config.__dataclass_fields__["joint"].default is False
    others = ("map", "nuts", "auto", "map-psis", "map-pred", "map-evidence", "map-laplace", "nuts-summary")
    for inference in ("map-waic", *others):
        d0 = _cfg(tmp_path, inference).to_dict()
        assert "joint" not in d0 and not fits.joint_of(_cfg(tmp_path, inference))
        assert _cfg(tmp_path, inference, joint=False).to_dict() == d0
    d0 = _cfg(tmp_path).to_dict()
    d1 = _cfg(tmp_path, joint=True).to_dict()
    assert d1["joint"] is True and {k: v for k, v in d1.items() if k != "joint"} == d0
    assert fits.joint_of(_cfg(tmp_path, joint=True)) and "joint" in fits.CACHE_KEYS
    sim = utils.metadata_is_similar
    assert sim(d0, dict(d0), include=fits.CACHE_KEYS) and sim(d1, dict(d1), include=fits.CACHE_KEYS)
    assert not sim(d0, d1, include=fits.CACHE_KEYS) and not sim(d1, d0, include=fits.CACHE_KEYS)
    for inference in others:
        with pytest.raises(ValueError, match="joint goes with inference 'map-waic'"):
            _cfg(tmp_path, inference, joint=True)
    # --psis-draws and --psis-adapt apply as to map-waic
    cfg = _cfg(tmp_path, joint=True, psis_draws=64, psis_adapt=2)
    assert fits.psis_draws_of(cfg) == 64 and fits.psis_adapt_of(cfg) == 2
    runner = CliRunner()
    base = ["fit", str(GOLDEN / "data_ancient.txt"), "--out-dir", str(tmp_path)]
    for inference in others:
        bad = runner.invoke(cli_app, base + ["--inference", inference, "--joint"])
        assert bad.exit_code != 0 and "--joint" in bad.output, inference
    assert "--joint" in runner.invoke(cli_app, ["fit", "--help"], terminal_width=200).output
    # the optional arrays behind (out, pred, status): adapt stays last once the joint block is taken out
    x, a = object(), object()
    assert fits._split_rest(_cfg(tmp_path, joint=True, psis_adapt=2), [x, a]) == (x, None, a)


# --------------------------------------------------------------------------
# frames
# --------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def test_frames_from_random_records(tmp_path, oracle_lib, ref_meta):
    from metadamage_amd import fits

    cfg = _cfg(tmp_path, joint=True)
    p = fits.pack_counts(pd.read_parquet(GOLDEN / "counts_data_ancient.parquet"), cfg)
    out3, _pred, st = oracle_lib.fit_batch(p.y, p.N, p.mm)
    assert (st == 0).all() and len(st) == 3
    # sixteen rows: every combination of valid, reliable, c free and adapted in the flags, a few NaN rows
    T = 16
    idx = np.arange(T) % 3
    pk = fits.Packed(p.tax_id[idx], p.tax_name[idx], p.tax_rank[idx], p.N_alignments[idx], p.y[idx], p.N[idx],
                     p.mm[idx])
    out = out3[idx]
    rng = np.random.default_rng(3)
    combos = np.array([(v, r, c, a) for v in (0, 1) for r in (0, 1) for c in (0, 1) for a in (0, 1)])
    flags = (combos[:, 0] * 1 + combos[:, 1] * 2 + 4 + 8 + combos[:, 2] * 16 + 32 + combos[:, 3] * 64).astype(np.float32)
    evid = (rng.standard_normal((T, 7, 8)) * 30).astype(np.float32)
    psis = rng.standard_normal((T, 3, 16)).astype(np.float32)
    waic = rng.standard_normal((T, 7, 8)).astype(np.float32)
    evid[:, :6, 7] = flags[:, None]
    evid[:, 6, 7] = (combos[:, 0] * 1 + combos[:, 0] * combos[:, 1] * 2).astype(np.float32)
    evid[3, 6, 0] = 200.0  # (damage_probability: exp(-log_bf) underflows ...
    evid[4, 6, 0] = -200.0  # ... and overflows)
    psis[:, :, 15] = np.stack([flags, np.roll(flags, 1), np.roll(flags, 5)], axis=1)
    waic[:, 6, 7] = evid[:, 6, 7]
    for t in (0, 7, 11):
        evid[t, :, :7] = np.nan
        psis[t, :, :15] = np.nan
    evid[9, 2] = np.nan  # (a NaN flags word too)
    psis[9, 1] = np.nan
    joint = np.concatenate([evid.reshape(T, -1), psis.reshape(T, -1)], axis=1)
    assert joint.shape == (T, 104)
    adapt = rng.standard_normal((T, 2)).astype(np.float32)
    base = ref_meta["fit_results_columns"]
    ev_cols = fits.MAP_EVIDENCE_COLUMNS + fits.MAP_EVIDENCE_UINT_COLUMNS
    ps_cols = fits.MAP_PSIS_COLUMNS + fits.MAP_PSIS_UINT_COLUMNS
    wa_cols = fits.MAP_WAIC_COLUMNS + fits.MAP_WAIC_UINT_COLUMNS
    assert ev_cols.index("damage_probability") == 7
    for keep in (np.ones(T, bool), np.arange(T) % 4 != 1):
        df = fits.make_df_fit_results(pk, out, keep, cfg, waic=waic, joint=joint)
        assert list(df.columns) == base + wa_cols + ev_cols + ps_cols and len(df) == int(keep.sum())
        de = fits.make_df_fit_results(pk, out, keep, cfg, evid=evid)
        dp = fits.make_df_fit_results(pk, out, keep, cfg, psis=psis)
        for ref, cols in ((de, ev_cols), (dp, ps_cols)):
            for c in cols:
                assert df[c].dtype == ref[c].dtype, c
                assert np.array_equal(_bits(df[c].to_numpy()), _bits(ref[c].to_numpy())), c
        # without joint the frame is today's
        today = fits.make_df_fit_results(pk, out, keep, cfg, waic=waic)
        assert list(today.columns) == base + wa_cols
        pd.testing.assert_frame_equal(df[today.columns], today)
        both = fits.make_df_fit_results(pk, out, keep, cfg, waic=waic, joint=joint, adapt=adapt)
        assert list(both.columns) == list(df.columns) + fits.ADAPT_COLUMNS  # the adapt columns stay last
    full = fits.make_df_fit_results(pk, out, np.ones(T, bool), cfg, waic=waic, joint=joint)
    assert full["map_evidence_valid"].tolist() == combos[:, 0].tolist()
    assert full["damage_probability"][3] == 1.0 and full["damage_probability"][4] == 0.0
    assert set(full["map_psis_valid"].tolist()) == {0, 1}
    with pytest.raises(ValueError, match="joint goes with waic"):
        fits.make_df_fit_results(pk, out, np.ones(T, bool), cfg, joint=joint)
    with pytest.raises(ValueError, match="joint goes with waic"):
        fits.make_df_fit_results(pk, out, np.ones(T, bool), cfg, waic=waic, joint=joint, psis=psis)
