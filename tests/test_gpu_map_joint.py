"""mdfit_map_joint / mdfit_map_joint_adapt on the GPU: the fused launch returns,
bit for bit, the waic record, pointwise, draws and adapt of mdfit_map_waic
[_adapt], the evid record of mdfit_map_evidence[_adapt] and the psis record of
mdfit_map_psis[_adapt] at equal (S, seed, index_base, rounds).

Inputs and configurations are those of tools/record_map_is_bits_golden.py and
its fixture tests/golden/map_is_bits_parent.npz (read, not changed): 64 taxa of
generate(300, seed=21) plus the crafted y > N taxon; S = 25 plain, S = 65 with
two rounds, S = 256 plain and with four rounds; seed 0, index_base 7.  The
reference is the three existing entries run here, in the same process.
"""

from __future__ import annotations

import numpy as np
import pytest

from tests.helpers import GOLDEN
from tests.test_gpu_map_is_bits import TOOL

pytestmark = pytest.mark.gpu

SEED, INDEX_BASE = TOOL.SEED, TOOL.INDEX_BASE
FLAG_VALID, FLAG_RELIABLE, FLAG_ADAPTED = 1, 2, 64


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    return torch


@pytest.fixture(scope="module")
def batch(torch_dev):
    """The fixture's 65 taxa on the device, fitted once by one MODE_MAP call."""
    from metadamage_amd import _lib, engine, synthetic

    golden = np.load(GOLDEN / "map_is_bits_parent.npz")
    y, N, mm = TOOL.inputs(synthetic, golden["indices"])
    ty, tN, tm = engine.to_device_counts(y, N, mm)
    res = engine.fit_batch_device(ty, tN, tm, _lib.default_opts(mode=_lib.MODE_MAP))
    torch_dev.cuda.synchronize()
    return {"y": y, "N": N, "mm": mm, "ty": ty, "tN": tN, "res": res}


def _host(*ts):
    return [np.ascontiguousarray(t.cpu().numpy()) for t in ts]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype.itemsize == 8 else a.view(np.int32)


def _reference(engine, b, S, rounds):
    """{name: host array} of the three existing entries."""
    kw = {} if rounds is None else {"adapt_rounds": rounds, "adapt": True}
    ty, tN, res = b["ty"], b["tN"], b["res"]
    w = engine.map_waic_device(ty, tN, res, S, SEED, INDEX_BASE, pointwise=True, draws=True, **kw)
    e = engine.map_evidence_device(ty, tN, res, S, SEED, INDEX_BASE, **kw)
    p = engine.map_psis_device(ty, tN, res, S, SEED, INDEX_BASE, **kw)
    ref = dict(zip(("waic", "pointwise", "draws"), _host(*w[:3])))
    if rounds is not None:
        ref["adapt"] = _host(w[3])[0]
        e, p = e[0], p[0]
    ref["evid"], ref["psis"] = _host(e, p)
    return ref


def _joint(engine, b, S, rounds, **more):
    kw = {} if rounds is None else {"adapt_rounds": rounds, "adapt": True}
    got = engine.map_joint_device(b["ty"], b["tN"], b["res"], S, SEED, INDEX_BASE, pointwise=True, draws=True,
                                  **kw, **more)
    names = ("waic", "evid", "psis", "pointwise", "draws") + (("adapt",) if rounds is not None else ())
    assert len(got) == len(names)
    return dict(zip(names, _host(*got)))


@pytest.fixture(scope="module")
def runs(torch_dev, batch):
    """Per configuration: (reference, fused), each computed once and left unchanged."""
    from metadamage_amd import engine

    out = {}
    for name, (S, _R, rounds) in TOOL.CONFIGS.items():
        ref, got = _reference(engine, batch, S, rounds), _joint(engine, batch, S, rounds)
        for a in (*ref.values(), *got.values()):
            a.setflags(write=False)
        out[name] = (ref, got)
    return out


@pytest.mark.parametrize("config", sorted(TOOL.CONFIGS))
def test_fused_launch_returns_the_three_entries_bits(runs, batch, config):
    S, _R, rounds = TOOL.CONFIGS[config]
    ref, got = runs[config]
    T = TOOL.N_TAXA + 1
    shapes = {"waic": (T, 7, 8), "evid": (T, 7, 8), "psis": (T, 3, 16), "pointwise": (T, 6, 30, 2),
              "draws": (T, 6, S, 6)}
    if rounds is not None:
        shapes["adapt"] = (T, 3, 4)
    assert set(ref) == set(got) == set(shapes)
    bad = []
    for name, shape in shapes.items():
        assert ref[name].shape == got[name].shape == shape and got[name].dtype == np.float64, name
        n = int((_bits(got[name]) != _bits(ref[name])).sum())
        print(f"{config}/{name}: {n} of {got[name].size} words differ from the separate entry's")
        if n:
            bad.append(name)
    assert not bad, bad


def test_compared_set_holds_every_kind_of_row(runs, batch):
    """Read off the reference's records, not the fused ones: over the four configurations each of the three
    records shows a taxon with a bad status, a fitted taxon's row without the valid bit and a valid row over the khat
    threshold; each configuration with rounds shows an adapted row."""
    st = _host(batch["res"].status)[0]
    ok = st == 0
    assert (~ok).any() and ok.sum() > 32
    for pick in (lambda r: r["waic"][:, :6, 7], lambda r: r["evid"][:, :6, 7], lambda r: r["psis"][:, :, 15]):
        invalid = over = False
        for config, (_S, _R, rounds) in TOOL.CONFIGS.items():
            ref = runs[config][0]
            fl = np.nan_to_num(pick(ref)).astype(np.int64)
            assert (fl[~ok] == 0).all()
            valid = (fl & FLAG_VALID) != 0
            invalid |= bool((~valid[ok]).any())
            over |= bool((valid & ((fl & FLAG_RELIABLE) == 0)).any())
            assert bool(((fl & FLAG_ADAPTED) != 0).any()) == (rounds is not None), config
        assert invalid and over
    for config in TOOL.CONFIGS:
        ref = runs[config][0]
        assert np.isnan(ref["evid"][~ok, :, :7]).all() and np.isnan(ref["psis"][~ok, :, :15]).all()
        assert np.isnan(ref["waic"][~ok, :, :7]).all()


def test_chunked_dispatch_equals_the_single_call(torch_dev, batch, monkeypatch):
    from metadamage_amd import _lib, engine

    S, rounds = 65, 2
    T = TOOL.N_TAXA + 1
    b = batch
    w, e, p, ad = engine.map_joint_device(b["ty"], b["tN"], b["res"], S, SEED, 0, adapt_rounds=rounds, adapt=True)
    want_w = _host(w)[0].astype(np.float32)
    want_j = np.concatenate([_host(e)[0].reshape(T, -1), _host(p)[0].reshape(T, -1)], axis=1).astype(np.float32)
    want_ad = _host(engine.adapt_summary(ad))[0]
    opts = _lib.default_opts(mode=_lib.MODE_MAP)
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "27")  # 65 = 21 + 22 + 22
    chunks = engine.plan_chunks(T, opts, with_waic=True, joint=True)
    assert len(chunks) == 3 and len({hi - lo for lo, hi in chunks}) > 1
    got = engine.fit_batch_host(b["y"], b["N"], b["mm"], opts, waic=True, joint=True, psis_draws=S, psis_adapt=rounds)
    assert len(got) == 6
    o, _pred, s, gw, gj, ga = got
    assert gw.shape == (T, 7, 8) and gj.shape == (T, _lib.NJOINTOUT) == (T, 104) and ga.shape == (T, 2)
    assert gw.dtype == gj.dtype == ga.dtype == np.float32
    assert np.array_equal(_bits(gw), _bits(want_w))
    assert np.array_equal(_bits(gj), _bits(want_j))
    assert np.array_equal(_bits(ga), _bits(want_ad))
    ge, gp = engine.split_joint(gj)
    assert np.array_equal(_bits(ge), _bits(_host(e)[0].astype(np.float32)))
    assert np.array_equal(_bits(gp), _bits(_host(p)[0].astype(np.float32)))
    # without the option: the waic run's tuple, the same waic block
    plain = engine.fit_batch_host(b["y"], b["N"], b["mm"], opts, waic=True, psis_draws=S, psis_adapt=rounds)
    assert len(plain) == 5
    assert np.array_equal(_bits(plain[3]), _bits(gw)) and np.array_equal(_bits(plain[4]), _bits(ga))
    assert np.array_equal(plain[0], o, equal_nan=True) and np.array_equal(plain[2], s)


def test_fit_packed_puts_the_columns_in_the_frame(torch_dev, batch, tmp_path):
    from metadamage_amd import _lib, fits, utils

    b = batch
    T = TOOL.N_TAXA + 1
    S = 65

    def packed():
        return fits.Packed(np.arange(T), np.array([f"t{i}" for i in range(T)]), np.array(["species"] * T),
                           np.full(T, 100, np.int64), np.array(b["y"]), np.array(b["N"]), np.array(b["mm"]))

    opts = _lib.default_opts(mode=_lib.MODE_MAP)
    got = fits.fit_packed(packed(), opts, shard=False, waic=True, joint=True, psis_draws=S)
    assert len(got) == 5 and got[4].shape == (T, 104)
    out, _pred, status, waic, joint = got
    cfg = utils.Config(out_dir=tmp_path, max_fits=10, max_cores=1, min_alignments=10, min_y_sum=10,
                       substitution_bases_forward="CT", substitution_bases_reverse="GA", forced=False,
                       version="0.0.0", inference="map-waic", joint=True)
    cfg.add_filename(GOLDEN / "data_ancient.txt")
    keep = status == _lib.OK
    assert not keep.all()
    df = fits.make_df_fit_results(packed(), out, keep, cfg, waic=waic, joint=joint)
    new = (fits.MAP_WAIC_COLUMNS + fits.MAP_WAIC_UINT_COLUMNS + fits.MAP_EVIDENCE_COLUMNS
           + fits.MAP_EVIDENCE_UINT_COLUMNS + fits.MAP_PSIS_COLUMNS + fits.MAP_PSIS_UINT_COLUMNS)
    assert list(df.columns[-len(new):]) == new and len(df) == int(keep.sum())
    # the values are the separate runs' values
    ev = fits.fit_packed(packed(), opts, shard=False, evidence=True, psis_draws=S)[3]
    ps = fits.fit_packed(packed(), opts, shard=False, psis=True, psis_draws=S)[3]
    de = fits.make_df_fit_results(packed(), out, keep, cfg, evid=ev)
    dp = fits.make_df_fit_results(packed(), out, keep, cfg, psis=ps)
    for ref, cols in ((de, fits.MAP_EVIDENCE_COLUMNS + fits.MAP_EVIDENCE_UINT_COLUMNS),
                      (dp, fits.MAP_PSIS_COLUMNS + fits.MAP_PSIS_UINT_COLUMNS)):
        for c in cols:
            assert df[c].dtype == ref[c].dtype and np.array_equal(_bits(df[c].to_numpy()), _bits(ref[c].to_numpy())), c
    assert (df["map_evidence_valid"] == 1).any() and (df["map_psis_valid"] == 1).any()
    # the sharded branch as rank 0 of a world of one: the gather record carries the joint tail
    from metadamage_amd import blocks

    dev = torch_dev.device("cuda", torch_dev.cuda.current_device())
    run = blocks.describe(opts, {"psis_adapt": 0, "joint": True}, with_waic=True, psis_draws=S, pred_draws=1000,
                          dmax_threshold=0.01)
    sh = fits._fit_sharded(packed(), opts, dev, 0, 1, run)
    assert len(sh) == 5 and np.array_equal(_bits(sh[4]), _bits(joint)) and np.array_equal(_bits(sh[3]), _bits(waic))


@pytest.mark.parametrize("rounds", (None, 2))
def test_capturable_in_a_graph_on_one_stream(torch_dev, batch, runs, rounds):
    from metadamage_amd import _lib, engine

    torch = torch_dev
    S = 65
    T = TOOL.N_TAXA + 1
    b = batch
    want = runs["B"][1] if rounds is not None else _joint(engine, b, S, None)
    dev = b["ty"].device
    dst = {"waic": torch.zeros((T, 7, 8), dtype=torch.float64, device=dev),
           "evid": torch.zeros((T, 7, 8), dtype=torch.float64, device=dev),
           "psis": torch.zeros((T, 3, 16), dtype=torch.float64, device=dev)}
    kw = {"adapt_rounds": rounds, "adapt": torch.zeros((T, 3, _lib.NMAPADAPT), dtype=torch.float64, device=dev)} \
        if rounds is not None else {}
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):  # one stream, one kernel node, no branches
        engine.map_joint_device(b["ty"], b["tN"], b["res"], S, SEED, INDEX_BASE, stream=torch.cuda.current_stream(),
                                **dst, **kw)
    for t in dst.values():
        t.fill_(0.0)
    g.replay()
    torch.cuda.synchronize()
    for name, t in dst.items():
        assert np.array_equal(_bits(_host(t)[0]), _bits(want[name])), name
    if rounds is not None:
        assert np.array_equal(_bits(_host(kw["adapt"])[0]), _bits(want["adapt"]))
