"""The table of the optional post-fit blocks (metadamage_amd/blocks.py) against
literals written out here, and what every layer derives from it: the chunk
plan's bytes, the gather record's layout, the one-block and mode rules."""

from __future__ import annotations

import itertools
import re

import numpy as np
import pytest

MAP, NUTS = 0, 1
# name: (switch, mode, attr, f32 shape out per taxon, bytes out, device bytes as computed; None: not chunked)
ROWS = {
    "laplace": ("with_laplace", MAP, "lap", (3, 8), 96, 192),
    "diag": ("with_diag", NUTS, "diag", (6, 12), 288, 576),
    "summary": ("with_summary", NUTS, "summ", (6, 16), 384, 768),
    "loo": ("with_loo", NUTS, "loo", (7, 8), 224, 448),
    "psis": ("with_psis", MAP, "psis", (3, 16), 192, 384),
    "waic": ("with_waic", MAP, "waic", (7, 8), 224, 448),
    "evidence": ("with_evidence", MAP, "evid", (7, 8), 224, 448),
    "ppred": ("with_ppred", MAP, "ppred", (106,), 424, 360 + 128),
    "auto": ("with_auto", None, "auto", (4,), 16, None),
}
REC = {"laplace": "LAP", "diag": "DIAG", "summary": "SUMM", "loo": "LOO", "psis": "PSIS", "waic": "WAIC",
       "evidence": "EVID", "ppred": "PPRED", "auto": "AUTO"}
INFERENCE = {"laplace": "map-laplace", "diag": "nuts-diag", "summary": "nuts-summary", "loo": "nuts-loo",
             "psis": "map-psis", "waic": "map-waic", "evidence": "map-evidence", "ppred": "map-pred", "auto": "auto"}
SAMPLED = {"psis", "waic", "evidence", "ppred", "auto"}
SWITCHES = [row[0] for row in ROWS.values()]
CHUNKED = [name for name, row in ROWS.items() if row[5] is not None]
BASE = 496  # the gather record without a block
# the tails, in the gather record's order.  name: (option, switch, the blocks it rides, f32 shape out per taxon, bytes
# out, device bytes as computed; None: not chunked)
TAIL_ROWS = {
    "ppc": ("ppc", "with_ppc", ("ppred",), (42,), 168, 30 * 4 + 12 * 8),
    "quant": ("quantiles", "with_quant", ("psis",), (48,), 192, 384),
    "joint": ("joint", "with_joint", ("waic",), (104,), 416, 832),
    "auto_pred": ("auto_pred", "with_auto_pred", ("auto",), (2,), 8, None),
    "adapt": ("psis_adapt", "with_adapt", ("psis", "waic", "evidence", "ppred", "auto"), (2,), 8, 96),
}
PPRED_ADAPT = "with_ppred_adapt"  # the ppred block's adapt tail keeps a switch of its own
PLANNED = ("ppc", "quant", "joint")  # the tails device_bytes and plan_chunks take (no psis_adapt: adapt is not counted)
# the refusals of a tail without a block it rides: by its option (engine), by its switch (distributed)
REFUSAL = {
    "ppc": ("ppc needs with_ppred: the check is of the predictive that mdfit_map_pred forms",
            "with_ppc goes with with_ppred"),
    "quant": ("quantiles needs with_psis: the order statistics are of the posterior mdfit_map_psis forms",
              "with_quant goes with with_psis"),
    "joint": ("joint needs with_waic: mdfit_map_joint writes the evidence and the posterior beside the waic record",
              "with_joint goes with with_waic"),
    "auto_pred": ("auto_pred goes with the auto inference", "with_auto_pred goes with with_auto"),
    "adapt": ("psis_adapt needs with_psis, with_waic, with_ppred or the auto inference",
              "with_adapt goes with with_psis, with_waic or with_auto"),
}
RIDES = [(tail, block) for tail, row in TAIL_ROWS.items() for block in row[2]]


def _tail_switch(tail, block):
    return PPRED_ADAPT if (tail, block) == ("adapt", "ppred") else TAIL_ROWS[tail][1]


def _opts(mode):
    from metadamage_amd import _lib

    assert (_lib.MODE_MAP, _lib.MODE_NUTS) == (MAP, NUTS)
    return _lib.default_opts(mode=mode, num_warmup=10, num_samples=100)


def _random_bytes(n, seed=0):
    import torch

    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def test_the_module_is_the_table_and_needs_no_torch():
    import subprocess
    import sys

    code = "import sys; from metadamage_amd import blocks; assert 'torch' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True)
    from metadamage_amd import blocks

    assert [b.name for b in blocks.BLOCKS] == list(ROWS)
    with pytest.raises(Exception):  # frozen
        blocks.BLOCKS[0].name = "x"


@pytest.mark.parametrize("name", list(ROWS))
def test_table_pins(name):
    from metadamage_amd import blocks, distributed as d, engine

    switch, mode, attr, shape, nbytes, dev = ROWS[name]
    (b,) = [b for b in blocks.BLOCKS if b.name == name]
    assert (b.switch, b.mode, b.attr, tuple(b.shape), b.out_bytes) == (switch, mode, attr, shape, nbytes)
    assert b.inference == INFERENCE[name] and b.sampled == (name in SAMPLED) and b.chunked == (dev is not None)
    assert int(np.prod(shape)) * 4 == nbytes == getattr(d, "REC_" + REC[name])
    assert attr in engine.FitBatch.__dataclass_fields__
    if dev is None:  # a layout entry only: the chunked dispatch refuses it
        for f in (engine.device_bytes, engine.plan_chunks):
            with pytest.raises(ValueError, match="fit_auto_chunks"):
                f(1000, _opts(NUTS), **{switch: True})
        return
    assert b.device_bytes == dev
    o = _opts(mode)
    assert engine.device_bytes(1000, o, **{switch: True}) - engine.device_bytes(1000, o) == 1000 * (dev + nbytes)
    assert (engine.device_bytes(1000, o, dest_on_device=True, **{switch: True})
            - engine.device_bytes(1000, o, dest_on_device=True)) == 1000 * dev
    assert engine.device_bytes(1000, o, **{switch: False}) == engine.device_bytes(1000, o)
    assert engine.plan_chunks(100, o, chunk_taxa=32, **{switch: True}) == engine.plan_chunks(100, o, chunk_taxa=32)


def test_engine_constants_come_from_the_table():
    from metadamage_amd import engine

    assert (engine.LAP_BYTES, engine.DIAG_BYTES, engine.SUMM_BYTES, engine.LOO_BYTES, engine.PSIS_BYTES,
            engine.WAIC_BYTES, engine.PPRED_BYTES, engine.PPRED_WORDS) == (96, 288, 384, 224, 192, 224, 424, 106)
    assert (engine.PSIS_DRAWS, engine.PRED_DRAWS) == (256, 1000)


@pytest.mark.filterwarnings("ignore:invalid value encountered in cast")  # (random bytes hold signalling NaNs)
@pytest.mark.parametrize("name", list(ROWS))
def test_layout_round_trip(name):
    import torch

    from metadamage_amd import distributed as d

    switch, _, attr, shape, nbytes, _ = ROWS[name]
    assert d.REC_BYTES == BASE
    rec = d.alloc_records(5, "cpu", **{switch: True})
    for other in ROWS.values():
        assert (getattr(rec, other[2]) is None) == (other[2] != attr), other[2]
    assert rec.adapt is None and rec.auto_pred is None
    view = getattr(rec, attr)
    assert rec.buf.numel() == 5 * (BASE + nbytes) and tuple(view.shape) == (5, *shape)
    assert view.data_ptr() == rec.buf.data_ptr() + 5 * BASE and view.is_contiguous()
    assert d.alloc_records(5, "cpu").buf.numel() == 5 * BASE
    # 13 taxa over two parts of capacity 7: the block comes back unchanged
    rng = np.random.default_rng(3)
    parts, want = [], []
    for r, k in enumerate((7, 6)):
        buf = _random_bytes(7 * (BASE + nbytes), seed=r)
        *base, v = d.packed_views(buf, 7, **{switch: True})
        assert [x.data_ptr() for x in base] == [x.data_ptr() for x in d.packed_views(buf[: 7 * BASE], 7)]
        assert tuple(v.shape) == (7, *shape) and v.data_ptr() == buf.data_ptr() + 7 * BASE
        w = rng.standard_normal((7, *shape)).astype(np.float32)
        w.reshape(-1)[1] = np.nan
        v.copy_(torch.from_numpy(w))
        parts.append(buf)
        want.append(w[:k])
    got = d.unpack_gathered(parts, 13, 2, **{switch: True})
    assert len(got) == 4 and got[3].dtype == np.float32
    assert np.array_equal(got[3].view(np.int32), np.concatenate(want).view(np.int32))
    assert len(d.unpack_gathered([p[: 7 * BASE] for p in parts], 13, 2)) == 3


@pytest.mark.parametrize("a, b", list(itertools.combinations(SWITCHES, 2)))
def test_every_pair_is_refused_everywhere(a, b):
    from metadamage_amd import distributed as d, engine

    kw = {a: True, b: True}
    buf = _random_bytes(4 * 2000)
    for opts in (_opts(MAP), _opts(NUTS), None):  # (exclusivity comes before the mode)
        with pytest.raises(ValueError, match="mutually exclusive: one extra block per run"):
            engine.device_bytes(10, opts, **kw)
        with pytest.raises(ValueError, match="mutually exclusive: one extra block per run"):
            engine.plan_chunks(10, opts, **kw)
    with pytest.raises(ValueError, match="mutually exclusive"):
        d.packed_views(buf, 4, **kw)
    with pytest.raises(ValueError, match="mutually exclusive"):
        d.alloc_records(4, "cpu", **kw)
    with pytest.raises(ValueError, match="mutually exclusive"):
        d.unpack_gathered([buf], 4, 1, **kw)


@pytest.mark.parametrize("name", CHUNKED)
def test_mode_is_checked_by_the_chunk_plan(name):
    from metadamage_amd import blocks, engine

    switch, mode = ROWS[name][:2]
    if mode == MAP:
        wrong, match = (_opts(NUTS),), r"needs MAP records \(opts.mode == MODE_MAP\)"
        assert blocks.resolve(None, **{switch: True}).name == name  # (None: the default options, MAP)
    else:
        wrong, match = (_opts(MAP), None), r"needs the chains of a sampling call \(opts.mode == MODE_NUTS\)"
    for opts in wrong:
        for f in (engine.device_bytes, engine.plan_chunks, blocks.resolve):
            with pytest.raises(ValueError, match=match):
                f(10, opts, **{switch: True}) if f is not blocks.resolve else f(opts, **{switch: True})


def test_unknown_switch_is_a_type_error():
    from metadamage_amd import blocks, distributed as d, engine

    buf = _random_bytes(4 * BASE)
    for call in (lambda: blocks.resolve(None, with_nothing=True), lambda: blocks.select(laplace=True),
                 lambda: engine.device_bytes(10, None, with_nothing=True),
                 lambda: engine.plan_chunks(10, None, with_nothing=True),
                 lambda: d.packed_views(buf, 4, with_nothing=True),
                 lambda: d.alloc_records(4, "cpu", with_nothing=True),
                 lambda: d.unpack_gathered([buf], 4, 1, with_nothing=True),
                 lambda: d.packed_views(buf, 4, with_adapt=True)):  # (the tail switches are Records')
        with pytest.raises(TypeError, match="with_laplace, with_diag"):
            call()
    assert blocks.resolve(_opts(NUTS)) is None and blocks.select(with_psis=False) is None


def test_tail_blocks_follow_the_block():
    from metadamage_amd import distributed as d

    n = 7
    assert (d.REC_ADAPT, d.REC_AUTO_PRED) == (8, 8)
    for name in ("psis", "waic", "evidence", "auto"):
        switch, _, attr, _, nbytes, _ = ROWS[name]
        rec = d.alloc_records(n, "cpu", with_adapt=True, **{switch: True})
        assert rec.buf.numel() == n * (BASE + nbytes + 8) and tuple(rec.adapt.shape) == (n, 2)
        assert getattr(rec, attr).data_ptr() == rec.buf.data_ptr() + n * BASE
        assert rec.adapt.data_ptr() == rec.buf.data_ptr() + n * (BASE + nbytes)
    for name in ("laplace", "diag", "summary", "loo", "ppred"):
        with pytest.raises(ValueError, match="with_adapt goes with with_psis, with_waic or with_auto"):
            d.alloc_records(n, "cpu", with_adapt=True, **{ROWS[name][0]: True})
    with pytest.raises(ValueError, match="with_adapt goes with"):
        d.alloc_records(n, "cpu", with_adapt=True)
    # the auto-pred tail: behind the auto block, before the adapt block
    rec = d.alloc_records(n, "cpu", with_auto=True, with_adapt=True, with_auto_pred=True)
    base = rec.buf.data_ptr() + n * (BASE + 16)
    assert rec.buf.numel() == n * (BASE + 16 + 8 + 8)
    assert rec.auto_pred.data_ptr() == base and rec.adapt.data_ptr() == base + n * 8
    for name in ROWS:
        if name != "auto":
            with pytest.raises(ValueError, match="with_auto_pred goes with with_auto"):
                d.alloc_records(n, "cpu", with_auto_pred=True, **{ROWS[name][0]: True})
        if name != "ppred":
            with pytest.raises(ValueError, match="with_ppred_adapt goes with with_ppred"):
                d.alloc_records(n, "cpu", with_ppred_adapt=True, **{ROWS[name][0]: True})
    # ppred's adapt tail has a switch of its own
    pp = d.alloc_records(n, "cpu", with_ppred=True, with_ppred_adapt=True)
    assert pp.buf.numel() == n * (BASE + 424 + 8) and pp.adapt.data_ptr() == pp.buf.data_ptr() + n * (BASE + 424)
    # and the tails come back in the record's order
    rec.buf.copy_(_random_bytes(rec.buf.numel()))
    got = d.unpack_gathered([rec.buf, rec.buf.clone()], 13, 2, with_auto=True, with_adapt=True, with_auto_pred=True)
    assert [a.shape for a in got[3:]] == [(13, 4), (13, 2), (13, 2)]
    for a, view in zip(got[3:], (rec.auto, rec.auto_pred, rec.adapt)):
        want = np.concatenate([view.numpy(), view.numpy()[:6]])
        assert np.array_equal(a.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("name", list(TAIL_ROWS))
def test_tail_table_pins(name):
    import inspect

    from metadamage_amd import blocks, distributed as d, engine, fits

    assert [t.name for t in blocks.TAILS] == list(TAIL_ROWS)  # the gather record's order
    option, switch, rides, shape, nbytes, dev = TAIL_ROWS[name]
    (t,) = [t for t in blocks.TAILS if t.name == name]
    assert (t.option, t.switch, tuple(t.rides), tuple(t.shape), t.out_bytes) == (option, switch, rides, shape, nbytes)
    assert (t.refusal, t.switch_refusal) == REFUSAL[name]
    assert int(np.prod(shape)) * 4 == nbytes == getattr(d, "REC_" + name.upper())
    assert t.device_bytes == (dev or 0) and (dev is None) == (t.device == ())
    assert dict(t.block_switches) == ({"ppred": PPRED_ADAPT} if name == "adapt" else {})
    assert name in engine.FitBatch.__dataclass_fields__
    assert name in inspect.signature(fits.make_df_fit_results).parameters
    assert option in inspect.signature(fits.fit_packed).parameters
    for f in (engine.device_bytes, engine.plan_chunks):  # (which take no psis_adapt: the adapt record is not counted)
        assert (option in inspect.signature(f).parameters) == (name in PLANNED)
    with pytest.raises(Exception):  # frozen
        t.name = "x"


@pytest.mark.parametrize("tail, block", [(t, b) for t, b in RIDES if t in PLANNED])
def test_tail_bytes_in_the_chunk_plan(tail, block):
    from metadamage_amd import engine

    option, _, _, _, nbytes, dev = TAIL_ROWS[tail]
    switch, mode = ROWS[block][:2]
    o = _opts(mode)
    kw = {switch: True}
    assert (engine.device_bytes(1000, o, **kw, **{option: True}) - engine.device_bytes(1000, o, **kw)
            == 1000 * (dev + nbytes))
    assert (engine.device_bytes(1000, o, dest_on_device=True, **kw, **{option: True})
            - engine.device_bytes(1000, o, dest_on_device=True, **kw)) == 1000 * dev
    assert engine.device_bytes(1000, o, **kw, **{option: False}) == engine.device_bytes(1000, o, **kw)


@pytest.mark.filterwarnings("ignore:invalid value encountered in cast")  # (random bytes hold signalling NaNs)
@pytest.mark.parametrize("block, tails", [("auto", ("auto_pred", "adapt")), ("ppred", ("ppc", "adapt")),
                                          ("psis", ("quant", "adapt")), ("waic", ("joint", "adapt"))]
                         + [(b, (t,)) for t, b in RIDES])
def test_tails_lie_and_come_back_in_the_records_order(block, tails):
    from metadamage_amd import distributed as d

    n = 7
    switch, _, attr, shape, nbytes, _ = ROWS[block]
    kw = dict({switch: True}, **{_tail_switch(t, block): True for t in tails})
    rec = d.alloc_records(n, "cpu", **kw)
    offset = BASE + nbytes
    assert getattr(rec, attr).data_ptr() == rec.buf.data_ptr() + n * BASE
    where = [(BASE, shape)]  # (byte offset per taxon, shape) of the block and of each tail, in the record's order
    for t in TAIL_ROWS:
        view = getattr(rec, t)
        assert (view is None) == (t not in tails), t
        if view is not None:
            assert tuple(view.shape) == (n, *TAIL_ROWS[t][3]) and view.is_contiguous()
            assert view.data_ptr() == rec.buf.data_ptr() + n * offset, t
            where.append((offset, TAIL_ROWS[t][3]))
            offset += TAIL_ROWS[t][4]
    assert rec.buf.numel() == n * offset
    # 13 taxa over two parts of capacity 7, random bytes: the arrays come back in that order, bit for bit
    parts = [_random_bytes(n * offset, seed=r) for r in (1, 2)]
    got = d.unpack_gathered(parts, 13, 2, **kw)
    assert len(got) == 3 + len(where)
    for a, (lo, shp) in zip(got[3:], where):
        words = int(np.prod(shp))
        pieces = [p.numpy()[n * lo: n * lo + 4 * n * words].view(np.int32).reshape(n, *shp) for p in parts]
        want = np.concatenate([pieces[0], pieces[1][:6]])
        assert a.dtype == np.float32 and a.shape == want.shape and np.array_equal(a.view(np.int32), want), (lo, shp)


@pytest.mark.parametrize("tail", list(TAIL_ROWS))
def test_a_tail_without_a_block_it_rides_is_refused_everywhere(tail):
    from metadamage_amd import distributed as d, engine

    option, switch, rides, _, _, _ = TAIL_ROWS[tail]
    by_option, by_switch = REFUSAL[tail]
    buf = _random_bytes(4 * 2000)
    for block in (None, *ROWS):
        if block in rides:
            continue
        kw = {ROWS[block][0]: True} if block is not None else {}
        if tail in PLANNED and block != "auto":  # (auto: the chunk plan refuses the block itself)
            o = _opts(ROWS[block][1]) if block is not None else None
            for f in (engine.device_bytes, engine.plan_chunks):
                with pytest.raises(ValueError, match=re.escape(by_option)):
                    f(10, o, **kw, **{option: True})
        for call in (lambda: d.alloc_records(4, "cpu", **kw, **{switch: True}),
                     lambda: d.unpack_gathered([buf], 4, 1, **kw, **{switch: True})):
            with pytest.raises(ValueError, match=re.escape(by_switch)):
                call()
    # the ppred block asks for its adapt tail by a switch of its own, which goes with no other block
    if tail == "adapt":
        for call in (lambda: d.alloc_records(4, "cpu", with_ppred=True, with_adapt=True),
                     lambda: d.unpack_gathered([buf], 4, 1, with_ppred=True, with_adapt=True)):
            with pytest.raises(ValueError, match=re.escape(by_switch)):
                call()
        for block in (None, *ROWS):
            if block != "ppred":
                kw = {ROWS[block][0]: True} if block is not None else {}
                with pytest.raises(ValueError, match="with_ppred_adapt goes with with_ppred"):
                    d.unpack_gathered([buf], 4, 1, with_ppred_adapt=True, **kw)
