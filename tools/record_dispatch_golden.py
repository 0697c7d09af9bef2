"""Record tests/golden/dispatch_parent.npz: the bits that the PARENT commit's
build returns on a GPU for the whole dispatch -- every post-fit block with every
tail that rides it, through the host route and through the device-destination
route -- at the inputs and configurations of tests/test_gpu_dispatch_bits.py.

    git worktree add /tmp/parent <parent commit>
    (cd /tmp/parent && python __graft_entry__.py)          # same toolchain
    python tools/record_dispatch_golden.py --checkout /tmp/parent --commit <sha>

The fixture is what a change of the Python that plans, launches and gathers the
chunks, and that claims to leave every value alone, must reproduce bit for bit,
so it is never recorded from the code under test: --checkout names a built
checkout of the commit the change starts from, and its package and library are
the ones imported.  Only names whose signatures such a change leaves alone are
called (fits.fit_packed, distributed.alloc_records / unpack_gathered,
engine.staging, ChunkedFitter.run_into_device, engine.fit_auto_chunks), so this
file runs against both trees.

Inputs: 13 taxa of generate(13, seed=21) and one crafted taxon with y > N at two
positions (a status that is not OK), in three uneven chunks (MDFIT_CHUNK_TAXA =
5: the third chunk takes the first chunk's buffer set).  Every returned array is
stored in full as an integer view.
"""

from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

HERE = Path(__file__).resolve().parents[1]
FIXTURE = HERE / "tests" / "golden" / "dispatch_parent.npz"

N_SYNTHETIC, POOL_SEED = 13, 21
CHUNK_TAXA = 5  # 14 taxa = 4 + 5 + 5
SEED, INDEX_BASE = 0, 7
PSIS_DRAWS, PRED_DRAWS, ROUNDS, DMAX_THRESHOLD = 65, 100, 2, 0.02  # (65: one draw past the 64-lane stride)
NUM_WARMUP, NUM_SAMPLES = 20, 40
NUTS_BLOCKS = ("diag", "summary", "loo")
# configuration -> (the block's name or None, the tail options of fits.fit_packed)
CONFIGS = {
    "none": (None, {}),
    "laplace": ("laplace", {}),
    "psis": ("psis", {}),
    "psis+quantiles": ("psis", {"quantiles": True}),
    "psis+quantiles+rounds": ("psis", {"quantiles": True, "psis_adapt": ROUNDS}),
    "waic": ("waic", {}),
    "waic+joint": ("waic", {"joint": True}),
    "waic+joint+rounds": ("waic", {"joint": True, "psis_adapt": ROUNDS}),
    "evidence": ("evidence", {}),
    "evidence+rounds": ("evidence", {"psis_adapt": ROUNDS}),
    "ppred": ("ppred", {}),
    "ppred+ppc": ("ppred", {"ppc": True}),
    "ppred+ppc+rounds": ("ppred", {"ppc": True, "psis_adapt": ROUNDS}),
    "diag": ("diag", {}),
    "summary": ("summary", {}),
    "loo": ("loo", {}),
    "auto": ("auto", {}),
    "auto+auto_pred+rounds": ("auto", {"auto_pred": True, "psis_adapt": ROUNDS}),
}
ROUTES = ("host", "device")
# the block's attribute on engine.FitBatch and distributed.Records
ATTR = {"laplace": "lap", "diag": "diag", "summary": "summ", "loo": "loo", "psis": "psis", "waic": "waic",
        "evidence": "evid", "ppred": "ppred", "auto": "auto"}
# the tail option -> its switch in distributed and its attribute (psis_adapt: ppred has a switch of its own)
TAIL = {"ppc": ("with_ppc", "ppc"), "quantiles": ("with_quant", "quant"), "joint": ("with_joint", "joint"),
        "auto_pred": ("with_auto_pred", "auto_pred"), "psis_adapt": ("with_adapt", "adapt")}


def inputs(synthetic):
    """(y, N, mm) uint32: the synthetic taxa, then the crafted one (a copy of the
    first with y > N at two positions)."""
    b = synthetic.generate(N_SYNTHETIC, seed=POOL_SEED)
    y = np.concatenate([b.y, b.y[:1]]).astype(np.uint32)
    N = np.concatenate([b.N, b.N[:1]]).astype(np.uint32)
    mm = np.concatenate([b.mm, b.mm[:1]]).astype(np.uint32)
    y[-1, 4] = N[-1, 4] + 1
    y[-1, 17] = N[-1, 17] + 3
    return y, N, mm


def modules():
    """The package's modules the routes call, as imported now (the checkout's, or the tree's in the test)."""
    import torch
    from metadamage_amd import _lib, distributed, engine, fits, synthetic

    return SimpleNamespace(torch=torch, _lib=_lib, distributed=distributed, engine=engine, fits=fits,
                           synthetic=synthetic)


def options(m, block):
    mode = m._lib.MODE_NUTS if block in NUTS_BLOCKS else m._lib.MODE_MAP
    return m._lib.default_opts(mode=mode, seed=SEED, index_base=INDEX_BASE, num_warmup=NUM_WARMUP,
                               num_samples=NUM_SAMPLES)


def host_route(m, y, N, mm, block, tails):
    """fits.fit_packed on this GPU alone: fit_batch_host, or fit_auto_chunks for auto."""
    T = y.shape[0]
    p = m.fits.Packed(np.arange(T), np.array([f"t{i}" for i in range(T)]), np.array(["species"] * T),
                      np.full(T, 100, np.int64), y.copy(), N.copy(), mm.copy())
    named = {block: True} if block is not None else {}
    return m.fits.fit_packed(p, options(m, block), shard=False, psis_draws=PSIS_DRAWS, pred_draws=PRED_DRAWS,
                             dmax_threshold=DMAX_THRESHOLD, **tails, **named)


def device_route(m, y, N, mm, block, tails):
    """The sharded fit's steps with no process group: the gather records, the
    dispatch into them, the staging of the result columns and the unpacking."""
    torch, engine, d = m.torch, m.engine, m.distributed
    T = y.shape[0]
    dev = torch.device("cuda", torch.cuda.current_device())
    opts = options(m, block)
    switch = {"with_" + block: True} if block is not None else {}
    layout, attrs = dict(switch), [ATTR[block]] if block is not None else []
    for option, on in tails.items():
        name, attr = TAIL[option]
        layout["with_ppred_adapt" if (option, block) == ("psis_adapt", "ppred") else name] = bool(on)
        attrs.append(attr)
    rec = d.alloc_records(T, dev, **layout)
    dest = engine.FitBatch(rec.out, rec.pred, rec.status, **{a: getattr(rec, a) for a in attrs})
    if block == "auto":
        engine.fit_auto_chunks(y, N, mm, opts, PSIS_DRAWS, device=dev, dest=dest, pred_draws=PRED_DRAWS, **tails)
    else:
        with engine._STAGING_LOCK:
            st = engine.staging(T, device=dev, opts=opts, with_mm=True, dest_on_device=True, psis_draws=PSIS_DRAWS,
                                pred_draws=PRED_DRAWS, dmax_threshold=DMAX_THRESHOLD, **tails, **switch)
            st.run_into_device(y, N, mm, opts, dest)
            torch.cuda.synchronize(dev)
    torch.cuda.synchronize(dev)
    buf = rec.stage()
    torch.cuda.synchronize(dev)
    return d.unpack_gathered([buf], T, 1, **layout)


def run(m, y, N, mm, configs=CONFIGS):
    """{(configuration, route): the returned arrays} with MDFIT_CHUNK_TAXA = CHUNK_TAXA."""
    before = os.environ.get("MDFIT_CHUNK_TAXA")
    os.environ["MDFIT_CHUNK_TAXA"] = str(CHUNK_TAXA)
    try:
        got = {}
        for name, (block, tails) in configs.items():
            for route, f in zip(ROUTES, (host_route, device_route)):
                got[name, route] = tuple(np.array(a) for a in f(m, y, N, mm, block, tails))
        return got
    finally:
        if before is None:
            del os.environ["MDFIT_CHUNK_TAXA"]
        else:
            os.environ["MDFIT_CHUNK_TAXA"] = before


def bits(a):
    """An array as the integers of its bytes (float64 -> int64, float32 / int32 -> int32)."""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype.itemsize == 8 else a.view(np.int32)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkout", required=True, help="built checkout of the parent commit")
    ap.add_argument("--commit", required=True, help="its commit id (stored in the fixture)")
    ap.add_argument("--out", default=str(FIXTURE))
    a = ap.parse_args()
    root = Path(a.checkout).resolve()
    sys.path.insert(0, str(root))
    m = modules()
    assert Path(m._lib.LIB_PATH).resolve().is_relative_to(root), m._lib.LIB_PATH
    for mod in (m.engine, m.fits, m.distributed):
        assert Path(mod.__file__).resolve().is_relative_to(root), mod.__file__

    y, N, mm = inputs(m.synthetic)
    got = run(m, y, N, mm)
    arrays = {"commit": np.array(a.commit)}
    for (name, route), arrs in got.items():
        status = arrs[2]
        assert status[-1] != 0 and (status[:-1] == 0).any(), (name, route, status)
        print(f"{name} / {route}: {len(arrs)} arrays, {int((status == 0).sum())} of {len(status)} taxa OK, "
              + ", ".join(f"{x.dtype}{list(x.shape)}" for x in arrs))
        arrays[f"{name}/{route}/n"] = np.array(len(arrs), np.int32)
        for i, x in enumerate(arrs):
            arrays[f"{name}/{route}/{i}"] = bits(x)
    for name in ("auto", "auto+auto_pred+rounds"):
        sampled = got[name, "host"][3][:, 1]
        print(f"{name}: the sampler ran for {int((sampled != 0).sum())} of {len(sampled)} taxa")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    size = Path(a.out).stat().st_size
    print(f"wrote {a.out} ({size} bytes)")
    assert size < 1_000_000, size


if __name__ == "__main__":
    main()
