"""Record tests/golden/map_is_bits_parent.npz: the bits that the PARENT commit's
build returns on a GPU for the MAP post-fit entries that share the importance
sampler (mdfit_map_laplace, mdfit_map_psis, mdfit_map_waic, mdfit_map_pred,
mdfit_map_evidence and their _adapt forms) at the inputs and configurations of
tests/test_gpu_map_is_bits.py.

    git worktree add /tmp/parent <parent commit>
    (cd /tmp/parent && python __graft_entry__.py)          # same toolchain
    python tools/record_map_is_bits_golden.py --checkout /tmp/parent --commit <sha>

The fixture is what a change of those kernels that claims to leave every
value's arithmetic alone must reproduce bit for bit, so it is never recorded
from the code under test: --checkout names a built checkout of the commit the
change starts from, and its package and library are the ones imported.

Inputs: 64 taxa of generate(300, seed=21) -- the recorder picks them from a
survey of all 300 so that every kind of row below occurs (an invalid PMD row is
told apart by the draws tap: the proposal invalid, or a valid proposal whose
round 0 weights were refused), and stores the index list -- then one crafted
taxon with some y > N; all fitted by one MODE_MAP call.  The records are stored in full as integer views, the taps (draws,
pointwise, index, counts, gh, u) as the SHA-256 of their bytes.
"""

from __future__ import annotations

import argparse
import hashlib
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parents[1]
FIXTURE = HERE / "tests" / "golden" / "map_is_bits_parent.npz"

N_POOL, POOL_SEED, N_TAXA = 300, 21, 64
SEED, INDEX_BASE = 0, 7
# name -> (S importance draws, R predictive draws, adapt rounds or None for the plain entries)
CONFIGS = {"A": (25, 25, None), "B": (65, 100, 2), "C": (256, 256, None), "C_adapt": (256, 256, 4)}
# the kinds of row the recorded taxa must show in some configuration
KINDS = ("status_not_ok", "pmd_proposal_invalid", "pmd_c_held", "best_round_gt0", "round_dropped", "khat_over_tau")
# kinds that are recorded where the pool has them, and noted in the fixture where it has none
NOTED = ("null_invalid", "pmd_round0_refused")
# read off the records alone (kinds) / off the draws taps (tap_kinds)
REC_KINDS = ("status_not_ok", "pmd_c_held", "best_round_gt0", "round_dropped", "khat_over_tau", "null_invalid")
TAP_KINDS = ("pmd_proposal_invalid", "pmd_round0_refused")


def inputs(synthetic, indices):
    """(y, N, mm) uint32: the taxa `indices` of the pool, then the crafted one
    (a copy of the first with y > N at two positions)."""
    b = synthetic.generate(N_POOL, seed=POOL_SEED)
    idx = np.asarray(indices, np.int64)
    y = np.concatenate([b.y[idx], b.y[idx[:1]]]).astype(np.uint32)
    N = np.concatenate([b.N[idx], b.N[idx[:1]]]).astype(np.uint32)
    mm = np.concatenate([b.mm[idx], b.mm[idx[:1]]]).astype(np.uint32)
    y[-1, 4] = N[-1, 4] + 1
    y[-1, 17] = N[-1, 17] + 3
    return y, N, mm


def run(engine, _lib, torch, y, N, mm, configs=CONFIGS):
    """One MODE_MAP call on (y, N, mm), then every entry in every configuration.
    Returns (records, taps): host arrays by name."""
    ty, tN, tm = engine.to_device_counts(y, N, mm)
    res = engine.fit_batch_device(ty, tN, tm, _lib.default_opts(mode=_lib.MODE_MAP))
    T = int(ty.shape[0])
    gh = torch.empty((T, 3, 20), dtype=torch.float64, device=ty.device)
    u = torch.empty((T, 3, 4), dtype=torch.float64, device=ty.device)
    lap = engine.map_laplace_device(ty, tN, res, gh=gh, u=u)
    rec = {"status": res.status, "lap": lap}
    tap = {"gh": gh, "u": u}
    for name, (S, R, rounds) in configs.items():
        kw = {} if rounds is None else {"adapt_rounds": rounds, "adapt": True}
        got = engine.map_psis_device(ty, tN, res, S, SEED, INDEX_BASE, draws=True, **kw)
        rec[f"{name}/psis"], tap[f"{name}/psis_draws"] = got[0], got[1]
        if rounds is not None:
            rec[f"{name}/psis_adapt"] = got[2]
        got = engine.map_waic_device(ty, tN, res, S, SEED, INDEX_BASE, pointwise=True, draws=True, **kw)
        rec[f"{name}/waic"], tap[f"{name}/pointwise"], tap[f"{name}/waic_draws"] = got[0], got[1], got[2]
        if rounds is not None:
            rec[f"{name}/waic_adapt"] = got[3]
        got = engine.map_evidence_device(ty, tN, res, S, SEED, INDEX_BASE, draws=True, **kw)
        rec[f"{name}/evid"], tap[f"{name}/evid_draws"] = got[0], got[1]
        if rounds is not None:
            rec[f"{name}/evid_adapt"] = got[2]
        got = engine.map_pred_device(ty, tN, res, S, R, SEED, INDEX_BASE, index=True, counts=True, **kw)
        rec[f"{name}/ppred"], rec[f"{name}/prec"] = got[0], got[1]
        tap[f"{name}/index"], tap[f"{name}/counts"] = got[2], got[3]
        if rounds is not None:
            rec[f"{name}/pred_adapt"] = got[4]
    torch.cuda.synchronize()
    host = lambda d: {k: np.ascontiguousarray(v.cpu().numpy()) for k, v in d.items()}  # noqa: E731
    return host(rec), host(tap)


def bits(a):
    """A record as the integers of its bytes (float64 -> int64, float32 / int32 -> int32)."""
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype.itemsize == 8 else a.view(np.int32)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def kinds(rec, configs=CONFIGS):
    """{kind: bool[T]} over the records of run(), for REC_KINDS: which taxa show
    each kind of row in some configuration."""
    st = rec["status"]
    T = st.shape[0]
    ok = st == 0
    k = {name: np.zeros(T, bool) for name in REC_KINDS}
    k["status_not_ok"] = ~ok
    for name, (_S, _R, rounds) in configs.items():
        fl = rec[f"{name}/psis"][:, :, 15]
        valid = np.nan_to_num(fl).astype(np.int64) & 1
        wfl = np.nan_to_num(rec[f"{name}/waic"][:, [1, 4, 5], 7]).astype(np.int64)
        k["null_invalid"] |= ok & ((wfl & 1) == 0).any(axis=1)
        # bits 2..5 of a row's flags: coordinate free; c is coordinate 2
        k["pmd_c_held"] |= ((valid == 1) & ((np.nan_to_num(fl).astype(np.int64) & 16) == 0)).any(axis=1)
        if rounds is None:
            continue
        ad = rec[f"{name}/psis_adapt"]
        k["best_round_gt0"] |= (ad[:, :, 2] > 0).any(axis=1)
        k["round_dropped"] |= (ad[:, :, 3] > ad[:, :, 2]).any(axis=1)
        k["khat_over_tau"] |= ((valid == 1) & ((np.nan_to_num(fl).astype(np.int64) & 2) == 0)).any(axis=1)
    return k


def tap_kinds(status, tap, configs=CONFIGS):
    """{kind: bool[T]} for TAP_KINDS, off mdfit_map_psis' draws tap [T, 3, S, 6]
    = u[4], lw, w: a PMD row of a fitted taxon that is invalid because its
    proposal is (no draw was made: the whole row of the tap is NaN) and one
    whose proposal was valid and whose round 0 psis_weights refused (u stands,
    the weights' column is NaN)."""
    ok = np.asarray(status) == 0
    k = {name: np.zeros(ok.shape[0], bool) for name in TAP_KINDS}
    for name in configs:
        dr = tap[f"{name}/psis_draws"]
        no_u = np.isnan(dr[:, :, :, :4]).all(axis=(2, 3))
        has_u = np.isfinite(dr[:, :, :, :4]).all(axis=(2, 3))
        no_w = np.isnan(dr[:, :, :, 5]).all(axis=2)
        k["pmd_proposal_invalid"] |= ok & (no_u & no_w).any(axis=1)
        k["pmd_round0_refused"] |= ok & (has_u & no_w).any(axis=1)
    return k


def choose(survey_kinds):
    """64 indices of the pool: up to three taxa of every kind, then the lowest others."""
    picked = []
    for name in (*KINDS, *NOTED):
        picked += np.flatnonzero(survey_kinds[name])[:3].tolist()
    picked = sorted(set(picked))
    rest = [i for i in range(N_POOL) if i not in picked]
    return sorted(picked + rest[: N_TAXA - len(picked)])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkout", required=True, help="built checkout of the parent commit")
    ap.add_argument("--commit", required=True, help="its commit id (stored in the fixture)")
    ap.add_argument("--out", default=str(FIXTURE))
    a = ap.parse_args()
    root = Path(a.checkout).resolve()
    sys.path.insert(0, str(root))
    import torch
    from metadamage_amd import _lib, engine, synthetic

    assert Path(_lib.LIB_PATH).resolve().is_relative_to(root), _lib.LIB_PATH
    assert Path(engine.__file__).resolve().is_relative_to(root), engine.__file__

    # the survey: all of the pool, for the choice of the 64
    b = synthetic.generate(N_POOL, seed=POOL_SEED)
    pool, pool_tap = run(engine, _lib, torch, b.y, b.N, b.mm)
    pk = {**kinds(pool), **tap_kinds(pool["status"], pool_tap)}
    for name, m in pk.items():
        print(f"pool: {name}: {int(m.sum())} of {N_POOL} taxa")
    indices = choose(pk)
    assert len(indices) == N_TAXA

    y, N, mm = inputs(synthetic, indices)
    rec, tap = run(engine, _lib, torch, y, N, mm)
    k = {**kinds(rec), **tap_kinds(rec["status"], tap)}
    assert rec["status"][-1] != 0, "the crafted taxon was fitted"
    for name in KINDS:
        n = int(k[name].sum())
        print(f"recorded: {name}: {n} of {N_TAXA + 1} taxa")
        if n == 0:
            raise SystemExit(f"no recorded taxon shows {name}: choose other indices")
    in_pool = {}
    for name in NOTED:
        in_pool[name], n = int(pk[name].sum()), int(k[name].sum())
        print(f"recorded: {name}: {n} taxa ({in_pool[name]} of the pool's {N_POOL})")
        if in_pool[name] > 0 and n == 0:
            raise SystemExit(f"the pool has a taxon with {name}, the recorded taxa none: choose other indices")

    arrays = {"commit": np.array(a.commit), "indices": np.asarray(indices, np.int32)}
    for name in NOTED:
        arrays[f"{name}_in_pool"] = np.array(in_pool[name], np.int32)
    for name in (*KINDS, *NOTED):
        arrays[f"kind/{name}"] = np.flatnonzero(k[name]).astype(np.int32)
    for name, v in rec.items():
        arrays[f"rec/{name}"] = bits(v)
    for name, v in tap.items():
        arrays[f"sha/{name}"] = np.array(digest(v))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    size = Path(a.out).stat().st_size
    print(f"wrote {a.out} ({size} bytes)")
    assert size < 1_000_000, size


if __name__ == "__main__":
    main()
