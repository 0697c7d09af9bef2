"""Record tests/golden/fit_overhead_records.npz: the MAP records, predictions
and status of the fit-overhead batch (tests/test_gpu_fit_overhead_bits.py) as
the PARENT commit's build computes them.

    git worktree add /tmp/parent <parent commit>
    (cd /tmp/parent && python __graft_entry__.py)          # same toolchain
    python tools/record_fit_overhead_golden.py --checkout /tmp/parent --commit <sha>

The fixture is what the fit kernel must reproduce bit for bit once its pad
lanes evaluate a neutral argument, so it is never recorded from the code under
test: --checkout names a built checkout of the commit the change starts from,
and its package and library are the ones imported.  Both lane layouts are run
there and must already agree bit for bit; the PPL-1 results are stored.

Two calls are stored: the whole 96-taxon batch (12 taxa in each of the fit
kernel's 8 queues: every wave of the one-point-per-lane layout holds two PMD
fits or two null fits) and its first N_ODD = 91 taxa (11 or 12 taxa per queue:
in a queue of 11 one wave holds the last PMD fit beside the first null fit).
"""

from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parents[1]

N_TAXA = 96
N_ODD = 91

# (A, q, c, phi, depth, copies): the crafted taxa, drawn as synthetic.generate
# draws its taxa.  With D(1) = A + c the pad lane's arguments at the mode are
# a0 = (A + c) phi and b0 = (1 - A - c) phi.
CRAFTED = [
    (0.10, 0.30, 0.010, 60.0, 1.0e4, 8),   # a0 ~ 6.6 < 10, every y >= 10 (far y ~ 100)
    (0.10, 0.30, 0.005, 60.0, 5.0e2, 8),   # a0 < 10, far y ~ 2.5: some y < 10
    (0.30, 0.40, 0.010, 5.0, 1.0e4, 8),    # phi < 10 (so a0, b0 < 10 too)
    (0.30, 0.40, 0.010, 3.0, 3.0e2, 6),    # phi < 10, shallow
    (0.50, 0.20, 0.030, 15.0, 1.0e4, 8),   # b0 ~ 7 < 10 with phi >= 10
    (0.30, 0.50, 0.001, 200.0, 1.0e2, 8),  # y = 0 at far positions
    (0.002, 0.40, 0.002, 800.0, 3.0e2, 6), # not ancient, shallow: y = 0 at most positions
    (0.25, 0.35, 0.015, 1000.0, 1.0e6, 7), # deep, every argument >= 10
    (0.40, 0.60, 0.020, 30.0, 1.0e5, 8),   # a0 ~ 12.6, b0 ~ 17: no shift at the pad
]


def _cases(root: Path):
    cases = json.loads((Path(root) / "tests" / "golden" / "map_boundary_cases.json").read_text())
    return cases, sorted(cases)


def order(n_boundary: int):
    """The batch's rows: ("b", i) the i-th boundary case, ("c", i) the i-th crafted taxon.  Every third taxon is a
    boundary case while they last: they are the long fits, and spread over the queues they sit beside short crafted
    ones.  batch() and boundary_rows() both read the rows from here."""
    n_crafted = sum(r[5] for r in CRAFTED)
    assert n_crafted + n_boundary == N_TAXA
    rows, bi, ci = [], 0, 0
    for t in range(N_TAXA):
        if (t % 3 == 1 and bi < n_boundary) or ci >= n_crafted:
            rows.append(("b", bi))
            bi += 1
        else:
            rows.append(("c", ci))
            ci += 1
    return rows


def batch(root: Path):
    """The 29 taxa of root/tests/golden/map_boundary_cases.json (sorted by name;
    they were collected for the polish phase, the saddle escape, the gradient
    fallback and the flat-tail rescue) interleaved with the 67 crafted taxa: y,
    N, mm.  The one definition of the batch: the tests load it from here."""
    cases, names = _cases(root)
    rng = np.random.Generator(np.random.PCG64(20261021))
    k = np.concatenate([np.arange(15), np.arange(15)]).astype(np.float64)
    rows = []
    for A, q, c, phi, depth, n in CRAFTED:
        for _ in range(n):
            D = np.clip(A * (1.0 - q) ** k + c, 1e-12, 1.0 - 1e-12)
            Nz = np.rint(depth * rng.uniform(0.85, 1.15, 30)).astype(np.int64)
            p = rng.beta(D * phi, (1.0 - D) * phi)
            rows.append((rng.binomial(Nz, p), Nz))
    y = np.zeros((N_TAXA, 32), np.uint32)
    N = np.zeros((N_TAXA, 32), np.uint32)
    mm = np.zeros((N_TAXA, 30, 12), np.uint32)
    for t, (kind, i) in enumerate(order(len(names))):
        if kind == "b":
            y[t, :30] = cases[names[i]]["y"]
            N[t, :30] = cases[names[i]]["N"]
        else:
            y[t, :30], N[t, :30] = rows[i]
    return y, N, mm


def boundary_rows(root: Path):
    """taxon row -> boundary case name, for the rows of batch() that hold one"""
    _, names = _cases(root)
    return {t: names[i] for t, (kind, i) in enumerate(order(len(names))) if kind == "b"}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkout", required=True, help="built checkout of the parent commit")
    ap.add_argument("--commit", required=True, help="its commit id (stored in the fixture)")
    ap.add_argument("--out", default=str(HERE / "tests" / "golden" / "fit_overhead_records.npz"))
    a = ap.parse_args()
    root = Path(a.checkout).resolve()
    sys.path.insert(0, str(root))
    from metadamage_amd import _lib, engine

    assert Path(_lib.LIB_PATH).resolve().is_relative_to(root), _lib.LIB_PATH
    y, N, mm = batch(HERE)
    recs = {}
    for ppl in ("1", "2"):
        os.environ["MDFIT_FIT_PPL"] = ppl
        for n in (N_TAXA, N_ODD):
            out, pred, st = engine.fit_batch(y[:n], N[:n], mm[:n])
            recs[ppl, n] = (np.asarray(out, np.float64), np.asarray(pred, np.float32), np.asarray(st))
    del os.environ["MDFIT_FIT_PPL"]
    for n in (N_TAXA, N_ODD):
        for a1, a2 in zip(recs["1", n], recs["2", n]):
            assert np.array_equal(a1, a2, equal_nan=True), ("the two lane layouts differ in the parent", n)
    out, pred, st = recs["1", N_TAXA]
    out_odd, pred_odd, st_odd = recs["1", N_ODD]
    print(f"{out.shape[0]} taxa, status {np.bincount(st)}; first {N_ODD} alone equal to the batch's rows: "
          f"{np.array_equal(out[:N_ODD], out_odd, equal_nan=True)}")
    np.savez_compressed(a.out, out=out, pred=pred, status=st, out_odd=out_odd, pred_odd=pred_odd, status_odd=st_odd,
                        commit=np.array(a.commit))
    print(f"wrote {a.out} ({Path(a.out).stat().st_size} bytes)")


if __name__ == "__main__":
    main()
