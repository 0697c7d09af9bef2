"""Record tests/golden/fit_logic_records.npz: the MAP records of the fit-logic
batch (tests/test_gpu_fit_logic.py) as the PARENT commit's build computes them.

    git worktree add /tmp/parent <parent commit>
    (cd /tmp/parent && python __graft_entry__.py)          # same toolchain
    python tools/record_fit_logic_golden.py --checkout /tmp/parent --commit <sha>

The fixture is what the restructured Newton logic must reproduce bit for bit,
so it is never recorded from the code under test: --checkout names a built
checkout of the commit the change starts from, and its package and library
are the ones imported.  Both lane layouts are run there and must already
agree bit for bit; the PPL-1 records are stored.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parents[1]


def batch(root: Path):
    """generate(512, seed=31) + the 29 taxa of root/tests/golden/map_boundary_cases.json
    (sorted by name, as tests/test_map_boundary.py builds them): y, N, mm.  The one
    definition of the batch: tests/test_gpu_fit_logic.py loads it from here."""
    from metadamage_amd.synthetic import generate

    cases = json.loads((Path(root) / "tests" / "golden" / "map_boundary_cases.json").read_text())
    names = sorted(cases)
    b = generate(512, seed=31)
    T = b.n_taxa + len(names)
    y = np.zeros((T, 32), np.uint32)
    N = np.zeros((T, 32), np.uint32)
    mm = np.zeros((T, 30, 12), np.uint32)
    y[: b.n_taxa], N[: b.n_taxa], mm[: b.n_taxa] = b.y, b.N, b.mm
    for i, n in enumerate(names):
        y[b.n_taxa + i, :30] = cases[n]["y"]
        N[b.n_taxa + i, :30] = cases[n]["N"]
    return y, N, mm


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkout", required=True, help="built checkout of the parent commit")
    ap.add_argument("--commit", required=True, help="its commit id (stored in the fixture)")
    ap.add_argument("--out", default=str(HERE / "tests" / "golden" / "fit_logic_records.npz"))
    a = ap.parse_args()
    root = Path(a.checkout).resolve()
    sys.path.insert(0, str(root))
    from metadamage_amd import _lib, engine

    assert Path(_lib.LIB_PATH).resolve().is_relative_to(root), _lib.LIB_PATH
    y, N, mm = batch(root)
    recs = {}
    for ppl in ("1", "2"):
        os.environ["MDFIT_FIT_PPL"] = ppl
        out, _, st = engine.fit_batch(y, N, mm)
        recs[ppl] = (np.asarray(out, np.float64), np.asarray(st))
    del os.environ["MDFIT_FIT_PPL"]
    out, st = recs["1"]
    assert np.array_equal(out, recs["2"][0], equal_nan=True) and np.array_equal(st, recs["2"][1])
    diag = out[:, _lib.F_DIAG : _lib.F_DIAG + _lib.NSUBFIT * _lib.DIAG_STRIDE].reshape(-1, _lib.NSUBFIT, _lib.DIAG_STRIDE)
    print(f"{out.shape[0]} taxa, status {np.bincount(st)}, polished sub-fits {int((diag[:, :, 7] == 1).sum())}, "
          f"sub-fits with >= 30 evaluations {int((diag[:, :, 5] >= 30).sum())} (max {int(diag[:, :, 5].max())})")
    np.savez_compressed(a.out, out=out, status=st, commit=np.array(a.commit))
    print(f"wrote {a.out} ({Path(a.out).stat().st_size} bytes)")


if __name__ == "__main__":
    main()
