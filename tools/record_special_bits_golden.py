"""Record tests/golden/special_bits_parent.npz: the bits that the PARENT commit's
build returns on a GPU for the log / lnGamma primitives of csrc/mdfit_special.h
(mdfit_primitive) at the points of tests/test_gpu_special_bits.py.

    git worktree add /tmp/parent <parent commit>
    (cd /tmp/parent && python __graft_entry__.py)          # same toolchain
    python tools/record_special_bits_golden.py --checkout /tmp/parent --commit <sha>

The fixture is what a change of lg3 / flog / lrise that claims to leave every
value's arithmetic alone must reproduce bit for bit, so it is never recorded
from the code under test: --checkout names a built checkout of the commit the
change starts from, and its package and library are the ones imported.
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parents[1]

# enum mdfit_primitive_id (include/mdfit.h)
FLOG, LG3_L, LG3_P, LG3_Q, LG3_FAST_L, LG3_FAST_P, LGDIFF, LRISE = 3, 9, 10, 11, 12, 13, 15, 16
# selector -> the grids of tests/golden/primitives_golden.npz whose x (and x2) it runs on
GRIDS = {FLOG: "flog_", LG3_L: "lg3_", LG3_P: "lg3_", LG3_Q: "lg3_", LG3_FAST_L: "lg3_", LG3_FAST_P: "lg3_",
         LGDIFF: "lgdiff_", LRISE: "lrise_"}
NAMES = {FLOG: "flog", LG3_L: "lg3.l", LG3_P: "lg3.p", LG3_Q: "lg3.q", LG3_FAST_L: "lg3<fast>.l",
         LG3_FAST_P: "lg3<fast>.p", LGDIFF: "lgdiff", LRISE: "lrise"}

# the edges of lg3's shift and of the logs inside it
EDGES = np.array([0.0, 5e-324, np.nextafter(10.0, 0.0), 10.0, np.nextafter(10.0, 20.0)])
# lrise: counts n against s, both sides of s <= n + 1 and of the shift at 10
RISE_N = np.array([0.0, 1.0, 8.0, 9.0, 1e3, 7e6, 4e9])
RISE_S = np.array([1e-3, 0.5, 9.5, 10.0, 50.0, 1e4])


def fixture_x(root: Path, prefix: str, field: str = "x") -> np.ndarray:
    g = np.load(Path(root) / "tests" / "golden" / "primitives_golden.npz")
    keys = sorted(k for k in g.files if k.startswith(prefix) and k.endswith("/" + field))
    return np.concatenate([g[k] for k in keys]).astype(np.float64)


def rise_cross():
    n, s = np.meshgrid(RISE_N, RISE_S, indexing="ij")
    return n.ravel(), s.ravel()


def points(root: Path, sel: int):
    """(x, x2) of selector `sel` (x2 None for a unary one): the x values of its
    grids in primitives_golden.npz, then the edges (unary) or the n x s cross
    (lrise).  The one definition of the points: the tests load it from here."""
    x = fixture_x(root, GRIDS[sel])
    if sel in (LGDIFF, LRISE):
        x2 = fixture_x(root, GRIDS[sel], "x2")
        if sel == LRISE:
            n, s = rise_cross()
            x, x2 = np.concatenate([x, n]), np.concatenate([x2, s])
        return x, x2
    return np.concatenate([x, EDGES]), None


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkout", required=True, help="built checkout of the parent commit")
    ap.add_argument("--commit", required=True, help="its commit id (stored in the fixture)")
    ap.add_argument("--out", default=str(HERE / "tests" / "golden" / "special_bits_parent.npz"))
    a = ap.parse_args()
    root = Path(a.checkout).resolve()
    sys.path.insert(0, str(root))
    from metadamage_amd import _lib, engine

    assert Path(_lib.LIB_PATH).resolve().is_relative_to(root), _lib.LIB_PATH
    arrays = {"commit": np.array(a.commit)}
    for sel in sorted(GRIDS):
        x, x2 = points(root, sel)
        assert x.size < 4000
        got = np.asarray(engine.primitive(sel, x, x2), np.float64)
        assert got.shape == x.shape
        arrays[f"bits_{sel}"] = got.view(np.uint64)
        print(f"{NAMES[sel]}: {x.size} points, {int(np.isnan(got).sum())} NaN, {int(np.isinf(got).sum())} infinite")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print(f"wrote {a.out} ({Path(a.out).stat().st_size} bytes)")


if __name__ == "__main__":
    main()
