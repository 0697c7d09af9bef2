"""Picks the 64 taxa of tests/test_gpu_auto.py's end-to-end test on the CPU.

From generate(400, seed=21), position by position (the importance draws of a
taxon are keyed by index_base + its row, so a taxon's Pareto k depends on where
it sits): the classes cycle deep ancient (mean N > 3e3), shallow ancient,
control-like, and a candidate is taken when the reference (tests/map_waic_ref.py
on the oracle's MAP fit, S = 256, seed 0) finds all six rows valid and its
largest k at least MARGIN from the threshold min(1 - 1 / log10 S, 0.7) -- so the
device's rounding cannot flip a route.  Prints the picks and their k.

    python tools/auto_pick_taxa.py
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

S, SEED, INDEX_BASE, T_PICK, MARGIN = 256, 0, 500, 64, 0.1


def main():
    from metadamage_amd.synthetic import generate
    from oracle.oracle import OracleLib
    from tests import map_psis_ref as pref
    from tests import map_waic_ref as ref

    lib = OracleLib()
    b = generate(400, seed=21)
    out, _pred, st = lib.fit_batch(b.y, b.N, b.mm)
    tau = float(pref.khat_threshold(S))
    deep = b.truth["ancient"] & (b.N[:, :30].mean(axis=1) > 3e3)
    cls = np.where(deep, 0, np.where(b.truth["ancient"], 1, 2))
    pools = [list(np.flatnonzero((cls == k) & (st == 0))) for k in range(3)]
    picks = []
    for pos in range(T_PICK):
        k = pos % 3
        while True:
            if not pools[k]:
                k = (k + 1) % 3
                continue
            t = int(pools[k].pop(0))
            rec = ref.waic_taxon(lib, b.y[t, :30], b.N[t, :30], out[t], 0, S, seed=SEED, g=INDEX_BASE + pos)["rec"]
            flags = [int(rec[s, ref.FLAGS]) for s in range(7)]
            if not all(f & 1 for f in flags):
                continue
            kmax = float(rec[6, 4])
            if abs(kmax - tau) < MARGIN:
                continue
            picks.append((t, k, kmax, kmax > tau))
            break
    n_s = sum(p[3] for p in picks)
    print(f"tau = {tau:.4f}; {n_s} sampled, {len(picks) - n_s} settled")
    print("PICKS = [" + ", ".join(str(p[0]) for p in picks) + "]")
    print("K_REF = [" + ", ".join(f"{p[2]:.2f}" for p in picks) + "]")
    print("CLASS = [" + ", ".join(str(p[1]) for p in picks) + "]")


if __name__ == "__main__":
    main()
