"""Cost of mdfit_map_laplace beside the MAP call it follows.

HIP events on one stream: the MAP call alone, and the call plus
mdfit_map_laplace, alternated, 20 warm repetitions each after 3 warm-ups, the
median taken; also the events around the Laplace launch alone.  10k taxa
(seed 1) and 125k taxa (seed 3).  The added time must stay under 5 % of the
same run's MAP call at both sizes.

    python tools/laplace_cost.py [--out profiles/laplace_cost.txt]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from metadamage_amd import _lib, engine  # noqa: E402
from metadamage_amd.synthetic import generate  # noqa: E402

WARM, REPS, LIMIT = 3, 20, 0.05


def measure(T, seed):
    b = generate(T, seed=seed)
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    o = _lib.default_opts(mode=_lib.MODE_MAP)
    res = engine.alloc_outputs(T, opts=o)
    lap = torch.empty((T, 3, _lib.NLAPLACE), dtype=torch.float64, device=ty.device)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    alone, both, kern = [], [], []
    for rep in range(WARM + REPS):
        e0, e1 = ev(), ev()
        e0.record()
        engine.fit_batch_device(ty, tN, tm, o, res)
        e1.record()
        f0, f1, f2 = ev(), ev(), ev()
        f0.record()
        engine.fit_batch_device(ty, tN, tm, o, res)
        f1.record()
        engine.map_laplace_device(ty, tN, res, lap=lap)
        f2.record()
        torch.cuda.synchronize()
        if rep >= WARM:
            alone.append(e0.elapsed_time(e1))
            both.append(f0.elapsed_time(f2))
            kern.append(f1.elapsed_time(f2))
    valid = float(((lap[:, 0, 7].to(torch.int64) & _lib.LAPLACE_VALID) != 0).double().mean())
    return np.median(alone), np.median(both), np.median(kern), valid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"mdfit_map_laplace beside the MAP call: {torch.cuda.get_device_name(0)}, medians of {REPS} warm "
             f"repetitions after {WARM} warm-ups, HIP events on one stream"]
    ok = True
    for T, seed in ((10_000, 1), (125_000, 3)):
        alone, both, kern, valid = measure(T, seed)
        added = both - alone
        ok = ok and added < LIMIT * alone and kern < LIMIT * alone
        lines.append(f"T={T:>7d} seed={seed}: MAP call {alone * 1e3:9.1f} us | call + laplace {both * 1e3:9.1f} us | "
                     f"added {added * 1e3:7.1f} us = {100 * added / alone:5.2f} % | laplace launch alone "
                     f"{kern * 1e3:7.1f} us = {100 * kern / alone:5.2f} % | PMD-all rows valid {100 * valid:.1f} %")
    lines.append(f"added time under {100 * LIMIT:.0f} % of the MAP call at both sizes: {'yes' if ok else 'NO'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
