"""Cost of mdfit_map_pred beside the MAP call it follows, the mdfit_map_psis
launch and the NUTS call it stands in for.

HIP events on one stream: the MAP call alone, the call plus mdfit_map_pred at S
= 256 and S = 1024 (R = 1000), and the mdfit_map_psis launch at the same S,
alternated, 10 warm repetitions each after 2 warm-ups, the median taken; also
the events around the launches alone.  The NUTS call (500 + 1000) on the same
taxa: the median of 2 repetitions after one warm-up at 10k taxa, one repetition
at 125k.  10k taxa (seed 1) and 125k taxa (seed 3).  There is no pass bar.

    python tools/map_pred_cost.py [--out profiles/map_pred_cost.txt] [--no-nuts]
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

WARM, REPS = 2, 10
DRAWS = (256, 1024)
R = 1000
# the one figure to hold the launch against: the sampler's post kernel spends 55 ms of a 20k-taxon call on the
# same 32 x 1000 predictive draws per taxon (profiles/r06_post_split.txt)
POST_MS_PER_TAXON = 55.0 / 20_000


def measure(T, seed, nuts):
    b = generate(T, seed=seed)
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    o = _lib.default_opts(mode=_lib.MODE_MAP)
    res = engine.alloc_outputs(T, opts=o)
    pp = torch.empty((T, _lib.NPRED, _lib.NPOS), dtype=torch.float32, device=ty.device)
    rec = torch.empty((T, _lib.NMAPPRED), dtype=torch.float64, device=ty.device)
    psis = torch.empty((T, 3, _lib.NMAPPSIS), dtype=torch.float64, device=ty.device)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    alone, flags = [], {}
    both, kern, pk = ({S: [] for S in DRAWS} for _ in range(3))
    for rep in range(WARM + REPS):
        e0, e1 = ev(), ev()
        e0.record()
        engine.fit_batch_device(ty, tN, tm, o, res)
        e1.record()
        torch.cuda.synchronize()
        if rep >= WARM:
            alone.append(e0.elapsed_time(e1))
        for S in DRAWS:
            f0, f1, f2, f3 = ev(), ev(), ev(), ev()
            f0.record()
            engine.fit_batch_device(ty, tN, tm, o, res)
            f1.record()
            engine.map_pred_device(ty, tN, res, S, R, 0, 0, ppred=pp, rec=rec)
            f2.record()
            engine.map_psis_device(ty, tN, res, S, 0, 0, psis=psis)
            f3.record()
            torch.cuda.synchronize()
            if rep >= WARM:
                both[S].append(f0.elapsed_time(f2))
                kern[S].append(f1.elapsed_time(f2))
                pk[S].append(f2.elapsed_time(f3))
            fl = rec[:, _lib.NMAPPRED - 1].to(torch.int64)
            ok = res.status == 0
            n = int(ok.sum())
            flags[S] = (int((((fl & 1) == 0) & ok).sum()) / n, int((((fl & 3) == 1) & ok).sum()) / n)
    nuts_ms = None
    if nuts:
        on = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=500, num_samples=1000)
        rn = engine.alloc_outputs(T, opts=on)
        times = []
        for rep in range(3 if T <= 20_000 else 1):
            e0, e1 = ev(), ev()
            e0.record()
            engine.fit_batch_device(ty, tN, tm, on, rn)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        nuts_ms = float(np.median(times[1:])) if len(times) > 1 else times[0]
    med = lambda d: {S: float(np.median(v)) for S, v in d.items()}  # noqa: E731
    return float(np.median(alone)), med(both), med(kern), med(pk), flags, nuts_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-nuts", action="store_true")
    a = ap.parse_args()
    lines = [f"mdfit_map_pred (R = {R}) beside the MAP call: {torch.cuda.get_device_name(0)}, medians of {REPS} warm "
             f"repetitions after {WARM} warm-ups, HIP events on one stream"]
    for T, seed in ((10_000, 1), (125_000, 3)):
        alone, both, kern, pk, flags, nuts_ms = measure(T, seed, not a.no_nuts)
        lines.append(f"T={T:>7d} seed={seed}: MAP call {alone * 1e3:9.1f} us"
                     + (f" | NUTS call (500 + 1000) {nuts_ms:9.1f} ms" if nuts_ms is not None else ""))
        for S in DRAWS:
            added = both[S] - alone
            expect = POST_MS_PER_TAXON * T + pk[S]
            lines.append(f"    S={S:>4d}: call + pred {both[S] * 1e3:9.1f} us | added {added * 1e3:9.1f} us = "
                         f"{added / alone:6.2f} x the MAP call | launch alone {kern[S] * 1e3:9.1f} us = "
                         f"{T * 32 * R / (kern[S] * 1e-3) / 1e9:5.2f} G predictive draws/s | map_psis launch "
                         f"{pk[S] * 1e3:9.1f} us: pred / psis {kern[S] / pk[S]:5.2f} x | post kernel's predictive "
                         f"share + map_psis {expect * 1e3:9.1f} us: pred / that {kern[S] / expect:5.2f} x"
                         + (f" | NUTS / (MAP + pred) {nuts_ms / both[S]:6.1f} x" if nuts_ms is not None else "")
                         + f" | taxa with an invalid row {100 * flags[S][0]:.1f} %, all valid with a khat over the "
                         f"threshold {100 * flags[S][1]:.1f} %")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
