"""Cost of mdfit_map_quant(_adapt) beside the mdfit_map_psis(_adapt) launch whose
phases 1-3 it repeats: that launch plus five regenerations of
the draws and five sorts per sub-fit.

HIP events on one stream around each launch alone, the two kernels alternated in
one session and in both run orders (quant then psis, psis then quant), 3 warm
repetitions of each order after 2 warm-ups, the median and the spread (min ..
max) taken over both orders: 10k taxa (seed 1) and 125k taxa (seed 3), S = 256
and 1024, without rounds and with three.  Then, on generate(10000, seed=1) at
S = 256: the share of valid rows, the draws in D_max's window and the width of
the interval beside 2 std.  There is no pass bar.

    python tools/map_quant_cost.py [--out profiles/map_quant_cost.txt] [--quick]
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

WARM, REPS = 2, 3
DRAWS = (256, 1024)
ROUNDS = (0, 3)
D0 = 0.01


def fitted(T, seed):
    b = generate(T, seed=seed)
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    o = _lib.default_opts(mode=_lib.MODE_MAP)
    res = engine.alloc_outputs(T, opts=o)
    engine.fit_batch_device(ty, tN, tm, o, res)
    torch.cuda.synchronize()
    return ty, tN, res


def timings(T, seed, reps, warm):
    ty, tN, res = fitted(T, seed)
    dev = ty.device
    quant = torch.empty((T, 3, _lib.NMAPQUANT), dtype=torch.float64, device=dev)
    psis = torch.empty((T, 3, _lib.NMAPPSIS), dtype=torch.float64, device=dev)
    adapt = torch.empty((T, 3, _lib.NMAPADAPT), dtype=torch.float64, device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    tq = {(S, R): [] for S in DRAWS for R in ROUNDS}
    tp = {(S, R): [] for S in DRAWS for R in ROUNDS}
    for rep in range(2 * (warm + reps)):
        quant_first = rep % 2 == 0
        for S in DRAWS:
            for R in ROUNDS:
                kw = {"adapt_rounds": R, "adapt": adapt} if R else {}
                qu = lambda: engine.map_quant_device(ty, tN, res, S, 0, 0, D0, quant=quant, **kw)  # noqa: E731
                ps = lambda: engine.map_psis_device(ty, tN, res, S, 0, 0, psis=psis, **kw)  # noqa: E731
                e0, e1, e2 = ev(), ev(), ev()
                e0.record()
                (qu if quant_first else ps)()
                e1.record()
                (ps if quant_first else qu)()
                e2.record()
                torch.cuda.synchronize()
                if rep >= 2 * warm:
                    a, b = e0.elapsed_time(e1), e1.elapsed_time(e2)
                    tq[(S, R)].append(a if quant_first else b)
                    tp[(S, R)].append(b if quant_first else a)
    return tq, tp


def clean_rates(T, seed, S):
    ty, tN, res = fitted(T, seed)
    ok = (res.status == 0).cpu().numpy()
    lines = []
    f, pf = _lib.MAPQUANT_FIELDS.index, _lib.MAPPSIS_FIELDS.index
    for R in ROUNDS:
        q = engine.map_quant_device(ty, tN, res, S, 0, 0, D0, adapt_rounds=R)
        p = engine.map_psis_device(ty, tN, res, S, 0, 0, adapt_rounds=R)
        torch.cuda.synchronize()
        q = (q[0] if isinstance(q, tuple) else q).cpu().numpy()[ok][:, 0]
        p = (p[0] if isinstance(p, tuple) else p).cpu().numpy()[ok][:, 0]
        v = (q[:, f("flags")].astype(np.int64) & _lib.MAPPSIS_VALID) != 0
        q, p = q[v], p[v]
        width = q[:, f("D_max_hi")] - q[:, f("D_max_lo")]
        skew = (p[:, pf("D_max_mean")] - q[:, f("D_max_median")]) / p[:, pf("D_max_std")]
        nw = q[:, f("n_window")]
        lines.append(f"    R={R}: PMD-all rows valid {int(v.sum())} of {int(ok.sum())} ({100 * v.mean():.1f} %) | "
                     f"draws in D_max's window: median {np.median(nw):.0f}, least {nw.min():.0f} "
                     f"of {S} | (hi - lo) / (2 std): median {np.median(width / (2 * p[:, pf('D_max_std')])):.3f} | "
                     f"(mean - median) / std: median {np.median(skew):+.3f}, largest {skew.max():+.3f} | "
                     f"P(D_max > {D0}) below 0.5: {100 * (q[:, f('D_max_p_above')] < 0.5).mean():.1f} %, "
                     f"above 0.95: {100 * (q[:, f('D_max_p_above')] > 0.95).mean():.1f} %")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="1,000 and 2,000 taxa, 1 repetition per order: a rehearsal")
    a = ap.parse_args()
    reps, warm = (1, 1) if a.quick else (REPS, WARM)
    lines = [f"mdfit_map_quant(_adapt) beside mdfit_map_psis(_adapt): {torch.cuda.get_device_name(0)}, launches alone, "
             f"alternated in one session in both run orders, medians (min .. max) of {2 * reps} warm repetitions "
             f"({reps} per order) after {2 * warm} warm-ups, HIP events on one stream"]
    for T, seed in (((1_000, 1), (2_000, 3)) if a.quick else ((10_000, 1), (125_000, 3))):
        tq, tp = timings(T, seed, reps, warm)
        lines.append(f"T={T:>7d} seed={seed}:")
        for S in DRAWS:
            for R in ROUNDS:
                mq, mp = float(np.median(tq[(S, R)])), float(np.median(tp[(S, R)]))
                first = float(np.median(tq[(S, R)][0::2])) / float(np.median(tp[(S, R)][0::2]))
                second = float(np.median(tq[(S, R)][1::2])) / float(np.median(tp[(S, R)][1::2]))
                lines.append(f"    S={S:>4d} R={R}: quant {mq * 1e3:10.1f} us ({min(tq[(S, R)]) * 1e3:.1f} .. "
                             f"{max(tq[(S, R)]) * 1e3:.1f}) | psis {mp * 1e3:10.1f} us ({min(tp[(S, R)]) * 1e3:.1f} .. "
                             f"{max(tp[(S, R)]) * 1e3:.1f}) | quant / psis {mq / mp:5.3f} (quant first {first:5.3f}, "
                             f"psis first {second:5.3f}) | quant - psis {(mq - mp) / (15 * T) * 1e6:7.1f} ns per sort")
    T = 1_000 if a.quick else 10_000
    lines.append(f"generate({T}, seed=1), S = 256, d0 = {D0}, clean synthetic data, the PMD-all row:")
    lines += clean_rates(T, 1, 256)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
