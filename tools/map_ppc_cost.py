"""Cost of mdfit_map_ppc(_adapt) beside the mdfit_map_pred(_adapt) launch whose
phases 1-4 and predictive draws it repeats.

HIP events on one stream around each launch alone, the two kernels alternated in
one session and in both run orders (ppc then pred, pred then ppc), 5 warm
repetitions of each order after 2 warm-ups, the median and the spread (min ..
max) taken over both orders: 10k taxa (seed 1) and 125k taxa (seed 3), S = 256
and 1024, R = 1000, without rounds and with three.  Then, on generate(10000,
seed=1) at S = 256: the share of valid records and of small p-values on clean
synthetic data.  There is no pass bar.

    python tools/map_ppc_cost.py [--out profiles/map_ppc_cost.txt] [--quick]
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

WARM, REPS = 2, 5
DRAWS = (256, 1024)
ROUNDS = (0, 3)
PRED = 1000


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
    ppos = torch.empty((T, _lib.NPOS), dtype=torch.float32, device=dev)
    crec = torch.empty((T, _lib.NMAPPPC), dtype=torch.float64, device=dev)
    ppred = torch.empty((T, _lib.NPRED, _lib.NPOS), dtype=torch.float32, device=dev)
    prec = torch.empty((T, _lib.NMAPPRED), dtype=torch.float64, device=dev)
    adapt = torch.empty((T, 3, _lib.NMAPADAPT), dtype=torch.float64, device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    tc = {(S, R): [] for S in DRAWS for R in ROUNDS}
    tp = {(S, R): [] for S in DRAWS for R in ROUNDS}
    for rep in range(2 * (warm + reps)):
        ppc_first = rep % 2 == 0
        for S in DRAWS:
            for R in ROUNDS:
                kw = {"adapt_rounds": R, "adapt": adapt} if R else {}
                ppc = lambda: engine.map_ppc_device(ty, tN, res, S, PRED, 0, 0, ppos=ppos, rec=crec, **kw)  # noqa: E731
                pred = lambda: engine.map_pred_device(ty, tN, res, S, PRED, 0, 0, ppred=ppred, rec=prec, **kw)  # noqa: E731
                e0, e1, e2 = ev(), ev(), ev()
                e0.record()
                (ppc if ppc_first else pred)()
                e1.record()
                (pred if ppc_first else ppc)()
                e2.record()
                torch.cuda.synchronize()
                if rep >= 2 * warm:
                    a, b = e0.elapsed_time(e1), e1.elapsed_time(e2)
                    tc[(S, R)].append(a if ppc_first else b)
                    tp[(S, R)].append(b if ppc_first else a)
    return tc, tp


def clean_rates(T, seed, S):
    ty, tN, res = fitted(T, seed)
    ok = (res.status == 0).cpu().numpy()
    lines = []
    f = _lib.MAPPPC_FIELDS.index
    for R in ROUNDS:
        got = engine.map_ppc_device(ty, tN, res, S, PRED, 0, 0, adapt_rounds=R)
        torch.cuda.synchronize()
        rec = got[1].cpu().numpy()[ok]
        fl = rec[:, f("flags")].astype(np.int64)
        v = (fl & _lib.MAPPPC_VALID) != 0
        rel = v & ((fl & _lib.MAPPPC_RELIABLE) != 0)
        po, ps = rec[v, f("p_outlier")], rec[v, f("p_strand")]
        ps = ps[np.isfinite(ps)]
        lines.append(f"    R={R}: valid {int(v.sum())} of {int(ok.sum())} ({100 * v.mean():.1f} %), valid and reliable "
                     f"{100 * rel.mean():.1f} %, a draw that is no count {int(((fl & _lib.MAPPPC_NONCOUNT) != 0).sum())} | "
                     f"p_outlier < 0.01: {100 * (po < 0.01).mean():.2f} %, < 0.05: {100 * (po < 0.05).mean():.2f} % | "
                     f"p_strand < 0.01: {100 * (ps < 0.01).mean():.2f} %, < 0.05: {100 * (ps < 0.05).mean():.2f} % | "
                     f"median n_low {np.median(rec[v, f('n_low')]):.0f}, mean {rec[v, f('n_low')].mean():.2f} of "
                     f"{rec[v, f('n_points')].mean():.1f} columns")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="1,000 and 2,000 taxa, 1 repetition per order: a rehearsal")
    a = ap.parse_args()
    reps, warm = (1, 1) if a.quick else (REPS, WARM)
    lines = [f"mdfit_map_ppc(_adapt) beside mdfit_map_pred(_adapt), R = {PRED}: {torch.cuda.get_device_name(0)}, launches "
             f"alone, alternated in one session in both run orders, medians (min .. max) of {2 * reps} warm repetitions "
             f"({reps} per order) after {2 * warm} warm-ups, HIP events on one stream"]
    for T, seed in (((1_000, 1), (2_000, 3)) if a.quick else ((10_000, 1), (125_000, 3))):
        tc, tp = timings(T, seed, reps, warm)
        lines.append(f"T={T:>7d} seed={seed}:")
        for S in DRAWS:
            for R in ROUNDS:
                mc, mp = float(np.median(tc[(S, R)])), float(np.median(tp[(S, R)]))
                first = float(np.median(tc[(S, R)][0::2])) / float(np.median(tp[(S, R)][0::2]))
                second = float(np.median(tc[(S, R)][1::2])) / float(np.median(tp[(S, R)][1::2]))
                lines.append(f"    S={S:>4d} R={R}: ppc {mc * 1e3:10.1f} us ({min(tc[(S, R)]) * 1e3:.1f} .. "
                             f"{max(tc[(S, R)]) * 1e3:.1f}) | pred {mp * 1e3:10.1f} us ({min(tp[(S, R)]) * 1e3:.1f} .. "
                             f"{max(tp[(S, R)]) * 1e3:.1f}) | ppc / pred {mc / mp:5.3f} (ppc first {first:5.3f}, pred first "
                             f"{second:5.3f})")
    T = 1_000 if a.quick else 10_000
    lines.append(f"generate({T}, seed=1), S = 256, R = {PRED}, clean synthetic data:")
    lines += clean_rates(T, 1, 256)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
