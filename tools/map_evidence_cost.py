"""Cost of mdfit_map_evidence(_adapt) beside the mdfit_map_waic(_adapt) launch
whose phases 1-3 it shares, and what the Bayes factor says beside n_sigma_waic
(DESIGN.md §3.14).

HIP events on one stream around each launch alone, the two kernels alternated in
one session, 10 warm repetitions each after 2 warm-ups, the median and the
spread (min .. max) taken: 10k taxa (seed 1) and 125k taxa (seed 3), S = 256 and
1024, without rounds and with three.  Then, on generate(10000, seed=1) at S =
256: the rows valid and reliable without rounds and with three, and the split of
log_bf against n_sigma_waic.  Then log_bf of the 26 taxa of generate(400, 21)
that §3.9 compares with NUTS.  There is no pass bar.

    python tools/map_evidence_cost.py [--out profiles/map_evidence_cost.txt] [--quick]
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
ROUNDS = (0, 3)
# §3.9's table: generate(400, 21), the first 10 ancient with mean N > 3e3, the first 8 ancient below, the first 8 others
NUTS_TAXA = (7, 10, 13, 16, 17, 23, 24, 29, 31, 37, 3, 36, 40, 57, 64, 70, 71, 80, 0, 1, 2, 4, 5, 6, 8, 9)


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
    evid = torch.empty((T, _lib.NEVIDROW, _lib.NMAPEVID), dtype=torch.float64, device=ty.device)
    waic = torch.empty((T, _lib.NWAICROW, _lib.NMAPWAIC), dtype=torch.float64, device=ty.device)
    adapt = torch.empty((T, 3, _lib.NMAPADAPT), dtype=torch.float64, device=ty.device)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    te = {(S, R): [] for S in DRAWS for R in ROUNDS}
    tw = {(S, R): [] for S in DRAWS for R in ROUNDS}
    for rep in range(warm + reps):
        for S in DRAWS:
            for R in ROUNDS:
                kw = {"adapt_rounds": R, "adapt": adapt} if R else {}
                e0, e1, e2 = ev(), ev(), ev()
                e0.record()
                engine.map_evidence_device(ty, tN, res, S, 0, 0, evid=evid, **kw)
                e1.record()
                engine.map_waic_device(ty, tN, res, S, 0, 0, waic=waic, **kw)
                e2.record()
                torch.cuda.synchronize()
                if rep >= warm:
                    te[(S, R)].append(e0.elapsed_time(e1))
                    tw[(S, R)].append(e1.elapsed_time(e2))
    return te, tw


def split(T, seed, S):
    ty, tN, res = fitted(T, seed)
    ok = (res.status == 0).cpu().numpy()
    lines = []
    waic = engine.map_waic_device(ty, tN, res, S, 0, 0)
    torch.cuda.synchronize()
    waic = waic.cpu().numpy()
    for R in ROUNDS:
        got = engine.map_evidence_device(ty, tN, res, S, 0, 0, adapt_rounds=R)
        torch.cuda.synchronize()
        e = (got[0] if isinstance(got, tuple) else got).cpu().numpy()
        fl = e[ok][:, :6, 7].astype(np.int64)
        f6 = e[ok][:, 6, 7].astype(np.int64)
        n = int(ok.sum())
        lines.append(f"    R={R}: rows valid {int((fl & 1).sum())} of {6 * n} ({100 * (fl & 1).mean():.1f} %), valid and "
                     f"reliable {int(((fl & 3) == 3).sum())} ({100 * ((fl & 3) == 3).mean():.1f} %), adapted "
                     f"{int(((fl & 64) != 0).sum())} | taxa with all six valid {100 * (f6 & 1).mean():.1f} %, all six "
                     f"reliable {100 * ((f6 & 3) == 3).mean():.1f} % | median log_bf_se "
                     f"{np.nanmedian(e[ok][:, 6, 4]):.3f}, 95th percentile {np.nanpercentile(e[ok][:, 6, 4], 95):.3f}")
        if R == 0:
            lbf, ns = e[:, 6, 0], waic[:, 6, 0]
            both = ok & np.isfinite(lbf) & np.isfinite(ns)
            lbf, ns = lbf[both], ns[both]
            rk = lambda v: np.argsort(np.argsort(v)).astype(float)  # noqa: E731
            rho = float(np.corrcoef(rk(lbf), rk(ns))[0, 1])
            lines.append(f"    log_bf against n_sigma_waic over {int(both.sum())} taxa with both: rank correlation "
                         f"{rho:.3f}; log_bf quantiles 5/25/50/75/95 % "
                         + " ".join(f"{np.percentile(lbf, q):.1f}" for q in (5, 25, 50, 75, 95)))
            for lo, hi, name in ((-np.inf, 0.0, "log_bf <= 0"), (0.0, 3.0, "0 < log_bf <= 3"),
                                 (3.0, np.inf, "log_bf > 3")):
                m = (lbf > lo) & (lbf <= hi)
                lines.append(f"        {name:>16s}: {int(m.sum()):5d} taxa | n_sigma_waic <= 2: {int((ns[m] <= 2).sum()):5d}, "
                             f"2 .. 3: {int(((ns[m] > 2) & (ns[m] <= 3)).sum()):5d}, > 3: {int((ns[m] > 3).sum()):5d}")
    return lines


def nuts_taxa(S):
    ty, tN, res = fitted(400, 21)
    out = res.out.cpu().numpy()
    waic = engine.map_waic_device(ty, tN, res, S, 0, 0)
    e0 = engine.map_evidence_device(ty, tN, res, S, 0, 0)
    e3 = engine.map_evidence_device(ty, tN, res, S, 0, 0, adapt_rounds=3)[0]
    torch.cuda.synchronize()
    waic, e0, e3 = waic.cpu().numpy(), e0.cpu().numpy(), e3.cpu().numpy()
    lines = ["    taxon | n_sigma MAP | n_sigma_waic | log_bf R=0 (se, khat max, flags) | log_bf R=3 (se, khat max, flags)"
             " | damage_probability R=3"]
    for t in NUTS_TAXA:
        lines.append(f"    {t:5d} | {out[t, 1]:7.2f} | {waic[t, 6, 0]:7.2f} | {e0[t, 6, 0]:8.2f} ({e0[t, 6, 4]:.3f}, "
                     f"{e0[t, 6, 5]:.2f}, {int(e0[t, 6, 7])}) | {e3[t, 6, 0]:8.2f} ({e3[t, 6, 4]:.3f}, {e3[t, 6, 5]:.2f}, "
                     f"{int(e3[t, 6, 7])}) | {1 / (1 + np.exp(-e3[t, 6, 0])):.4f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="1,000 and 2,000 taxa, 2 repetitions: a rehearsal")
    a = ap.parse_args()
    reps, warm = (2, 1) if a.quick else (REPS, WARM)
    lines = [f"mdfit_map_evidence(_adapt) beside mdfit_map_waic(_adapt): {torch.cuda.get_device_name(0)}, launches "
             f"alone, alternated in one session, medians (min .. max) of {reps} warm repetitions after {warm} warm-ups, "
             "HIP events on one stream"]
    for T, seed in (((1_000, 1), (2_000, 3)) if a.quick else ((10_000, 1), (125_000, 3))):
        te, tw = timings(T, seed, reps, warm)
        lines.append(f"T={T:>7d} seed={seed}:")
        for S in DRAWS:
            for R in ROUNDS:
                me, mw = float(np.median(te[(S, R)])), float(np.median(tw[(S, R)]))
                lines.append(f"    S={S:>4d} R={R}: evidence {me * 1e3:10.1f} us ({min(te[(S, R)]) * 1e3:.1f} .. "
                             f"{max(te[(S, R)]) * 1e3:.1f}) | waic {mw * 1e3:10.1f} us ({min(tw[(S, R)]) * 1e3:.1f} .. "
                             f"{max(tw[(S, R)]) * 1e3:.1f}) | evidence / waic {me / mw:5.3f}")
    T = 1_000 if a.quick else 10_000
    lines.append(f"generate({T}, seed=1), S = 256:")
    lines += split(T, 1, 256)
    lines.append("the 26 taxa of generate(400, 21) that DESIGN.md §3.9 compares with NUTS, S = 256, seed 0 (flags: bit 0 all "
                 "six rows valid, bit 1 and reliable):")
    lines += nuts_taxa(256)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
