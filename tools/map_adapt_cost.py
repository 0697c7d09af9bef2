"""Cost and effect of the moment-matched proposal rounds of the MAP importance
sampling (MDFIT-ADAPT v1).

1. Launch cost: mdfit_map_psis_adapt and mdfit_map_waic_adapt at R = 3 against
   the mdfit_map_psis and mdfit_map_waic launches of a baseline library
   (--baseline-lib: the parent commit's libmdfit.so, loaded beside this tree's;
   without it this tree's own v1 entries, and the report says so), 10k taxa
   (seed 1) and 125k taxa (seed 3), S = 256 and 1024.  HIP events around the
   launch on one stream, the two alternated, 10 repetitions after 2 warm-ups,
   the median taken.
2. The share of valid PMD rows, and of taxa with a valid row, over the k
   threshold at 10k taxa with and without the rounds.
3. The auto inference (engine.fit_auto_device, 500 + 1000, S = 256) at 10k taxa
   with psis_adapt 0 and 3 beside the plain NUTS call: sampled share, sampler
   stage and whole call, alternated, the median of --auto-reps repetitions
   after one warm-up.  --baseline-root: a checkout of the parent commit with its
   libraries built; its auto call and NUTS call are then timed in a child
   process of this run by the same statements (--baseline-child).
There is no pass bar.

    python tools/map_adapt_cost.py [--out profiles/map_adapt_cost.txt] [--baseline-lib PATH]
                                   [--baseline-root DIR] [--skip-125k] [--auto-reps 10]
"""
import argparse
import ctypes
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

WARM, REPS = 2, 10
DRAWS = (256, 1024)
R = 3
S_AUTO = 256


def _root():
    for i, a in enumerate(sys.argv):
        if a == "--root" and i + 1 < len(sys.argv):
            return Path(sys.argv[i + 1]).resolve()
    return Path(__file__).resolve().parents[1]


ROOT = _root()
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from metadamage_amd import _lib, engine  # noqa: E402
from metadamage_amd.synthetic import generate  # noqa: E402


def ev():
    return torch.cuda.Event(enable_timing=True)


def timed(fn):
    e0, e1 = ev(), ev()
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def baseline_launchers(path):
    """(psis(ty, tN, res, S, out), waic(...)) of the v1 entries: a baseline
    library's when given, else this tree's."""
    if path is None:
        return (lambda ty, tN, res, S, out: engine.map_psis_device(ty, tN, res, S, 0, 0, psis=out),
                lambda ty, tN, res, S, out: engine.map_waic_device(ty, tN, res, S, 0, 0, waic=out))
    lib = ctypes.CDLL(str(path))
    vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    lib.mdfit_map_psis.argtypes = [vp, vp, vp, vp, i64, i32, u64, i64, vp, vp, vp]
    lib.mdfit_map_waic.argtypes = [vp, vp, vp, vp, i64, i32, u64, i64, vp, vp, vp, vp]
    lib.mdfit_map_psis.restype = lib.mdfit_map_waic.restype = ctypes.c_int

    def stream():
        return vp(torch.cuda.current_stream().cuda_stream)

    def psis(ty, tN, res, S, out):
        rc = lib.mdfit_map_psis(vp(ty.data_ptr()), vp(tN.data_ptr()), vp(res.out.data_ptr()),
                                vp(res.status.data_ptr()), int(ty.shape[0]), S, 0, 0, vp(out.data_ptr()), None, stream())
        assert rc == 0

    def waic(ty, tN, res, S, out):
        rc = lib.mdfit_map_waic(vp(ty.data_ptr()), vp(tN.data_ptr()), vp(res.out.data_ptr()),
                                vp(res.status.data_ptr()), int(ty.shape[0]), S, 0, 0, vp(out.data_ptr()), None, None,
                                stream())
        assert rc == 0

    return psis, waic


def launch_cost(T, seed, base_psis, base_waic):
    b = generate(T, seed=seed)
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    o = _lib.default_opts(mode=_lib.MODE_MAP)
    res = engine.fit_batch_device(ty, tN, tm, o)
    torch.cuda.synchronize()
    p0 = torch.empty((T, 3, _lib.NMAPPSIS), dtype=torch.float64, device=ty.device)
    p1 = torch.empty_like(p0)
    w0 = torch.empty((T, _lib.NWAICROW, _lib.NMAPWAIC), dtype=torch.float64, device=ty.device)
    w1 = torch.empty_like(w0)
    ad = torch.empty((T, 3, _lib.NMAPADAPT), dtype=torch.float64, device=ty.device)
    ok = (res.status == 0)
    rows = []
    for S in DRAWS:
        t = {"psis": [], "psis_adapt": [], "waic": [], "waic_adapt": []}
        for rep in range(WARM + REPS):
            for name, fn in (("psis", lambda: base_psis(ty, tN, res, S, p0)),
                             ("psis_adapt", lambda: engine.map_psis_device(ty, tN, res, S, 0, 0, psis=p1,
                                                                           adapt_rounds=R, adapt=ad)),
                             ("waic", lambda: base_waic(ty, tN, res, S, w0)),
                             ("waic_adapt", lambda: engine.map_waic_device(ty, tN, res, S, 0, 0, waic=w1,
                                                                           adapt_rounds=R, adapt=ad))):
                ms, _ = timed(fn)
                if rep >= WARM:
                    t[name].append(ms)
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()}
        # rows and taxa over the threshold, before and after; the rounds
        f0, f1 = p0[:, :, -1].to(torch.int64), p1[:, :, -1].to(torch.int64)
        valid = ((f0 & 1) != 0) & ok[:, None]
        over0, over1 = valid & ((f0 & 2) == 0), valid & ((f1 & 2) == 0)
        taxa = valid.any(dim=1)
        best = ad[:, :, 2][valid]
        tried = ad[:, :, 3][valid]
        same = bool(torch.equal(p0[~((f1 & 64) != 0)].view(torch.int64), p1[~((f1 & 64) != 0)].view(torch.int64)))
        rows.append({"T": T, "S": S, "ms": med, "spread": spread, "n_valid": int(valid.sum()),
                     "rows_over": (int(over0.sum()), int(over1.sum())), "n_taxa": int(taxa.sum()),
                     "taxa_over": (int((over0.any(dim=1) & taxa).sum()), int((over1.any(dim=1) & taxa).sum())),
                     "best_rounds": [int((best == r).sum()) for r in range(R + 1)],
                     "passes": float(tried.sum() + ((tried > best).sum())) / max(1, int(valid.sum())),
                     "untouched_rows_equal_baseline": same})
    return rows


def auto_cost(T, reps, adapt_values):
    """{psis_adapt or "nuts": medians}: the calls alternated, one warm-up each."""
    b = generate(T, seed=1)
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    opts = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=500, num_samples=1000, seed=0)
    rn = engine.alloc_outputs(T, opts=opts)
    got = {"nuts": {"whole": []}}
    for a in adapt_values:
        got[a] = {"whole": [], "sampler": [], "psis": [], "waic": [], "n_sampled": None}
    for rep in range(reps + 1):
        ms, _ = timed(lambda: engine.fit_batch_device(ty, tN, tm, opts, rn))
        if rep:
            got["nuts"]["whole"].append(ms)
        for a in adapt_values:
            kw = {"psis_adapt": a} if a else {}
            tm_ = {}
            ms, _ = timed(lambda: engine.fit_auto_device(ty, tN, tm, opts, S_AUTO, timings=tm_, **kw))
            if rep:
                got[a]["whole"].append(ms)
                for k in ("sampler", "psis", "waic"):
                    got[a][k].append(tm_[k])
            got[a]["n_sampled"] = tm_["n_sampled"]
    out = {}
    for k, v in got.items():
        out[str(k)] = {n: (float(np.median(x)) if isinstance(x, list) else x) for n, x in v.items()}
        out[str(k)]["whole_spread"] = (float(np.min(v["whole"])), float(np.max(v["whole"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=None, help="the checkout to import the package from (default: this tool's)")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--baseline-root", default=None)
    ap.add_argument("--baseline-child", action="store_true", help="print the baseline's auto timings as JSON and exit")
    ap.add_argument("--skip-125k", action="store_true")
    ap.add_argument("--skip-auto", action="store_true")
    ap.add_argument("--taxa", type=int, default=10_000)
    ap.add_argument("--auto-reps", type=int, default=REPS)
    a = ap.parse_args()
    if a.baseline_child:
        print("BASELINE " + json.dumps(auto_cost(a.taxa, a.auto_reps, [0])))
        return
    name = torch.cuda.get_device_name(0)
    base = (f"the baseline build's {Path(a.baseline_lib).name}, loaded beside this tree's" if a.baseline_lib
            else "this tree's own v1 entries (no baseline library)")
    lines = [f"MDFIT-ADAPT v1, R = {R}: {name}; medians of {REPS} repetitions after {WARM} warm-ups, HIP events around "
             f"each launch on one stream, the four launches alternated; v1 launches: {base}", ""]
    bp, bw = baseline_launchers(a.baseline_lib)
    sizes = [(a.taxa, 1)] + ([] if a.skip_125k else [(125_000, 3)])
    lines.append("launch cost (ms; min .. max in brackets)")
    lines.append(f"{'taxa':>7} {'S':>5} {'map_psis':>22} {'map_psis_adapt':>22} {'ratio':>6} {'map_waic':>22} "
                 f"{'map_waic_adapt':>22} {'ratio':>6}")
    all_rows = []
    for T, seed in sizes:
        for r in launch_cost(T, seed, bp, bw):
            all_rows.append(r)
            m, s = r["ms"], r["spread"]
            c = lambda k: f"{m[k]:8.2f} [{s[k][0]:.2f} .. {s[k][1]:.2f}]"  # noqa: E731
            lines.append(f"{r['T']:>7} {r['S']:>5} {c('psis'):>22} {c('psis_adapt'):>22} "
                         f"{m['psis_adapt'] / m['psis']:6.3f} {c('waic'):>22} {c('waic_adapt'):>22} "
                         f"{m['waic_adapt'] / m['waic']:6.3f}")
    lines += ["", "valid PMD rows and taxa over the k threshold, v1 -> adapted; best round 0 / 1 / 2 / 3; extra passes "
              "of phases 2-3 per valid row (rounds tried, plus the re-run after a dropped round)"]
    for r in all_rows:
        lines.append(f"{r['T']:>7} {r['S']:>5}  rows {r['rows_over'][0]} -> {r['rows_over'][1]} of {r['n_valid']} "
                     f"({100 * r['rows_over'][0] / r['n_valid']:.1f} % -> {100 * r['rows_over'][1] / r['n_valid']:.1f} %)"
                     f"  taxa {r['taxa_over'][0]} -> {r['taxa_over'][1]} of {r['n_taxa']} "
                     f"({100 * r['taxa_over'][0] / r['n_taxa']:.1f} % -> {100 * r['taxa_over'][1] / r['n_taxa']:.1f} %)"
                     f"  best {r['best_rounds']}  passes +{r['passes']:.3f}"
                     f"  rows not adapted equal the v1 launch's bit for bit: {r['untouched_rows_equal_baseline']}")
    if not a.skip_auto:
        own = auto_cost(a.taxa, a.auto_reps, [0, R])
        parent = None
        if a.baseline_root:
            broot = str(Path(a.baseline_root).resolve())
            cmd = [sys.executable, str(Path(__file__).resolve()), "--root", broot, "--baseline-child",
                   "--taxa", str(a.taxa), "--auto-reps", str(a.auto_reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=broot, timeout=900)
            if r.returncode != 0:
                raise SystemExit("baseline child failed:\n" + r.stderr[-3000:])
            parent = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("BASELINE ")][-1][9:])
        T = a.taxa
        lines += ["", f"auto inference at {T} taxa (seed 1), 500 + 1000, S = {S_AUTO}: medians of {a.auto_reps} "
                  "repetitions after one warm-up, the calls alternated (ms)",
                  f"{'':>28} {'sampled':>8} {'share':>7} {'psis':>8} {'waic':>8} {'sampler':>9} {'whole':>9} "
                  f"{'whole min .. max':>22} {'/ NUTS':>7}"]

        def row(label, d, nuts):
            return (f"{label:>28} {d['n_sampled']:>8} {100 * d['n_sampled'] / T:6.1f}% {d['psis']:8.2f} {d['waic']:8.2f} "
                    f"{d['sampler']:9.1f} {d['whole']:9.1f} {d['whole_spread'][0]:10.1f} .. {d['whole_spread'][1]:<8.1f} "
                    f"{d['whole'] / nuts:7.3f}")

        if parent is not None:
            pn = parent["nuts"]["whole"]
            lines.append(f"{'baseline: plain NUTS call':>28} {'':>8} {'':>7} {'':>8} {'':>8} {'':>9} {pn:9.1f} "
                         f"{parent['nuts']['whole_spread'][0]:10.1f} .. {parent['nuts']['whole_spread'][1]:<8.1f}")
            lines.append(row("baseline: auto", parent["0"], pn))
        nn = own["nuts"]["whole"]
        lines.append(f"{'plain NUTS call':>28} {'':>8} {'':>7} {'':>8} {'':>8} {'':>9} {nn:9.1f} "
                     f"{own['nuts']['whole_spread'][0]:10.1f} .. {own['nuts']['whole_spread'][1]:<8.1f}")
        lines.append(row("auto, psis_adapt 0", own["0"], nn))
        lines.append(row(f"auto, psis_adapt {R}", own[str(R)], nn))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
