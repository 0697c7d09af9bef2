"""Cost and accuracy of the auto inference with the posterior predictive
(MDFIT-AUTO v1.1).

1. Launch cost: mdfit_map_pred of a baseline library (--baseline-lib: the parent
   commit's libmdfit.so, loaded beside this tree's; without it the column is
   left out) against mdfit_map_pred and mdfit_map_pred_adapt (R = 0 and 3) of
   this build: 10k taxa (seed 1) and 125k taxa (seed 3), S = 256 and 1024,
   R_pred = 1000.  HIP events around each launch on one stream, the launches
   alternated, 10 repetitions after 2 warm-ups, the median taken.
2. The auto call (engine.fit_auto_device, 10k taxa, seed 1, 500 + 1000, S = 256,
   psis_adapt 3) with and without auto_pred beside the plain NUTS call: stage
   times, the sampled share, the taxa MDFIT_ROUTE_PRED alone adds; alternated,
   medians of --auto-reps repetitions after one warm-up.
3. Accuracy on the settled taxa of that batch against two plain NUTS calls
   (seeds 0 and 1): the ratio of the 68 % window of D_max to NUTS's and |D_max -
   NUTS| in units of 1 / N_z1 for the composed record, the MAP record and the
   composed record of the taxa carrying MDFIT_FLAG_ADAPTED, each beside the
   seed-to-seed figure.
There is no pass bar.

    python tools/auto_pred_cost.py [--out profiles/auto_pred_cost.txt] [--baseline-lib PATH] [--skip-125k]
                                   [--taxa 10000] [--auto-reps 10]
"""
import argparse
import ctypes
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
R, R_PRED, S_AUTO = 3, 1000, 256


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def baseline_pred(path):
    lib = ctypes.CDLL(str(path))
    vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    lib.mdfit_map_pred.argtypes = [vp, vp, vp, vp, i64, i32, i32, u64, i64, vp, vp, vp, vp, vp]
    lib.mdfit_map_pred.restype = ctypes.c_int

    def pred(ty, tN, res, S, pp, rec):
        rc = lib.mdfit_map_pred(vp(ty.data_ptr()), vp(tN.data_ptr()), vp(res.out.data_ptr()),
                                vp(res.status.data_ptr()), int(ty.shape[0]), S, R_PRED, 0, 0, vp(pp.data_ptr()),
                                vp(rec.data_ptr()), None, None, vp(torch.cuda.current_stream().cuda_stream))
        assert rc == 0

    return pred


def launch_cost(T, seed, base):
    b = generate(T, seed=seed)
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    res = engine.fit_batch_device(ty, tN, tm, _lib.default_opts(mode=_lib.MODE_MAP))
    torch.cuda.synchronize()
    pps = [torch.empty((T, _lib.NPRED, _lib.NPOS), dtype=torch.float32, device=ty.device) for _ in range(4)]
    recs = [torch.empty((T, _lib.NMAPPRED), dtype=torch.float64, device=ty.device) for _ in range(4)]
    ad = torch.empty((T, 3, _lib.NMAPADAPT), dtype=torch.float64, device=ty.device)
    rows = []
    for S in DRAWS:
        fns = [("pred", lambda: engine.map_pred_device(ty, tN, res, S, R_PRED, 0, 0, ppred=pps[1], rec=recs[1])),
               ("adapt0", lambda: engine.map_pred_device(ty, tN, res, S, R_PRED, 0, 0, ppred=pps[2], rec=recs[2],
                                                         adapt_rounds=0, adapt=ad)),
               ("adapt3", lambda: engine.map_pred_device(ty, tN, res, S, R_PRED, 0, 0, ppred=pps[3], rec=recs[3],
                                                         adapt_rounds=R, adapt=ad))]
        if base is not None:
            fns.insert(0, ("parent", lambda: base(ty, tN, res, S, pps[0], recs[0])))
        t = {name: [] for name, _ in fns}
        for rep in range(WARM + REPS):
            for name, fn in fns:
                ms, _ = timed(fn)
                if rep >= WARM:
                    t[name].append(ms)

        def bits(x):
            return x.view(torch.int64 if x.dtype == torch.float64 else torch.int32)

        same_parent = (base is None or (torch.equal(bits(pps[0]), bits(pps[1])) and
                                        torch.equal(bits(recs[0]), bits(recs[1]))))
        same_zero = torch.equal(bits(pps[1]), bits(pps[2])) and torch.equal(bits(recs[1]), bits(recs[2]))
        f1, f3 = recs[1][:, -1].to(torch.int64), recs[3][:, -1].to(torch.int64)
        rows.append({"T": T, "S": S, "ms": {k: float(np.median(v)) for k, v in t.items()},
                     "spread": {k: (float(np.min(v)), float(np.max(v))) for k, v in t.items()},
                     "same_parent": bool(same_parent), "same_zero": bool(same_zero),
                     "valid": int(((f1 & 1) != 0).sum()),
                     "reliable": (int(((f1 & 2) != 0).sum()), int(((f3 & 2) != 0).sum())),
                     "adapted": int(((f3 & 64) != 0).sum())})
    return rows


def auto_cost(T, reps):
    b = generate(T, seed=1)
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    opts = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=500, num_samples=1000, seed=0)
    rn = engine.alloc_outputs(T, opts=opts)
    stages = ("map", "psis", "waic", "pred", "route", "gather", "sampler", "scatter")
    got = {"nuts": {"whole": []}}
    for k in (False, True):
        got[k] = {"whole": [], **{s: [] for s in stages}}
    keep = {}
    for rep in range(reps + 1):
        ms, _ = timed(lambda: engine.fit_batch_device(ty, tN, tm, opts, rn))
        if rep:
            got["nuts"]["whole"].append(ms)
        for k in (False, True):
            tm_ = {}
            ms, r = timed(lambda: engine.fit_auto_device(ty, tN, tm, opts, S_AUTO, timings=tm_, psis_adapt=R,
                                                         auto_pred=k))
            if rep:
                got[k]["whole"].append(ms)
                for s in stages:
                    got[k][s].append(tm_.get(s, 0.0))
            got[k]["n_sampled"] = tm_["n_sampled"]
            keep[k] = r
    out = {}
    for k, v in got.items():
        out[k] = {n: (float(np.median(x)) if isinstance(x, list) else x) for n, x in v.items()}
        out[k]["spread"] = (float(np.min(v["whole"])), float(np.max(v["whole"])))
    route = keep[True][1]
    out["pred_alone"] = int((route == _lib.ROUTE_PRED).sum())
    out["routes"] = torch.bincount(route.to(torch.int64), minlength=24).tolist()
    return out, (b, ty, tN, tm, opts, rn, keep)


def accuracy(state):
    """The settled taxa (route 0 with auto_pred) against NUTS seeds 0 and 1."""
    b, ty, tN, tm, opts, rn, keep = state
    res, route, _ = keep[True]
    T = int(ty.shape[0])
    F = _lib.RESULT_FIELDS.index
    cols = [F("D_max"), F("D_max_lower_hpdi"), F("D_max_upper_hpdi")]
    comp = res.out[:, cols].cpu().numpy()
    m = engine.fit_batch_device(ty, tN, tm, engine.auto_opts(opts)[0])
    psis, _ = engine.map_psis_device(ty, tN, m, S_AUTO, 0, 0, adapt_rounds=R)
    torch.cuda.synchronize()
    mapr = m.out[:, cols].cpu().numpy()
    adapted = ((psis[:, :, -1].to(torch.int64) & _lib.MAPPSIS_ADAPTED) != 0).any(dim=1).cpu().numpy()
    nuts = []
    for seed in (0, 1):
        o = _lib.MdfitOpts.from_buffer_copy(opts)
        o.seed = seed
        r = engine.fit_batch_device(ty, tN, tm, o, rn)
        torch.cuda.synchronize()
        nuts.append((r.out[:, cols].cpu().numpy(), r.status.cpu().numpy().copy()))
    (n0, s0), (n1, s1) = nuts
    settled = (route.cpu().numpy() == 0) & (s0 == 0) & (s1 == 0) & (b.N[:T, 0] > 0)
    nz1 = b.N[:T, 0].astype(np.float64)

    def stats(rec, ref, sel):
        with np.errstate(all="ignore"):
            w = (rec[sel, 2] - rec[sel, 1]) / (ref[sel, 2] - ref[sel, 1])
            d = np.abs(rec[sel, 0] - ref[sel, 0]) * nz1[sel]
        w, d = w[np.isfinite(w)], d[np.isfinite(d)]
        q = lambda x: tuple(float(v) for v in np.percentile(x, (5, 50, 95)))  # noqa: E731
        return {"n": int(sel.sum()), "width": q(w), "dist": q(d), "dist_mean": float(d.mean())}

    return {"composed": stats(comp, n0, settled), "map": stats(mapr, n0, settled),
            "composed, adapted taxa": stats(comp, n0, settled & adapted),
            "map, adapted taxa": stats(mapr, n0, settled & adapted),
            "NUTS seed 1 (seed to seed)": stats(n1, n0, settled),
            "NUTS seed 1, adapted taxa": stats(n1, n0, settled & adapted)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--skip-125k", action="store_true")
    ap.add_argument("--skip-auto", action="store_true")
    ap.add_argument("--taxa", type=int, default=10_000)
    ap.add_argument("--auto-reps", type=int, default=REPS)
    a = ap.parse_args()
    name = torch.cuda.get_device_name(0)
    base = baseline_pred(a.baseline_lib) if a.baseline_lib else None
    lines = [f"MDFIT-AUTO v1.1, R = {R}, R_pred = {R_PRED}: {name}; medians of {REPS} repetitions after {WARM} warm-ups, "
             "HIP events around each launch on one stream, the launches alternated; parent: "
             + (f"the baseline build's {Path(a.baseline_lib).name}, loaded beside this tree's" if base else "not loaded"),
             "", "launch cost (ms; min .. max in brackets)",
             f"{'taxa':>7} {'S':>5} {'parent map_pred':>26} {'map_pred':>26} {'map_pred_adapt R=0':>26} "
             f"{'map_pred_adapt R=3':>26} {'R=3 / map_pred':>14}"]
    sizes = [(a.taxa, 1)] + ([] if a.skip_125k else [(125_000, 3)])
    rows = []
    for T, seed in sizes:
        for r in launch_cost(T, seed, base):
            rows.append(r)
            m, s = r["ms"], r["spread"]
            c = lambda k: f"{m[k]:8.2f} [{s[k][0]:.2f} .. {s[k][1]:.2f}]" if k in m else "-"  # noqa: E731
            lines.append(f"{r['T']:>7} {r['S']:>5} {c('parent'):>26} {c('pred'):>26} {c('adapt0'):>26} {c('adapt3'):>26} "
                         f"{m['adapt3'] / m['pred']:14.3f}")
    lines.append("")
    for r in rows:
        inside = ""
        if "parent" in r["ms"]:
            lo, hi = r["spread"]["parent"]
            inside = f"  map_pred median inside the parent's min .. max: {lo <= r['ms']['pred'] <= hi};"
        lines.append(f"{r['T']:>7} {r['S']:>5}{inside}  map_pred equals the parent's bit for bit: {r['same_parent']};  "
                     f"R = 0 equals map_pred bit for bit: {r['same_zero']};  taxa valid {r['valid']}, reliable "
                     f"{r['reliable'][0]} -> {r['reliable'][1]}, adapted {r['adapted']}")
    if not a.skip_auto:
        T = a.taxa
        own, state = auto_cost(T, a.auto_reps)
        nn = own["nuts"]["whole"]
        lines += ["", f"auto inference at {T} taxa (seed 1), 500 + 1000, S = {S_AUTO}, psis_adapt {R}: medians of "
                  f"{a.auto_reps} repetitions after one warm-up, the calls alternated (ms)",
                  f"{'':>22} {'sampled':>8} {'share':>7} {'map':>7} {'psis':>7} {'waic':>7} {'pred':>7} {'sampler':>9} "
                  f"{'whole':>9} {'whole min .. max':>22} {'/ NUTS':>7}",
                  f"{'plain NUTS call':>22} {'':>8} {'':>7} {'':>7} {'':>7} {'':>7} {'':>7} {'':>9} {nn:9.1f} "
                  f"{own['nuts']['spread'][0]:10.1f} .. {own['nuts']['spread'][1]:<8.1f}"]
        for k, label in ((False, "auto"), (True, "auto, auto_pred")):
            d = own[k]
            lines.append(f"{label:>22} {d['n_sampled']:>8} {100 * d['n_sampled'] / T:6.1f}% {d['map']:7.2f} "
                         f"{d['psis']:7.2f} {d['waic']:7.2f} {d['pred']:7.2f} {d['sampler']:9.1f} {d['whole']:9.1f} "
                         f"{d['spread'][0]:10.1f} .. {d['spread'][1]:<8.1f} {d['whole'] / nn:7.3f}")
        lines.append(f"taxa sampled for MDFIT_ROUTE_PRED alone (route == 16): {own['pred_alone']}; routes 0 .. 23: "
                     f"{own['routes']}")
        acc = accuracy(state)
        lines += ["", "accuracy on the settled taxa (route 0 with auto_pred, N_z1 > 0, both NUTS calls valid) against "
                  "the plain NUTS call with seed 0: 68 % window of D_max over NUTS's, and |D_max - NUTS| x N_z1; "
                  "5 % / median / 95 % over the taxa",
                  f"{'record':>28} {'taxa':>6} {'window ratio':>26} {'|D_max - NUTS| x N_z1':>30} {'mean':>7}"]
        for label, s in acc.items():
            lines.append(f"{label:>28} {s['n']:>6} {s['width'][0]:8.3f} {s['width'][1]:8.3f} {s['width'][2]:8.3f} "
                         f"{s['dist'][0]:10.3f} {s['dist'][1]:9.3f} {s['dist'][2]:9.3f} {s['dist_mean']:7.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
