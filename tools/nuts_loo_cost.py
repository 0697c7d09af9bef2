"""Cost of mdfit_nuts_loo beside the NUTS call it follows.

HIP events on one stream around the sampling call (500 warmup, 1000 samples:
the reference's setting), around the loo launch that follows it and, for
comparison, around a mdfit_nuts_summary launch on the same workspace; 3
repetitions after 1 warm-up, the median taken; 10k taxa (seed 1) and 100k taxa
(seed 3, config C3).  The plain call's kernels are the ones a run without the
loo pass launches, so its time is the comparison.

The kernel's three parts are separated without another kernel.  With one NaN
written into every chain's first draw the launch takes its whole pass over the
draws (every pointwise log-likelihood), finds each sub-fit not finite and skips
every sort and fit: that launch is the log-likelihood pass alone.  With every
draw of a chain overwritten by its first draw each series is constant: the
launch takes the pass and the 120 sorts (the network does not depend on the
data), finds every tail constant and skips the Pareto fit and the smoothing.
The rest of the full launch is the fits.  Reports what is measured; there is
no pass/fail line.

    python tools/nuts_loo_cost.py [--out profiles/nuts_loo_cost.txt] [--sizes 10000,100000]
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

WARM, REPS = 1, 3


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(T, seed):
    b = generate(T, seed=seed)
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    o = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=500, num_samples=1000)
    res = engine.alloc_outputs(T, opts=o)
    loo = torch.empty((T, _lib.NLOOROW, _lib.NNUTSLOO), dtype=torch.float64, device=ty.device)
    summ = torch.empty((T, _lib.NSUBFIT, _lib.NNUTSSUMM), dtype=torch.float64, device=ty.device)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    call, kern, skern = [], [], []
    for rep in range(WARM + REPS):
        e0, e1, e2, e3 = ev(), ev(), ev(), ev()
        e0.record()
        engine.fit_batch_device(ty, tN, tm, o, res)
        e1.record()
        engine.nuts_loo_device(ty, tN, res, T, o, loo=loo)
        e2.record()
        engine.nuts_summary_device(res, T, o, summ=summ)
        e3.record()
        torch.cuda.synchronize()
        if rep >= WARM:
            call.append(e0.elapsed_time(e1))
            kern.append(e1.elapsed_time(e2))
            skern.append(e2.elapsed_time(e3))
    r = loo.cpu().numpy()
    out = res.out.cpu().numpy()
    valid = r[:, 6, _lib.NNUTSLOO - 1] == 1.0
    bad = r[valid, 6, 5]
    diff = np.abs(r[valid, 6, 0] - out[valid, _lib.RESULT_FIELDS.index("n_sigma")])
    good = bad == 0
    draws = engine.samples_view(res, T, o)
    # the pass and the sorts: every series constant, so no tail is fitted
    draws.copy_(draws[:, :, :1, :].expand(-1, -1, draws.shape[2], -1).clone())
    torch.cuda.synchronize()
    sorts = [_timed(lambda: engine.nuts_loo_device(ty, tN, res, T, o, loo=loo)) for _ in range(WARM + REPS)][WARM:]
    k = loo[:, :6, 3]
    assert bool(((k == 0.0) | torch.isnan(k)).all().item())
    # the pass alone: every sub-fit not finite, so no point reaches its sort
    draws[:, :, 0, 0] = float("nan")
    torch.cuda.synchronize()
    only = [_timed(lambda: engine.nuts_loo_device(ty, tN, res, T, o, loo=loo)) for _ in range(WARM + REPS)][WARM:]
    assert not (loo[:, :, _lib.NNUTSLOO - 1] != 0.0).any().item()
    return (np.median(call), np.median(kern), np.median(skern), np.median(only), np.median(sorts), valid.mean(),
            good.mean(), np.median(bad), np.nanmedian(diff[good]) if good.any() else np.nan,
            np.nanmedian(diff[~good]) if (~good).any() else np.nan)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="10000,100000")
    a = ap.parse_args()
    lines = [f"mdfit_nuts_loo after the NUTS call (500 warmup + 1000 samples): {torch.cuda.get_device_name(0)}, "
             f"medians of {REPS} repetitions after {WARM} warm-up, HIP events on one stream"]
    for T, seed in zip((int(s) for s in a.sizes.split(",")), (1, 3, 5, 7)):
        call, kern, skern, only, sorts, valid, good, bad, rlo, rhi = measure(T, seed)
        lines.append(f"T={T:>7d} seed={seed}: NUTS call {call:9.1f} ms | call + loo {call + kern:9.1f} ms | loo launch "
                     f"{kern:8.2f} ms = {100 * kern / call:6.3f} % of the call (nuts_summary launch on the same draws "
                     f"{skern:8.3f} ms) | the log-likelihood pass alone {only:8.2f} ms = {100 * only / kern:4.1f} % of "
                     f"the launch, the 120 sorts per taxon {sorts - only:8.2f} ms = {100 * (sorts - only) / kern:4.1f} %, "
                     f"the Pareto fits, smoothing and sums {kern - sorts:8.2f} ms = {100 * (kern - sorts) / kern:4.1f} % | "
                     f"taxa valid {100 * valid:.2f} % | without a bad point {100 * good:.1f} % (median bad points "
                     f"{bad:.0f} of 120) | median |n_sigma_loo - n_sigma| there {rlo:.3f}, elsewhere {rhi:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
