"""Cost of mdfit_nuts_diag beside the NUTS call it follows.

HIP events on one stream around the sampling call (500 warmup, 1000 samples:
the reference's setting) and around the diag launch that follows it, 3
repetitions after 1 warm-up, the median taken; 10k taxa (seed 1) and 100k taxa
(seed 3, config C3).  The plain call's kernels are the ones a run without the
diag pass launches, so its time is the comparison.  Reports what is measured;
there is no pass/fail line.

    python tools/nuts_diag_cost.py [--out profiles/nuts_diag_cost.txt] [--sizes 10000,100000]
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


def measure(T, seed):
    b = generate(T, seed=seed)
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    o = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=500, num_samples=1000)
    res = engine.alloc_outputs(T, opts=o)
    diag = torch.empty((T, _lib.NSUBFIT, _lib.NNUTSDIAG), dtype=torch.float64, device=ty.device)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    call, kern = [], []
    for rep in range(WARM + REPS):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        engine.fit_batch_device(ty, tN, tm, o, res)
        e1.record()
        engine.nuts_diag_device(res, T, o, diag=diag)
        e2.record()
        torch.cuda.synchronize()
        if rep >= WARM:
            call.append(e0.elapsed_time(e1))
            kern.append(e1.elapsed_time(e2))
    d = diag.cpu().numpy()
    valid = d[:, :, 11] == 1.0
    f = _lib.NUTSDIAG_FIELDS.index
    ess = d[:, 0, f("ess_D_max")][valid[:, 0]]
    rhat = d[:, 0, f("rhat_D_max")][valid[:, 0]]
    draws_gb = T * 6 * 1000 * 32 / 1e9
    return np.median(call), np.median(kern), valid.mean(), np.median(ess), np.quantile(rhat, 0.99), draws_gb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="10000,100000")
    a = ap.parse_args()
    lines = [f"mdfit_nuts_diag after the NUTS call (500 warmup + 1000 samples): {torch.cuda.get_device_name(0)}, "
             f"medians of {REPS} repetitions after {WARM} warm-up, HIP events on one stream"]
    for T, seed in zip((int(s) for s in a.sizes.split(",")), (1, 3, 5, 7)):
        call, kern, valid, ess, rhat99, gb = measure(T, seed)
        lines.append(f"T={T:>7d} seed={seed}: NUTS call {call:9.1f} ms | diag launch {kern:8.3f} ms = "
                     f"{100 * kern / call:6.3f} % of the call | {gb:5.2f} GB of draws at {gb / (kern * 1e-3):6.0f} GB/s | "
                     f"rows valid {100 * valid:.2f} % | PMD-all D_max: median ESS {ess:.0f}, 99th-percentile R-hat {rhat99:.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
