"""Cost of mdfit_nuts_summary beside the NUTS call it follows.

HIP events on one stream around the sampling call (500 warmup, 1000 samples:
the reference's setting), around the summary launch that follows it and, for
comparison, around a mdfit_nuts_diag launch on the same workspace; 3
repetitions after 1 warm-up, the median taken; 10k taxa (seed 1) and 100k taxa
(seed 3, config C3).  The plain call's kernels are the ones a run without the
summary pass launches, so its time is the comparison.

The kernel's two phases are separated without another kernel: with one NaN
written into every row's first draw the launch does its whole pass over the
draws, finds the row not finite and returns before any sort, so that launch is
the pass alone and the rest of the full launch is the three sorts and the window
searches.  Reports what is measured; there is no pass/fail line.

    python tools/nuts_summary_cost.py [--out profiles/nuts_summary_cost.txt] [--sizes 10000,100000]
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
    summ = torch.empty((T, _lib.NSUBFIT, _lib.NNUTSSUMM), dtype=torch.float64, device=ty.device)
    diag = torch.empty((T, _lib.NSUBFIT, _lib.NNUTSDIAG), dtype=torch.float64, device=ty.device)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    call, kern, dkern = [], [], []
    for rep in range(WARM + REPS):
        e0, e1, e2, e3 = ev(), ev(), ev(), ev()
        e0.record()
        engine.fit_batch_device(ty, tN, tm, o, res)
        e1.record()
        engine.nuts_summary_device(res, T, o, summ=summ)
        e2.record()
        engine.nuts_diag_device(res, T, o, diag=diag)
        e3.record()
        torch.cuda.synchronize()
        if rep >= WARM:
            call.append(e0.elapsed_time(e1))
            kern.append(e1.elapsed_time(e2))
            dkern.append(e2.elapsed_time(e3))
    s = summ.cpu().numpy()
    valid = s[:, :, _lib.NNUTSSUMM - 1] == 1.0
    f = _lib.NUTSSUMM_FIELDS.index
    sig = s[:, 0, f("significance")][valid[:, 0]]
    width = (s[:, 0, f("D_max_hi")] - s[:, 0, f("D_max_lo")])[valid[:, 0]]
    # the pass alone: every row not finite, so no row reaches its sorts
    engine.samples_view(res, T, o)[:, :, 0, 0] = float("nan")
    torch.cuda.synchronize()
    only = [_timed(lambda: engine.nuts_summary_device(res, T, o, summ=summ)) for _ in range(WARM + REPS)][WARM:]
    assert not (summ[:, :, _lib.NNUTSSUMM - 1] != 0.0).any().item()
    draws_gb = T * 6 * 1000 * 32 / 1e9
    return (np.median(call), np.median(kern), np.median(dkern), np.median(only), valid.mean(), np.median(sig),
            np.median(width), draws_gb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="10000,100000")
    a = ap.parse_args()
    lines = [f"mdfit_nuts_summary after the NUTS call (500 warmup + 1000 samples): {torch.cuda.get_device_name(0)}, "
             f"medians of {REPS} repetitions after {WARM} warm-up, HIP events on one stream"]
    for T, seed in zip((int(s) for s in a.sizes.split(",")), (1, 3, 5, 7)):
        call, kern, dkern, only, valid, sig, width, gb = measure(T, seed)
        lines.append(f"T={T:>7d} seed={seed}: NUTS call {call:9.1f} ms | call + summary {call + kern:9.1f} ms | summary launch "
                     f"{kern:8.3f} ms = {100 * kern / call:6.3f} % of the call (nuts_diag launch on the same draws "
                     f"{dkern:8.3f} ms) | the pass over {gb:5.2f} GB of draws alone {only:8.3f} ms = "
                     f"{gb / (only * 1e-3):6.0f} GB/s, the three sorts and window searches the other "
                     f"{kern - only:8.3f} ms = {100 * (kern - only) / kern:4.1f} % of the launch | rows valid "
                     f"{100 * valid:.2f} % | PMD-all: median significance {sig:.2f}, median 68 % HPDI width of D_max "
                     f"{width:.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
