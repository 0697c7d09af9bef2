"""Cost of the auto inference (engine.fit_auto_device) beside
the plain NUTS call on the same taxa, and how far its importance-sampled columns
sit from the sampler's on the taxa it does not sample.

10k synthetic taxa (seed 1), the reference's 500 + 1000, S = 256.  HIP events on
one stream: the stages of the auto call (its `timings`), the whole auto call and
the plain NUTS call, the median of REPS repetitions after one warm-up each.
Then, over the taxa the auto call settled without the sampler, the nine composed
columns against the plain NUTS call (seed 0), beside the difference between two
NUTS seeds (0 and 1) on the same taxa.  There is no pass bar.

    python tools/auto_cost.py [--out profiles/auto_cost.txt] [--taxa 10000]
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

REPS = 3
S = 256


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--taxa", type=int, default=10_000)
    a = ap.parse_args()
    T = a.taxa
    b = generate(T, seed=1)
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    opts = _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=500, num_samples=1000, seed=0)
    lines = [f"auto inference beside the plain NUTS call: {torch.cuda.get_device_name(0)}, T = {T} (seed 1), "
             f"500 + 1000, S = {S}; medians of {REPS} repetitions after one warm-up, HIP events on one stream"]
    # the plain NUTS call (its buffers allocated once)
    rn = engine.alloc_outputs(T, opts=opts)
    nuts_ms = [timed(lambda: engine.fit_batch_device(ty, tN, tm, opts, rn))[0] for _ in range(REPS + 1)][1:]
    nuts_out = rn.out[:, :_lib.NRESULT].cpu().numpy()
    # the auto call: whole, and by stage
    whole, stages = [], []
    for rep in range(REPS + 1):
        ms, (res, route, auto) = timed(lambda: engine.fit_auto_device(ty, tN, tm, opts, S))
        tm_ = {}
        engine.fit_auto_device(ty, tN, tm, opts, S, timings=tm_)
        if rep:
            whole.append(ms)
            stages.append(tm_)
    route = route.cpu().numpy()
    auto_out = res.out[:, :_lib.NRESULT].cpu().numpy()
    sampled = (route & _lib.ROUTE_SAMPLE) != 0
    n_s = int(sampled.sum())
    lines.append(f"taxa sampled: {n_s} of {T} = {100 * n_s / T:.1f} %; routes "
                 + ", ".join(f"{r}: {int((route == r).sum())}" for r in range(9) if (route == r).any())
                 + f"; sampler sub-chunks {stages[-1]['n_sub_chunks']}")
    med = {k: float(np.median([s[k] for s in stages])) for k in engine.AUTO_STAGES}
    lines.append("stages (ms): " + " | ".join(f"{k} {med[k]:.2f}" for k in engine.AUTO_STAGES)
                 + f" | sum {sum(med.values()):.2f}   (gather: from the route to the sampler's launch -- the host "
                 "synchronisation, nonzero, the auto block and the row gather)")
    w, n = float(np.median(whole)), float(np.median(nuts_ms))
    lines.append(f"whole auto call {w:.1f} ms (min {min(whole):.1f}, max {max(whole):.1f}) | plain NUTS call {n:.1f} ms "
                 f"(min {min(nuts_ms):.1f}, max {max(nuts_ms):.1f}) | auto / NUTS {w / n:.3f} | sampler stage per "
                 f"sampled taxon {1e3 * med['sampler'] / max(n_s, 1):.1f} us, NUTS call per taxon {1e3 * n / T:.1f} us")
    # sampled rows are the plain call's
    same = np.array_equal(auto_out[sampled].view(np.int64), nuts_out[sampled].view(np.int64))
    lines.append(f"sampled rows equal the plain NUTS call's bit for bit: {same}")
    # agreement on the settled taxa, beside the seed-to-seed spread of the sampler
    o1 = _lib.MdfitOpts.from_buffer_copy(opts)
    o1.seed = 1
    engine.fit_batch_device(ty, tN, tm, o1, rn)
    torch.cuda.synchronize()
    nuts1 = rn.out[:, :_lib.NRESULT].cpu().numpy()
    ok = (~sampled) & (route == 0)
    lines.append(f"the nine composed columns over the {int(ok.sum())} settled taxa: |auto - NUTS(seed 0)| beside "
                 "|NUTS(seed 1) - NUTS(seed 0)|, median / 90 % / 99 % / max")
    q = lambda d: " / ".join(f"{v:.3g}" for v in (*np.nanquantile(d, [0.5, 0.9, 0.99]), np.nanmax(d)))  # noqa: E731
    for name in _lib.AUTO_COMPOSED_FIELDS:
        c = _lib.RESULT_FIELDS.index(name)
        da, ds = np.abs(auto_out[ok, c] - nuts_out[ok, c]), np.abs(nuts1[ok, c] - nuts_out[ok, c])
        lines.append(f"    {name:<24s} auto {q(da):<36s} | seeds {q(ds)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
