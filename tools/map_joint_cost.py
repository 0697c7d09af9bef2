"""Cost of the fused mdfit_map_joint(_adapt) launch beside the three launches it
replaces, mdfit_map_waic, mdfit_map_evidence and mdfit_map_psis (and their
_adapt forms).

HIP events on one stream around each launch alone, the four kernels alternated
in one session and one process, 5 warm repetitions each after 2 warm-ups, the
range (min .. max) taken: 10k taxa (seed 1) and 125k taxa (seed 3), S = 256 and
1024, without rounds and with three.  `sum` is, repetition by repetition, the
three separate launches' times added.  There is no pass bar.

    python tools/map_joint_cost.py [--out profiles/map_joint_cost.txt] [--quick]
"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from metadamage_amd import _lib, engine  # noqa: E402
from metadamage_amd.synthetic import generate  # noqa: E402

WARM, REPS = 2, 5
DRAWS = (256, 1024)
ROUNDS = (0, 3)


def fitted(T, seed):
    b = generate(T, seed=seed)
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    o = _lib.default_opts(mode=_lib.MODE_MAP)
    res = engine.alloc_outputs(T, opts=o)
    engine.fit_batch_device(ty, tN, tm, o, res)
    torch.cuda.synchronize()
    return ty, tN, res


def timings(T, seed, reps, warm):
    """{(S, R): {"joint" | "waic" | "evid" | "psis": [ms per repetition]}}"""
    ty, tN, res = fitted(T, seed)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=ty.device)  # noqa: E731
    waic, evid, psis = f64(T, _lib.NWAICROW, _lib.NMAPWAIC), f64(T, _lib.NEVIDROW, _lib.NMAPEVID), f64(T, 3, _lib.NMAPPSIS)
    adapt = f64(T, 3, _lib.NMAPADAPT)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    t = {(S, R): {k: [] for k in ("joint", "waic", "evid", "psis")} for S in DRAWS for R in ROUNDS}
    for rep in range(warm + reps):
        for S in DRAWS:
            for R in ROUNDS:
                kw = {"adapt_rounds": R, "adapt": adapt} if R else {}
                e = [ev() for _ in range(5)]
                e[0].record()
                engine.map_joint_device(ty, tN, res, S, 0, 0, waic=waic, evid=evid, psis=psis, **kw)
                e[1].record()
                engine.map_waic_device(ty, tN, res, S, 0, 0, waic=waic, **kw)
                e[2].record()
                engine.map_evidence_device(ty, tN, res, S, 0, 0, evid=evid, **kw)
                e[3].record()
                engine.map_psis_device(ty, tN, res, S, 0, 0, psis=psis, **kw)
                e[4].record()
                torch.cuda.synchronize()
                if rep >= warm:
                    for j, k in enumerate(("joint", "waic", "evid", "psis")):
                        t[(S, R)][k].append(e[j].elapsed_time(e[j + 1]))
    return t


def rng(v):
    return f"{min(v):9.2f} .. {max(v):9.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="1,000 and 2,000 taxa, 2 repetitions: a rehearsal")
    a = ap.parse_args()
    reps, warm = (2, 1) if a.quick else (REPS, WARM)
    lines = [f"mdfit_map_joint(_adapt) beside mdfit_map_waic, mdfit_map_evidence and mdfit_map_psis (_adapt): "
             f"{torch.cuda.get_device_name(0)}, launches alone, alternated in one session and process, ranges (min .. "
             f"max, ms) of {reps} warm repetitions after {warm} warm-ups, HIP events on one stream; sum = waic + evidence "
             "+ psis of the same repetition"]
    for T, seed in (((1_000, 1), (2_000, 3)) if a.quick else ((10_000, 1), (125_000, 3))):
        t = timings(T, seed, reps, warm)
        lines.append(f"T={T:>7d} seed={seed}:")
        for S in DRAWS:
            for R in ROUNDS:
                d = t[(S, R)]
                total = [w + e + p for w, e, p in zip(d["waic"], d["evid"], d["psis"])]
                rw = [j / w for j, w in zip(d["joint"], d["waic"])]
                rs = [j / s for j, s in zip(d["joint"], total)]
                below = max(d["joint"]) < min(total)
                lines.append(f"    S={S:>4d} R={R}: joint {rng(d['joint'])} | waic {rng(d['waic'])} | evidence "
                             f"{rng(d['evid'])} | psis {rng(d['psis'])} | sum {rng(total)} | joint / waic "
                             f"{min(rw):.3f} .. {max(rw):.3f} | joint / sum {min(rs):.3f} .. {max(rs):.3f} | every joint "
                             f"run below every sum: {'yes' if below else 'no'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
