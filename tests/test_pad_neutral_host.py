"""CPU test of the pad lane's neutral argument in csrc/mdfit_model.h
(point_accum<true>), on the host build of the unmodified header
(tests/pad_neutral_host_main.cpp through tests/host_shim_lanes, which replays
the row broadcast and the row exchange lane by lane).

A lane that holds no point (lane 15 of a row: y = N = 0) evaluates lg3(y + a),
lg3(N - y + b) and, without null_row, lg3(a), lg3(b) at a fixed argument >= 10
whenever those triples are not read.  On every lane that holds a point, every
accumulator and the returned log-likelihood are the bits of the form that
evaluates the pad at its own a0 = D(1) phi, b0 = (1 - D(1)) phi; and under
null_row the triples broadcast from the pad are still lg3(a0), lg3(b0): the
bits of every lane evaluating lg3(a), lg3(b) itself.

The rows cover a0 < 10 with every real y >= 10 and with some y < 10, b0 < 10,
phi < 10, y = 0 at far positions and arguments all >= 10, in the lnGamma-sum
and the polish phase's value form, for both models and the three ways the
a, b triples are obtained (own calls, the exchange between the rows of an
all-position fit, the pad's broadcast).
"""

from __future__ import annotations

import itertools
import subprocess

import numpy as np
import pytest

from tests import special_cases as sc

ROOT = sc.ROOT
NACC = 17  # 16 accumulators and the returned log-likelihood


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pad_neutral_host") / "pad_neutral_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", f"-I{ROOT / 'tests' / 'host_shim_lanes'}",
                    str(ROOT / "tests" / "pad_neutral_host_main.cpp"), "-o", str(exe)], check=True)
    return exe


# (q, A, c, phi, depth, what)
ROWS = [
    (0.30, 0.10, 0.010, 60.0, 1.0e4, "a0 = 6.6 < 10, every real y >= 10"),
    (0.30, 0.10, 0.005, 60.0, 5.0e2, "a0 < 10, some y < 10"),
    (0.20, 0.50, 0.030, 15.0, 1.0e4, "b0 = 7 < 10, phi >= 10"),
    (0.40, 0.30, 0.010, 5.0, 1.0e4, "phi < 10"),
    (0.40, 0.30, 0.010, 2.0 + 1e-9, 3.0e2, "phi at its lower end"),
    (0.50, 0.30, 0.001, 200.0, 1.0e2, "y = 0 at far positions"),
    (0.35, 0.25, 0.015, 1000.0, 1.0e6, "every argument >= 10"),
    (0.60, 0.40, 0.020, 30.0, 1.0e5, "a0, b0 just above 10"),
]


def cases():
    rng = np.random.default_rng(11)
    out = []
    for (q, A, c, phi, depth, what), pmd, accf in itertools.product(ROWS, (1, 0), (0, 1)):
        k = np.tile(np.arange(16), 2).astype(np.float64)
        D = A * (1.0 - q) ** k + c if pmd else np.full(32, q)
        N = np.rint(depth * rng.uniform(0.85, 1.15, 32))
        y = rng.binomial(N.astype(np.int64), rng.beta(D * phi, (1.0 - D) * phi)).astype(np.float64)
        if "y = 0" in what:
            y[[10, 11, 12, 13, 14, 26, 27, 28, 29, 30]] = 0.0
        if "every real y >= 10" in what:
            y = np.maximum(y, 10.0)
        y[[15, 31]] = N[[15, 31]] = 0.0
        # null_row is the model_null form; whole_pair needs the two rows at the same parameters (they are)
        forms = [(0, 0), (0, 1)] + ([(1, 0), (1, 1)] if not pmd else [])
        for null_row, whole_pair in forms:
            out.append(dict(pmd=pmd, accf=accf, null_row=null_row, whole_pair=whole_pair, q=q, A=A, c=c, phi=phi, y=y, N=N,
                            what=what))
    return out


CASES = cases()


@pytest.fixture(scope="module")
def result(program, tmp_path_factory):
    src = tmp_path_factory.mktemp("pad_neutral_in") / "cases.txt"
    lines = [str(len(CASES))]
    for k in CASES:
        lines.append(f"{k['pmd']} {k['accf']} {k['null_row']} {k['whole_pair']} "
                     + " ".join(float(k[n]).hex() for n in ("q", "A", "c", "phi")))
        lines += [f"{float(a).hex()} {float(b).hex()}" for a, b in zip(k["y"], k["N"])]
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(program), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    rows = [line.split() for line in r.stdout.splitlines()]
    assert len(rows) == 32 * len(CASES)
    got = np.array([[int(t, 16) for t in row[2:]] for row in rows], dtype=np.uint64)
    return got.reshape(len(CASES), 32, 3, NACC)  # case, lane, form (header's, replaced, no broadcast), column


REAL = np.array([lane for lane in range(32) if lane % 16 != 15])


def test_rows_cover_the_cases():
    whats = {k["what"] for k in CASES}
    assert len(whats) == len(ROWS)
    for k in CASES:
        a0 = (k["A"] + k["c"] if k["pmd"] else k["q"]) * k["phi"]
        real_y = k["y"][REAL]
        if "every real y >= 10" in k["what"] and k["pmd"]:
            assert a0 < 10 and real_y.min() >= 10
        if "some y < 10" in k["what"] and k["pmd"]:
            assert a0 < 10 and real_y.min() < 10
        if k["what"].startswith("b0") and k["pmd"]:
            assert (1 - k["A"] - k["c"]) * k["phi"] < 10 <= k["phi"]
    assert any(k["null_row"] for k in CASES) and any(k["whole_pair"] and not k["null_row"] for k in CASES)
    assert any(k["accf"] for k in CASES)


def test_real_lanes_keep_their_bits(result):
    for i, k in enumerate(CASES):
        new, old = result[i, REAL, 0], result[i, REAL, 1]
        bad = np.argwhere(new != old)
        assert bad.size == 0, (k["what"], {n: k[n] for n in ("pmd", "accf", "null_row", "whole_pair")},
                               [(int(REAL[a]), int(b)) for a, b in bad[:5]])
        # a pad adds nothing to any accumulator, in either form
        assert (result[i][[15, 31], 0, :16] == 0).all() and (result[i][[15, 31], 1, :16] == 0).all()
        # the rows do evaluate something: finite, non-zero terms on the real lanes
        v = new[:, :16].view(np.float64)
        assert np.isfinite(v).all() and (v[:, 1] > 0).all()


def test_null_row_broadcasts_the_pads_own_triples(result):
    n = 0
    for i, k in enumerate(CASES):
        if not k["null_row"]:
            continue
        n += 1
        new, own = result[i, REAL, 0], result[i, REAL, 2]
        bad = np.argwhere(new != own)
        assert bad.size == 0, (k["what"], k["accf"], k["whole_pair"], [(int(REAL[a]), int(b)) for a, b in bad[:5]])
    assert n >= 2 * len(ROWS)
