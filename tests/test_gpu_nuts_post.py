"""GPU tests of the NUTS post kernel through mdfit_nuts_post:
the kernel of the default inference mode's result columns, alone, on crafted
draws written straight into a workspace (tests/nuts_post_cases.py), against the
reference of tests/nuts_post_ref.py and -- draw for draw -- the oracle's
oracle_nuts_post; and tied to the product launch bit for bit on real chains.

Measured on the MI355X (2026-10-20); every test prints its own:
  draws differing from the oracle's, all 39 cases, per regime class (a draw may
  be in several): boost 0 of 988,382, tiny alpha 0 of 287,296, inversion 0 of
  1,507,733, BTRS at N <= 1e6 0 of 3,771,318, BTRS at N >= 1e8 0 of 354,628, flip
  0 of 223,146, clamped D 0 of 327,700; worst job 0 %
  waic_i against mpmath: worst 0.387 of the bar (constant theta at N ~ 3e5, S = 63);
  above S = 100 against the oracle's: worst 0.229 of 1.5 bars
  n_sigma x3 / asymmetry: worst 0.019 of the bar;  means: worst 0.342 of the bar
  distribution (S = 4096): worst |z| 2.67, least chi-square tail probability
  0.0127 -- the oracle's figures exactly, its draws being the kernel's
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import nuts_post_cases as cases
from tests.test_nuts_post import (CASES, F_DIAG, STRIDE, check_distribution, check_means, check_median_hpdi,
                                  check_n_sigma, check_status_paths, check_waic, draw_shares, same)

pytestmark = pytest.mark.gpu

NPOS, NHALF = 30, 15


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    return torch


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def seeded(torch, group, S, with_pred=True):
    """The crafted workspace of the case with all four chain slots seeded: (res, opts)."""
    from metadamage_amd import _lib
    from tests.test_gpu_nuts_summary import crafted_on_device

    x, status, y, N, _ = cases.case(group, S)
    res, opts = crafted_on_device(torch, np.array(x), status)
    T = x.shape[0]
    res.out[:, _lib.F_DIAG:].view(T, 6, _lib.DIAG_STRIDE)[:, :, 4:] = torch.tensor(cases.diag_slots(status),
                                                                                  device=res.out.device)
    opts.seed = cases.POST_SEED
    if not with_pred:
        res.pred = None
    return res, opts


def host(res, taps):
    waic, counts, flags = taps
    return {"out": res.out.cpu().numpy(), "pred": res.pred.cpu().numpy() if res.pred is not None else None,
            "status": res.status.cpu().numpy(), "waic": waic.cpu().numpy(),
            "counts": counts.cpu().numpy().view(np.uint32), "flags": flags.cpu().numpy()}


def run_post(torch, group, S, poison=False, with_pred=True, with_mm=True):
    """mdfit_nuts_post with both taps on the crafted case -> host arrays; checks
    on the way that the call only reads its inputs."""
    from metadamage_amd import _lib, engine

    x, status, y, N, _ = cases.case(group, S)
    T = x.shape[0]
    ty, tN, tm = engine.to_device_counts(np.array(y), np.array(N), cases.mm_of(group, S) if with_mm else None)
    res, opts = seeded(torch, group, S, with_pred)
    before = [t.clone() for t in (res.workspace, ty, tN)]
    if poison:
        _lib.check(_lib.load().mdfit_poison_lds(_stream(torch)))
    taps = engine.nuts_post_device(ty, tN, res, T, opts, mm=tm, taps=True)
    torch.cuda.synchronize()
    for b, a in zip(before, (res.workspace, ty, tN)):
        assert torch.equal(b, a)
    return host(res, taps)


@pytest.fixture(scope="module")
def crafted(torch_dev):
    """Every crafted case through the kernel once: {(group, S): arrays}, read only."""
    got = {}
    for group, S in CASES:
        got[(group, S)] = run_post(torch_dev, group, S)
        for a in got[(group, S)].values():
            a.setflags(write=False)
    return got


def equal_bits(a, b):
    return all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in a)


# --------------------------------------------------------------------------
# 1. the tapped entry is the product's post kernel
# --------------------------------------------------------------------------
@pytest.mark.parametrize("S", (100, 600, 1030))  # the LDS sort below 513, the register sort, the LDS sort above 1024
def test_entry_equals_the_product_launch_bit_for_bit(torch_dev, S):
    torch = torch_dev
    from metadamage_amd import _lib, engine
    from metadamage_amd.synthetic import generate

    b = generate(16, seed=23)
    T = b.n_taxa
    opts = _lib.default_opts(mode=_lib.MODE_NUTS, num_samples=S, num_warmup=20, seed=9)
    ty, tN, tm = engine.to_device_counts(b.y, b.N, b.mm)
    prod = engine.fit_batch_device(ty, tN, tm, opts=opts)
    torch.cuda.synchronize()
    assert (prod.status.cpu().numpy() == 0).all()
    ws = prod.workspace.clone()

    def again(poison):
        res = engine.FitBatch(torch.zeros_like(prod.out), torch.full_like(prod.pred, -7.0),
                              torch.full_like(prod.status, -7), prod.workspace)
        slots = res.out[:, _lib.F_DIAG:].view(T, 6, _lib.DIAG_STRIDE)
        slots[:, :, 4:] = prod.out[:, _lib.F_DIAG:].view(T, 6, _lib.DIAG_STRIDE)[:, :, 4:]
        if poison:
            _lib.check(_lib.load().mdfit_poison_lds(_stream(torch)))
        taps = engine.nuts_post_device(ty, tN, res, T, opts, mm=tm, taps=True)
        torch.cuda.synchronize()
        return res, taps

    for poison in (False, True):
        res, taps = again(poison)
        assert torch.equal(res.out.view(torch.int64), prod.out.view(torch.int64)), poison
        assert torch.equal(res.pred.view(torch.int32), prod.pred.view(torch.int32)), poison
        assert torch.equal(res.status, prod.status), poison
        assert torch.equal(prod.workspace, ws)  # the call only reads the workspace
        if not poison:
            first = [t.clone() for t in taps]
        else:
            assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, taps))
    waic, counts, flags = (t.cpu().numpy() for t in taps)
    assert (flags == 0).all() and np.isfinite(waic[:, :2]).all()
    assert (counts.view(np.uint32)[:, :NPOS] <= b.N[:, :NPOS, None]).all()
    # without the taps and without pred: the same record
    res = engine.FitBatch(torch.zeros_like(prod.out), None, torch.full_like(prod.status, -7), prod.workspace)
    res.out[:, _lib.F_DIAG:].view(T, 6, 8)[:, :, 4:] = prod.out[:, _lib.F_DIAG:].view(T, 6, 8)[:, :, 4:]
    assert engine.nuts_post_device(ty, tN, res, T, opts, mm=tm) == (None, None, None)
    torch.cuda.synchronize()
    assert torch.equal(res.out.view(torch.int64), prod.out.view(torch.int64)) and torch.equal(res.status, prod.status)
    print(f"S={S}: out, pred and status of mdfit_nuts_post equal the product call's, {T} taxa")


# --------------------------------------------------------------------------
# 2. sort, median and HPDI on the kernel's own counts
# --------------------------------------------------------------------------
@pytest.mark.parametrize("group,S", CASES)
def test_median_hpdi_equal_reference_on_the_tapped_counts(crafted, group, S):
    g = crafted[(group, S)]
    n = check_median_hpdi(group, S, g["out"], g["pred"], g["counts"], g["flags"])
    print(f"{group} S={S}: {n} jobs equal np.median / hpdi of their tapped counts")
    assert n > 0


def test_pad_value_as_a_count_and_tied_windows(crafted):
    """N = 4294967295 with D clamped to 1 draws the sort's pad value itself; N = 1
    and 2 tie almost every window: both are held by the exact comparison above,
    here that the cases do contain them."""
    for S in (3, 100, 513, 1000, 1025):
        g = crafted[("rows", S)]
        t = cases.TAXA["rows"].index("Nmax")
        assert (g["flags"][t] == 0).all() and (g["counts"][t, 31, ::2] == 0xFFFFFFFF).all()
        assert g["counts"][t, 31, 1] < 0xFFFFFFFF and np.isfinite(g["out"][t, 19])
        t = cases.TAXA["rows"].index("N1")
        assert set(np.unique(g["counts"][t, :NPOS])) <= {0, 1} and set(np.unique(g["pred"][t])) <= {0.0, 0.5, 1.0}


# --------------------------------------------------------------------------
# 3. draw parity with the oracle
# --------------------------------------------------------------------------
def test_predictive_draws_equal_the_oracles_up_to_flipped_comparisons(crafted):
    """Tapped counts, kernel against oracle_nuts_post: equal except where a
    last-bit difference of rsqrt, the shared 1 / bb, sincos, flog_t / fexp_t or
    lg3 flips a comparison -- at most 0.5 % of the draws of a regime class, 3 %
    of a job's (S >= 100), none of a job whose D is clamped on every draw.  The
    cases are known not to sit on the sampler's decision boundaries
    (tests/test_nuts_post.py::test_draws_are_insensitive_to_a_last_bit_of_theta)."""
    tot = {c: [0, 0] for c in cases.CLASSES}
    worst_job = (0.0, None)
    for group, S in CASES:
        x, status, y, N, names = cases.case(group, S)
        g, o = crafted[(group, S)], cases.oracle_post(group, S)
        assert np.array_equal(g["flags"], o[5]), (group, S)
        assert np.array_equal(g["status"], o[2]), (group, S)
        per_class, per_job, clamped_all, diff = draw_shares(x, N, g["counts"], o[4], g["flags"], o[5])
        for c, (d, n) in per_class.items():
            tot[c][0] += d
            tot[c][1] += n
        assert (per_job[clamped_all] == 0).all(), (group, S)
        if S >= 100:
            t, j = np.unravel_index(np.argmax(per_job), per_job.shape)
            if per_job[t, j] > worst_job[0]:
                worst_job = (float(per_job[t, j]), (group, S, names[t], int(j)))
            assert per_job.max() <= 0.03, (group, S, names[t], j, per_job[t, j])
    for c, (d, n) in tot.items():
        print(f"{c}: {d} of {n} draws differ from the oracle's ({100.0 * d / max(n, 1):.4f} %)")
    print(f"worst job (S >= 100): {100.0 * worst_job[0]:.3f} % at {worst_job[1]}")
    for c, (d, n) in tot.items():
        assert n > 0 and d <= 0.005 * n, (c, d, n)


# --------------------------------------------------------------------------
# 4. the draws follow the Beta-Binomial (kernel; the oracle's half runs without a GPU)
# --------------------------------------------------------------------------
def test_predictive_counts_follow_the_beta_binomial(crafted):
    check_distribution(lambda group: crafted[(group, 4096)]["counts"], z_max=5.0, label="kernel ")
    check_distribution(lambda group: cases.oracle_post(group, 4096)[4], z_max=4.0, label="oracle ")


# --------------------------------------------------------------------------
# 5. - 7. waic_i, n_sigma / asymmetry, the means
# --------------------------------------------------------------------------
def test_waic_against_mpmath(crafted):
    worst = 0.0
    for group, S in CASES:
        worst = max(worst, check_waic(group, S, crafted[(group, S)]["waic"], label="kernel ",
                                      other=cases.oracle_post(group, S)[3]))
    print(f"waic_i: worst fraction of the bar {worst:.3f}")


def test_grouped_and_per_column_waic_agree_on_identical_likelihoods(crafted):
    """The `same` taxon: each null chain's draws are its PMD partner's with A = 0,
    so D, a, b and every lp are the same doubles.  PMD-all takes waic_cols<2>,
    the null chains waic_cols<MDFIT_WAIC_GROUP>, PMD forward / reverse the
    per-column pass: the same expression and accumulators, so the same bits --
    and every difference 0 makes each n_sigma 0 / 0 = NaN."""
    t = cases.TAXA["paths"].index("same")
    for S in cases.S_VALUES:
        g = crafted[("paths", S)]
        w = g["waic"][t]
        assert np.isfinite(w[0]).all()
        assert same(w[0], w[1]), (S, np.flatnonzero(w[0] != w[1]))  # <2> against <GROUP>
        assert same(w[2], w[4]) and same(w[3], w[5]), S  # per column against <GROUP>
        assert np.isnan(g["out"][t, [1, 15, 18]]).all(), (S, g["out"][t, [1, 15, 18]])
        assert np.isfinite(g["out"][t, 21])  # asymmetry: the forward / reverse chains are other draws


def test_n_sigma_and_asymmetry_on_the_tapped_waic(crafted):
    worst = 0.0
    for group, S in CASES:
        g = crafted[(group, S)]
        worst = max(worst, check_n_sigma(group, S, g["out"], g["waic"], label="kernel "))
    print(f"n_sigma x3, asymmetry: worst fraction of the bar {worst:.3f}")


def test_posterior_means(crafted):
    worst = 0.0
    for group, S in CASES:
        worst = max(worst, check_means(group, S, crafted[(group, S)]["out"], label="kernel "))
    print(f"posterior means: worst fraction of the bar {worst:.3f}")


# --------------------------------------------------------------------------
# 8. status paths, optional inputs, stale LDS
# --------------------------------------------------------------------------
def test_status_paths_with_and_without_pred_and_mm(torch_dev, crafted):
    for group, S in CASES:
        g = crafted[(group, S)]
        check_status_paths(group, S, g["out"], g["pred"], g["status"])
    for group in cases.GROUPS:
        for S in (65, 1000):
            full = crafted[(group, S)]
            g = run_post(torch_dev, group, S, with_pred=False, with_mm=False)
            check_status_paths(group, S, g["out"], None, g["status"], with_mm=False)
            keep = [c for c in range(80) if c not in (22, 23, 24)]
            assert same(g["out"][:, keep], full["out"][:, keep]), (group, S)
            assert g["counts"].tobytes() == full["counts"].tobytes() and same(g["waic"], full["waic"])
            g = run_post(torch_dev, group, S, with_pred=True, with_mm=False)
            assert same(g["pred"], full["pred"]) and g["status"].tobytes() == full["status"].tobytes()
    names = cases.TAXA["paths"]
    g = crafted[("paths", 65)]
    t = names.index("nan")  # the NaN draw sits in the forward chain: its job alone is NaN
    assert g["flags"][t, 30] == 1 and (np.delete(g["flags"][t], 30) == 0).all()
    assert np.isnan(g["out"][t, 16]) and np.isfinite(g["out"][t, [0, 2, 3, 19]]).all()
    assert np.isfinite(g["pred"][t]).all()
    t = names.index("neginf")  # lp = -inf on every draw (null-rev) or some (null-fwd): the reference's NaN
    assert np.isnan(g["waic"][t, 5, NHALF:]).all() and np.isnan(g["waic"][t, 4, :NHALF]).all()
    assert np.isnan(g["out"][t, [15, 18]]).all() and np.isfinite(g["out"][t, [1, 21]]).all()


def test_poisoned_lds_same_bits(torch_dev, crafted):
    for group, S in (("rows", 3), ("series", 65), ("paths", 100), ("rows", 513), ("paths", 1000), ("series", 1025),
                     ("rows", 4096)):
        assert equal_bits(run_post(torch_dev, group, S, poison=True), crafted[(group, S)]), (group, S)


def test_record_does_not_depend_on_the_batch(torch_dev, crafted):
    """One taxon alone (index_base set to its place) gives its row of the batch."""
    from metadamage_amd import engine

    torch = torch_dev
    group, S = "series", 65
    x, status, y, N, names = cases.case(group, S)
    full = crafted[(group, S)]
    mm = cases.mm_of(group, S)
    for t in (0, 3, 7):
        from tests.test_gpu_nuts_summary import crafted_on_device

        res, opts = crafted_on_device(torch, np.array(x[t:t + 1]), status[t:t + 1])
        res.out[:, F_DIAG:].view(1, 6, STRIDE)[:, :, 4:] = torch.tensor(cases.diag_slots(status)[t:t + 1],
                                                                       device=res.out.device)
        opts.seed, opts.index_base = cases.POST_SEED, t
        ty, tN, tm = engine.to_device_counts(np.array(y[t:t + 1]), np.array(N[t:t + 1]), mm[t:t + 1])
        taps = engine.nuts_post_device(ty, tN, res, 1, opts, mm=tm, taps=True)
        torch.cuda.synchronize()
        one = host(res, taps)
        for k in one:
            assert one[k][0].tobytes() == full[k][t].tobytes(), (names[t], k)


def test_argument_checks(torch_dev):
    from metadamage_amd import _lib, engine

    torch = torch_dev
    res, opts = seeded(torch, "rows", 3)
    x, status, y, N, _ = cases.case("rows", 3)
    ty, tN, _ = engine.to_device_counts(np.array(y), np.array(N))
    bad = _lib.default_opts(mode=_lib.MODE_NUTS, num_samples=1)
    with pytest.raises(Exception):
        engine.nuts_post_device(ty, tN, res, 8, bad)
    with pytest.raises(Exception):
        engine.nuts_post_device(ty, tN, res, 8, _lib.default_opts())  # MODE_MAP
    with pytest.raises(ValueError):
        engine.nuts_post_device(ty, tN, res, 8, opts, taps=True, waic=torch.empty(3, device="cuda"))
    assert engine.nuts_post_device(ty, tN, res, 0, opts) == (None, None, None)
