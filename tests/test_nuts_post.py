"""CPU tests of the oracle's record assembly (oracle_nuts_post, the post part of
nuts_taxon) on the crafted cases of tests/nuts_post_cases.py against the
reference of tests/nuts_post_ref.py, and the checkers that
tests/test_gpu_nuts_post.py applies to the kernel's results.

  * median / HPDI: bit-equal to np.median and numpyro's hpdi on the tapped counts;
  * waic_i: within half the derived bar of the mpmath fixture
    (tests/golden/nuts_post_waic.npz) -- the oracle's libm lgamma against the
    bar of the device's fast lnGamma contract;
  * n_sigma x3 and asymmetry: the longdouble formulas on the tapped waic_i;
  * posterior means against longdouble; the status paths;
  * oracle_nuts_batch(keep_samples) = oracle_nuts_post on those samples, bit for bit;
  * the crafted draws do not sit on decision boundaries of the predictive
    sampler (the sensitivity check behind the GPU draw-parity test);
  * the predictive counts follow the Beta-Binomial (chi-square / exact moments).
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

from tests import nuts_post_cases as cases
from tests import nuts_post_ref as ref
from tests.helpers import GOLDEN

NPOS, NHALF = 30, 15
F = {"D_max": 0, "n_sigma": 1, "lo": 2, "hi": 3, "q_mean": 4, "concentration_mean": 5, "D_max_marginalized_mean": 6,
     "n_sigma_forward": 15, "D_max_forward": 16, "q_mean_forward": 17, "n_sigma_reverse": 18, "D_max_reverse": 19,
     "q_mean_reverse": 20, "asymmetry": 21, "noise": 22}
NRESULT, F_DIAG, STRIDE = 25, 32, 8
CASES = [(g, S) for g in cases.GROUPS for S in cases.S_VALUES]


def same(a, b):
    """Equal bit for bit, any NaN equal to any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


@functools.lru_cache(maxsize=None)
def fixture():
    return np.load(GOLDEN / "nuts_post_waic.npz")


def runs_post(status, y, N):
    """ok[T]: the taxa whose record is assembled (no y > N, every chain OK)."""
    return (status == 0).all(axis=1) & ~(y[:, :NPOS] > N[:, :NPOS]).any(axis=1)


# ---------------------------------------------------------------------------
# checkers (the GPU tests apply them to the kernel's results)
# ---------------------------------------------------------------------------
def check_median_hpdi(group, S, out, pred, counts, flags):
    """out's D_max columns and pred equal the reference on the tapped counts, exactly."""
    x, status, y, N, names = cases.case(group, S)
    ok = runs_post(status, y, N)
    n_jobs = 0
    for t in range(x.shape[0]):
        if not ok[t]:
            assert (flags[t] == 255).all() and (counts[t] == ref.NO_COUNT).all(), names[t]
            assert np.isnan(out[t, :NRESULT]).all() and (pred is None or np.isnan(pred[t]).all()), names[t]
            continue
        for j in range(32):
            col = cases.JOB_COL[j]
            n = int(N[t, col])
            assert flags[t, j] == (2 if n == 0 else flags[t, j]) and flags[t, j] in (0, 1, 2), (names[t], j)
            if flags[t, j] == 0:
                assert (counts[t, j] <= n).all(), (names[t], j)
            else:
                assert flags[t, j] == 1 or (counts[t, j] == ref.NO_COUNT).all(), (names[t], j)
            want = ref.median_hpdi(counts[t, j], n, valid=flags[t, j] == 0)
            if j < NPOS:
                if pred is not None:
                    assert same(pred[t, :, j], want.astype(np.float32)), (names[t], j, pred[t, :, j], want)
                if j == 0:
                    assert same(out[t, [F["D_max"], F["lo"], F["hi"]]], want), (names[t], out[t, :4], want)
            else:
                assert same(out[t, F["D_max_forward"] if j == NPOS else F["D_max_reverse"]], want[0]), (names[t], j)
            n_jobs += 1
    return n_jobs


def check_waic(group, S, waic, share=1.0, label="", other=None):
    """waic[T, 6, 30] against the reference: at S <= 130 within share x the bar
    of the mpmath fixture, the value class (finite / NaN) everywhere; NaN where
    the kernel forms none.  Above S = 130 there is no mpmath value: `other`, the
    oracle's waic_i (within half the bar of mpmath wherever that is known), must
    then be within 1.5 bars, the bar's magnitudes from the float64 log-likelihoods.
    Returns the worst fraction of the bar (of 1.5 bars above S = 130)."""
    x, status, y, N, names = cases.case(group, S)
    ok = runs_post(status, y, N)
    assert np.isnan(waic[~ok]).all()
    for k in range(6):
        outside = [c for c in range(NPOS) if c not in ref.points_of(k)]
        assert np.isnan(waic[:, k, outside]).all(), k
    worst, where = 0.0, None
    if S in cases.S_MPMATH:
        fx = fixture()
        assert str(fx[f"{group}/{S}/hash"]) == cases.case_hash(group, S), \
            "tests/golden/nuts_post_waic.npz was made from other inputs: rerun tests/golden/make_golden_nuts_post.py"
        want, mag = fx[f"{group}/{S}/waic"], fx[f"{group}/{S}/mag"]
    else:
        want, mag = cases.waic64(group, S)
        if other is None:
            mag = None
    for t in np.flatnonzero(ok):
        for k in range(6):
            for col in ref.points_of(k):
                w, g = want[t, k, col], waic[t, k, col]
                if not np.isfinite(w):
                    assert not np.isfinite(g), (names[t], k, col, g)  # the reference's class: NaN / inf
                    continue
                assert np.isfinite(g), (names[t], k, col, g, w)
                if mag is None:
                    continue
                bar = ref.waic_bar(S, *mag[t, k, col])
                if S not in cases.S_MPMATH:
                    w, bar = other[t, k, col], 1.5 * bar
                frac = abs(g - w) / bar
                if frac > worst:
                    worst, where = frac, (names[t], k, col, g, w, bar)
    print(f"{label}waic {group} S={S}: worst fraction of the bar {worst:.3f} at {where}")
    assert worst <= share, where
    return worst


def check_n_sigma(group, S, out, waic, label=""):
    """n_sigma x3 and asymmetry of out against the longdouble formulas on the
    tapped waic: within 64 eps kappa; 0 / 0 is NaN on both sides."""
    x, status, y, N, names = cases.case(group, S)
    worst = 0.0
    cols = [F["n_sigma"], F["n_sigma_forward"], F["n_sigma_reverse"], F["asymmetry"]]
    for t in np.flatnonzero(runs_post(status, y, N)):
        for c, (val, bar) in zip(cols, ref.n_sigma_block(waic[t])):
            got = out[t, c]
            if not np.isfinite(val):
                assert np.isnan(got) if np.isnan(val) else got == val, (names[t], c, got, val)
                continue
            frac = float(abs(got - val) / bar)
            worst = max(worst, frac)
            assert frac <= 1.0, (names[t], c, got, float(val), float(bar))
    print(f"{label}n_sigma {group} S={S}: worst fraction of the bar {worst:.3f}")
    return worst


def check_means(group, S, out, label="", serial=False):
    """The posterior means of out (diag slots 0..3 and the five result columns)
    against longdouble, within (ceil(S / 64) + 6) eps mean|x| (serial: the
    oracle's one running sum, (S + 2) eps mean|x|)."""
    x, status, y, N, names = cases.case(group, S)
    m, ma, dmm, dmm_abs = ref.means(x)
    worst = 0.0
    invalid = (y[:, :NPOS] > N[:, :NPOS]).any(axis=1)
    ok = runs_post(status, y, N)

    def one(got, want, mabs, what):
        nonlocal worst
        if np.isnan(want):
            assert np.isnan(got), what
            return
        bar = ref.mean_bar(S, mabs, serial)
        err = abs(np.longdouble(got) - want)
        assert err <= bar, (what, got, float(want), float(bar))
        if bar > 0:
            worst = max(worst, float(err / bar))

    for t in range(x.shape[0]):
        if invalid[t]:
            continue
        for k in range(6):  # kept for a failed chain too
            for j in range(4):
                one(out[t, F_DIAG + STRIDE * k + j], m[t, k, j], ma[t, k, j], (names[t], k, j))
        if ok[t]:
            one(out[t, F["q_mean"]], m[t, 0, 0], ma[t, 0, 0], (names[t], "q_mean"))
            one(out[t, F["concentration_mean"]], m[t, 0, 3], ma[t, 0, 3], (names[t], "concentration_mean"))
            one(out[t, F["D_max_marginalized_mean"]], dmm[t], dmm_abs[t], (names[t], "D_max_marginalized_mean"))
            one(out[t, F["q_mean_forward"]], m[t, 2, 0], ma[t, 2, 0], (names[t], "q_mean_forward"))
            one(out[t, F["q_mean_reverse"]], m[t, 3, 0], ma[t, 3, 0], (names[t], "q_mean_reverse"))
    print(f"{label}means {group} S={S}: worst fraction of the bar {worst:.3f}")
    return worst


def check_status_paths(group, S, out, pred, st, with_mm=True):
    """Status, the NaN pattern of a failed chain and of y > N, the kept diag
    slots, the sums, and the noise columns with and without mm."""
    x, status, y, N, names = cases.case(group, S)
    diag = cases.diag_slots(status)
    invalid = (y[:, :NPOS] > N[:, :NPOS]).any(axis=1)
    for t in range(x.shape[0]):
        if invalid[t]:
            assert st[t] == 3 and np.isnan(out[t]).all(), names[t]
            assert pred is None or np.isnan(pred[t]).all()
            continue
        assert st[t] == int(status[t].max()), names[t]
        slots = out[t, F_DIAG:].reshape(6, STRIDE)
        assert np.array_equal(slots[:, 4:], diag[t]), names[t]  # the chains' slots pass through
        if status[t].max() != 0:
            assert np.isnan(out[t, :NRESULT]).all() and (out[t, NRESULT:F_DIAG] == 0).all(), names[t]
            assert pred is None or np.isnan(pred[t]).all()
            assert np.isfinite(slots[:, :4]).all(), names[t]  # the diag means are kept
            continue
        Nf, yf = N[t, :NPOS].astype(float), y[t, :NPOS].astype(float)
        assert out[t, 7] == Nf[0] and out[t, 8] == Nf[NHALF]
        assert out[t, 9] == Nf[:NHALF].sum() and out[t, 10] == Nf[NHALF:].sum() and out[t, 11] == Nf.sum()
        assert out[t, 12] == yf[:NHALF].sum() and out[t, 13] == yf[NHALF:].sum() and out[t, 14] == yf.sum()
        noise = out[t, F["noise"]:F["noise"] + 3]
        assert np.isfinite(noise).all() if with_mm else np.isnan(noise).all(), (names[t], noise)
        if pred is not None:  # N = 0 columns are NaN, and no others unless a draw is NaN
            assert np.isnan(pred[t][:, Nf == 0]).all(), names[t]


def draw_shares(x, N, a, b, fa, fb):
    """Per regime class and per job the share of predictive draws whose tapped
    counts a, b [T, 32, S] differ, over the jobs both sides ran (flags 0 or 1)."""
    cls = cases.draw_classes(x, N)
    ran = ((fa <= 1) & (fb <= 1))[:, :, None]
    diff = (a != b) & ran
    per_class = {}
    for i, name in enumerate(cases.CLASSES):
        n = int((cls[..., i] & ran).sum())
        per_class[name] = (int((diff & cls[..., i]).sum()), n)
    per_job = diff.mean(axis=2)
    clamped_all = cls[..., 6].all(axis=2) & ran[..., 0]
    return per_class, per_job, clamped_all, diff


# ---------------------------------------------------------------------------
# the oracle against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("group,S", CASES)
def test_oracle_median_hpdi_equal_reference_on_its_counts(oracle_lib, group, S):
    out, pred, st, waic, counts, flags = cases.oracle_post(group, S)
    assert check_median_hpdi(group, S, out, pred, counts, flags) > 0


@pytest.mark.parametrize("group,S", CASES)
def test_oracle_waic_n_sigma_means_and_status(oracle_lib, group, S):
    out, pred, st, waic, counts, flags = cases.oracle_post(group, S)
    check_waic(group, S, waic, share=0.5, label="oracle ")
    check_n_sigma(group, S, out, waic, label="oracle ")
    check_means(group, S, out, label="oracle ", serial=True)
    check_status_paths(group, S, out, pred, st)


def test_oracle_without_mm_and_the_special_values(oracle_lib):
    S = 65
    for group in cases.GROUPS:
        x, status, y, N, names = cases.case(group, S)
        out, pred, st = oracle_lib.nuts_post(y, N, x, diag=cases.diag_slots(status), seed=cases.POST_SEED)
        check_status_paths(group, S, out, pred, st, with_mm=False)
        full = cases.oracle_post(group, S)
        assert same(np.delete(out, [22, 23, 24], axis=1), np.delete(full[0], [22, 23, 24], axis=1))
    out, pred, st, waic, counts, flags = cases.oracle_post("paths", S)
    names = cases.TAXA["paths"]
    t = names.index("same")  # identical likelihoods: every difference 0, n_sigma 0 / 0
    assert same(waic[t, 0], waic[t, 1]) and same(waic[t, 2], waic[t, 4]) and same(waic[t, 3], waic[t, 5])
    assert np.isnan(out[t, [1, 15, 18]]).all()
    t = names.index("nan")  # the NaN draw is in the forward chain: its job alone
    assert flags[t, 30] == 1 and (flags[t, :30] == 0).all() and flags[t, 31] == 0
    assert np.isnan(out[t, 16]) and np.isfinite(out[t, [0, 2, 3, 19]]).all() and np.isfinite(pred[t]).all()
    t = names.index("neginf")
    assert np.isnan(waic[t, 5, NHALF:]).all() and np.isnan(waic[t, 4, :NHALF]).all() and np.isnan(out[t, [15, 18]]).all()
    assert np.isfinite(out[t, [1, 21]]).all()
    out, pred, st, waic, counts, flags = cases.oracle_post("series", S)
    names = cases.TAXA["series"]
    t = names.index("zeroD")
    assert (counts[t] == 0).all()
    t = names.index("clampD")  # D = 1 at column 0 of every PMD chain: all N
    x, status, y, N, _ = cases.case("series", S)
    for j in (0, 30, 31):
        assert (counts[t, j] == N[t, 0]).all()
    out, pred, st, waic, counts, flags = cases.oracle_post("rows", S)
    t = cases.TAXA["rows"].index("Nmax")
    # the sort's pad value as a count: every other draw of job 31, and none of them marks a bad draw
    assert (flags[t] == 0).all() and (counts[t, 31, ::2] == ref.NO_COUNT).all() and counts[t, 31, 1] < ref.NO_COUNT
    assert out[t, 19] > 0.6 and np.isfinite(out[t, :4]).all()


def test_batch_with_kept_samples_equals_post_on_them(oracle_lib):
    from metadamage_amd.synthetic import generate

    b = generate(4, seed=11)
    S = 30
    out, pred, st, smp = oracle_lib.nuts_batch(b.y, b.N, b.mm, seed=5, num_warmup=20, num_samples=S, index_base=7,
                                               keep_samples=True)
    diag = out[:, F_DIAG:].reshape(-1, 6, STRIDE)[:, :, 4:]
    out2, pred2, st2 = oracle_lib.nuts_post(b.y, b.N, smp, diag=diag, mm=b.mm, seed=5, index_base=7)
    assert out.tobytes() == out2.tobytes() and pred.tobytes() == pred2.tobytes() and st.tobytes() == st2.tobytes()


# ---------------------------------------------------------------------------
# the crafted draws do not sit on decision boundaries
# ---------------------------------------------------------------------------
SENS_S = (100, 1000)


@pytest.mark.parametrize("S", SENS_S)
def test_draws_are_insensitive_to_a_last_bit_of_theta(oracle_lib, S):
    """The oracle at theta and at theta (1 +- 2^-50) differs in under 0.1 % of
    the draws of each regime class: a kernel whose expressions differ in the
    last bits has no excuse on these cases beyond the caps of the GPU test."""
    tot = {c: [0, 0] for c in cases.CLASSES}
    for group in cases.GROUPS:
        x, status, y, N, names = cases.case(group, S)
        base = cases.oracle_post(group, S)
        for sign in (1.0, -1.0):
            xp = x * (1.0 + sign * 2.0 ** -50)
            got = oracle_lib.nuts_post(y, N, xp, diag=cases.diag_slots(status), seed=cases.POST_SEED, taps=True)
            per_class, per_job, clamped_all, _ = draw_shares(x, N, base[4], got[4], base[5], got[5])
            for c, (d, n) in per_class.items():
                tot[c][0] += d
                tot[c][1] += n
            assert (per_job[clamped_all] == 0).all()
    for c, (d, n) in tot.items():
        print(f"S={S} {c}: {d} of {n} draws differ ({100.0 * d / max(n, 1):.4f} %)")
        assert n > 0 and d <= 0.001 * n, (c, d, n)


# ---------------------------------------------------------------------------
# the predictive counts follow the Beta-Binomial
# ---------------------------------------------------------------------------
DIST_TAXA = (("series", "const"), ("paths", "constbig"))


def check_distribution(counts_of, z_max, label=""):
    """The constant-theta taxa at S = 4096: per job the tapped counts against
    BetaBinomial(N, D phi, (1 - D) phi) -- chi-square at N <= 40 (tail
    probability >= 1e-6), else the mean and the variance against the exact
    moments (|z| <= z_max).  counts_of(group) -> counts[T, 32, S]."""
    S = 4096
    worst_z, worst_p = 0.0, 1.0
    for group, name in DIST_TAXA:
        x, status, y, N, names = cases.case(group, S)
        t = names.index(name)
        counts = counts_of(group)
        for j in range(32):
            th = x[t, cases.JOB_CHAIN[j], 0]
            col = cases.JOB_COL[j]
            D = float(ref.d_of(th[None, :], True, col)[0])
            a, b, n = D * th[3], (1.0 - D) * th[3], int(N[t, col])
            c = counts[t, j]
            assert (c <= n).all()
            if n <= 40:
                p, bins = ref.chi_square_tail(c, n, a, b)
                worst_p = min(worst_p, p)
                assert p >= 1e-6, (name, j, n, p, bins)
            else:
                zm, zv = ref.moment_z(c, n, a, b)
                worst_z = max(worst_z, abs(zm), abs(zv))
                assert abs(zm) <= z_max and abs(zv) <= z_max, (name, j, n, zm, zv)
    print(f"{label}distribution: worst |z| {worst_z:.2f}, least chi-square tail probability {worst_p:.3g}")
    return worst_z, worst_p


def test_oracle_predictive_counts_follow_the_beta_binomial(oracle_lib):
    check_distribution(lambda group: cases.oracle_post(group, 4096)[4], z_max=4.0, label="oracle ")


def test_reference_pieces():
    """The reference's own parts on known answers."""
    c = np.array([0, 0, 1, 1, 1, 0, 1, 0, 0, 1], np.uint32)  # N = 1: the first of the tied windows
    m3 = ref.median_hpdi(c, 1)
    assert m3.tolist() == [0.5, 0.0, 1.0]
    assert ref.median_hpdi(np.array([5, 5, 5], np.uint32), 10).tolist() == [0.5, 0.5, 0.5]
    assert np.isnan(ref.median_hpdi(c, 0)).all() and np.isnan(ref.median_hpdi(c, 1, valid=False)).all()
    from scipy import stats

    m1, mu2, mu4 = ref.betabinom_central_moments(30, 2.5, 7.0)
    k = np.arange(31)
    pmf = stats.betabinom.pmf(k, 30, 2.5, 7.0)
    mean = (k * pmf).sum()
    assert abs(m1 - mean) < 1e-10 and abs(mu2 - ((k - mean) ** 2 * pmf).sum()) < 1e-9
    assert abs(mu4 - ((k - mean) ** 4 * pmf).sum()) < 1e-6 * mu4
    lp = np.array([-3.0, -2.5, -4.0])
    from oracle import oracle as orc

    assert abs(ref.waic_two_pass(lp) - orc.lppd_and_waic(lp[:, None])["waic_i"][0]) < 1e-14
    w = np.random.default_rng(3).normal(50, 5, (6, NPOS))
    (ns, _), (nf, _), (nr, _), (asy, _) = ref.n_sigma_block(w)
    d = lambda a: {"waic_i": a, "waic": a.sum()}  # noqa: E731
    assert abs(float(ns) - orc.n_sigma(d(w[0]), d(w[1]))) < 1e-12
    assert abs(float(nf) - orc.n_sigma(d(w[2, :NHALF]), d(w[4, :NHALF]))) < 1e-12
    assert abs(float(nr) - orc.n_sigma(d(w[3, NHALF:]), d(w[5, NHALF:]))) < 1e-12
    assert abs(float(asy) - orc.asymmetry(d(w[0]), d(w[2, :NHALF]), d(w[3, NHALF:]))) < 1e-12
