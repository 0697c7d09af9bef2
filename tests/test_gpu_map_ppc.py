"""GPU tests of mdfit_map_ppc and mdfit_map_ppc_adapt (MDFIT-PPC v1, DESIGN.md
§3.16): khat, ess, n_distinct, the index and the replicated counts against
mdfit_map_pred's row 0 bit for bit, the discrepancy tap against
tests/map_ppc_ref.py fed the kernel's own draws, index and counts, the record
and ppos from the taps exactly, the edge cases, the invariance of the record
under every way of calling, the rounds, the rejections and the CLI."""

from __future__ import annotations

import numpy as np
import pytest

from tests import map_ppc_ref as ref
from tests import map_pred_ref as qref
from tests import map_psis_ref as pref
from tests.test_gpu_map_pred import _bits, _map_fit, torch_dev  # noqa: F401  (torch_dev: the module fixture)

pytestmark = pytest.mark.gpu

S_A, R_A, T_A = 256, 1000, 64
SEED = 0
OTHER = ((25, 25), (65, 100), (1024, 1024))
T_OTHER = 8
ROUNDS = 3
# the discrepancy tap against the reference: 30 terms of a few ulp each, about 1.4e-14, with two orders of margin
# left for the two pows
TOL = 1e-12


def _sub(res, lo, hi):
    from metadamage_amd import engine

    return engine.FitBatch(res.out[lo:hi], None, res.status[lo:hi], None)


def _host(torch, *xs):
    torch.cuda.synchronize()
    out = []
    for x in xs:
        a = x.cpu().numpy()
        out.append(a.view(np.uint32) if a.dtype == np.int32 and a.ndim == 3 else a)  # (the counts tap)
    return out


def _run(torch, ty, tN, res, S, R, T, rounds=None, seed=SEED, base=0):
    """mdfit_map_ppc with its three taps, mdfit_map_pred with its two and
    mdfit_map_psis with its draws (the _adapt entries with `rounds`) on the
    first T taxa -> host arrays."""
    from metadamage_amd import engine

    sub = _sub(res, 0, T)
    kw = {} if rounds is None else {"adapt_rounds": rounds, "adapt": True}
    c = engine.map_ppc_device(ty[:T], tN[:T], sub, S, R, seed, base, index=True, counts=True, disc=True, **kw)
    q = engine.map_pred_device(ty[:T], tN[:T], sub, S, R, seed, base, index=True, counts=True, **kw)
    p = engine.map_psis_device(ty[:T], tN[:T], sub, S, seed, base, draws=True, **kw)
    torch.cuda.synchronize()
    got = {"ppos": c[0], "rec": c[1], "index": c[2], "counts": c[3], "disc": c[4], "q_rec": q[1], "q_index": q[2],
           "q_counts": q[3], "psis": p[0], "draws": p[1]}
    if rounds is not None:
        got.update(adapt=c[5], q_adapt=q[4])
    got = {k: v.cpu().numpy() for k, v in got.items()}
    for k in ("counts", "q_counts"):
        got[k] = got[k].view(np.uint32)
    for a in got.values():
        a.setflags(write=False)
    return got


@pytest.fixture(scope="module")
def batch_a(torch_dev):
    """generate(300, seed=21) fitted by one MAP call; the three entries with
    their taps on the first 64 taxa at S = 256, R = 1000 (computed once)."""
    from metadamage_amd.synthetic import generate

    torch = torch_dev
    b = generate(300, seed=21)
    ty, tN, res = _map_fit(torch, b.y, b.N, b.mm)
    before = (res.out.clone(), res.pred.clone(), res.status.clone())
    host = _run(torch, ty, tN, res, S_A, R_A, T_A)
    assert torch.equal(before[0].view(torch.int64), res.out.view(torch.int64))  # out, pred and status are read only
    assert torch.equal(before[1].view(torch.int32), res.pred.view(torch.int32)) and torch.equal(before[2], res.status)
    host.update(b=b, ty=ty, tN=tN, res=res, st=res.status.cpu().numpy())
    return host


# --------------------------------------------------------------------------
# the checks, each on the kernel's own inputs
# --------------------------------------------------------------------------
def _has_weights(got):
    return (got["index"] >= 0).all(axis=1)


def _check_siblings(got, T):
    """Words 8-10 and the valid / reliable bits are mdfit_map_psis's and
    mdfit_map_pred's row 0; the index and the counts are mdfit_map_pred's."""
    rec, q, psis = got["rec"], got["q_rec"], got["psis"]
    has = _has_weights(got)
    pf = psis[:, 0, pref.FLAGS].astype(int)
    fl = rec[:, ref.FLAGS].astype(int)
    assert np.array_equal(has, (pf & pref.VALID) != 0) and np.array_equal(has, ((q[:, qref.FLAGS].astype(int) >> 2) & 1) != 0)
    assert np.array_equal(_bits(rec[:, ref.KHAT]), _bits(q[:, qref.KHAT])), "khat"
    assert np.array_equal(_bits(rec[:, ref.ESS]), _bits(q[:, qref.ESS])), "ess"
    assert np.array_equal(_bits(rec[:, ref.NDISTINCT]), _bits(q[:, qref.NDISTINCT])), "n_distinct"
    assert np.array_equal(_bits(rec[:, ref.KHAT]), _bits(psis[:, 0, pref.KHAT]))
    assert np.array_equal(_bits(rec[:, ref.ESS]), _bits(psis[:, 0, pref.ESS]))
    nonc = (fl & ref.NONCOUNT) != 0
    assert np.array_equal((fl & ref.VALID) != 0, has & ~nonc)
    assert np.array_equal((fl & ref.RELIABLE) != 0, (pf & pref.RELIABLE) != 0)
    assert np.array_equal(got["index"], got["q_index"][:, 0])
    assert np.array_equal(got["counts"], got["q_counts"][:, :30])
    assert ((fl & ~(ref.VALID | ref.RELIABLE | ref.NONCOUNT | ref.ADAPTED)) == 0).all()
    return int(has.sum())


def _check_disc(oracle_lib, got, y, N, S, R, T, label):
    """The discrepancy tap against the reference fed the kernel's own draws,
    index and counts."""
    worst_out = worst_str = 0.0
    n = 0
    for t in range(T):
        if not _has_weights(got)[t]:
            assert np.isnan(got["disc"][t]).all(), t
            continue
        want = ref.ppc_given(oracle_lib, y[t, :30], N[t, :30], got["psis"][t], got["draws"][t], S, R, seed=SEED, g=t,
                             index=got["index"][t], counts=got["counts"][t])
        d, w = got["disc"][t], want["disc"]
        assert np.isfinite(d).all(), t
        for j in (0, 1):
            dev = np.abs(d[:, j] - w[:, j]) / np.maximum(np.abs(w[:, j]), np.finfo(float).tiny)
            dev = np.where(d[:, j] == w[:, j], 0.0, dev)
            worst_out = max(worst_out, float(dev.max()))
        scale = np.maximum(want["abs_sum"], np.finfo(float).tiny)
        for j in (2, 3):
            worst_str = max(worst_str, float((np.abs(d[:, j] - w[:, j]) / scale).max()))
        n += 1
    print(f"{label}: {n} taxa; worst relative deviation of T_out {worst_out:.3e}, "
          f"worst |T_str - reference| / sum |r_i| {worst_str:.3e} (bounds {TOL:.0e})")
    assert worst_out <= TOL and worst_str <= TOL
    return n


def _check_record(got, y, N, S, R, T):
    """The record and ppos follow from the disc and counts taps: the p-values,
    worst_pos, p_worst, n_low, n_points and the flags exactly (integer counts
    over R), the two means within their rounding."""
    tau = pref.khat_threshold(S)
    has = _has_weights(got)
    n = 0
    for t in range(T):
        rec, ppos = got["rec"][t], got["ppos"][t]
        if not has[t]:
            assert np.isnan(rec[:11]).all() and rec[ref.FLAGS] == 0 and np.isnan(ppos).all(), (t, rec)
            assert (got["counts"][t] == ref.NO_COUNT).all() and np.isnan(got["disc"][t]).all(), t
            continue
        gt, eq, live, nonc = ref.column_counts(y[t, :30], N[t, :30], got["counts"][t])
        adapted = bool(int(rec[ref.FLAGS]) & ref.ADAPTED)
        want, wpos = ref.record_from(got["disc"][t], gt, eq, live, nonc, R, rec[ref.KHAT], rec[ref.ESS],
                                     rec[ref.NDISTINCT], tau, adapted)
        exact = [ref.P_OUT, ref.P_STR, ref.WORST, ref.P_WORST, ref.N_LOW, ref.N_POINTS, ref.FLAGS]
        assert np.array_equal(_bits(rec[exact]), _bits(want[exact])), (t, rec, want)
        assert np.array_equal(_bits(ppos), _bits(wpos)), t
        assert abs(rec[ref.T_OUT] - want[ref.T_OUT]) <= TOL * abs(want[ref.T_OUT]), t
        assert abs(rec[ref.T_STR] - want[ref.T_STR]) <= TOL * np.abs(got["disc"][t][:, 2]).mean(), t
        assert (got["counts"][t][~live] == ref.NO_COUNT).all()
        n += 1
    return n


def test_sibling_bits(batch_a):
    assert _check_siblings(batch_a, T_A) >= 58


def test_discrepancy_tap_vs_reference_on_the_kernels_draws(batch_a, oracle_lib):
    b = batch_a["b"]
    assert _check_disc(oracle_lib, batch_a, b.y, b.N, S_A, R_A, T_A, f"S = {S_A}, R = {R_A}, {T_A} taxa") >= 58


def test_record_and_ppos_follow_from_the_taps(batch_a):
    b = batch_a["b"]
    assert _check_record(batch_a, b.y, b.N, S_A, R_A, T_A) >= 58
    rec = batch_a["rec"]
    ok = (rec[:, ref.FLAGS].astype(int) & ref.VALID) != 0
    # clean synthetic data: the check does not cry wolf (tests/test_map_ppc.py pins this on the reference)
    print(f"clean data on the device: min p_outlier {rec[ok, ref.P_OUT].min():.4f}, "
          f"min p_strand {np.nanmin(rec[ok, ref.P_STR]):.4f}")
    assert not (rec[ok, ref.P_OUT] < 0.01).any() and not (rec[ok, ref.P_STR] < 0.01).any()


@pytest.mark.parametrize("S,R", OTHER)
def test_other_draw_counts(torch_dev, batch_a, oracle_lib, S, R):
    b = batch_a["b"]
    got = _run(torch_dev, batch_a["ty"], batch_a["tN"], batch_a["res"], S, R, T_OTHER)
    assert _check_siblings(got, T_OTHER) >= 6
    assert _check_disc(oracle_lib, got, b.y, b.N, S, R, T_OTHER, f"S = {S}, R = {R}, {T_OTHER} taxa") >= 6
    assert _check_record(got, b.y, b.N, S, R, T_OTHER) >= 6


# --------------------------------------------------------------------------
# edges
# --------------------------------------------------------------------------
def test_edges(torch_dev, batch_a, ref_golden):
    torch = torch_dev
    b = batch_a["b"]
    # the whole batch, cheaply: the taxa whose fit failed and the rows importance sampling cannot serve
    S, R = 64, 25
    full = _run(torch, batch_a["ty"], batch_a["tN"], batch_a["res"], S, R, 300)
    _check_siblings(full, 300)
    _check_record(full, b.y, b.N, S, R, 300)
    st = batch_a["st"]
    failed = np.flatnonzero(st != 0)
    no_w = np.flatnonzero((st == 0) & ~_has_weights(full))
    print(f"status != 0: {failed.tolist()}; status 0 without weights at S = {S}: {no_w.tolist()}")
    for t in list(failed) + list(no_w):
        assert np.isnan(full["rec"][t, :11]).all() and full["rec"][t, ref.FLAGS] == 0, t
        assert np.isnan(full["ppos"][t]).all() and (full["index"][t] == -1).all(), t

    # a crafted batch
    U32 = np.iinfo(np.uint32).max
    T = 8
    y = np.zeros((T, 32), np.uint32)
    N = np.zeros((T, 32), np.uint32)
    y[:, :30], N[:, :30] = b.y[3, :30], b.N[3, :30]
    y[0, 4] = N[0, 4] + 1  # y > N at one position: status 3
    dead = [0, 13, 14, 27]
    y[1, dead] = N[1, dead] = 0  # columns with N = 0
    y[2, 15:30] = N[2, 15:30] = 0  # a whole strand with N = 0
    y[3, :30] = 0  # y = 0 everywhere
    y[4, :30] = N[4, :30]  # y = N everywhere
    N[5, :30] = ref_golden["data_ancient__N"][0]
    y[5, :30] = ref_golden["data_ancient__y"][0]
    frac = y[5, 7] / N[5, 7]
    N[5, 7] = U32  # one column with N = 2^32 - 1, its damage frequency kept
    y[5, 7] = np.uint32(frac * float(U32))
    y[6, :15] = N[6, :15] = 0  # the other strand
    # taxon 7: the plain one
    ty, tN, res = _map_fit(torch, y, N)
    before = (res.out.clone(), res.status.clone())
    S, R = 64, 100
    got = _run(torch, ty, tN, res, S, R, T)
    assert torch.equal(before[0].view(torch.int64), res.out.view(torch.int64)) and torch.equal(before[1], res.status)
    stc = res.status.cpu().numpy()
    has = _has_weights(got)
    fl = got["rec"][:, ref.FLAGS].astype(int)
    print(f"crafted batch: status {stc.tolist()}, weights {has.astype(int).tolist()}, flags {fl.tolist()}, "
          f"p_outlier {got['rec'][:, ref.P_OUT].tolist()}, p_strand {got['rec'][:, ref.P_STR].tolist()}")
    assert stc[0] == 3 and not has[0]
    _check_siblings(got, T)
    _check_record(got, y, N, S, R, T)
    rec = got["rec"]
    assert has[1] and rec[1, ref.N_POINTS] == 26 and np.isnan(got["ppos"][1][dead]).all()
    live = [c for c in range(30) if c not in dead]
    assert np.isfinite(got["ppos"][1][live]).all() and np.isfinite(rec[1, ref.P_STR])
    for t in (2, 6):  # one strand alone: no strand comparison, everything else stands
        if has[t]:
            assert rec[t, ref.N_POINTS] == 15 and np.isnan(rec[t, ref.P_STR]) and np.isfinite(rec[t, ref.P_OUT])
            assert np.isfinite(rec[t, ref.T_STR]) and fl[t] & ref.VALID
    assert has[2] or has[6]
    assert has[5] and has[7] and fl[5] & ref.VALID and fl[7] & ref.VALID
    assert (got["counts"][5].astype(np.float64) <= N[5, :30, None]).all()
    assert not (fl & ref.NONCOUNT).any()
    # the rows without weights among taxa whose fit is fine: an invalid proposal or a refused smoothing
    assert no_w.size + int((~has[1:]).sum()) >= 1


# --------------------------------------------------------------------------
# invariance
# --------------------------------------------------------------------------
def test_record_does_not_depend_on_the_call(torch_dev, monkeypatch, batch_a):
    torch = torch_dev
    from metadamage_amd import _lib, distributed as d, engine, fits

    b, res = batch_a["b"], batch_a["res"]
    T, S, R = 8, 64, 100
    ty, tN = batch_a["ty"][:T], batch_a["tN"][:T]

    def same(got, want):
        return len(got) == len(want) and all(np.array_equal(_bits(a), _bits(w)) for a, w in zip(got, want))

    def call(lo=0, hi=T, base=0, seed=SEED, **kw):
        return engine.map_ppc_device(ty[lo:hi], tN[lo:hi], _sub(res, lo, hi), S, R, seed, base, **kw)

    base = _host(torch, *call(index=True, counts=True, disc=True))  # ppos, rec, index, counts, disc
    assert len(base) == 5 and np.isfinite(base[1][:, ref.P_OUT]).sum() >= 6
    # the module's call holds the same taxa at its own S and R
    big = _host(torch, *engine.map_ppc_device(batch_a["ty"][:T_A + 1], batch_a["tN"][:T_A + 1], _sub(res, 0, T_A + 1),
                                              S_A, R_A, SEED, 0))
    assert same([big[0][:T_A], big[1][:T_A]], [batch_a["ppos"], batch_a["rec"]])
    # without the taps, with each of them
    assert same(_host(torch, *call()), base[:2])
    assert same(_host(torch, *call(index=True)), base[:3])
    assert same(_host(torch, *call(counts=True)), base[:2] + base[3:4])
    assert same(_host(torch, *call(disc=True)), base[:2] + base[4:])
    # two calls split with index_base
    a, c = call(0, 3), call(3, T, base=3)
    assert same(_host(torch, torch.cat([a[0], c[0]]), torch.cat([a[1], c[1]])), base[:2])
    assert not same(_host(torch, *call(3, T, base=0)), [base[0][3:], base[1][3:]])  # (the streams are the global taxon's)
    assert not same(_host(torch, *call(seed=SEED + 1)), base[:2])
    # on a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = call(stream=side)
    side.synchronize()
    assert same(_host(torch, *on_side), base[:2])
    # through the chunked dispatch in chunks of 3, and into the gather record of a world of one
    opts = _lib.default_opts(mode=_lib.MODE_MAP)
    q = _host(torch, *engine.map_pred_device(ty, tN, _sub(res, 0, T), S, R, SEED, 0))
    want_pp = np.concatenate([q[0].reshape(T, 90), q[1].astype(np.float32)], axis=1)
    want_pc = np.concatenate([base[0], base[1].astype(np.float32)], axis=1)
    y, N, mm = b.y[:T], b.N[:T], b.mm[:T]
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "3")
    assert len(engine.plan_chunks(T, opts, with_ppred=True, ppc=True)) == 3
    o5, p5, s5, w5, c5 = engine.fit_batch_host(y, N, mm, opts, ppred=True, ppc=True, psis_draws=S, pred_draws=R)
    assert c5.shape == (T, _lib.NPPCOUT) and c5.dtype == np.float32
    assert np.array_equal(c5.view(np.int32), want_pc.view(np.int32))
    assert np.array_equal(w5.view(np.int32), want_pp.view(np.int32))
    plain4 = engine.fit_batch_host(y, N, mm, opts, ppred=True, psis_draws=S, pred_draws=R)
    assert len(plain4) == 4  # (without the option: today's four arrays, bit for bit)
    for x, z in zip(plain4, (o5, p5, s5, w5)):
        assert x.dtype == z.dtype and np.array_equal(x, z, equal_nan=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    rec = d.alloc_records(T, dev, with_ppred=True, with_ppc=True)
    fitter = engine.ChunkedFitter(3, opts=opts, dest_on_device=True, with_ppred=True, ppc=True, psis_draws=S,
                                  pred_draws=R)
    fitter.run_into_device(y, N, mm, opts, engine.FitBatch(rec.out, rec.pred, rec.status, ppred=rec.ppred,
                                                           ppc=rec.ppc),
                           chunks=engine.plan_chunks(T, opts, chunk_taxa=3))
    buf = rec.stage()
    torch.cuda.synchronize()
    og, pg, sg, wg, cg = d.unpack_gathered(d.gather_records(buf, T, 0, 1), T, 1, with_ppred=True, with_ppc=True)
    assert np.array_equal(cg.view(np.int32), want_pc.view(np.int32))
    assert np.array_equal(wg.view(np.int32), want_pp.view(np.int32)) and np.array_equal(sg, s5)
    with pytest.raises(ValueError, match="dest.ppc"):
        fitter.run_into_device(y, N, mm, opts, engine.FitBatch(rec.out, rec.pred, rec.status, ppred=rec.ppred))
    # through fit_packed, with the rounds too: the adapt block stays last
    names = np.array([f"t{i}" for i in range(T)])

    def packed():
        return fits.Packed(np.arange(T), names, np.array(["species"] * T), np.full(T, 100, np.int64), np.array(y),
                           np.array(N), np.array(mm))

    got = fits.fit_packed(packed(), opts, shard=False, ppred=True, ppc=True, psis_draws=S, pred_draws=R)
    assert len(got) == 5 and np.array_equal(got[4].view(np.int32), want_pc.view(np.int32))
    assert np.array_equal(got[3].view(np.int32), want_pp.view(np.int32))
    got = fits.fit_packed(packed(), opts, shard=False, ppred=True, ppc=True, psis_draws=S, pred_draws=R,
                          psis_adapt=ROUNDS)
    ad = _host(torch, *call(adapt_rounds=ROUNDS, adapt=True))
    qa = _host(torch, *engine.map_pred_device(ty, tN, _sub(res, 0, T), S, R, SEED, 0, adapt_rounds=ROUNDS))
    assert len(got) == 6 and got[5].shape == (T, _lib.NADAPTOUT)
    want_pca = np.concatenate([ad[0], ad[1].astype(np.float32)], axis=1)
    assert np.array_equal(got[4].view(np.int32), want_pca.view(np.int32))
    want_ad = engine.adapt_summary(torch.from_numpy(qa[2]).to(ty.device)).cpu().numpy()
    assert np.array_equal(got[5].view(np.int32), want_ad.view(np.int32))
    with pytest.raises(ValueError, match="ppc needs with_ppred"):
        fits.fit_packed(packed(), opts, shard=False, psis=True, ppc=True)
    # the sharded branch as rank 0 of a world of one: the gather record carries the check before the adapt tail
    from metadamage_amd import blocks

    run = blocks.describe(opts, {"psis_adapt": ROUNDS, "ppc": True}, with_ppred=True, psis_draws=S, pred_draws=R)
    sh = fits._fit_sharded(packed(), opts, dev, 0, 1, run)
    assert len(sh) == 6 and np.array_equal(sh[4].view(np.int32), want_pca.view(np.int32))
    assert np.array_equal(sh[5].view(np.int32), want_ad.view(np.int32)) and np.array_equal(sh[3], got[3], equal_nan=True)


# --------------------------------------------------------------------------
# the rounds
# --------------------------------------------------------------------------
@pytest.mark.parametrize("S,R", ((S_A, R_A),) + OTHER)
def test_no_rounds_is_map_ppc_bit_for_bit(torch_dev, batch_a, S, R):
    from metadamage_amd import engine

    torch = torch_dev
    T = T_A if S == S_A else T_OTHER
    ty, tN, res = batch_a["ty"][:T], batch_a["tN"][:T], batch_a["res"]
    kw = dict(index=True, counts=True, disc=True)
    if S == S_A:
        plain = [batch_a[k] for k in ("ppos", "rec", "index", "counts", "disc")]
    else:
        plain = _host(torch, *engine.map_ppc_device(ty, tN, _sub(res, 0, T), S, R, SEED, 0, **kw))
    zero = _host(torch, *engine.map_ppc_device(ty, tN, _sub(res, 0, T), S, R, SEED, 0, adapt_rounds=0, adapt=True, **kw))
    assert len(zero) == 6
    for a, z in zip(plain, zero[:5]):
        assert np.array_equal(_bits(a), _bits(z))
    adp, rec = zero[5], zero[1]
    assert np.array_equal(_bits(adp[:, 0, 0]), _bits(rec[:, ref.KHAT]))  # adapt row 0 reads (khat, ess, 0, 0)
    has = np.isfinite(adp[:, 0, 0])
    assert has.sum() >= 6 and (adp[:, 0, 2:][has] == 0).all() and np.isnan(adp[:, 1:]).all()


def test_rounds_are_map_pred_adapts_row_0(torch_dev, batch_a, oracle_lib):
    b = batch_a["b"]
    got = _run(torch_dev, batch_a["ty"], batch_a["tN"], batch_a["res"], S_A, R_A, T_A, rounds=ROUNDS)
    assert _check_siblings(got, T_A) >= 58
    assert np.array_equal(_bits(got["adapt"][:, 0]), _bits(got["q_adapt"][:, 0]))
    assert np.isnan(got["adapt"][:, 1:]).all()  # rows 1 and 2 are not run
    fl = got["rec"][:, ref.FLAGS].astype(int)
    best = np.nan_to_num(got["adapt"][:, 0, 2])
    assert np.array_equal((fl & ref.ADAPTED) != 0, best > 0) and (best > 0).sum() >= 5
    assert np.array_equal((fl & ref.ADAPTED) != 0, (got["psis"][:, 0, pref.FLAGS].astype(int) & ref.ADAPTED) != 0)
    # an adapted taxon draws from other weights than round 0's, the others from the same
    same = (got["index"] == batch_a["index"]).all(axis=1)
    assert same[best == 0].all() and not same[best > 0].any()
    assert _check_record(got, b.y, b.N, S_A, R_A, T_A) >= 58
    assert _check_disc(oracle_lib, got, b.y, b.N, S_A, R_A, 16, f"S = {S_A}, R = {R_A}, 16 taxa, {ROUNDS} rounds") >= 14


# --------------------------------------------------------------------------
# rejections
# --------------------------------------------------------------------------
def test_rejections(torch_dev, batch_a):
    from metadamage_amd import _lib, engine

    torch = torch_dev
    ty, tN, res = batch_a["ty"][:2], batch_a["tN"][:2], batch_a["res"]
    two = _sub(res, 0, 2)
    for S in (24, 1025):
        with pytest.raises(_lib.MdfitError, match="num_draws"):
            engine.map_ppc_device(ty, tN, two, S, 1000)
    for R in (24, 1025):
        with pytest.raises(_lib.MdfitError, match="num_pred"):
            engine.map_ppc_device(ty, tN, two, 256, R)
    for rounds in (-1, 5):
        with pytest.raises(_lib.MdfitError, match="adapt_rounds"):
            engine.map_ppc_device(ty, tN, two, 256, 100, adapt_rounds=rounds)
    R = 100
    shapes = {"ppos": ((2, 30), torch.float32), "rec": ((2, 12), torch.float64), "index": ((2, R), torch.int32),
              "counts": ((2, 30, R), torch.int32), "disc": ((2, R, 4), torch.float64),
              "adapt": ((2, 3, 4), torch.float64)}
    for name, (shape, dt) in shapes.items():
        wrong_dt = torch.float64 if dt != torch.float64 else torch.float32
        for bad in (torch.empty(shape, dtype=wrong_dt, device="cuda"),
                    torch.empty((shape[0] + 1, *shape[1:]), dtype=dt, device="cuda"),
                    torch.empty(shape, dtype=dt, device="cpu")):
            with pytest.raises(ValueError, match=name):
                engine.map_ppc_device(ty, tN, two, 256, R, **{name: bad})
    with pytest.raises(ValueError, match="res must hold"):
        engine.map_ppc_device(ty, tN, _sub(res, 0, 3), 256, R)
    opts = _lib.default_opts(mode=_lib.MODE_MAP)
    for kw in ({}, {"with_psis": True}, {"with_waic": True}):
        with pytest.raises(ValueError, match="ppc needs with_ppred"):
            engine.ChunkedFitter(8, opts=opts, ppc=True, **kw)
    with pytest.raises(ValueError, match="MODE_MAP"):
        engine.ChunkedFitter(8, opts=_lib.default_opts(mode=_lib.MODE_NUTS), with_ppred=True, ppc=True)


# --------------------------------------------------------------------------
# the CLI
# --------------------------------------------------------------------------
def test_cli_map_pred_ppc(tmp_path):
    import pandas as pd
    from typer.testing import CliRunner

    from metadamage_amd import fits, io
    from metadamage_amd.cli import cli_app
    from tests.helpers import GOLDEN

    def run(out_dir, *args):
        r = CliRunner().invoke(cli_app, ["fit", "--out-dir", str(out_dir), *args, str(GOLDEN / "data_ancient.txt")])
        assert r.exit_code == 0, (r.output, r.exception)
        return io.Parquet(out_dir / "fit_results" / "data_ancient.parquet")

    out_dir = tmp_path / "out"
    pq = run(out_dir, "--inference", "map-pred", "--ppc")
    df = pq.load()
    assert len(df.columns) == 48 and list(df.columns[40:]) == fits.PPC_COLUMNS
    meta = pq.load_metadata()
    assert meta["inference"] == "map-pred" and meta["ppc"] is True
    valid = df["ppc_valid"].to_numpy()
    assert valid.dtype == bool and valid.sum() * 2 > len(df)
    p = df.loc[valid, ["ppc_p_outlier", "ppc_p_worst"]].to_numpy()
    assert ((p >= 0) & (p <= 1)).all() and (df.loc[valid, "ppc_t_outlier"] >= 0).all()
    z = df.loc[valid, "ppc_worst_position"].to_numpy()
    assert ((np.abs(z) >= 1) & (np.abs(z) <= 15)).all()
    pa = io.Parquet(out_dir / "fit_predictions" / "data_ancient.parquet").load()
    assert list(pa.columns)[-1] == "ppc_p" and pa["ppc_p"].dtype == np.float32
    assert np.isfinite(pa["ppc_p"].to_numpy()).any()
    # the worst position's two-sided mid-p is the frame's own ppc_p there
    t0 = df.index[valid][0]
    rows = pa.iloc[30 * t0:30 * t0 + 30]
    pw = rows.loc[rows["position"] == df.loc[t0, "ppc_worst_position"], "ppc_p"].to_numpy()[0]
    assert 2 * min(float(pw), 1 - float(pw)) == pytest.approx(float(df.loc[t0, "ppc_p_worst"]), abs=1e-6)
    # a second run hits the cache; a run without --ppc does not reuse it
    stamp = (out_dir / "fit_results" / "data_ancient.parquet").stat().st_mtime_ns
    again = run(out_dir, "--inference", "map-pred", "--ppc").load()
    assert (out_dir / "fit_results" / "data_ancient.parquet").stat().st_mtime_ns == stamp
    pd.testing.assert_frame_equal(again, df)
    plain = run(out_dir, "--inference", "map-pred").load()
    assert (out_dir / "fit_results" / "data_ancient.parquet").stat().st_mtime_ns != stamp
    assert len(plain.columns) == 40
    pd.testing.assert_frame_equal(df[plain.columns], plain)  # map-pred's columns are the run's without the option
