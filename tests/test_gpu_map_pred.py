"""GPU tests of mdfit_map_pred (MDFIT-PPRED v1): the weights
against mdfit_map_psis bit for bit, the resampling, the index and counts taps
and the summaries against tests/map_pred_ref.py fed the kernel's own inputs,
the edge cases, and the invariance of the record under every way of calling."""

from __future__ import annotations

import ctypes
import time

import numpy as np
import pytest

from oracle import oracle as oracle_mod
from tests import map_pred_cases as cases
from tests import map_pred_ref as ref
from tests import map_psis_ref as pref
from tests.test_nuts_post import draw_shares

pytestmark = pytest.mark.gpu

S_A, R_A, T_A = 256, 1000, 64
SEED = 0
OTHER = ((25, 25), (65, 100), (1024, 1024))
T_OTHER = 8
# flipped comparisons between the device's and the oracle's last bits (the caps of tests/test_gpu_nuts_post.py)
CLASS_CAP, JOB_CAP = 0.005, 0.03


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no HIP device is visible")
    return torch


def _map_fit(torch, y, N, mm=None, **opts):
    from metadamage_amd import _lib, engine

    ty, tN, tm = engine.to_device_counts(y, N, mm)
    res = engine.fit_batch_device(ty, tN, tm, _lib.default_opts(mode=_lib.MODE_MAP, **opts))
    torch.cuda.synchronize()
    return ty, tN, res


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _run(torch, ty, tN, res, S, R, T=None, seed=SEED, base=0, lo=0):
    """mdfit_map_pred with both taps and mdfit_map_psis with its draws on the
    taxa [lo, lo + T) -> host arrays."""
    from metadamage_amd import engine

    T = int(ty.shape[0]) - lo if T is None else T
    sub = engine.FitBatch(res.out[lo:lo + T], None, res.status[lo:lo + T], None)
    pp, rec, idx, cnt = engine.map_pred_device(ty[lo:lo + T], tN[lo:lo + T], sub, S, R, seed, base, index=True,
                                               counts=True)
    psis, dr = engine.map_psis_device(ty[lo:lo + T], tN[lo:lo + T], sub, S, seed, base, draws=True)
    torch.cuda.synchronize()
    got = {"ppred": pp.cpu().numpy(), "rec": rec.cpu().numpy(), "index": idx.cpu().numpy(),
           "counts": cnt.cpu().numpy().view(np.uint32), "psis": psis.cpu().numpy(), "draws": dr.cpu().numpy()}
    for a in got.values():
        a.setflags(write=False)
    return got


@pytest.fixture(scope="module")
def batch_a(torch_dev):
    """generate(300, seed=21) fitted by one MAP call; mdfit_map_pred with its
    taps and mdfit_map_psis with its draws on the first 64 taxa at S = 256, R =
    1000 (computed once, read only)."""
    from metadamage_amd.synthetic import generate

    torch = torch_dev
    b = generate(300, seed=21)
    ty, tN, res = _map_fit(torch, b.y, b.N, b.mm)
    before = (res.out.clone(), res.pred.clone(), res.status.clone())
    host = _run(torch, ty, tN, res, S_A, R_A, T_A)
    # out, pred and status are read only
    assert torch.equal(before[0].view(torch.int64), res.out.view(torch.int64))
    assert torch.equal(before[1].view(torch.int32), res.pred.view(torch.int32)) and torch.equal(before[2], res.status)
    out, st = res.out.cpu().numpy(), res.status.cpu().numpy()
    out.setflags(write=False), st.setflags(write=False)
    host.update(b=b, out=out, st=st, ty=ty, tN=tN, res=res)
    return host


# --------------------------------------------------------------------------
# the pieces, each on the kernel's own inputs
# --------------------------------------------------------------------------
def _check_weights(got, S, T):
    """khat, ess and the flag bits are mdfit_map_psis's on the same call."""
    rec, psis = got["rec"], got["psis"]
    pf = psis[:, :, pref.FLAGS].astype(int)
    fl = rec[:, ref.FLAGS].astype(int)
    for row in range(3):
        assert np.array_equal(_bits(rec[:, ref.KHAT + row]), _bits(psis[:, row, pref.KHAT])), row
        assert np.array_equal(_bits(rec[:, ref.ESS + row]), _bits(psis[:, row, pref.ESS])), row
        assert np.array_equal((fl >> (2 + row)) & 1, pf[:, row] & pref.VALID), row
    assert np.array_equal(fl & ref.VALID, (pf & pref.VALID).all(axis=1).astype(int))
    assert np.array_equal((fl & ref.RELIABLE) != 0, ((pf & pref.RELIABLE) != 0).all(axis=1))
    return int((pf & pref.VALID).sum())


def _check_index(got, S, R, T):
    """The index tap is the reference's resampling of the kernel's own weights."""
    n = 0
    for t in range(T):
        for row in range(3):
            if int(got["psis"][t, row, pref.FLAGS]) & pref.VALID:
                w = got["draws"][t, row, :, 5]
                want, nd = ref.resample(w, R)
                assert np.array_equal(got["index"][t, row], want), (t, row)
                assert got["rec"][t, ref.NDISTINCT + row] == nd and (w[want] > 0).all()
                n += 1
            else:
                assert (got["index"][t, row] == -1).all() and np.isnan(got["rec"][t, ref.NDISTINCT + row])
    return n


def _kernel_flags(got, N, T):
    """The oracle's job flags as the kernel's outputs show them: 2 N = 0, 1 a
    draw that is no count, 0 counts; 255 a job not run (an invalid row)."""
    fl = np.zeros((T, ref.NJOB), np.uint8)
    rowok = (got["rec"][:, ref.FLAGS].astype(int)[:, None] >> (2 + np.arange(3))[None, :]) & 1
    for j, (row, col, k, ncol) in enumerate(ref.JOBS):
        m = got["ppred"][:, 0, j] if j < 30 else got["rec"][:, 3 + j - 30]
        fl[:, j] = np.where(N[:T, ncol] == 0, 2, np.where(np.isnan(m), 1, 0))
        fl[rowok[:, row] == 0, j] = 255
    return fl


def _check_counts(oracle_lib, got, y, N, S, R, T, label):
    """The counts tap against the oracle's post step fed the kernel's own
    theta (its u through the reference's transform) at the kernel's index:
    equal up to flipped comparisons, the job flags equal."""
    x = np.full((T, 6, R, 4), 0.5)
    for t in range(T):
        for row in range(3):
            if int(got["psis"][t, row, pref.FLAGS]) & pref.VALID:
                th = pref.constrained(np.asarray(got["draws"][t, row, :, :4], np.float64)).astype(np.float64)
                x[t, ref.STREAM_SUB[row]] = th[got["index"][t, row]]
    want = oracle_lib.nuts_post(y[:T], N[:T], x, seed=SEED, taps=True)
    kf = _kernel_flags(got, N, T)
    of = want[5].copy()
    of[kf == 255] = 255
    assert np.array_equal(kf, of), np.argwhere(kf != of)
    per_class, per_job, _, diff = draw_shares(x, N[:T], got["counts"], want[4], kf, of)
    print(f"{label}: " + ", ".join(f"{c} {d}/{n}" for c, (d, n) in per_class.items())
          + f"; worst job {100.0 * per_job.max():.3f} %; {int(diff.sum())} of {int((kf <= 1).sum()) * R} draws differ")
    for c, (d, n) in per_class.items():
        assert d <= CLASS_CAP * n, (c, d, n)
    assert per_job.max() <= JOB_CAP
    not_run = kf == 255
    assert (got["counts"][not_run] == ref.NO_COUNT).all() and (got["counts"][kf == 2] == ref.NO_COUNT).all()
    return per_class


def _check_summaries(got, N, T):
    """ppred and rec are np.median / numpyro's hpdi of the tapped counts."""
    n = 0
    for t in range(T):
        for j, (row, col, k, ncol) in enumerate(ref.JOBS):
            want = ref.summary(oracle_mod, got["counts"][t, j], float(N[t, ncol]))
            have = got["ppred"][t, :, j] if j < 30 else got["rec"][t, 3 + j - 30:4 + j - 30]
            want = want.astype(np.float32) if j < 30 else want[:1]
            assert np.array_equal(have, want, equal_nan=True), (t, j, have, want)
            n += int(np.isfinite(want).all())
        assert np.array_equal(got["rec"][t, :3], ref.summary(oracle_mod, got["counts"][t, 0], float(N[t, 0])),
                              equal_nan=True)
    return n


def test_weights_are_map_psis_bit_for_bit(batch_a):
    assert _check_weights(batch_a, S_A, T_A) >= 170  # of 192 rows


def test_index_tap_is_the_reference_resampling_of_the_kernels_weights(batch_a):
    assert _check_index(batch_a, S_A, R_A, T_A) >= 170


def test_counts_tap_vs_oracle_on_the_kernels_theta(batch_a, oracle_lib):
    b = batch_a["b"]
    pc = _check_counts(oracle_lib, batch_a, b.y, b.N, S_A, R_A, T_A, f"S = {S_A}, R = {R_A}, {T_A} taxa")
    for c in ("inversion", "btrs_small", "boost"):
        assert pc[c][1] > 0, c


def test_summaries_are_median_and_hpdi_of_the_tapped_counts(batch_a):
    assert _check_summaries(batch_a, batch_a["b"].N, T_A) >= 30 * 55


@pytest.mark.parametrize("S,R", OTHER)
def test_other_draw_counts(torch_dev, batch_a, oracle_lib, S, R):
    b = batch_a["b"]
    got = _run(torch_dev, batch_a["ty"], batch_a["tN"], batch_a["res"], S, R, T_OTHER)
    assert _check_weights(got, S, T_OTHER) >= 18
    assert _check_index(got, S, R, T_OTHER) >= 18
    _check_counts(oracle_lib, got, b.y, b.N, S, R, T_OTHER, f"S = {S}, R = {R}, {T_OTHER} taxa")
    assert _check_summaries(got, b.N, T_OTHER) >= 30 * 6


def test_resampling_helper_equals_reference(torch_dev):
    from metadamage_amd import engine

    items = cases.all_weight_series()
    groups = {}
    for S, R, kind, w in items:
        groups.setdefault((S, R), []).append((kind, w))
    assert len(groups) >= 20
    for (S, R), series in groups.items():
        idx, nd = engine.resample(np.stack([w for _, w in series]), R)
        for i, (kind, w) in enumerate(series):
            want, want_nd = ref.resample(w, R)
            assert np.array_equal(idx[i], want) and nd[i] == want_nd, (S, R, kind)


# --------------------------------------------------------------------------
# edges
# --------------------------------------------------------------------------
def test_edges(torch_dev, batch_a, oracle_lib, ref_golden):
    from metadamage_amd import engine

    torch = torch_dev
    b = batch_a["b"]
    S, R = 64, 25
    # the whole batch, cheaply: rows importance sampling cannot serve are NaN in their jobs alone
    full = _run(torch, batch_a["ty"], batch_a["tN"], batch_a["res"], S, R)
    _check_weights(full, S, 300)
    fl = full["rec"][:, ref.FLAGS].astype(int)
    st = batch_a["st"]
    failed = np.flatnonzero(st != 0)
    for t in failed:
        assert np.isnan(full["rec"][t, :15]).all() and fl[t] == 0 and np.isnan(full["ppred"][t]).all()
        assert (full["index"][t] == -1).all() and (full["counts"][t] == ref.NO_COUNT).all()
    rowok = (fl[:, None] >> (2 + np.arange(3))[None, :]) & 1
    bad_rows = [(t, r) for t in np.flatnonzero(st == 0) for r in range(3) if not rowok[t, r]]
    print(f"psis-invalid rows at S = {S}: {bad_rows}")
    assert bad_rows
    for t, r in bad_rows:
        assert not fl[t] & ref.VALID and not fl[t] & ref.RELIABLE
        assert np.isnan(full["rec"][t, [ref.KHAT + r, ref.ESS + r, ref.NDISTINCT + r]]).all()
        if r == 0:
            assert np.isnan(full["ppred"][t]).all() and np.isnan(full["rec"][t, :3]).all()
        else:
            assert np.isnan(full["rec"][t, 2 + r])
            if rowok[t, 0]:
                live = b.N[t, :30] > 0
                assert np.isfinite(full["ppred"][t][:, live]).all() and np.isfinite(full["rec"][t, :3]).all()
    ok_all = np.flatnonzero((fl & ref.VALID) != 0)
    assert ok_all.size >= 250
    for t in ok_all[:40]:
        live = b.N[t, :30] > 0
        assert np.isfinite(full["ppred"][t][:, live]).all() and np.isnan(full["ppred"][t][:, ~live]).all()
    assert (full["rec"][ok_all, ref.NNONCOUNT] == 0).all()

    # a crafted batch: y > N; N = 0 columns; N = 1 columns; N = 4e9; y = 0 everywhere
    T = 5
    y = np.zeros((T, 32), np.uint32)
    N = np.zeros((T, 32), np.uint32)
    y[:, :30], N[:, :30] = b.y[3, :30], b.N[3, :30]
    y[0, 4] = N[0, 4] + 1  # y > N at one position: status 3
    dead = [0, 13, 14, 27]
    y[1, dead] = N[1, dead] = 0  # N = 0, column 0 among them: D_max and both half fits' jobs are NaN
    ones = [1, 2, 16]
    N[1, ones] = 1
    y[1, ones] = [1, 0, 1]
    N[2, :30] = ref_golden["data_ancient__N"][0]
    y[2, :30] = ref_golden["data_ancient__y"][0]
    k = int(4.0e9 // N[2, :30].max())
    N[2, :30] *= np.uint32(k)
    y[2, :30] *= np.uint32(k)
    assert 3.9e9 < N[2, :30].max() <= 4.0e9
    y[3, :30] = 0  # no damage at all
    N[4, 5] = 1
    y[4, 5] = 0
    ty, tN, res = _map_fit(torch, y, N)
    before = (res.out.clone(), res.status.clone())
    S, R = 64, 100
    got = _run(torch, ty, tN, res, S, R, T)
    assert torch.equal(before[0].view(torch.int64), res.out.view(torch.int64)) and torch.equal(before[1], res.status)
    stc = res.status.cpu().numpy()
    assert stc[0] == 3 and (stc[1:] == 0).all(), stc
    assert np.isnan(got["rec"][0, :15]).all() and got["rec"][0, 15] == 0 and np.isnan(got["ppred"][0]).all()
    assert (got["index"][0] == -1).all() and (got["counts"][0] == ref.NO_COUNT).all()
    _check_weights(got, S, T)
    _check_index(got, S, R, T)
    _check_counts(oracle_lib, got, y, N, S, R, T, "edge batch")
    _check_summaries(got, N, T)
    # NaN exactly where the reference fed the kernel's weights and u has it, and the same flags
    for t in range(1, T):
        want = ref.pred_given(oracle_lib, N[t, :30], got["psis"][t], got["draws"][t], S, R, seed=SEED, g=t)
        assert int(got["rec"][t, ref.FLAGS]) == int(want["rec"][ref.FLAGS]), t
        assert np.array_equal(np.isnan(got["rec"][t]), np.isnan(want["rec"])), (t, got["rec"][t], want["rec"])
        assert np.array_equal(np.isnan(got["ppred"][t]), np.isnan(want["ppred"])), t
        assert np.array_equal(got["index"][t], want["index"]), t
    f1 = int(got["rec"][1, ref.FLAGS])
    if f1 & 4:
        assert np.isnan(got["ppred"][1][:, dead]).all() and np.isnan(got["rec"][1, :3]).all()
        live = [c for c in range(30) if c not in dead]
        assert np.isfinite(got["ppred"][1][:, live]).all()
        assert set(np.unique(got["ppred"][1][:, ones])) <= {0.0, 0.5, 1.0}  # N = 1: counts 0 and 1
    assert np.isnan(got["rec"][1, 3:5]).all()  # jobs 30 and 31 read N[0] = 0
    assert int(got["rec"][2, ref.FLAGS]) & 4 and np.isfinite(got["ppred"][2]).all()
    assert (got["counts"][2, :30].astype(np.float64) <= N[2, :30, None]).all()


# --------------------------------------------------------------------------
# invariance
# --------------------------------------------------------------------------
def test_record_does_not_depend_on_the_call(torch_dev, monkeypatch, batch_a):
    torch = torch_dev
    from metadamage_amd import _lib, distributed as d, engine

    b, res = batch_a["b"], batch_a["res"]
    T = 65  # one more than batch_a's: the first 64 are compared with it
    S, R = 64, 100
    ty, tN = batch_a["ty"][:T], batch_a["tN"][:T]
    out0, pred0, st0 = res.out.clone(), res.pred.clone(), res.status.clone()

    def sub(lo, hi):
        return engine.FitBatch(res.out[lo:hi], None, res.status[lo:hi], None)

    def host(*xs):
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in xs]

    def same(got, want):
        return all(np.array_equal(_bits(a), _bits(w)) for a, w in zip(got, want))

    base = host(*engine.map_pred_device(ty, tN, sub(0, T), S, R, SEED, 0, index=True, counts=True))
    # T = 64 at the module's S and R: the first taxa of a larger call are the call of batch_a
    big = host(*engine.map_pred_device(ty, tN, sub(0, T), S_A, R_A, SEED, 0))
    assert same([big[0][:T_A], big[1][:T_A]], [batch_a["ppred"], batch_a["rec"]])
    # without the taps, with one of them
    assert same(host(*engine.map_pred_device(ty, tN, sub(0, T), S, R, SEED, 0)), base[:2])
    assert same(host(*engine.map_pred_device(ty, tN, sub(0, T), S, R, SEED, 0, index=True)), base[:3])
    assert same(host(*engine.map_pred_device(ty, tN, sub(0, T), S, R, SEED, 0, counts=True)), base[:2] + base[3:])
    # T = 1, 3
    for n in (1, 3):
        got = host(*engine.map_pred_device(ty[:n], tN[:n], sub(0, n), S, R, SEED, 0))
        assert same(got, [base[0][:n], base[1][:n]]), n
    # two calls split with index_base
    a = engine.map_pred_device(ty[:30], tN[:30], sub(0, 30), S, R, SEED, 0)
    c = engine.map_pred_device(ty[30:], tN[30:], sub(30, T), S, R, SEED, 30)
    wrong = engine.map_pred_device(ty[30:], tN[30:], sub(30, T), S, R, SEED, 0)
    assert same(host(torch.cat([a[0], c[0]]), torch.cat([a[1], c[1]])), base[:2])
    assert not same(host(*wrong), [base[0][30:], base[1][30:]])  # (the streams are the global taxon's)
    assert not same(host(*engine.map_pred_device(ty, tN, sub(0, T), S, R, SEED + 1, 0)), base[:2])
    # after a poisoning of the LDS
    _lib.check(_lib.load().mdfit_poison_lds(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert same(host(*engine.map_pred_device(ty, tN, sub(0, T), S, R, SEED, 0)), base[:2])
    # under graph capture and replay
    s = torch.cuda.Stream()
    dpp = torch.zeros((T, _lib.NPRED, _lib.NPOS), dtype=torch.float32, device=ty.device)
    drec = torch.zeros((T, _lib.NMAPPRED), dtype=torch.float64, device=ty.device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        engine.map_pred_device(ty, tN, sub(0, T), S, R, SEED, 0, ppred=dpp, rec=drec,
                               stream=torch.cuda.current_stream())
    for _ in range(2):
        dpp.fill_(0.0)
        drec.fill_(0.0)
        g.replay()
        assert same(host(dpp, drec), base[:2])
    # out, pred and status are unchanged by all of it
    assert torch.equal(out0.view(torch.int64), res.out.view(torch.int64)) and torch.equal(st0, res.status)
    assert torch.equal(pred0.view(torch.int32), res.pred.view(torch.int32))
    # through the chunked dispatch in two chunks, and into the gather record of a world of one
    opts = _lib.default_opts(mode=_lib.MODE_MAP)
    want32 = np.concatenate([base[0].reshape(T, 90), base[1].astype(np.float32)], axis=1)
    y, N, mm = b.y[:T], b.N[:T], b.mm[:T]
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "33")
    assert len(engine.plan_chunks(T, opts, with_ppred=True)) == 2
    o4, p4, s4, w4 = engine.fit_batch_host(y, N, mm, opts, ppred=True, psis_draws=S, pred_draws=R)
    assert w4.shape == (T, engine.PPRED_WORDS) and w4.dtype == np.float32 and engine.PPRED_WORDS == 106
    assert np.array_equal(w4.view(np.int32), want32.view(np.int32))
    pp4, rec4 = engine.split_ppred(w4)
    assert pp4.shape == (T, 3, 30) and rec4.shape == (T, 16) and np.array_equal(_bits(pp4), _bits(base[0]))
    plain3 = engine.fit_batch_host(y, N, mm, opts)
    assert len(plain3) == 3
    for x, z in zip(plain3, (o4, p4, s4)):
        assert x.dtype == z.dtype and np.array_equal(x, z, equal_nan=True)
    rec = d.alloc_records(T, torch.device("cuda", torch.cuda.current_device()), with_ppred=True)
    assert rec.buf.numel() == T * (d.REC_BYTES + d.REC_PPRED)
    fitter = engine.ChunkedFitter(33, opts=opts, dest_on_device=True, with_ppred=True, psis_draws=S, pred_draws=R)
    fitter.run_into_device(y, N, mm, opts, engine.FitBatch(rec.out, rec.pred, rec.status, ppred=rec.ppred),
                           chunks=engine.plan_chunks(T, opts, chunk_taxa=33))
    buf = rec.stage()
    torch.cuda.synchronize()
    og, pg, sg, wg = d.unpack_gathered(d.gather_records(buf, T, 0, 1), T, 1, with_ppred=True)
    assert np.array_equal(wg.view(np.int32), want32.view(np.int32))
    assert np.array_equal(og, d.round_like_gather(batch_a["out"][:T]), equal_nan=True) and np.array_equal(sg, s4)
    assert np.array_equal(pg, p4, equal_nan=True)


def test_rejections(torch_dev, batch_a):
    from metadamage_amd import _lib, engine

    ty, tN, res = batch_a["ty"], batch_a["tN"], batch_a["res"]
    two = engine.FitBatch(res.out[:2], None, res.status[:2], None)
    for S in (24, 1025):
        with pytest.raises(_lib.MdfitError, match="num_draws"):
            engine.map_pred_device(ty[:2], tN[:2], two, S, 1000)
    for R in (24, 1025):
        with pytest.raises(_lib.MdfitError, match="num_pred"):
            engine.map_pred_device(ty[:2], tN[:2], two, 256, R)
    with pytest.raises(ValueError, match="MODE_MAP"):
        engine.ChunkedFitter(8, opts=_lib.default_opts(mode=_lib.MODE_NUTS), with_ppred=True)
    with pytest.raises(ValueError, match="mutually exclusive"):
        engine.ChunkedFitter(8, opts=_lib.default_opts(mode=_lib.MODE_MAP), with_ppred=True, with_psis=True)


# --------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------
def test_end_to_end_vs_reference_on_its_own_draws(batch_a, oracle_lib):
    """Every stage is pinned above on the kernel's own inputs; on the
    reference's own draws and weights the flags and the NaN positions are
    equal, and the share of equal indices and the worst |delta| are printed."""
    b, T = batch_a["b"], 12
    t0 = time.time()
    eq = tot = 0
    worst = 0.0
    near = 0
    for t in range(T):
        want = ref.pred_taxon(oracle_lib, b.y[t, :30], b.N[t, :30], batch_a["out"][t], int(batch_a["st"][t]), S_A, R_A,
                              seed=SEED, g=t)
        got_f, want_f = int(batch_a["rec"][t, ref.FLAGS]), int(want["rec"][ref.FLAGS])
        kh = batch_a["rec"][t, ref.KHAT:ref.KHAT + 3]
        if got_f != want_f and (got_f | ref.RELIABLE) == (want_f | ref.RELIABLE) and \
                np.nanmin(np.abs(kh - pref.khat_threshold(S_A))) < 1e-6:
            near += 1  # a khat within 1e-6 of its threshold: the reliable bit is not the data's
            continue
        assert got_f == want_f, (t, got_f, want_f)
        assert np.array_equal(np.isnan(batch_a["rec"][t]), np.isnan(want["rec"])), t
        assert np.array_equal(np.isnan(batch_a["ppred"][t]), np.isnan(want["ppred"])), t
        ok = want["index"] >= 0
        eq += int((batch_a["index"][t][ok] == want["index"][ok]).sum())
        tot += int(ok.sum())
        with np.errstate(invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.abs(batch_a["ppred"][t] - want["ppred"]), initial=0.0)))
    print(f"end to end, {T} taxa ({near} left out): {eq} of {tot} indices equal ({100.0 * eq / max(tot, 1):.2f} %), "
          f"worst |ppred - reference| {worst:.3e}; {time.time() - t0:.1f} s")
    assert near <= 1


# --------------------------------------------------------------------------
# the CLI
# --------------------------------------------------------------------------
def test_cli_map_pred(tmp_path):
    import pandas as pd
    from typer.testing import CliRunner

    from metadamage_amd import io
    from metadamage_amd.cli import cli_app
    from tests.helpers import GOLDEN
    from tests.test_map_pred import NEW_COLUMNS, NEW_PREDICTION_COLUMNS

    def run(out_dir, *args):
        r = CliRunner().invoke(cli_app, ["fit", "--out-dir", str(out_dir), *args, str(GOLDEN / "data_ancient.txt")])
        assert r.exit_code == 0, (r.output, r.exception)
        return io.Parquet(out_dir / "fit_results" / "data_ancient.parquet")

    out_dir = tmp_path / "out"
    pq = run(out_dir, "--inference", "map-pred")
    df = pq.load()
    assert len(df.columns) == 40 and list(df.columns[30:]) == NEW_COLUMNS
    meta = pq.load_metadata()
    assert meta["inference"] == "map-pred" and int(meta["psis_draws"]) == 256 and int(meta["pred_draws"]) == 1000
    valid = df["map_pred_valid"].to_numpy() == 1
    assert valid.any()
    assert np.isfinite(df.loc[valid, NEW_COLUMNS[:7]].to_numpy()).all()
    assert (df.loc[valid, "pred_ess_min"] > 1).all() and (df.loc[valid, "pred_distinct_min"] > 1).all()
    lo, mid, hi = (df.loc[valid, c].to_numpy() for c in ("D_max_predictive_lower_hpdi", "D_max_predictive",
                                                         "D_max_predictive_upper_hpdi"))
    assert (lo <= mid).all() and (mid <= hi).all()
    # the interval holds the parameter uncertainty the mode's window leaves out: not narrower on the whole
    w_map = (df.loc[valid, "D_max_upper_hpdi"] - df.loc[valid, "D_max_lower_hpdi"]).to_numpy()
    assert np.median((hi - lo) / w_map) >= 1.0
    plain = run(tmp_path / "plain", "--inference", "map").load()
    assert len(plain.columns) == 30
    pd.testing.assert_frame_equal(df[plain.columns], plain)  # the 25 result columns (and the names) are the MAP call's
    pa = io.Parquet(out_dir / "fit_predictions" / "data_ancient.parquet").load()
    pb = io.Parquet(tmp_path / "plain" / "fit_predictions" / "data_ancient.parquet").load()
    assert list(pa.columns) == list(pb.columns) + NEW_PREDICTION_COLUMNS
    pd.testing.assert_frame_equal(pa[pb.columns], pb)  # median, hdpi_lower, hdpi_upper too
    assert np.isfinite(pa[NEW_PREDICTION_COLUMNS].to_numpy()).any()
    first = pa["position"].to_numpy() == 1
    np.testing.assert_array_equal(pa.loc[first, "median_posterior"].to_numpy(), df["D_max_predictive"].to_numpy())
    f = out_dir / "fit_results" / "data_ancient.parquet"
    m1 = f.stat().st_mtime_ns
    run(out_dir, "--inference", "map-pred")  # cache hit: file untouched
    assert f.stat().st_mtime_ns == m1
    pq2 = run(out_dir, "--inference", "map-pred", "--pred-draws", "100")  # other draws: the cache is not reused
    assert f.stat().st_mtime_ns != m1 and int(pq2.load_metadata()["pred_draws"]) == 100
