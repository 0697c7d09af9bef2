"""GPU tests of mdfit_map_pred_adapt (MDFIT-AUTO v1.1): khat,
ess, the valid / reliable bits and the adapt rows against mdfit_map_psis_adapt
bit for bit, the index tap against the reference's resampling of that entry's
best-round weights, the counts tap against the oracle fed the kernel's own
best-round theta, the summaries, the identity with mdfit_map_pred at no rounds,
and the invariance of the record under every way of calling."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import map_adapt_ref as ad
from tests import map_pred_ref as ref
from tests import map_psis_ref as pref
from tests.test_gpu_map_pred import (_bits, _check_counts, _check_index, _check_summaries, _check_weights, _map_fit,
                                     torch_dev)  # noqa: F401  (torch_dev: the module fixture)

pytestmark = pytest.mark.gpu

S_A, R_A, T_A, ROUNDS = 256, 1000, 64, 3
SEED = 0
OTHER = ((25, 25), (65, 100), (1024, 1024))
T_OTHER = 8


def _run(torch, ty, tN, res, S, R, T, rounds=ROUNDS, seed=SEED, base=0):
    """mdfit_map_pred_adapt with both taps and its adapt record, and
    mdfit_map_psis_adapt with its draws and adapt record, on the first T taxa."""
    from metadamage_amd import engine

    sub = engine.FitBatch(res.out[:T], None, res.status[:T], None)
    pp, rec, idx, cnt, adp = engine.map_pred_device(ty[:T], tN[:T], sub, S, R, seed, base, index=True, counts=True,
                                                    adapt_rounds=rounds, adapt=True)
    psis, dr, adq = engine.map_psis_device(ty[:T], tN[:T], sub, S, seed, base, draws=True, adapt_rounds=rounds,
                                           adapt=True)
    torch.cuda.synchronize()
    got = {"ppred": pp.cpu().numpy(), "rec": rec.cpu().numpy(), "index": idx.cpu().numpy(),
           "counts": cnt.cpu().numpy().view(np.uint32), "adapt": adp.cpu().numpy(), "psis": psis.cpu().numpy(),
           "draws": dr.cpu().numpy(), "psis_adapt": adq.cpu().numpy()}
    for a in got.values():
        a.setflags(write=False)
    return got


@pytest.fixture(scope="module")
def batch_a(torch_dev):
    """generate(300, seed=21) fitted by one MAP call; the two adapting entries
    on the first 64 taxa at S = 256, R = 1000, three rounds (computed once)."""
    from metadamage_amd.synthetic import generate

    torch = torch_dev
    b = generate(300, seed=21)
    ty, tN, res = _map_fit(torch, b.y, b.N, b.mm)
    before = (res.out.clone(), res.pred.clone(), res.status.clone())
    host = _run(torch, ty, tN, res, S_A, R_A, T_A)
    assert torch.equal(before[0].view(torch.int64), res.out.view(torch.int64))  # out, pred and status are read only
    assert torch.equal(before[1].view(torch.int32), res.pred.view(torch.int32)) and torch.equal(before[2], res.status)
    host.update(b=b, ty=ty, tN=tN, res=res)
    return host


def _check_adapt(got, S):
    """The adapt rows are mdfit_map_psis_adapt's bit for bit, and the record's
    MDFIT_FLAG_ADAPTED says that some valid row's best round is > 0.  Returns
    (rows with best round > 0, rows over tau in round 0, rows over tau after)."""
    assert np.array_equal(_bits(got["adapt"]), _bits(got["psis_adapt"]))
    pf = got["psis"][:, :, pref.FLAGS].astype(int)
    valid = (pf & pref.VALID) != 0
    best = got["adapt"][:, :, 2]
    assert np.array_equal(valid, np.isfinite(best))
    assert np.array_equal((pf & ad.ADAPTED) != 0, valid & (np.nan_to_num(best) > 0))
    fl = got["rec"][:, ref.FLAGS].astype(int)
    assert np.array_equal((fl & ad.ADAPTED) != 0, ((pf & ad.ADAPTED) != 0).any(axis=1))
    assert ((fl & ~(31 | ad.ADAPTED)) == 0).all()
    tau = pref.khat_threshold(S)
    over0 = int((got["adapt"][:, :, 0][valid] > tau).sum())
    over1 = int((got["psis"][:, :, pref.KHAT][valid] > tau).sum())
    return int((np.nan_to_num(best) > 0).sum()), over0, over1


def test_weights_and_adapt_rows_are_map_psis_adapt_bit_for_bit(batch_a):
    assert _check_weights(batch_a, S_A, T_A) >= 170  # of 192 rows
    n_adapted, over0, over1 = _check_adapt(batch_a, S_A)
    print(f"S = {S_A}, {T_A} taxa: {n_adapted} rows with best round > 0; over tau {over0} -> {over1}")
    assert n_adapted >= 25 and over1 < over0  # (DESIGN.md §3.12 measured 37 -> 6 rows over tau here)


def test_index_tap_is_the_reference_resampling_of_the_best_round_weights(batch_a):
    assert _check_index(batch_a, S_A, R_A, T_A) >= 170
    # an adapted row draws from other weights than round 0's
    from metadamage_amd import engine

    sub = engine.FitBatch(batch_a["res"].out[:T_A], None, batch_a["res"].status[:T_A], None)
    _, _, idx0 = engine.map_pred_device(batch_a["ty"][:T_A], batch_a["tN"][:T_A], sub, S_A, R_A, SEED, 0, index=True)
    idx0 = idx0.cpu().numpy()
    best = np.nan_to_num(batch_a["adapt"][:, :, 2], nan=-1.0)
    same = (idx0 == batch_a["index"]).all(axis=2)
    assert same[best == 0].all() and same[best < 0].all() and not same[best > 0].any()


def test_counts_tap_vs_oracle_on_the_kernels_best_round_theta(batch_a, oracle_lib):
    b = batch_a["b"]
    _check_counts(oracle_lib, batch_a, b.y, b.N, S_A, R_A, T_A, f"S = {S_A}, R = {R_A}, {T_A} taxa, {ROUNDS} rounds")


def test_summaries_are_median_and_hpdi_of_the_tapped_counts(batch_a):
    assert _check_summaries(batch_a, batch_a["b"].N, T_A) >= 30 * 55


@pytest.mark.parametrize("S,R", OTHER)
def test_other_draw_counts(torch_dev, batch_a, oracle_lib, S, R):
    b = batch_a["b"]
    got = _run(torch_dev, batch_a["ty"], batch_a["tN"], batch_a["res"], S, R, T_OTHER)
    assert _check_weights(got, S, T_OTHER) >= 18
    _check_adapt(got, S)
    assert _check_index(got, S, R, T_OTHER) >= 18
    _check_counts(oracle_lib, got, b.y, b.N, S, R, T_OTHER, f"S = {S}, R = {R}, {T_OTHER} taxa, {ROUNDS} rounds")
    assert _check_summaries(got, b.N, T_OTHER) >= 30 * 6


@pytest.mark.parametrize("S,R", ((S_A, R_A),) + OTHER)
def test_no_rounds_is_map_pred_bit_for_bit(torch_dev, batch_a, S, R):
    from metadamage_amd import engine

    torch = torch_dev
    T = T_A if S == S_A else T_OTHER
    ty, tN, res = batch_a["ty"][:T], batch_a["tN"][:T], batch_a["res"]
    sub = engine.FitBatch(res.out[:T], None, res.status[:T], None)
    plain = engine.map_pred_device(ty, tN, sub, S, R, SEED, 0, index=True, counts=True)
    zero = engine.map_pred_device(ty, tN, sub, S, R, SEED, 0, index=True, counts=True, adapt_rounds=0, adapt=True)
    torch.cuda.synchronize()
    assert len(plain) == 4 and len(zero) == 5
    for a, z in zip(plain, zero[:4]):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(z.cpu().numpy()))
    adp, rec = zero[4].cpu().numpy(), zero[1].cpu().numpy()
    # adapt reads (khat, ess, 0, 0)
    assert np.array_equal(_bits(adp[:, :, 0]), _bits(rec[:, ref.KHAT:ref.KHAT + 3]))
    valid = np.isfinite(adp[:, :, 0])
    assert valid.sum() >= 18 and (adp[:, :, 2:][valid] == 0).all() and np.isnan(adp[~valid]).all()
    np.testing.assert_allclose(adp[:, :, 1][valid], rec[:, ref.ESS:ref.ESS + 3][valid], rtol=1e-13)


def test_record_does_not_depend_on_the_call(torch_dev, monkeypatch, batch_a):
    torch = torch_dev
    from metadamage_amd import _lib, distributed as d, engine

    b, res = batch_a["b"], batch_a["res"]
    T = 65  # one more than batch_a's: the first 64 are compared with it
    S, R = 64, 100
    ty, tN = batch_a["ty"][:T], batch_a["tN"][:T]
    out0, pred0, st0 = res.out.clone(), res.pred.clone(), res.status.clone()
    kw = {"adapt_rounds": ROUNDS}

    def sub(lo, hi):
        return engine.FitBatch(res.out[lo:hi], None, res.status[lo:hi], None)

    def host(*xs):
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in xs]

    def same(got, want):
        return len(got) == len(want) and all(np.array_equal(_bits(a), _bits(w)) for a, w in zip(got, want))

    # base: ppred, rec, index, counts, adapt
    base = host(*engine.map_pred_device(ty, tN, sub(0, T), S, R, SEED, 0, index=True, counts=True, **kw))
    assert len(base) == 5 and (np.nan_to_num(base[4][:, :, 2]) > 0).sum() >= 10
    big = host(*engine.map_pred_device(ty, tN, sub(0, T), S_A, R_A, SEED, 0, **kw))
    assert same([big[0][:T_A], big[1][:T_A], big[2][:T_A]], [batch_a["ppred"], batch_a["rec"], batch_a["adapt"]])
    # without the taps, with one of them, with a given adapt tensor
    assert same(host(*engine.map_pred_device(ty, tN, sub(0, T), S, R, SEED, 0, **kw)), base[:2] + base[4:])
    assert same(host(*engine.map_pred_device(ty, tN, sub(0, T), S, R, SEED, 0, index=True, **kw)),
                base[:3] + base[4:])
    assert same(host(*engine.map_pred_device(ty, tN, sub(0, T), S, R, SEED, 0, counts=True, **kw)),
                base[:2] + base[3:])
    # without the adapt record: the entry itself with adapt = NULL
    lib = _lib.load()
    pp = torch.zeros((T, _lib.NPRED, _lib.NPOS), dtype=torch.float32, device=ty.device)
    rec = torch.zeros((T, _lib.NMAPPRED), dtype=torch.float64, device=ty.device)
    p = ctypes.c_void_p
    _lib.check(lib.mdfit_map_pred_adapt(p(ty.data_ptr()), p(tN.data_ptr()), p(res.out.data_ptr()),
                                        p(res.status.data_ptr()), T, S, R, ROUNDS, SEED, 0, p(pp.data_ptr()),
                                        p(rec.data_ptr()), None, None, None,
                                        p(torch.cuda.current_stream().cuda_stream)))
    assert same(host(pp, rec), base[:2])
    for rounds in (-1, 5):
        rc = lib.mdfit_map_pred_adapt(p(ty.data_ptr()), p(tN.data_ptr()), p(res.out.data_ptr()),
                                      p(res.status.data_ptr()), T, S, R, rounds, SEED, 0, p(pp.data_ptr()),
                                      p(rec.data_ptr()), None, None, None, None)
        assert rc == -1 and b"adapt_rounds" in lib.mdfit_last_error()
        with pytest.raises(_lib.MdfitError, match="adapt_rounds"):
            engine.map_pred_device(ty[:2], tN[:2], sub(0, 2), S, R, SEED, 0, adapt_rounds=rounds)
    # T = 1, 3
    for n in (1, 3):
        got = host(*engine.map_pred_device(ty[:n], tN[:n], sub(0, n), S, R, SEED, 0, **kw))
        assert same(got, [base[0][:n], base[1][:n], base[4][:n]]), n
    # two calls split with index_base
    a = engine.map_pred_device(ty[:30], tN[:30], sub(0, 30), S, R, SEED, 0, **kw)
    c = engine.map_pred_device(ty[30:], tN[30:], sub(30, T), S, R, SEED, 30, **kw)
    wrong = engine.map_pred_device(ty[30:], tN[30:], sub(30, T), S, R, SEED, 0, **kw)
    assert same(host(*(torch.cat([x, z]) for x, z in zip(a, c))), base[:2] + base[4:])
    assert not same(host(*wrong), [base[0][30:], base[1][30:], base[4][30:]])  # (the streams are the global taxon's)
    # after a poisoning of the LDS
    _lib.check(lib.mdfit_poison_lds(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert same(host(*engine.map_pred_device(ty, tN, sub(0, T), S, R, SEED, 0, **kw)), base[:2] + base[4:])
    # under graph capture and replay
    s = torch.cuda.Stream()
    dpp = torch.zeros((T, _lib.NPRED, _lib.NPOS), dtype=torch.float32, device=ty.device)
    drec = torch.zeros((T, _lib.NMAPPRED), dtype=torch.float64, device=ty.device)
    dad = torch.zeros((T, 3, _lib.NMAPADAPT), dtype=torch.float64, device=ty.device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        engine.map_pred_device(ty, tN, sub(0, T), S, R, SEED, 0, ppred=dpp, rec=drec, adapt=dad,
                               stream=torch.cuda.current_stream(), **kw)
    for _ in range(2):
        dpp.fill_(0.0)
        drec.fill_(0.0)
        dad.fill_(0.0)
        g.replay()
        assert same(host(dpp, drec, dad), base[:2] + base[4:])
    # out, pred and status are unchanged by all of it
    assert torch.equal(out0.view(torch.int64), res.out.view(torch.int64)) and torch.equal(st0, res.status)
    assert torch.equal(pred0.view(torch.int32), res.pred.view(torch.int32))
    # through the chunked dispatch in two chunks, and into the gather record of a world of one
    opts = _lib.default_opts(mode=_lib.MODE_MAP)
    want32 = np.concatenate([base[0].reshape(T, 90), base[1].astype(np.float32)], axis=1)
    want_ad = engine.adapt_summary(torch.from_numpy(base[4]).to(ty.device)).cpu().numpy()
    y, N, mm = b.y[:T], b.N[:T], b.mm[:T]
    monkeypatch.setenv("MDFIT_CHUNK_TAXA", "33")
    assert len(engine.plan_chunks(T, opts, with_ppred=True)) == 2
    o5, p5, s5, w5, a5 = engine.fit_batch_host(y, N, mm, opts, ppred=True, psis_draws=S, pred_draws=R,
                                               psis_adapt=ROUNDS)
    assert w5.shape == (T, engine.PPRED_WORDS) and a5.shape == (T, _lib.NADAPTOUT) and a5.dtype == np.float32
    assert np.array_equal(w5.view(np.int32), want32.view(np.int32))
    assert np.array_equal(a5.view(np.int32), want_ad.view(np.int32))
    plain4 = engine.fit_batch_host(y, N, mm, opts, ppred=True, psis_draws=S, pred_draws=R)
    assert len(plain4) == 4  # (no rounds: today's four arrays)
    for x, z in zip(plain4[:3], (o5, p5, s5)):
        assert x.dtype == z.dtype and np.array_equal(x, z, equal_nan=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    rec = d.alloc_records(T, dev, with_ppred=True, with_ppred_adapt=True)
    assert rec.buf.numel() == T * (d.REC_BYTES + d.REC_PPRED + d.REC_ADAPT)
    fitter = engine.ChunkedFitter(33, opts=opts, dest_on_device=True, with_ppred=True, psis_draws=S, pred_draws=R,
                                  psis_adapt=ROUNDS)
    fitter.run_into_device(y, N, mm, opts, engine.FitBatch(rec.out, rec.pred, rec.status, ppred=rec.ppred,
                                                           adapt=rec.adapt),
                           chunks=engine.plan_chunks(T, opts, chunk_taxa=33))
    buf = rec.stage()
    torch.cuda.synchronize()
    og, pg, sg, wg, ag = d.unpack_gathered(d.gather_records(buf, T, 0, 1), T, 1, with_ppred=True, with_ppred_adapt=True)
    assert np.array_equal(wg.view(np.int32), want32.view(np.int32))
    assert np.array_equal(ag.view(np.int32), want_ad.view(np.int32))
    assert np.array_equal(sg, s5) and np.array_equal(pg, p5, equal_nan=True)
