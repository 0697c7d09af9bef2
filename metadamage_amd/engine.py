"""Device-side entry points: PyTorch-ROCm tensors in, C-ABI call, tensors out.

PyTorch only provides device memory and the stream; every computation runs in
the HIP kernels of libmdfit.so (metadamage_amd/csrc/mdfit.hip).  There is no
CPU fallback: without a GPU these functions raise.
"""

from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from math import prod

import numpy as np

from . import _lib, blocks


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise _lib.MdfitError("no HIP device available: the mdfit engine runs on MI355X only")
    return torch


def _stream_handle(torch, stream=None) -> ctypes.c_void_p:
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


# --------------------------------------------------------------------------
# what every *_device wrapper shares: pointers, buffers, checks, the call
# --------------------------------------------------------------------------
def _ptr(t):
    """A tensor's device pointer for ctypes; None stays None (NULL)."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _buffer(torch, name: str, given, shape, dtype, device, required: bool = False):
    """An entry's output or tap: None stays None (required: allocated), True is
    allocated, a tensor must be contiguous, on the device, of dtype and of
    shape's size."""
    if given is True or (given is None and required):
        return torch.empty(shape, dtype=dtype, device=device)
    if given is not None and not (given.is_cuda and given.is_contiguous() and given.dtype == dtype
                                  and given.numel() == prod(shape)):
        kind = str(dtype).removeprefix("torch.")
        raise ValueError(f"{name} must be a contiguous cuda {kind} tensor of {prod(shape)} elements")
    return given


def _check_fit_inputs(torch, ty, tN, tm, T: int) -> None:
    """y, N (and mm, or None) as mdfit_fit_batch takes them."""
    for name, t in (("y", ty), ("N", tN)):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.int32 and tuple(t.shape) == (T, _lib.LD)):
            raise ValueError(f"{name} must be a contiguous cuda int32/uint32 view of shape [T, {_lib.LD}]")
    if tm is not None and not (tm.is_cuda and tm.is_contiguous() and tm.numel() == T * _lib.NPOS * _lib.NMM):
        raise ValueError("mm must be a contiguous cuda tensor of T*30*12 uint32")


def _check_counts(ty, tN, T: int) -> None:
    """y, N as the post-fit entries read them: the finished call's counts."""
    for name, a in (("y", ty), ("N", tN)):
        if not (a.is_cuda and a.is_contiguous() and a.element_size() == 4 and a.numel() >= T * _lib.LD):
            raise ValueError(f"{name} must be the call's contiguous cuda 32-bit counts [T, {_lib.LD}]")


def _check_records(res, T: int) -> None:
    """res as the MAP post-fit entries read it: exactly these T taxa's records."""
    if not (res.out.is_contiguous() and res.status.is_contiguous() and int(res.out.shape[0]) == T):
        raise ValueError("res must hold the contiguous records of these T taxa")


def _check_map(ty, tN, res, T: int) -> None:
    """The inputs of a MAP post-fit entry: (ty, tN, res, T)."""
    _check_counts(ty, tN, T)
    _check_records(res, T)


def _check_nuts(res, T: int, opts) -> None:
    """The inputs of a NUTS post-fit entry: the records of at least T taxa and,
    in the sampling mode, a workspace that holds their draws under opts."""
    if not (res.out.is_contiguous() and int(res.out.shape[0]) >= T):
        raise ValueError("res must hold the contiguous records of these T taxa")
    if int(opts.mode) == _lib.MODE_NUTS and (res.workspace is None or res.workspace.numel() < workspace_bytes(T, opts)):
        raise ValueError("res.workspace does not hold the draws of T taxa under opts")


def _map_is(torch, stem: str, head, keys, outputs, taps, adapt_rounds, adapt, stream):
    """Call a MAP importance-sampling entry, mdfit_map_<stem> or mdfit_map_<stem>_adapt.

    head: (y, N, res, T, S[, R]); keys: (seed, index_base[, d0]); outputs: the
    records; taps: the optional ones (None: NULL).  The _adapt entry runs when
    adapt_rounds != 0 or adapt is given (True: allocated; False: the rounds
    without their record, NULL); its argument list is the plain one with
    adapt_rounds behind the head and adapt behind the outputs (include/mdfit.h).
    Returns the outputs, the taps asked for and the adapt record -- the record
    itself when it is all there is."""
    ty, tN, res, T, *counts = head
    no_record = adapt is False
    adapt = None if no_record else adapt
    use_adapt = int(adapt_rounds) != 0 or adapt is not None
    if use_adapt and not no_record:
        adapt = _buffer(torch, "adapt", adapt, (T, 3, _lib.NMAPADAPT), torch.float64, ty.device, required=True)
    _check_map(ty, tN, res, T)
    args = [_ptr(ty), _ptr(tN), _ptr(res.out), _ptr(res.status), T, *counts]
    if use_adapt:
        args.append(int(adapt_rounds))
    args += [*keys, *map(_ptr, outputs)]
    if use_adapt:
        args.append(_ptr(adapt))
    fn = getattr(_lib.load(), f"mdfit_map_{stem}_adapt" if use_adapt else f"mdfit_map_{stem}")
    _lib.check(fn(*args, *map(_ptr, taps), _stream_handle(torch, stream)))
    got = (*outputs, *(t for t in taps if t is not None), *((adapt,) if adapt is not None else ()))
    return got[0] if len(got) == 1 else got


@dataclass
class FitBatch:
    """Device-resident results of one mdfit_fit_batch call."""

    out: "object"  # torch.float64 [T, NOUT]
    pred: "object"  # torch.float32 [T, 3, 30]
    status: "object"  # torch.int32 [T]
    workspace: "object" = None  # torch.uint8 [mdfit_workspace_bytes(T, opts)] (work queues; NUTS: the draws)
    # the run's one optional block, float32 [T, *shape] of its blocks.BLOCKS entry, under the entry's attr (ppred:
    # split_ppred; auto: fit_auto_chunks), and the tail blocks behind it:
    # adapt float32 [T, NADAPTOUT], largest round-0 khat, largest best round (psis_adapt > 0);
    # auto_pred float32 [T, NAUTOPRED], pred_ess_min, pred_distinct_min (auto with auto_pred);
    # ppc float32 [T, NPPCOUT] = ppos | rec, the posterior predictive check (ppred with ppc; split_ppc);
    # quant float32 [T, NQUANTOUT], the three rows of the weighted order statistics (psis with quantiles);
    # joint float32 [T, NJOINTOUT] = evid | psis, the fused launch's other two records (waic with joint; split_joint)
    lap: "object" = None
    diag: "object" = None
    summ: "object" = None
    loo: "object" = None
    psis: "object" = None
    waic: "object" = None
    ppred: "object" = None
    auto: "object" = None
    adapt: "object" = None
    auto_pred: "object" = None
    evid: "object" = None
    ppc: "object" = None
    quant: "object" = None
    joint: "object" = None


def to_device_counts(y, N, mm=None, device="cuda"):
    """Host uint32 arrays -> device tensors in the engine's dense layout."""
    torch = _torch()
    y = np.ascontiguousarray(y, dtype=np.uint32)
    N = np.ascontiguousarray(N, dtype=np.uint32)
    if y.ndim != 2 or y.shape[1] != _lib.LD or N.shape != y.shape:
        raise ValueError(f"y, N must be uint32[T][{_lib.LD}], got {y.shape} / {N.shape}")
    ty = torch.from_numpy(y.view(np.int32)).to(device)
    tN = torch.from_numpy(N.view(np.int32)).to(device)
    tm = None
    if mm is not None:
        mm = np.ascontiguousarray(mm, dtype=np.uint32)
        if mm.shape != (y.shape[0], _lib.NPOS, _lib.NMM):
            raise ValueError(f"mm must be uint32[T][30][12], got {mm.shape}")
        tm = torch.from_numpy(mm.view(np.int32)).to(device)
    return ty, tN, tm


def alloc_outputs(n_taxa: int, device="cuda", with_pred: bool = True, opts: _lib.MdfitOpts | None = None) -> FitBatch:
    torch = _torch()
    out = torch.empty((n_taxa, _lib.NOUT), dtype=torch.float64, device=device)
    pred = (
        torch.empty((n_taxa, _lib.NPRED, _lib.NPOS), dtype=torch.float32, device=device)
        if with_pred
        else None
    )
    status = torch.empty((n_taxa,), dtype=torch.int32, device=device)
    return FitBatch(out, pred, status, alloc_workspace(n_taxa, device, opts))


def workspace_bytes(n_taxa: int, opts: _lib.MdfitOpts | None = None) -> int:
    lib = _lib.load()
    return int(lib.mdfit_workspace_bytes(int(n_taxa), ctypes.byref(opts) if opts is not None else None))


def alloc_workspace(n_taxa: int, device="cuda", opts: _lib.MdfitOpts | None = None):
    """Device scratch mdfit_fit_batch needs for n_taxa taxa under opts (work
    queues; in the sampling mode also every chain's draws)."""
    torch = _torch()
    return torch.empty((workspace_bytes(n_taxa, opts),), dtype=torch.uint8, device=device)


def samples_view(res: FitBatch, n_taxa: int, opts: _lib.MdfitOpts):
    """The sampling mode's draws in the workspace: float64 [T][6][S][4] = (q, A, c, phi)."""
    torch = _torch()
    S = int(opts.num_samples)
    n = n_taxa * 6 * S * 4
    return res.workspace[_lib.SAMPLES_OFFSET:_lib.SAMPLES_OFFSET + 8 * n].view(torch.float64).view(n_taxa, 6, S, 4)


def fit_batch_device(ty, tN, tm=None, opts: _lib.MdfitOpts | None = None, res: FitBatch | None = None,
                     stream=None) -> FitBatch:
    """Launch mdfit_fit_batch on device tensors (asynchronous on `stream`)."""
    torch = _torch()
    lib = _lib.load()
    T = int(ty.shape[0])
    _check_fit_inputs(torch, ty, tN, tm, T)
    if res is None:
        res = alloc_outputs(T, device=ty.device, opts=opts)
    o = opts if opts is not None else _lib.default_opts()
    if res.workspace is None or res.workspace.numel() < workspace_bytes(T, o):
        res.workspace = alloc_workspace(T, ty.device, o)
    _lib.check(lib.mdfit_fit_batch(_ptr(ty), _ptr(tN), _ptr(tm), T, ctypes.byref(o), _ptr(res.out), _ptr(res.pred),
                                   _ptr(res.status), _ptr(res.workspace), _stream_handle(torch, stream)))
    return res


def map_laplace_device(ty, tN, res: FitBatch, lap=None, gh=None, stream=None, u=None):
    """Launch mdfit_map_laplace on the records of a finished MAP call
    (asynchronous on `stream`): the Laplace standard errors of the three PMD
    sub-fits, float64 lap[T, 3, NLAPLACE] (_lib.LAPLACE_FIELDS).  gh
    (float64[T, 3, 20], optional) receives g[4] then H[4][4] at the rebuilt
    mode and u (float64[T, 3, 4], optional; mdfit_map_laplace_u) that mode itself
    (parity tests).  Returns lap."""
    torch = _torch()
    lib = _lib.load()
    T = int(ty.shape[0])
    lap = _buffer(torch, "lap", lap, (T, 3, _lib.NLAPLACE), torch.float64, ty.device, required=True)
    _buffer(torch, "gh", gh, (T, 3, 20), torch.float64, ty.device)
    _buffer(torch, "u", u, (T, 3, 4), torch.float64, ty.device)
    _check_records(res, T)
    args = [_ptr(ty), _ptr(tN), _ptr(res.out), _ptr(res.status), T, _ptr(lap), _ptr(gh)]
    if u is not None:
        _lib.check(lib.mdfit_map_laplace_u(*args, _ptr(u), _stream_handle(torch, stream)))
    else:
        _lib.check(lib.mdfit_map_laplace(*args, _stream_handle(torch, stream)))
    return lap


def map_psis_device(ty, tN, res: FitBatch, num_draws: int = 256, seed: int = 0, index_base: int = 0, psis=None,
                    draws=None, stream=None, adapt_rounds: int = 0, adapt=None):
    """Launch mdfit_map_psis on the records of a finished MAP call (asynchronous
    on `stream`): the importance-sampled posterior of the three PMD sub-fits
    (MDFIT-PSIS v1), float64 psis[T, 3, NMAPPSIS] (_lib.MAPPSIS_FIELDS).  The
    Philox streams are keyed by (seed, index_base + taxon, sub-fit).  draws:
    None, True (allocated) or a float64 tensor [T, 3, num_draws, 6] = u[4], the
    raw log-weight, the weight.  Returns psis, or (psis, draws) when draws is
    asked for.

    adapt_rounds > 0, or adapt given (True: allocated, or a float64 tensor [T, 3,
    NMAPADAPT]): mdfit_map_psis_adapt (MDFIT-ADAPT v1) with at most adapt_rounds
    moment-matched proposal rounds per row; the adapt block (_lib.MAPADAPT_FIELDS)
    is then the last element of the returned tuple, and draws are the best
    round's."""
    torch = _torch()
    T, S, dev = int(ty.shape[0]), int(num_draws), ty.device
    psis = _buffer(torch, "psis", psis, (T, 3, _lib.NMAPPSIS), torch.float64, dev, required=True)
    draws = _buffer(torch, "draws", draws, (T, 3, S, 6), torch.float64, dev)
    return _map_is(torch, "psis", (ty, tN, res, T, S), (int(seed), int(index_base)), (psis,), (draws,),
                   adapt_rounds, adapt, stream)


def map_quant_device(ty, tN, res: FitBatch, num_draws: int = 256, seed: int = 0, index_base: int = 0,
                     d0: float = 0.01, quant=None, values=None, stream=None, adapt_rounds: int = 0, adapt=None):
    """Launch mdfit_map_quant on the records of a finished MAP call (asynchronous
    on `stream`): the weighted median, 68 % HPDI, quantiles and P(D_max > d0) of
    the importance-sampled posterior of the three PMD sub-fits (MDFIT-QUANT v1),
    float64 quant[T, 3, NMAPQUANT] (_lib.MAPQUANT_FIELDS).  The draws, weights,
    khat, ess and flags are map_psis_device's at the same (seed, index_base,
    num_draws, adapt_rounds).  values: None, True (allocated) or a float64
    tensor [T, 3, num_draws, 6] = D_max, q, A, c, phi and the smoothed weight of
    each draw.  Returns quant, or (quant, values) when values is asked for.

    adapt_rounds > 0, or adapt given (True, or a float64 tensor [T, 3,
    NMAPADAPT]): mdfit_map_quant_adapt; the adapt block is then the last element
    of the returned tuple.  adapt=False: the rounds without their record (the
    chunked dispatch, whose map_psis launch has written it)."""
    torch = _torch()
    T, S, dev = int(ty.shape[0]), int(num_draws), ty.device
    quant = _buffer(torch, "quant", quant, (T, 3, _lib.NMAPQUANT), torch.float64, dev, required=True)
    values = _buffer(torch, "values", values, (T, 3, S, 6), torch.float64, dev)
    return _map_is(torch, "quant", (ty, tN, res, T, S), (int(seed), int(index_base), float(d0)), (quant,), (values,),
                   adapt_rounds, adapt, stream)


def weighted_order_stats(v, w, d0: float = 0.01, device="cuda"):
    """res[n, 8] float64 (host) = median, lo, hi, q05, q95, p_above, n_window, ok
    of the series v[n, S] under the weights w[n, S] by the device's weighted
    order statistics (MDFIT-QUANT v1, mdfit_weighted_order_stats)."""
    torch = _torch()
    lib = _lib.load()
    tv = torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device=device)
    tw = torch.as_tensor(np.ascontiguousarray(w, dtype=np.float64), device=device)
    n, S = int(tv.shape[0]), int(tv.shape[1])
    if tuple(tw.shape) != (n, S):
        raise ValueError("v and w must have one shape [n, S]")
    res = torch.empty((n, _lib.NQUANTRES), dtype=torch.float64, device=device)
    _lib.check(lib.mdfit_weighted_order_stats(ctypes.c_void_p(tv.data_ptr()), ctypes.c_void_p(tw.data_ptr()), n, S,
                                              float(d0), ctypes.c_void_p(res.data_ptr()),
                                              _stream_handle(torch, None)))
    return res.cpu().numpy()


def map_waic_device(ty, tN, res: FitBatch, num_draws: int = 256, seed: int = 0, index_base: int = 0, waic=None,
                    pointwise=None, draws=None, stream=None, adapt_rounds: int = 0, adapt=None):
    """Launch mdfit_map_waic on the records of a finished MAP call (asynchronous
    on `stream`): the importance-weighted WAIC of the six sub-fits and the
    reference's comparisons on it (MDFIT-WAIC v1), float64 waic[T, 7, NMAPWAIC]
    (_lib.MAPWAIC_FIELDS; row 6 _lib.MAPWAIC_COMPARE_FIELDS).  The Philox
    streams are keyed by (seed, index_base + taxon, sub-fit).  pointwise: None,
    True (allocated) or a float64 tensor [T, 6, 30, 2] = (lppd_i, p_i); draws:
    None, True or a float64 tensor [T, 6, num_draws, 6] = u[4], the raw
    log-weight, the weight.  Returns waic, or the tuple (waic[, pointwise][,
    draws]) of what was asked for.

    adapt_rounds > 0, or adapt given (True, or a float64 tensor [T, 3,
    NMAPADAPT]): mdfit_map_waic_adapt, the PMD rows with mdfit_map_psis_adapt's
    rounds; the adapt block is then the last element of the returned tuple."""
    torch = _torch()
    T, S, dev = int(ty.shape[0]), int(num_draws), ty.device
    waic = _buffer(torch, "waic", waic, (T, _lib.NWAICROW, _lib.NMAPWAIC), torch.float64, dev, required=True)
    pointwise = _buffer(torch, "pointwise", pointwise, (T, _lib.NSUBFIT, _lib.NPOS, 2), torch.float64, dev)
    draws = _buffer(torch, "draws", draws, (T, _lib.NSUBFIT, S, 6), torch.float64, dev)
    return _map_is(torch, "waic", (ty, tN, res, T, S), (int(seed), int(index_base)), (waic,), (pointwise, draws),
                   adapt_rounds, adapt, stream)


def map_evidence_device(ty, tN, res: FitBatch, num_draws: int = 256, seed: int = 0, index_base: int = 0, evid=None,
                        draws=False, adapt_rounds: int = 0, adapt=None, stream=None):
    """Launch mdfit_map_evidence on the records of a finished MAP call
    (asynchronous on `stream`): the importance-sampled marginal likelihood of
    the six sub-fits and the Bayes factors PMD : null on it (MDFIT-EVID v1),
    float64 evid[T, 7, NMAPEVID] (_lib.MAPEVID_FIELDS; row 6
    _lib.MAPEVID_COMPARE_FIELDS).  The Philox streams are keyed by (seed,
    index_base + taxon, sub-fit).  draws: False / None, True (allocated) or a
    float64 tensor [T, 6, num_draws, 6] = u[4], the raw log-weight, the weight.
    Returns evid, or the tuple (evid[, draws]) of what was asked for.

    adapt_rounds > 0, or adapt given (True, or a float64 tensor [T, 3,
    NMAPADAPT]): mdfit_map_evidence_adapt, the PMD rows with
    mdfit_map_psis_adapt's rounds; the adapt block is then the last element of
    the returned tuple."""
    torch = _torch()
    T, S, dev = int(ty.shape[0]), int(num_draws), ty.device
    evid = _buffer(torch, "evid", evid, (T, _lib.NEVIDROW, _lib.NMAPEVID), torch.float64, dev, required=True)
    draws = _buffer(torch, "draws", None if draws is False else draws, (T, _lib.NSUBFIT, S, 6), torch.float64, dev)
    return _map_is(torch, "evidence", (ty, tN, res, T, S), (int(seed), int(index_base)), (evid,), (draws,),
                   adapt_rounds, adapt, stream)


def map_joint_device(ty, tN, res: FitBatch, num_draws: int = 256, seed: int = 0, index_base: int = 0, waic=None,
                     evid=None, psis=None, pointwise=None, draws=None, stream=None, adapt_rounds: int = 0,
                     adapt=None):
    """Launch mdfit_map_joint on the records of a finished MAP call (asynchronous
    on `stream`): one launch that forms each sub-fit's weights once and writes
    float64 waic[T, 7, NMAPWAIC], evid[T, 7, NMAPEVID] and psis[T, 3, NMAPPSIS],
    the records of map_waic_device, map_evidence_device and map_psis_device at
    the same (num_draws, seed, index_base, adapt_rounds) bit for bit.  pointwise
    and draws: as map_waic_device's.  Returns (waic, evid, psis[, pointwise][,
    draws]).

    adapt_rounds > 0, or adapt given (True, or a float64 tensor [T, 3,
    NMAPADAPT]): mdfit_map_joint_adapt; the adapt block is then the last element
    of the returned tuple."""
    torch = _torch()
    T, S, dev = int(ty.shape[0]), int(num_draws), ty.device
    waic = _buffer(torch, "waic", waic, (T, _lib.NWAICROW, _lib.NMAPWAIC), torch.float64, dev, required=True)
    evid = _buffer(torch, "evid", evid, (T, _lib.NEVIDROW, _lib.NMAPEVID), torch.float64, dev, required=True)
    psis = _buffer(torch, "psis", psis, (T, 3, _lib.NMAPPSIS), torch.float64, dev, required=True)
    pointwise = _buffer(torch, "pointwise", pointwise, (T, _lib.NSUBFIT, _lib.NPOS, 2), torch.float64, dev)
    draws = _buffer(torch, "draws", draws, (T, _lib.NSUBFIT, S, 6), torch.float64, dev)
    return _map_is(torch, "joint", (ty, tN, res, T, S), (int(seed), int(index_base)), (waic, evid, psis),
                   (pointwise, draws), adapt_rounds, adapt, stream)


def fit_batch_indexed_device(ty, tN, tm, taxon_index, opts: _lib.MdfitOpts, res: FitBatch | None = None,
                             stream=None) -> FitBatch:
    """Launch mdfit_fit_batch_indexed on device tensors (asynchronous on
    `stream`): the sampling call whose row t draws from the streams of the
    global taxon opts.index_base + taxon_index[t] (int64 [T] on the device, or
    None: mdfit_fit_batch itself), so that rows idx of a batch fitted with
    taxon_index = idx are the rows idx of the full call bit for bit."""
    torch = _torch()
    lib = _lib.load()
    T = int(ty.shape[0])
    _check_fit_inputs(torch, ty, tN, tm, T)
    if taxon_index is not None:
        if not (taxon_index.is_cuda and taxon_index.is_contiguous() and taxon_index.dtype == torch.int64
                and taxon_index.numel() == T):
            raise ValueError("taxon_index must be a contiguous cuda int64 tensor of T entries")
    if res is None:
        res = alloc_outputs(T, device=ty.device, opts=opts)
    if res.workspace is None or res.workspace.numel() < workspace_bytes(T, opts):
        res.workspace = alloc_workspace(T, ty.device, opts)
    if not (res.out.is_contiguous() and res.status.is_contiguous() and int(res.out.shape[0]) >= T
            and (res.pred is None or res.pred.is_contiguous())):
        raise ValueError("res must hold contiguous records of at least T taxa")
    _lib.check(lib.mdfit_fit_batch_indexed(_ptr(ty), _ptr(tN), _ptr(tm), T, _ptr(taxon_index), ctypes.byref(opts),
                                           _ptr(res.out), _ptr(res.pred), _ptr(res.status), _ptr(res.workspace),
                                           _stream_handle(torch, stream)))
    return res


def auto_route_device(res: FitBatch, psis, waic, route=None, stream=None):
    """Launch mdfit_auto_route on the records of a finished MAP call and its
    mdfit_map_psis / mdfit_map_waic records (float64 [T, 3, NMAPPSIS] and [T, 7,
    NMAPWAIC]; asynchronous on `stream`): writes route int32 [T] (_lib.ROUTE_*)
    and composes res.out's row of every taxon with route 0 in place.  Returns
    route."""
    torch = _torch()
    T = int(res.out.shape[0])
    route = _route_inputs(torch, res, T, route, (("psis", psis, (T, 3, _lib.NMAPPSIS), torch.float64),
                                                 ("waic", waic, (T, _lib.NWAICROW, _lib.NMAPWAIC), torch.float64)))
    _lib.check(_lib.load().mdfit_auto_route(_ptr(res.status), _ptr(psis), _ptr(waic), T, _ptr(res.out), _ptr(route),
                                            _stream_handle(torch, stream)))
    return route


def _route_inputs(torch, res, T: int, route, records):
    """The checks the two routing entries share: the given records (name, tensor, shape, dtype), the route tensor
    (None: allocated; returned) and res."""
    for name, t, shape, dtype in records:
        if t is None:
            raise ValueError(f"{name} is required")
        _buffer(torch, name, t, shape, dtype, res.out.device)
    route = _buffer(torch, "route", route, (T,), torch.int32, res.out.device, required=True)
    if not (res.out.is_contiguous() and res.status.is_contiguous() and res.status.numel() == T):
        raise ValueError("res must hold the contiguous records of these T taxa")
    return route


def auto_route_pred_device(res: FitBatch, psis, waic, prec, ppred, route=None, stream=None):
    """Launch mdfit_auto_route_pred (MDFIT-AUTO v1.1): auto_route_device with the
    records of mdfit_map_pred_adapt -- prec float64 [T, NMAPPRED], ppred float32
    [T, 3, 30] -- in the rule (_lib.ROUTE_PRED) and the composition: a taxon with
    route 0 also gets its five predictive columns from prec and, where res.pred
    is not None, its 90 prediction floats from ppred.  Returns route."""
    torch = _torch()
    T = int(res.out.shape[0])
    route = _route_inputs(torch, res, T, route, (("psis", psis, (T, 3, _lib.NMAPPSIS), torch.float64),
                                                 ("waic", waic, (T, _lib.NWAICROW, _lib.NMAPWAIC), torch.float64),
                                                 ("prec", prec, (T, _lib.NMAPPRED), torch.float64),
                                                 ("ppred", ppred, (T, _lib.NPRED, _lib.NPOS), torch.float32)))
    if res.pred is not None and not (res.pred.is_contiguous() and res.pred.dtype == torch.float32
                                     and res.pred.numel() == T * _lib.NPRED * _lib.NPOS):
        raise ValueError("res.pred must be a contiguous float32 tensor [T, 3, 30]")
    _lib.check(_lib.load().mdfit_auto_route_pred(_ptr(res.status), _ptr(psis), _ptr(waic), _ptr(prec), _ptr(ppred), T,
                                                 _ptr(res.out), _ptr(res.pred), _ptr(route),
                                                 _stream_handle(torch, stream)))
    return route


AUTO_BYTES = _lib.NAUTO * 4  # one taxon's auto block on the way out: f32 (route, sampled, khat_max, ess_min)
AUTO_STAGES = ("map", "psis", "waic", "route", "gather", "sampler", "scatter")
AUTO_PRED_BYTES = _lib.NAUTOPRED * 4  # one taxon's auto-pred block on the way out: f32 (pred_ess_min, pred_distinct_min)


def auto_opts(opts: _lib.MdfitOpts | None):
    """The two option sets of an auto call, copies of one (None: the defaults):
    (MAP, NUTS) -- mode differs; max_iter / tol_step, seed / num_warmup /
    num_samples and index_base are shared."""
    o = opts if opts is not None else _lib.default_opts()
    o_map, o_nuts = _lib.MdfitOpts.from_buffer_copy(o), _lib.MdfitOpts.from_buffer_copy(o)
    o_map.mode, o_nuts.mode = _lib.MODE_MAP, _lib.MODE_NUTS
    return o_map, o_nuts


def adapt_summary(adapt, out=None):
    """The adapt block that leaves the device, float32 [T, NADAPTOUT], from the
    adapt record float64 [T, 3, NMAPADAPT], reduced on the device: the largest
    round-0 khat and the largest best round over the taxon's valid PMD rows (NaN
    when it has none)."""
    torch = _torch()
    neg = torch.nan_to_num(adapt[:, :, [0, 2]], nan=-float("inf")).amax(dim=1)
    neg = torch.where(torch.isneginf(neg), torch.full_like(neg, float("nan")), neg)
    if out is None:
        return neg.to(torch.float32)
    out.copy_(neg)
    return out


def fit_auto_device(ty, tN, tm=None, opts: _lib.MdfitOpts | None = None, psis_draws: int = 256,
                    res: FitBatch | None = None, stream=None, budget_bytes: int | None = None,
                    sub_chunk_taxa: int = 0, timings: dict | None = None, psis_adapt: int = 0,
                    auto_pred: bool = False, pred_draws: int | None = None):
    """The auto inference of a device-resident batch (MDFIT-AUTO v1, DESIGN.md
    §3.10): the MAP fit, mdfit_map_psis and mdfit_map_waic with psis_draws draws
    per sub-fit, mdfit_auto_route -- which composes the record of every taxon
    the importance sampling settles -- and then the sampler over the others
    alone: idx = nonzero(route & ROUTE_SAMPLE), the rows idx of y, N, mm
    gathered, mdfit_fit_batch_indexed with taxon_index = idx and the batch's
    index_base (so a sampled row is the row of the plain NUTS call over the
    whole batch bit for bit), in sub-chunks sized by plan_chunks' budget for the
    sampler (budget_bytes, default default_budget; sub_chunk_taxa > 0 caps
    them) whose workspace is the sub-chunk's, not the batch's, and the records,
    predictions and status scattered back.  opts: one option set for both fits
    (auto_opts; its mode is ignored).  An empty subset launches no sampler.

    Taking idx reads the route on the host: the call's one host
    synchronisation, so it cannot be captured in a graph.  Everything runs on
    `stream` (default: the current stream).

    Returns (res, route int32 [T], auto float32 [T, NAUTO] = route, sampled 0/1,
    khat_max, ess_min -- row 6 fields 4, 5 of the waic record).  psis_adapt > 0:
    both launches run at most that many moment-matched proposal rounds per PMD
    row (MDFIT-ADAPT v1; the routing rule is untouched) and res.adapt is the
    float32 [T, NADAPTOUT] block of adapt_summary.  timings (a
    dict): filled with the milliseconds of each of AUTO_STAGES, n_sampled and
    n_sub_chunks (adds a synchronisation at the end).

    auto_pred (MDFIT-AUTO v1.1): after the waic launch,
    mdfit_map_pred_adapt on the whole batch with psis_draws, psis_adapt, the
    call's seed and index_base and pred_draws predictive draws per job (default
    PRED_DRAWS); mdfit_auto_route_pred in place of mdfit_auto_route, so a settled
    taxon's five predictive columns and res.pred (which must exist) are the
    importance-weighted posterior predictive, and idx = nonzero(route &
    ROUTE_SAMPLE_PRED).  res.auto_pred is the float32 [T, NAUTOPRED] block
    (pred_ess_min, pred_distinct_min over the three rows; NaN for a sampled
    taxon), and timings gains "pred".  False: nothing of this is launched."""
    torch = _torch()
    T = int(ty.shape[0])
    dev = ty.device
    auto_pred = bool(auto_pred)
    n_pred = int(pred_draws) if pred_draws is not None else PRED_DRAWS
    sample_mask = _lib.ROUTE_SAMPLE_PRED if auto_pred else _lib.ROUTE_SAMPLE
    o_map, o_nuts = auto_opts(opts)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    marks = []

    def mark(name):
        if timings is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record(s)
            marks.append((name, ev))

    with torch.cuda.stream(s):
        if res is None:
            res = alloc_outputs(T, device=dev, opts=o_map)
        if res.workspace is None or res.workspace.numel() < workspace_bytes(T, o_map):
            res.workspace = alloc_workspace(T, dev, o_map)
        if auto_pred and res.pred is None:
            raise ValueError("auto_pred composes the prediction rows: res.pred must exist")
        mark("start")
        fit_batch_device(ty, tN, tm, o_map, res, stream=s)
        mark("map")
        if int(psis_adapt) > 0:  # (MDFIT-ADAPT v1 in both launches: their PMD rows agree bit for bit)
            psis, ad = map_psis_device(ty, tN, res, psis_draws, int(o_map.seed), int(o_map.index_base), stream=s,
                                       adapt_rounds=psis_adapt)
            mark("psis")
            waic, _ = map_waic_device(ty, tN, res, psis_draws, int(o_map.seed), int(o_map.index_base), stream=s,
                                      adapt_rounds=psis_adapt, adapt=ad)
            mark("waic")
            res.adapt = adapt_summary(ad)
            del ad
        else:
            psis = map_psis_device(ty, tN, res, psis_draws, int(o_map.seed), int(o_map.index_base), stream=s)
            mark("psis")
            waic = map_waic_device(ty, tN, res, psis_draws, int(o_map.seed), int(o_map.index_base), stream=s)
            mark("waic")
        if auto_pred:
            got = map_pred_device(ty, tN, res, psis_draws, n_pred, int(o_map.seed), int(o_map.index_base), stream=s,
                                  adapt_rounds=int(psis_adapt))
            ppred, prec = got[0], got[1]
            mark("pred")
            route = auto_route_pred_device(res, psis, waic, prec, ppred, stream=s)
        else:
            route = auto_route_device(res, psis, waic, stream=s)
        mark("route")
        idx = torch.nonzero(route & sample_mask).reshape(-1)  # (the host synchronisation: its size)
        n = int(idx.numel())
        auto = torch.empty((T, _lib.NAUTO), dtype=torch.float32, device=dev)
        auto[:, 0] = route
        auto[:, 1] = (route & sample_mask) != 0
        auto[:, 2:4] = waic[:, 6, 4:6]
        if auto_pred:
            ap = torch.stack((prec[:, 8:11].amin(dim=1), prec[:, 11:14].amin(dim=1)), dim=1)
            ap[(route & sample_mask) != 0] = float("nan")
            res.auto_pred = ap.to(torch.float32)
            del ppred, prec, got, ap
        del psis, waic
        chunks = []
        t_gather = t_sampler = t_scatter = 0.0
        if n > 0:
            budget = budget_bytes if budget_bytes is not None else default_budget(dev)
            chunks = plan_chunks(n, o_nuts, budget, chunk_taxa=sub_chunk_taxa, n_sets=1, with_mm=tm is not None,
                                 with_pred=res.pred is not None)
            cap = max(hi - lo for lo, hi in chunks)
            sub = alloc_outputs(cap, device=dev, with_pred=res.pred is not None, opts=o_nuts)
            for lo, hi in chunks:
                m = hi - lo
                sel = idx[lo:hi].contiguous()
                sy, sN = ty.index_select(0, sel), tN.index_select(0, sel)
                sm = tm.reshape(T, _lib.NPOS, _lib.NMM).index_select(0, sel) if tm is not None else None
                mark("gather")
                part = FitBatch(sub.out[:m], sub.pred[:m] if sub.pred is not None else None, sub.status[:m],
                                sub.workspace)
                fit_batch_indexed_device(sy, sN, sm, sel, o_nuts, part, stream=s)
                mark("sampler")
                res.out.index_copy_(0, sel, part.out)
                if res.pred is not None:
                    res.pred.index_copy_(0, sel, part.pred)
                res.status.index_copy_(0, sel, part.status)
                mark("scatter")
        if timings is not None:
            s.synchronize()
            for name in AUTO_STAGES + (("pred",) if auto_pred else ()):
                timings[name] = 0.0
            for (_, e0), (name, e1) in zip(marks[:-1], marks[1:]):
                timings[name] += e0.elapsed_time(e1)
            timings["n_sampled"], timings["n_sub_chunks"], timings["n_taxa"] = n, len(chunks), T
    return res, route, auto


def fit_auto_chunks(y, N, mm, opts: _lib.MdfitOpts | None = None, psis_draws: int = 256, device="cuda",
                    dest: FitBatch | None = None, budget_bytes: int | None = None, psis_adapt: int = 0,
                    auto_pred: bool = False, pred_draws: int | None = None):
    """fit_auto_device over host counts (uint32 y, N [T, LD], mm [T, 30, 12] or
    None) chunk by chunk: the chunks of plan_chunks under the device budget
    (MDFIT_CHUNK_TAXA caps them), each with its global index_base, so any split
    gives the records of one call bit for bit.  dest (device out [T, NOUT], pred,
    status, auto f32 [T, NAUTO]): the rows are written in place and dest is
    returned; None: host arrays (out[T, 25] f64, pred, status, auto) are.  The
    chunks run one after another -- a chunk's two passes are separated by a host
    synchronisation -- with no transfer overlap.  psis_adapt > 0: passed to
    fit_auto_device; dest.adapt (f32 [T, NADAPTOUT]) is written too, or one more
    host array returned, last.  auto_pred (with pred_draws): passed to
    fit_auto_device; dest.auto_pred (f32 [T, NAUTOPRED]) is written too, or one
    more host array returned behind auto and before adapt."""
    torch = _torch()
    T = int(y.shape[0])
    dev = torch.device(device)
    o_map, _ = auto_opts(opts)
    parts = blocks.describe(None, {"psis_adapt": psis_adapt, "auto_pred": auto_pred}, psis_draws=psis_draws,
                            pred_draws=pred_draws, with_auto=True).parts  # (auto, then the tails asked for)
    budget = budget_bytes if budget_bytes is not None else default_budget(dev)
    # (the MAP pass's buffers, its psis and waic records beside them: two sets' worth is an upper bound)
    chunks = plan_chunks(T, o_map, budget, with_mm=mm is not None, dest_on_device=dest is not None, with_waic=True)
    if dest is None:
        h_out = np.empty((T, H_OUT_COLS), np.float64)
        h_pred = np.empty((T, _lib.NPRED, _lib.NPOS), np.float32)
        h_status = np.empty((T,), np.int32)
        h_parts = {p.attr: np.empty((T, *p.shape), np.float32) for p in parts}
    for lo, hi in chunks:
        ty, tN, tm = to_device_counts(y[lo:hi], N[lo:hi], mm[lo:hi] if mm is not None else None, device=dev)
        o = _lib.MdfitOpts.from_buffer_copy(o_map)
        o.index_base = o_map.index_base + lo
        res = None
        if dest is not None:
            res = FitBatch(dest.out[lo:hi], dest.pred[lo:hi] if dest.pred is not None else None, dest.status[lo:hi])
        res, _route, auto = fit_auto_device(ty, tN, tm, o, psis_draws, res=res, budget_bytes=budget_bytes,
                                            psis_adapt=psis_adapt, auto_pred=auto_pred, pred_draws=pred_draws)
        res.auto = auto  # (beside res.auto_pred and res.adapt, which fit_auto_device has set)
        for p in parts:
            if dest is not None:
                getattr(dest, p.attr)[lo:hi].copy_(getattr(res, p.attr))
            else:
                h_parts[p.attr][lo:hi] = getattr(res, p.attr).cpu().numpy()
        if dest is None:
            h_out[lo:hi] = res.out[:, :H_OUT_COLS].cpu().numpy()
            h_pred[lo:hi] = res.pred.cpu().numpy()
            h_status[lo:hi] = res.status.cpu().numpy()
    if dest is not None:
        return dest
    return (h_out, h_pred, h_status, *h_parts.values())


def map_pred_device(ty, tN, res: FitBatch, num_draws: int = 256, num_pred: int = 1000, seed: int = 0,
                    index_base: int = 0, ppred=None, rec=None, index=None, counts=None, stream=None,
                    adapt_rounds: int = 0, adapt=None):
    """Launch mdfit_map_pred on the records of a finished MAP call (asynchronous
    on `stream`): the reference's posterior predictive from importance-weighted
    draws (MDFIT-PPRED v1): float32 ppred[T, 3, 30] in pred's layout and float64
    rec[T, NMAPPRED] (_lib.MAPPRED_FIELDS).  The Philox streams are keyed by
    (seed, index_base + taxon, sub-fit).  index: None, True (allocated) or an
    int32 tensor [T, 3, num_pred], the importance draw each predictive draw
    took; counts: None, True or an int32 tensor [T, 32, num_pred] holding the
    unsorted counts of each job as uint32 (0xFFFFFFFF: no count or job not run).
    Returns (ppred, rec[, index][, counts]).

    adapt_rounds > 0, or adapt given (True, or a float64 tensor [T, 3,
    NMAPADAPT]): mdfit_map_pred_adapt (MDFIT-AUTO v1.1), each row with
    mdfit_map_psis_adapt's rounds and the predictive drawn from the best round;
    the adapt block is then the last element of the returned tuple."""
    torch = _torch()
    T, S, R, dev = int(ty.shape[0]), int(num_draws), int(num_pred), ty.device
    ppred = _buffer(torch, "ppred", ppred, (T, _lib.NPRED, _lib.NPOS), torch.float32, dev, required=True)
    rec = _buffer(torch, "rec", rec, (T, _lib.NMAPPRED), torch.float64, dev, required=True)
    index = _buffer(torch, "index", index, (T, 3, R), torch.int32, dev)
    counts = _buffer(torch, "counts", counts, (T, _lib.NPREDJOB, R), torch.int32, dev)
    return _map_is(torch, "pred", (ty, tN, res, T, S, R), (int(seed), int(index_base)), (ppred, rec), (index, counts),
                   adapt_rounds, adapt, stream)


def map_ppc_device(ty, tN, res: FitBatch, num_draws: int = 256, num_pred: int = 1000, seed: int = 0,
                   index_base: int = 0, ppos=None, rec=None, index=None, counts=None, disc=None, stream=None,
                   adapt_rounds: int = 0, adapt=None):
    """Launch mdfit_map_ppc on the records of a finished MAP call (asynchronous
    on `stream`): the posterior predictive check of the PMD fit on all positions
    (MDFIT-PPC v1): float32 ppos[T, 30], the upper mid-p of each column, and
    float64 rec[T, NMAPPPC] (_lib.MAPPPC_FIELDS).  The streams, the importance
    draws and the replicated counts are map_pred_device's row 0 at the same
    (seed, index_base, num_draws, num_pred).  index: None, True (allocated) or
    an int32 tensor [T, num_pred]; counts: None, True or an int32 tensor [T, 30,
    num_pred] holding the replicated counts as uint32 (0xFFFFFFFF: no count);
    disc: None, True or a float64 tensor [T, num_pred, 4] = T_out(obs),
    T_out(rep), T_str(obs), T_str(rep).  Returns (ppos, rec[, index][, counts]
    [, disc]).

    adapt_rounds > 0, or adapt given (True, or a float64 tensor [T, 3,
    NMAPADAPT]): mdfit_map_ppc_adapt; the adapt block (rows 1 and 2 NaN) is then
    the last element of the returned tuple.  adapt=False: the rounds without
    their record (the chunked dispatch, whose map_pred launch has written it)."""
    torch = _torch()
    T, S, R, dev = int(ty.shape[0]), int(num_draws), int(num_pred), ty.device
    ppos = _buffer(torch, "ppos", ppos, (T, _lib.NPOS), torch.float32, dev, required=True)
    rec = _buffer(torch, "rec", rec, (T, _lib.NMAPPPC), torch.float64, dev, required=True)
    index = _buffer(torch, "index", index, (T, R), torch.int32, dev)
    counts = _buffer(torch, "counts", counts, (T, _lib.NPOS, R), torch.int32, dev)
    disc = _buffer(torch, "disc", disc, (T, R, 4), torch.float64, dev)
    return _map_is(torch, "ppc", (ty, tN, res, T, S, R), (int(seed), int(index_base)), (ppos, rec),
                   (index, counts, disc), adapt_rounds, adapt, stream)


def resample(w, num_pred: int, device="cuda"):
    """(idx[n, R] int32, n_distinct[n] int32) host arrays of the weight series
    w[n, S] by the device's midpoint systematic resampling (MDFIT-PPRED v1,
    mdfit_resample; parity tests)."""
    torch = _torch()
    lib = _lib.load()
    w = np.array(w, dtype=np.float64, order="C")
    n, S = w.shape
    R = int(num_pred)
    t = torch.from_numpy(w).to(device)
    idx = torch.empty((n, R), dtype=torch.int32, device=device)
    nd = torch.empty(n, dtype=torch.int32, device=device)
    _lib.check(lib.mdfit_resample(ctypes.c_void_p(t.data_ptr()), n, S, R, ctypes.c_void_p(idx.data_ptr()),
                                  ctypes.c_void_p(nd.data_ptr()), _stream_handle(torch, None)))
    torch.cuda.current_stream().synchronize()
    return idx.cpu().numpy(), nd.cpu().numpy()


def psis_weights(lw, device="cuda"):
    """(w[n, S], khat[n]) float64 host arrays of the raw log-weight series
    lw[n, S] by the device's smoothing (MDFIT-PSIS v1, mdfit_psis_weights;
    parity tests)."""
    torch = _torch()
    lib = _lib.load()
    lw = np.array(lw, dtype=np.float64, order="C")  # (a copy: the caller's array may be read only)
    n, S = lw.shape
    t = torch.from_numpy(lw).to(device)
    w = torch.empty((n, S), dtype=torch.float64, device=device)
    khat = torch.empty(n, dtype=torch.float64, device=device)
    _lib.check(lib.mdfit_psis_weights(ctypes.c_void_p(t.data_ptr()), n, S, ctypes.c_void_p(w.data_ptr()),
                                      ctypes.c_void_p(khat.data_ptr()), _stream_handle(torch, None)))
    torch.cuda.current_stream().synchronize()
    return w.cpu().numpy(), khat.cpu().numpy()


def adapt_proposal(u, w, mask, c_held, K, device="cuda"):
    """The refit of one round of MDFIT-ADAPT v1 by the device's function
    (mdfit_adapt_proposal; a test helper): draws u[n, S, 4], normalised weights
    w[n, S], free mask[n], c_held[n], shift K[n, 4] -> (m[n, 4], d[n, 4], F[n, 4,
    4], gc[n], ok[n]); NaN where ok is 0."""
    torch = _torch()
    lib = _lib.load()
    tu = torch.as_tensor(np.ascontiguousarray(u, dtype=np.float64), device=device)
    tw = torch.as_tensor(np.ascontiguousarray(w, dtype=np.float64), device=device)
    n, S = int(tw.shape[0]), int(tw.shape[1])
    tm = torch.as_tensor(np.ascontiguousarray(mask, dtype=np.int32), device=device)
    tc = torch.as_tensor(np.ascontiguousarray(c_held, dtype=np.int32), device=device)
    tK = torch.as_tensor(np.ascontiguousarray(K, dtype=np.float64), device=device)
    prop = torch.empty((n, 25), dtype=torch.float64, device=device)
    ok = torch.empty(n, dtype=torch.int32, device=device)
    _lib.check(lib.mdfit_adapt_proposal(ctypes.c_void_p(tu.data_ptr()), ctypes.c_void_p(tw.data_ptr()),
                                        ctypes.c_void_p(tm.data_ptr()), ctypes.c_void_p(tc.data_ptr()),
                                        ctypes.c_void_p(tK.data_ptr()), n, S, ctypes.c_void_p(prop.data_ptr()),
                                        ctypes.c_void_p(ok.data_ptr()), _stream_handle(torch)))
    torch.cuda.synchronize()
    p = prop.cpu().numpy()
    return p[:, 0:4], p[:, 4:8], p[:, 8:24].reshape(n, 4, 4), p[:, 24], ok.cpu().numpy()


def nuts_diag_device(res: FitBatch, n_taxa: int, opts: _lib.MdfitOpts, diag=None, stream=None):
    """Launch mdfit_nuts_diag on the chains a finished NUTS call left in
    res.workspace (asynchronous on `stream`; before the next call on that
    workspace): per sub-fit the ESS and split R-hat of q, A, c, phi and D_max and
    the MCSE of D_max, float64 diag[T, 6, NNUTSDIAG] (_lib.NUTSDIAG_FIELDS).
    Reads res.workspace and res.out only.  Returns diag."""
    torch = _torch()
    T = int(n_taxa)
    diag = _buffer(torch, "diag", diag, (T, _lib.NSUBFIT, _lib.NNUTSDIAG), torch.float64, res.out.device, required=True)
    _check_nuts(res, T, opts)
    _lib.check(_lib.load().mdfit_nuts_diag(_ptr(res.workspace), _ptr(res.out), T, ctypes.byref(opts), _ptr(diag),
                                           _stream_handle(torch, stream)))
    return diag


def nuts_summary_device(res: FitBatch, n_taxa: int, opts: _lib.MdfitOpts, summ=None, stream=None):
    """Launch mdfit_nuts_summary on the chains a finished NUTS call left in
    res.workspace (asynchronous on `stream`; before the next call on that
    workspace): per sub-fit the standard deviations of q, A, c, phi and D_max,
    the median and 68 % HPDI of D_max and q, phi's median, the A-c correlation
    and mean / std of D_max, float64 summ[T, 6, NNUTSSUMM]
    (_lib.NUTSSUMM_FIELDS).  Reads res.workspace and res.out only; independent
    of nuts_diag_device (either order on one workspace).  Returns summ."""
    torch = _torch()
    T = int(n_taxa)
    summ = _buffer(torch, "summ", summ, (T, _lib.NSUBFIT, _lib.NNUTSSUMM), torch.float64, res.out.device, required=True)
    _check_nuts(res, T, opts)
    _lib.check(_lib.load().mdfit_nuts_summary(_ptr(res.workspace), _ptr(res.out), T, ctypes.byref(opts), _ptr(summ),
                                              _stream_handle(torch, stream)))
    return summ


def nuts_loo_device(y, N, res: FitBatch, n_taxa: int, opts: _lib.MdfitOpts, loo=None, pointwise=None, stream=None):
    """Launch mdfit_nuts_loo on the chains a finished NUTS call left in
    res.workspace (asynchronous on `stream`; before the next call on that
    workspace): PSIS-LOO per sub-fit -- elpd_loo, p_loo, its standard error, the
    largest Pareto k and where, the count of bad points, lppd -- and in row 6 the
    n_sigma comparisons on looic, float64 loo[T, 7, NNUTSLOO]
    (_lib.NUTSLOO_FIELDS, _lib.NUTSLOO_COMPARE_FIELDS).  y, N: the call's device
    counts [T, LD].  pointwise: None, True (allocated) or a float64 tensor [T, 6,
    30, 2] = (elpd_i, khat_i).  Reads y, N, res.workspace and res.out only;
    independent of nuts_diag_device and nuts_summary_device (any order on one
    workspace).  Returns loo, or (loo, pointwise) when pointwise is asked for."""
    torch = _torch()
    T, dev = int(n_taxa), res.out.device
    loo = _buffer(torch, "loo", loo, (T, _lib.NLOOROW, _lib.NNUTSLOO), torch.float64, dev, required=True)
    pointwise = _buffer(torch, "pointwise", pointwise, (T, _lib.NSUBFIT, _lib.NPOS, 2), torch.float64, dev)
    _check_counts(y, N, T)
    _check_nuts(res, T, opts)
    _lib.check(_lib.load().mdfit_nuts_loo(_ptr(y), _ptr(N), _ptr(res.workspace), _ptr(res.out), T, ctypes.byref(opts),
                                          _ptr(loo), _ptr(pointwise), _stream_handle(torch, stream)))
    return loo if pointwise is None else (loo, pointwise)


def nuts_post_device(y, N, res: FitBatch, n_taxa: int, opts: _lib.MdfitOpts, mm=None, taps: bool = False,
                     waic=None, counts=None, count_flags=None, stream=None):
    """Launch mdfit_nuts_post (test entry; asynchronous on `stream`): the record
    assembly of a NUTS call alone -- the post kernel, the product launch's
    source lines -- on the draws in res.workspace and the chain diag slots 4..7
    (step, leapfrogs, status, divergences of each sub-fit) in res.out, whose
    other slots are zero.  Fills res.out, res.pred (unless None) and
    res.status.  y, N (and mm, or None): the device counts [T, LD] ([T, 30,
    12]).  taps=True allocates the taps (or pass tensors): waic float64 [T, 6,
    30] (NaN where the kernel forms none), counts int32-typed uint32 [T, 32, S]
    (the unsorted predictive counts of the 32 jobs; 0xFFFFFFFF = no count or job
    not run) and count_flags uint8 [T, 32] (0 counts, 1 some draw was none, 2 N
    = 0, 255 not reached).  Returns (waic, counts, count_flags)."""
    torch = _torch()
    lib = _lib.load()
    T, S = int(n_taxa), int(opts.num_samples)
    dev = res.out.device
    if taps:
        waic = torch.empty((T, _lib.NSUBFIT, _lib.NPOS), dtype=torch.float64, device=dev) if waic is None else waic
        counts = torch.empty((T, _lib.LD, S), dtype=torch.int32, device=dev) if counts is None else counts
        count_flags = torch.empty((T, _lib.LD), dtype=torch.uint8, device=dev) if count_flags is None else count_flags
    for name, t, n, size in (("waic", waic, T * _lib.NSUBFIT * _lib.NPOS, 8), ("counts", counts, T * _lib.LD * S, 4),
                             ("count_flags", count_flags, T * _lib.LD, 1)):
        if t is not None and not (t.is_cuda and t.is_contiguous() and t.element_size() == size and t.numel() == n):
            raise ValueError(f"{name} must be a contiguous cuda tensor of {n} elements of {size} bytes")
    _check_counts(y, N, T)
    if mm is not None and not (mm.is_cuda and mm.is_contiguous() and mm.element_size() == 4
                               and mm.numel() == T * _lib.NPOS * _lib.NMM):
        raise ValueError("mm must be a contiguous cuda tensor of T*30*12 uint32")
    if res.status.numel() < T:
        raise ValueError("res must hold the contiguous records of these T taxa")
    if res.pred is not None and not (res.pred.is_contiguous() and res.pred.numel() >= T * _lib.NPRED * _lib.NPOS):
        raise ValueError("res.pred must be contiguous float32 [T, 3, 30]")
    _check_nuts(res, T, opts)
    _lib.check(lib.mdfit_nuts_post(_ptr(y), _ptr(N), _ptr(mm), T, ctypes.byref(opts), _ptr(res.workspace),
                                   _ptr(res.out), _ptr(res.pred), _ptr(res.status), _ptr(waic), _ptr(counts),
                                   _ptr(count_flags), _stream_handle(torch, stream)))
    return waic, counts, count_flags


def psis(ll, device="cuda"):
    """(elpd[n], khat[n]) float64 host arrays of the pointwise log-likelihood
    series ll[n, S] by the device's PSIS estimator (MDFIT-LOO v1, mdfit_psis;
    parity tests)."""
    torch = _torch()
    lib = _lib.load()
    ll = np.ascontiguousarray(ll, dtype=np.float64)
    n, S = ll.shape
    t = torch.from_numpy(ll).to(device)
    elpd = torch.empty(n, dtype=torch.float64, device=device)
    khat = torch.empty(n, dtype=torch.float64, device=device)
    _lib.check(lib.mdfit_psis(ctypes.c_void_p(t.data_ptr()), n, S, ctypes.c_void_p(elpd.data_ptr()),
                              ctypes.c_void_p(khat.data_ptr()), _stream_handle(torch, None)))
    torch.cuda.current_stream().synchronize()
    return elpd.cpu().numpy(), khat.cpu().numpy()


def fit_batch(y, N, mm=None, opts: _lib.MdfitOpts | None = None, device="cuda"):
    """Host arrays in, host arrays out: (out[T,80] f64, pred[T,3,30] f32, status[T] i32)."""
    torch = _torch()
    ty, tN, tm = to_device_counts(y, N, mm, device=device)
    res = fit_batch_device(ty, tN, tm, opts)
    torch.cuda.current_stream().synchronize()
    return res.out.cpu().numpy(), res.pred.cpu().numpy(), res.status.cpu().numpy()


# --------------------------------------------------------------------------
# bounded-memory chunked dispatch (the reference's 1,000-taxon chunks,
# fits.py:692-706, as device-memory-sized chunks on two streams)
# --------------------------------------------------------------------------
MAX_CALL_TAXA = 1 << 25  # mdfit_fit_batch's per-call limit (MAP: int32 position indices)
N_SETS = 2  # device buffer sets in flight: chunk k+1's H2D (and fit) beside chunk k's fit and D2H
_BUDGET_FRAC = 0.6  # default device budget of a staging: this fraction of the free device memory


_PART = {p.name: p for p in (*blocks.BLOCKS, *blocks.TAILS)}
# one taxon's block or tail as it leaves the device (f32), bytes
(LAP_BYTES, DIAG_BYTES, SUMM_BYTES, LOO_BYTES, PSIS_BYTES, WAIC_BYTES, PPRED_BYTES, PPC_BYTES, QUANT_BYTES,
 JOINT_BYTES) = (_PART[name].out_bytes for name in ("laplace", "diag", "summary", "loo", "psis", "waic", "ppred",
                                                    "ppc", "quant", "joint"))
PPRED_WORDS = PPRED_BYTES // 4
PSIS_DRAWS = 256  # the default number of importance draws per sub-fit
PRED_DRAWS = 1000  # predictive draws per job of mdfit_map_pred where the caller gives none (the reference's)


def _pieces(block, part) -> tuple:
    """Views of one f32 block [T, *part.shape] (torch or numpy), one per piece of part.device, shaped as computed:
    the pieces lie in consecutive word ranges of a taxon's row."""
    T = block.shape[0]
    flat, views, lo = block.reshape(T, prod(part.shape)), [], 0
    for shape, _dtype in part.device:
        views.append(flat[:, lo:lo + prod(shape)].reshape(T, *shape))
        lo += prod(shape)
    return tuple(views)


def split_ppred(block):
    """(ppred[T, 3, 30], rec[T, NMAPPRED]) views of a posterior predictive block [T, PPRED_WORDS]."""
    return _pieces(block, _PART["ppred"])


def split_ppc(block):
    """(ppos[T, 30], rec[T, NMAPPPC]) views of a posterior predictive check block [T, NPPCOUT]."""
    return _pieces(block, _PART["ppc"])


def split_joint(block):
    """(evid[T, 7, NMAPEVID], psis[T, 3, NMAPPSIS]) views of a joint block [T, NJOINTOUT]."""
    return _pieces(block, _PART["joint"])


def _check_psis_adapt(psis_adapt: int, importance_sampled: bool) -> int:
    """psis_adapt (MDFIT-ADAPT v1's round cap) is 0 .. ADAPT_MAX_ROUNDS and, when
    not 0, goes with an importance-sampled block (blocks.Block.sampled)."""
    return blocks.check_rounds(psis_adapt, importance_sampled)


def _set_bytes(C: int, opts, run: blocks.Run, with_mm: bool, with_pred: bool, dest_on_device: bool) -> int:
    """device_bytes for a run already described.  The adapt tail (96 B computed + 8 B out per taxon) is not counted:
    a known gap that device_bytes and plan_chunks, which take no psis_adapt, have always had."""
    b = C * (2 * _lib.LD * 4 + (_lib.NPOS * _lib.NMM * 4 if with_mm else 0))
    if not dest_on_device:
        b += C * (_lib.NOUT * 8 + (_lib.NPRED * _lib.NPOS * 4 if with_pred else 0) + 4)
    for part in run.parts:
        if part is not blocks.ADAPT:
            b += C * (part.device_bytes + (0 if dest_on_device else part.out_bytes))
    return b + workspace_bytes(C, opts)


def device_bytes(C: int, opts: _lib.MdfitOpts | None = None, with_mm: bool = True, with_pred: bool = True,
                 dest_on_device: bool = False, ppc: bool = False, quantiles: bool = False,
                 dmax_threshold: float = 0.01, joint: bool = False, **switches) -> int:
    """Device bytes one buffer set of a C-taxon chunk takes: the inputs (y, N:
    256 B; mm: 1,440 B), the outputs (record 640 B, predictions 360 B, status 4
    B -- unless the chunk writes into the caller's device buffers) and the
    call's workspace (mdfit_workspace_bytes: MAP ~48 B below 60k taxa and
    ~4.9 KB from 60k, NUTS 6 x num_samples x 32 B, the draws).  switches (one
    with_* of blocks.BLOCKS) and ppc, quantiles, joint (the tails of blocks.TAILS
    that ride it; blocks.describe checks them): each as its launch computes it
    and -- unless it goes to the caller's device buffer -- as it leaves, rounded
    to f32.  (No psis_adapt: the adapt record is not counted)"""
    run = blocks.describe(opts, {"ppc": ppc, "quantiles": quantiles, "joint": joint}, chunked=True,
                          dmax_threshold=dmax_threshold, **switches)
    return _set_bytes(int(C), opts, run, with_mm, with_pred, dest_on_device)


def plan_chunks(T: int, opts: _lib.MdfitOpts | None = None, budget_bytes: int | None = None, *,
                chunk_taxa: int = 0, n_sets: int = N_SETS, with_mm: bool = True, with_pred: bool = True,
                dest_on_device: bool = False, ppc: bool = False, quantiles: bool = False,
                dmax_threshold: float = 0.01, joint: bool = False, **switches) -> list[tuple[int, int]]:
    """Split T taxa into near-equal contiguous chunks [lo, hi) such that n_sets
    buffer sets of the largest chunk (device_bytes, with the run's block and
    tails) fit in budget_bytes (None: no memory bound), no chunk exceeds the
    per-call limit (2^25 taxa) or chunk_taxa (> 0; env MDFIT_CHUNK_TAXA when 0).
    Taxa are independent and the sampler's streams are keyed by the global taxon
    index (opts.index_base + lo), so any split gives the records of one call bit
    for bit."""
    run = blocks.describe(opts, {"ppc": ppc, "quantiles": quantiles, "joint": joint}, chunked=True,
                          dmax_threshold=dmax_threshold, **switches)
    return _chunks(int(T), opts, run, budget_bytes, chunk_taxa, n_sets, with_mm, with_pred, dest_on_device)


def _chunks(T: int, opts, run: blocks.Run, budget_bytes, chunk_taxa: int, n_sets: int, with_mm: bool,
            with_pred: bool, dest_on_device: bool) -> list[tuple[int, int]]:
    """plan_chunks for a run already described."""
    if T <= 0:
        return []
    cap = min(T, MAX_CALL_TAXA)
    if chunk_taxa <= 0:
        chunk_taxa = int(os.environ.get("MDFIT_CHUNK_TAXA", "0") or 0)
    if chunk_taxa > 0:
        cap = min(cap, int(chunk_taxa))
    if budget_bytes is not None:
        def per(c):
            return n_sets * _set_bytes(c, opts, run, with_mm, with_pred, dest_on_device)

        if per(1) > budget_bytes:
            raise _lib.MdfitError(f"device budget {budget_bytes} B below one taxon's {per(1)} B")
        if per(cap) > budget_bytes:  # largest c with per(c) <= budget (per is monotone in c)
            lo, hi = 1, cap
            while lo < hi:
                mid = (lo + hi + 1) // 2
                if per(mid) <= budget_bytes:
                    lo = mid
                else:
                    hi = mid - 1
            cap = lo
    n = -(-T // cap)
    return [(T * i // n, T * (i + 1) // n) for i in range(n)]


def default_budget(device) -> int:
    """The device budget of a staging (bytes): MDFIT_DEVICE_BUDGET_GB, else
    _BUDGET_FRAC of the device memory free now."""
    torch = _torch()
    env = os.environ.get("MDFIT_DEVICE_BUDGET_GB")
    if env:
        return int(float(env) * (1 << 30))
    free, _total = torch.cuda.mem_get_info(torch.device(device))
    return int(_BUDGET_FRAC * free)


class _Set:
    """One chunk's device buffers (the workspace is the fitter's: the calls
    run one after another on the compute stream)."""

    def __init__(self, torch, C: int, device, with_pred: bool, with_mm: bool, dest_on_device: bool, parts=()):
        self.d_y = torch.empty((C, _lib.LD), dtype=torch.int32, device=device)
        self.d_N = torch.empty((C, _lib.LD), dtype=torch.int32, device=device)
        self.d_mm = torch.empty((C, _lib.NPOS, _lib.NMM), dtype=torch.int32, device=device) if with_mm else None
        self.out = self.pred = self.status = None
        if not dest_on_device:
            self.out = torch.empty((C, _lib.NOUT), dtype=torch.float64, device=device)
            self.pred = (torch.empty((C, _lib.NPRED, _lib.NPOS), dtype=torch.float32, device=device)
                         if with_pred else None)
            self.status = torch.empty((C,), dtype=torch.int32, device=device)
        # by attr, the run's block and each tail: as its launch writes it, and as one f32 block for the way out
        self.computed = {p.attr: [torch.empty((C, *shape), dtype=getattr(torch, dtype), device=device)
                                  for shape, dtype in p.device] for p in parts}
        self.f32 = {} if dest_on_device else {
            p.attr: torch.empty((C, *p.shape), dtype=torch.float32, device=device) for p in parts}


H_OUT_COLS = _lib.NRESULT  # record columns the host gets back: the 25 result columns


# One launch function per chunked block, and per tail that has a launch of its own: its *_device call on the first n
# taxa of buffer set st, whose records res holds, into c = st.computed (by attr) on the compute stream comp.  f: the
# fitter (f.plan: the draw counts, the threshold, the tails); o: the chunk's options (its index_base is the chunk's
# global taxon index, which keys the Philox streams beside o.seed); ad_kw: adapt_rounds and adapt of the sampled
# blocks when psis_adapt > 0 (the launch is then the *_adapt entry).  The MAP blocks read the final records; the
# NUTS blocks read this chunk's draws in the one workspace, which the stream keeps until the next chunk's fit.
def _launch_laplace(f, st, n, res, o, comp, c, ad_kw):
    map_laplace_device(st.d_y[:n], st.d_N[:n], res, lap=c["lap"][0][:n], stream=comp)


def _launch_diag(f, st, n, res, o, comp, c, ad_kw):
    nuts_diag_device(res, n, o, diag=c["diag"][0][:n], stream=comp)


def _launch_summary(f, st, n, res, o, comp, c, ad_kw):
    nuts_summary_device(res, n, o, summ=c["summ"][0][:n], stream=comp)


def _launch_loo(f, st, n, res, o, comp, c, ad_kw):
    nuts_loo_device(st.d_y[:n], st.d_N[:n], res, n, o, loo=c["loo"][0][:n], stream=comp)


def _launch_psis(f, st, n, res, o, comp, c, ad_kw):
    map_psis_device(st.d_y[:n], st.d_N[:n], res, f.plan.psis_draws, int(o.seed), int(o.index_base),
                    psis=c["psis"][0][:n], stream=comp, **ad_kw)


def _launch_waic(f, st, n, res, o, comp, c, ad_kw):
    if "joint" in c:  # the fused launch: the same waic record, and the joint tail's evidence and psis records beside it
        map_joint_device(st.d_y[:n], st.d_N[:n], res, f.plan.psis_draws, int(o.seed), int(o.index_base),
                         waic=c["waic"][0][:n], evid=c["joint"][0][:n], psis=c["joint"][1][:n], stream=comp, **ad_kw)
        return
    map_waic_device(st.d_y[:n], st.d_N[:n], res, f.plan.psis_draws, int(o.seed), int(o.index_base),
                    waic=c["waic"][0][:n], stream=comp, **ad_kw)


def _launch_evidence(f, st, n, res, o, comp, c, ad_kw):
    map_evidence_device(st.d_y[:n], st.d_N[:n], res, f.plan.psis_draws, int(o.seed), int(o.index_base),
                        evid=c["evid"][0][:n], stream=comp, **ad_kw)


def _launch_ppred(f, st, n, res, o, comp, c, ad_kw):
    map_pred_device(st.d_y[:n], st.d_N[:n], res, f.plan.psis_draws, f.plan.pred_draws, int(o.seed), int(o.index_base),
                    ppred=c["ppred"][0][:n], rec=c["ppred"][1][:n], stream=comp, **ad_kw)


# The two tails with a launch of their own follow their block's on the same stream with the same draws and rounds;
# the block's launch has written the rounds' record, so theirs runs without it (adapt=False).  The joint tail has no
# launch (_launch_waic writes it) and neither has adapt (the block's launch writes it).
def _launch_ppc(f, st, n, res, o, comp, c, ad_kw):
    map_ppc_device(st.d_y[:n], st.d_N[:n], res, f.plan.psis_draws, f.plan.pred_draws, int(o.seed), int(o.index_base),
                   ppos=c["ppc"][0][:n], rec=c["ppc"][1][:n], stream=comp,
                   **(dict(ad_kw, adapt=False) if ad_kw else {}))


def _launch_quant(f, st, n, res, o, comp, c, ad_kw):
    map_quant_device(st.d_y[:n], st.d_N[:n], res, f.plan.psis_draws, int(o.seed), int(o.index_base),
                     f.plan.dmax_threshold, quant=c["quant"][0][:n], stream=comp,
                     **(dict(ad_kw, adapt=False) if ad_kw else {}))


_LAUNCH = {"laplace": _launch_laplace, "diag": _launch_diag, "summary": _launch_summary, "loo": _launch_loo,
           "psis": _launch_psis, "waic": _launch_waic, "evidence": _launch_evidence, "ppred": _launch_ppred,
           "ppc": _launch_ppc, "quant": _launch_quant}


# How a part's computed pieces become its f32 block on the way out (on the compute stream): one rounding copy per
# piece into the piece's word range, but for two.
def _leave(torch, part, computed, block32, res):
    for view, piece in zip(_pieces(block32, part), computed):
        view.copy_(piece)


def _leave_diag(torch, part, computed, block32, res):
    """... and the flags also carry the chain's divergence count (the record's slot 7, not among the columns that
    leave the device): valid + 2 * divergences."""
    _leave(torch, part, computed, block32, res)
    div = torch.nan_to_num(res.out[:, _lib.F_DIAG + 7::_lib.DIAG_STRIDE], nan=0.0)
    block32[:, :, _lib.NNUTSDIAG - 1] += (2.0 * div).to(torch.float32)


def _leave_adapt(torch, part, computed, block32, res):
    """The adapt record leaves reduced to its two columns."""
    adapt_summary(computed[0], out=block32)


_LEAVE = {"diag": _leave_diag, "adapt": _leave_adapt}


class ChunkedFitter:
    """Host-to-device fits of any number of taxa in chunks of at most
    `chunk_cap` taxa (the reference handles any number of taxa in 1,000-taxon
    chunks, fits.py:692-706; one call per file had a capacity cliff: the NUTS
    draws are 192 KB per taxon, ~1.4M taxa per GPU).  Device memory is
    N_SETS x device_bytes(chunk_cap) whatever the batch size.

    Two streams: the caller's current stream runs the calls, one after another
    (mdfit_fit_batch with mm = NULL, then mdfit_noise once the chunk's mismatch
    counts are on the device); a copy stream runs every transfer.  So the fit
    starts as soon as its y, N (256 B per taxon) are in, the mismatch counts
    (1,440 B per taxon) cross PCIe while it runs, and -- with several chunks --
    chunk k's results come back while chunk k+1 fits (N_SETS buffer sets).  The
    transfers of one chunk are ordered y, N before mm so the fit's inputs are
    not behind the bulk.  (Two streams of ours beside the library's two side
    streams: four hardware queues, GPU_MAX_HW_QUEUES on the box; more streams
    would share queues and serialise.)

    Outputs go to pinned host buffers (run: the 25 result columns, the
    predictions, the status; grown as needed and reused) or, run_into_device,
    straight into the caller's device tensors (the sharded fit's gather
    records).

    switches (one with_* of blocks.BLOCKS; one optional block per run keeps the
    gather record's layout a single switch): the block's launch (_LAUNCH)
    follows each chunk's fit on the compute stream -- no further stream or
    hardware queue --, its records are rounded to f32 there and leave with the
    chunk's other results (run's fourth array; run_into_device writes dest's
    attribute of the block).  The sampled blocks take psis_draws draws per
    sub-fit (ppred also pred_draws predictive draws per job).

    psis_adapt, ppc, quantiles (with dmax_threshold) and joint ask for the tails
    of blocks.TAILS, which says what each rides, computes and sends out: a tail
    with a launch of its own (_LAUNCH) follows the block's on the compute stream
    with the same draws, seed, index_base and rounds -- no further stream --,
    and every tail leaves behind the block as one more f32 block, rounded on
    the device, in TAILS' order (run's further arrays; dest's attribute of the
    tail's name).  psis_adapt = R > 0: the sampled block's launch runs at most R
    moment-matched proposal rounds per PMD row (MDFIT-ADAPT v1) and the adapt
    tail is their record reduced on the device (adapt_summary)."""

    def __init__(self, chunk_cap: int, device="cuda", opts: _lib.MdfitOpts | None = None, with_pred: bool = True,
                 with_mm: bool = True, dest_on_device: bool = False, psis_draws: int = PSIS_DRAWS,
                 pred_draws: int = PRED_DRAWS, psis_adapt: int = 0, ppc: bool = False, quantiles: bool = False,
                 dmax_threshold: float = 0.01, joint: bool = False, **switches):
        tails = {"psis_adapt": psis_adapt, "ppc": ppc, "quantiles": quantiles, "joint": joint}
        self.plan = plan = blocks.describe(opts, tails, chunked=True, psis_draws=psis_draws, pred_draws=pred_draws,
                                           dmax_threshold=dmax_threshold, **switches)
        torch = _torch()
        self.block, self.parts, self.psis_adapt = plan.block, plan.parts, plan.rounds
        self.chunk_cap = int(chunk_cap)
        self.device = torch.device(device)
        self.with_pred, self.with_mm, self.dest_on_device = with_pred, with_mm, dest_on_device
        self.sets = [_Set(torch, self.chunk_cap, self.device, with_pred, with_mm, dest_on_device, self.parts)
                     for _ in range(N_SETS)]
        self.ws = alloc_workspace(self.chunk_cap, self.device, opts)
        self.copy = torch.cuda.Stream(device=self.device)
        self.full_cap = False  # (staging: the chunk capacity is the device budget's, not the batch's)
        self.capacity = 0  # pinned host buffers (input staging for pageable sources, outputs)
        self.h_y = self.h_N = self.h_mm = self.h_out = self.h_pred = self.h_status = None
        self.h_parts = {}  # by attr: the block's and each tail's f32 array on the way out
        self._end = None  # the previous run's last event (its transfers use the pinned buffers)

    def _host(self, T: int):
        if T <= self.capacity:
            return
        torch = _torch()
        cap = int(1.25 * T) + 1
        self.h_y = torch.empty((cap, _lib.LD), dtype=torch.int32).pin_memory()
        self.h_N = torch.empty((cap, _lib.LD), dtype=torch.int32).pin_memory()
        self.h_mm = torch.empty((cap, _lib.NPOS, _lib.NMM), dtype=torch.int32).pin_memory() if self.with_mm else None
        if not self.dest_on_device:
            self.h_out = torch.empty((cap, H_OUT_COLS), dtype=torch.float64).pin_memory()
            self.h_pred = (torch.empty((cap, _lib.NPRED, _lib.NPOS), dtype=torch.float32).pin_memory()
                           if self.with_pred else None)
            self.h_status = torch.empty((cap,), dtype=torch.int32).pin_memory()
            self.h_parts = {p.attr: torch.empty((cap, *p.shape), dtype=torch.float32).pin_memory()
                            for p in self.parts}
        self.capacity = cap

    def _sources(self, y, N, mm, pinned):
        """Pinned int32 views of the inputs: the PinnedPack's, or a copy into
        the staging's own pinned buffers (H2D from pageable memory would be a
        synchronous staged copy)."""
        T = int(y.shape[0])
        use_mm = mm is not None and self.with_mm
        if pinned is not None:
            return pinned.h_y[:T], pinned.h_N[:T], pinned.h_mm[:T] if use_mm else None
        if self._end is not None:  # the previous run's H2D may still read the staging buffers
            self._end.synchronize()
        self._host(T)
        self.h_y[:T].numpy()[:] = np.asarray(y, dtype=np.uint32).view(np.int32)
        self.h_N[:T].numpy()[:] = np.asarray(N, dtype=np.uint32).view(np.int32)
        if use_mm:
            self.h_mm[:T].numpy()[:] = np.asarray(mm, dtype=np.uint32).view(np.int32)
        return self.h_y[:T], self.h_N[:T], self.h_mm[:T] if use_mm else None

    def _launch(self, chunks, src, opts, dest=None):
        """Enqueue every chunk (asynchronous); returns the event after which
        every result is in place (host outputs: copied back)."""
        torch = _torch()
        lib = _lib.load()
        o0 = opts if opts is not None else _lib.default_opts()
        if self.block is not None:
            blocks.resolve(o0, **{self.block.switch: True})  # (this run's options, not only the constructor's)
        for p in self.parts if dest is not None else ():
            if getattr(dest, p.attr, None) is None:
                asked = p.switch if p is self.block else p.option
                raise ValueError(f"{asked}: dest.{p.attr} (float32 [T, {', '.join(map(str, p.shape))}]) required")
        src_y, src_N, src_mm = src
        comp = torch.cuda.current_stream(self.device)
        cp = self.copy
        h_s = _stream_handle(torch, comp)
        start = torch.cuda.Event()
        start.record(comp)  # after the caller's prior work (and the previous run's)
        cp.wait_event(start)
        last_d2h = None
        done = []  # per chunk: its call (and noise) finished on the compute stream
        for k, (lo, hi) in enumerate(chunks):
            st = self.sets[k % N_SETS]
            n = hi - lo
            o = _lib.MdfitOpts.from_buffer_copy(o0)
            o.index_base = o0.index_base + lo  # the sampler's streams: global taxon index
            # transfers in: y, N first, then the mismatch counts (copy stream),
            # once the set's previous chunk has finished reading them
            if k >= N_SETS:
                cp.wait_event(done[k - N_SETS])
            with torch.cuda.stream(cp):
                st.d_y[:n].copy_(src_y[lo:hi], non_blocking=True)
                st.d_N[:n].copy_(src_N[lo:hi], non_blocking=True)
                ev_yn = torch.cuda.Event()
                ev_yn.record(cp)
                ev_mm = None
                if src_mm is not None:
                    st.d_mm[:n].copy_(src_mm[lo:hi], non_blocking=True)
                    ev_mm = torch.cuda.Event()
                    ev_mm.record(cp)
            if dest is not None:
                res = FitBatch(dest.out[lo:hi], dest.pred[lo:hi] if dest.pred is not None else None,
                               dest.status[lo:hi], self.ws)
            else:
                res = FitBatch(st.out[:n], st.pred[:n] if st.pred is not None else None, st.status[:n], self.ws)
            # the call (compute stream) once y, N are in; the noise once mm is
            comp.wait_event(ev_yn)
            fit_batch_device(st.d_y[:n], st.d_N[:n], None, o, res, stream=comp)
            self.ws = res.workspace
            if ev_mm is not None:
                comp.wait_event(ev_mm)
                _lib.check(lib.mdfit_noise(_ptr(st.d_y), _ptr(st.d_N), _ptr(st.d_mm), n, _ptr(res.out), h_s))
            # the records are final: the block, then each tail in the record's order -- its launch where it has one
            # (the others' pieces are written by now), then its one f32 block for the way out
            ad_kw = ({"adapt_rounds": self.psis_adapt, "adapt": st.computed["adapt"][0][:n]}
                     if self.psis_adapt > 0 else {})
            leaving = {}
            for p in self.parts:
                if p.name in _LAUNCH:
                    _LAUNCH[p.name](self, st, n, res, o, comp, st.computed, ad_kw)
                block32 = leaving[p.attr] = getattr(dest, p.attr)[lo:hi] if dest is not None else st.f32[p.attr][:n]
                with torch.cuda.stream(comp):
                    _LEAVE.get(p.name, _leave)(torch, p, [c[:n] for c in st.computed[p.attr]], block32, res)
            ev_done = torch.cuda.Event()
            ev_done.record(comp)
            done.append(ev_done)
            if dest is None:  # results out on the copy stream, behind this chunk's call
                cp.wait_event(ev_done)
                with torch.cuda.stream(cp):
                    self.h_out[lo:hi].copy_(res.out[:, :H_OUT_COLS], non_blocking=True)
                    if res.pred is not None:
                        self.h_pred[lo:hi].copy_(res.pred, non_blocking=True)
                    self.h_status[lo:hi].copy_(res.status, non_blocking=True)
                    for attr, block32 in leaving.items():
                        self.h_parts[attr][lo:hi].copy_(block32, non_blocking=True)
                last_d2h = cp
        end = torch.cuda.Event()
        end.record(cp if last_d2h is not None else comp)
        self._end = end
        return end

    def run(self, y, N, mm=None, opts: _lib.MdfitOpts | None = None, sync: bool = True,
            pinned: PinnedPack | None = None, chunks=None):
        """Fit len(y) taxa; returns numpy views (out[:, :25], pred, status, then
        the run's block and tails, f32 [T, *shape] each, in blocks.Run.parts'
        order) of the pinned buffers (valid until the next run).  pinned: y, N,
        mm are that PinnedPack's views.  chunks: the split (default plan_chunks
        at this staging's chunk_cap)."""
        T = int(y.shape[0])
        if chunks is None:
            chunks = plan_chunks(T, opts, chunk_taxa=self.chunk_cap)
        if chunks and max(hi - lo for lo, hi in chunks) > self.chunk_cap:
            raise ValueError(f"a chunk exceeds this staging's {self.chunk_cap} taxa")
        self._host(T)
        end = self._launch(chunks, self._sources(y, N, mm, pinned), opts)
        if sync:
            end.synchronize()
        return (self.h_out[:T].numpy(), self.h_pred[:T].numpy() if self.h_pred is not None else None,
                self.h_status[:T].numpy(), *(self.h_parts[p.attr][:T].numpy() for p in self.parts))

    def run_into_device(self, y, N, mm, opts, dest: FitBatch, chunks=None):
        """Fit len(y) taxa chunk by chunk into the caller's device tensors dest
        (out[T, NOUT], pred, status -- and the run's block and tails under their
        attributes: rows written in place), ordered on the caller's current
        stream."""
        T = int(y.shape[0])
        if chunks is None:
            chunks = plan_chunks(T, opts, chunk_taxa=self.chunk_cap)
        self._launch(chunks, self._sources(y, N, mm, None), opts, dest=dest)
        return dest


class PinnedPack:
    """A pinned host buffer set for one file's packed counts (y, N: uint32
    [cap][32], mm: uint32[cap][30][12]): fits.pack_counts writes into it on a
    reader thread and ChunkedFitter.run copies it to the device directly (no
    host copy into the staging buffers: ~170 MB per 100k-taxon file)."""

    def __init__(self, capacity: int):
        torch = _torch()
        self.capacity = int(capacity)
        T = self.capacity
        self.h_y = torch.empty((T, _lib.LD), dtype=torch.int32).pin_memory()
        self.h_N = torch.empty((T, _lib.LD), dtype=torch.int32).pin_memory()
        self.h_mm = torch.empty((T, _lib.NPOS, _lib.NMM), dtype=torch.int32).pin_memory()

    def views(self, T: int):
        """numpy uint32 views (y, N, mm) of the first T taxa."""
        return (self.h_y[:T].numpy().view(np.uint32), self.h_N[:T].numpy().view(np.uint32),
                self.h_mm[:T].numpy().view(np.uint32))


_PINNED_FREE: list = []
_PINNED_N = 0
_PINNED_MAX = 3  # files in flight in main.main: N_READERS ahead + the one being fitted
_PINNED_LOCK = __import__("threading").Lock()


def acquire_pinned_pack(T: int) -> PinnedPack | None:
    """A free PinnedPack of at least T taxa (x1.25 headroom when one is made),
    or None when every set is in use (the caller then packs into pageable
    memory) or no HIP device is visible."""
    import torch

    if not torch.cuda.is_available():
        return None
    global _PINNED_N
    with _PINNED_LOCK:
        for i, pp in enumerate(_PINNED_FREE):
            if pp.capacity >= T:
                return _PINNED_FREE.pop(i)
        if _PINNED_FREE:  # too small: replaced by a larger one
            _PINNED_FREE.pop(0)
            _PINNED_N -= 1
        if _PINNED_N >= _PINNED_MAX:
            return None
        _PINNED_N += 1
    return PinnedPack(int(1.25 * T) + 1)


def release_pinned_pack(pp: PinnedPack) -> None:
    with _PINNED_LOCK:
        _PINNED_FREE.append(pp)


_STAGING: dict = {}
_STAGING_LOCK = __import__("threading").Lock()


def staging(n_taxa: int, device="cuda", opts: _lib.MdfitOpts | None = None, with_mm: bool = True,
            dest_on_device: bool = False, budget_bytes: int | None = None, psis_draws: int = PSIS_DRAWS,
            pred_draws: int = PRED_DRAWS, psis_adapt: int = 0, ppc: bool = False, quantiles: bool = False,
            dmax_threshold: float = 0.01, joint: bool = False, **switches) -> ChunkedFitter:
    """The ChunkedFitter for batches of n_taxa on this device, reused across calls
    of this process (per device, buffer kind, sampler length and the run's
    blocks.Run.key: its block of switches with the draw counts it uses, its
    rounds, its tails and their threshold): the
    multi-file pipeline fits one file after another, and pinned + device
    buffers allocated per file cost more host time than the fit.  Its chunk
    capacity is the largest chunk N_SETS buffer sets of which fit the device
    budget (default_budget), or n_taxa (x1.25 headroom) when smaller; a larger
    batch than the chunk capacity is split into chunks (plan_chunks), so the
    device memory it takes is bounded whatever the batch size.  Callers hold
    _STAGING_LOCK around its use (concurrent host threads take turns)."""
    torch = _torch()
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    o = opts if opts is not None else _lib.default_opts()
    env_chunk = int(os.environ.get("MDFIT_CHUNK_TAXA", "0") or 0)
    tails = {"psis_adapt": psis_adapt, "ppc": ppc, "quantiles": quantiles, "joint": joint}
    plan = blocks.describe(o, tails, chunked=True, psis_draws=psis_draws, pred_draws=pred_draws,
                           dmax_threshold=dmax_threshold, **switches)
    key = (str(dev), bool(with_mm), bool(dest_on_device), int(o.mode), int(o.num_samples), env_chunk, plan.key)
    st = _STAGING.get(key)
    T = max(1, int(n_taxa))
    if st is not None and (st.chunk_cap >= T or st.full_cap):
        return st
    _STAGING.pop(key, None)
    del st
    budget = budget_bytes if budget_bytes is not None else default_budget(dev)
    # the largest chunk the budget allows (x1.25 headroom over this batch: the
    # files of a run differ in taxon count by a few %)
    want = int(1.25 * T) + 1
    # (not across the library's stream / after-the-fit HPDI switch: from 60k
    # taxa the MAP workspace holds every position's wide-window record, ~4.8 KB
    # per taxon that batches below 60k never touch)
    if T < _lib.STREAM_MAX_TAXA:
        want = min(want, _lib.STREAM_MAX_TAXA - 1)
    cap = _chunks(want, o, plan, budget, env_chunk, N_SETS, with_mm, True, dest_on_device)[0]
    cap = cap[1] - cap[0]
    st = ChunkedFitter(cap, device=dev, opts=o, with_mm=with_mm, dest_on_device=dest_on_device, **plan.options,
                       **switches)
    # (chunk capacity below the batch: memory-bound, no regrow for larger batches)
    st.full_cap = cap < want
    _STAGING[key] = st
    return st


def fit_batch_host(y, N, mm=None, opts: _lib.MdfitOpts | None = None, noise=None, device="cuda",
                   pinned: PinnedPack | None = None, psis_draws: int = PSIS_DRAWS, pred_draws: int = PRED_DRAWS,
                   psis_adapt: int = 0, ppc: bool = False, quantiles: bool = False, dmax_threshold: float = 0.01,
                   joint: bool = False, **named):
    """The product's host-to-host fit: (out[T, 25], pred, status) -- and, with
    named (one chunked block of blocks.BLOCKS by its name, e.g. laplace=True), a
    fourth array, the block's f32 [T, *shape], and behind it the f32 array of
    each tail asked for (blocks.TAILS, in its order; ChunkedFitter documents
    the options) --, chunked through the device budget.  mm goes to the device
    (the assembly computes the
    noise columns); without it, `noise` (float64[T][3], ingest.noise) fills them
    when given.  pinned: y, N, mm are views of that PinnedPack (copied to the
    device from there)."""
    T = int(y.shape[0])
    with _STAGING_LOCK:
        st = staging(T, device=device, opts=opts, with_mm=mm is not None, psis_draws=psis_draws,
                     pred_draws=pred_draws, psis_adapt=psis_adapt, ppc=ppc, quantiles=quantiles,
                     dmax_threshold=dmax_threshold, joint=joint,
                     **{"with_" + k: v for k, v in named.items()})
        got = st.run(y, N, mm, opts, pinned=pinned, chunks=plan_chunks(T, opts, chunk_taxa=st.chunk_cap))
        got = tuple(a.copy() for a in got)
    out, status = got[0], got[2]
    if mm is None and noise is not None:
        ok = status != _lib.INVALID
        out[ok, _lib.RESULT_FIELDS.index("normalized_noise"):_lib.NRESULT] = np.asarray(noise)[ok]
    return got


def special(x, device="cuda"):
    """(lgamma, digamma, trigamma) of x on the device (parity tests)."""
    torch = _torch()
    lib = _lib.load()
    tx = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=device)
    o = torch.empty((tx.numel(), 3), dtype=torch.float64, device=device)
    _lib.check(lib.mdfit_special(ctypes.c_void_p(tx.data_ptr()), tx.numel(), ctypes.c_void_p(o.data_ptr()),
                                 _stream_handle(torch)))
    torch.cuda.current_stream().synchronize()
    return o.cpu().numpy()


def primitive(which, x, x2=None, device="cuda"):
    """The device primitive `which` (enum mdfit_primitive_id: rcp, flog, fexp_t,
    lg3, lrise, ...) of csrc/mdfit_special.h at x, or at (x, x2) (parity tests)."""
    torch = _torch()
    lib = _lib.load()
    tx = torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64).ravel(), device=device)
    t2 = None if x2 is None else torch.as_tensor(np.ascontiguousarray(x2, dtype=np.float64).ravel(), device=device)
    if t2 is not None and t2.numel() != tx.numel():
        raise ValueError("x and x2 differ in size")
    o = torch.empty(tx.numel(), dtype=torch.float64, device=device)
    _lib.check(lib.mdfit_primitive(int(which), ctypes.c_void_p(tx.data_ptr()),
                                   None if t2 is None else ctypes.c_void_p(t2.data_ptr()), tx.numel(),
                                   ctypes.c_void_p(o.data_ptr()), _stream_handle(torch)))
    torch.cuda.current_stream().synchronize()
    return o.cpu().numpy()


def betabinom_logpmf(y, N, a, b, device="cuda"):
    """Pointwise beta-binomial log-pmf and (d/dalpha, d/dbeta) on the device."""
    torch = _torch()
    lib = _lib.load()
    ts = [torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device=device) for v in (y, N, a, b)]
    n = ts[0].numel()
    o = torch.empty(n, dtype=torch.float64, device=device)
    g = torch.empty((n, 2), dtype=torch.float64, device=device)
    _lib.check(lib.mdfit_betabinom_logpmf(*[ctypes.c_void_p(t.data_ptr()) for t in ts], n,
                                          ctypes.c_void_p(o.data_ptr()), ctypes.c_void_p(g.data_ptr()),
                                          _stream_handle(torch)))
    torch.cuda.current_stream().synchronize()
    return o.cpu().numpy(), g.cpu().numpy()


def hpdi68(N, a, b, device="cuda"):
    """68 % predictive window [lo, hi] of BetaBinomial(a, b, N) on the device
    (MDFIT-HPDI v2, mdfit_hpdi68; parity tests)."""
    torch = _torch()
    lib = _lib.load()
    shape = np.broadcast(N, a, b).shape
    # np.array copies: a broadcast view is read-only (torch warns on those)
    ts = [torch.as_tensor(np.array(np.broadcast_to(v, shape), dtype=np.float64).ravel(), device=device)
          for v in (N, a, b)]
    n = ts[0].numel()
    lo = torch.empty(n, dtype=torch.float64, device=device)
    hi = torch.empty(n, dtype=torch.float64, device=device)
    _lib.check(lib.mdfit_hpdi68(*[ctypes.c_void_p(t.data_ptr()) for t in ts], n, ctypes.c_void_p(lo.data_ptr()),
                                ctypes.c_void_p(hi.data_ptr()), _stream_handle(torch)))
    torch.cuda.current_stream().synchronize()
    return lo.cpu().numpy(), hi.cpu().numpy()


def peak_probe(n_waves: int, iters: int, stream=None, nuts: bool = False):
    """Launch the register-only point-evaluation probe (MAP: value + gradient +
    Hessian; nuts: the sampler's potential, value + gradient); returns the sink
    tensor."""
    torch = _torch()
    lib = _lib.load()
    sink = torch.empty(n_waves * 64, dtype=torch.float64, device="cuda")
    fn = lib.mdfit_nuts_peak_probe if nuts else lib.mdfit_peak_probe
    _lib.check(fn(n_waves, iters, ctypes.c_void_p(sink.data_ptr()), _stream_handle(torch, stream)))
    return sink


def nuts_potential(model, subset, y, N, v, device="cuda"):
    """Sampling-mode potential and gradient per item (mdfit_nuts_potential)."""
    torch = _torch()
    lib = _lib.load()
    n = len(model)
    tm = torch.as_tensor(np.ascontiguousarray(model, dtype=np.int32), device=device)
    ts = torch.as_tensor(np.ascontiguousarray(subset, dtype=np.int32), device=device)
    ty = torch.from_numpy(np.ascontiguousarray(y, dtype=np.uint32).view(np.int32)).to(device)
    tN = torch.from_numpy(np.ascontiguousarray(N, dtype=np.uint32).view(np.int32)).to(device)
    tv = torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device=device)
    U = torch.empty(n, dtype=torch.float64, device=device)
    g = torch.empty((n, 4), dtype=torch.float64, device=device)
    _lib.check(lib.mdfit_nuts_potential(*(ctypes.c_void_p(t.data_ptr()) for t in (tm, ts, ty, tN, tv)), n,
                                        ctypes.c_void_p(U.data_ptr()), ctypes.c_void_p(g.data_ptr()),
                                        _stream_handle(torch)))
    torch.cuda.synchronize()
    return U.cpu().numpy(), g.cpu().numpy()


def profile_enable(on: bool = True, fit_only: bool = False) -> None:
    """Record HIP events around every following mdfit_fit_batch call (and its
    fit kernel) on the call's stream; fit_only: only the two around the fit
    kernel (profile_read's call time is then -1)."""
    _lib.check(_lib.load().mdfit_profile_enable((2 if fit_only else 1) if on else 0))


def profile_read():
    """(call_ms_sum, fit_kernel_ms_sum, n_calls) over the calls recorded since
    profile_enable / the last read (synchronises on the events)."""
    a, b, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int32()
    _lib.check(_lib.load().mdfit_profile_read(ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)))
    return a.value, b.value, n.value


def objective(model, subset, y, N, u, device="cuda", form=None):
    """Per-item sub-fit objective (F, g[4], H[4,4], ell[30]) evaluated by the
    fit kernel's code path (mdfit_objective).  form: a sum of the
    MDFIT_FORM_* bits of include/mdfit.h (1 accf, 2 null_row, 4 whole_pair), the
    point evaluation's other forms (mdfit_objective_form); None: the plain entry."""
    torch = _torch()
    lib = _lib.load()
    n = len(model)
    tm = torch.as_tensor(np.ascontiguousarray(model, dtype=np.int32), device=device)
    ts = torch.as_tensor(np.ascontiguousarray(subset, dtype=np.int32), device=device)
    ty = torch.from_numpy(np.ascontiguousarray(y, dtype=np.uint32).view(np.int32)).to(device)
    tN = torch.from_numpy(np.ascontiguousarray(N, dtype=np.uint32).view(np.int32)).to(device)
    tu = torch.as_tensor(np.ascontiguousarray(u, dtype=np.float64), device=device)
    F = torch.empty(n, dtype=torch.float64, device=device)
    g = torch.empty((n, 4), dtype=torch.float64, device=device)
    H = torch.empty((n, 4, 4), dtype=torch.float64, device=device)
    ell = torch.empty((n, 30), dtype=torch.float64, device=device)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    if form is None:
        _lib.check(lib.mdfit_objective(ptr(tm), ptr(ts), ptr(ty), ptr(tN), ptr(tu), n, ptr(F), ptr(g), ptr(H),
                                       ptr(ell), _stream_handle(torch)))
    else:
        _lib.check(lib.mdfit_objective_form(ptr(tm), ptr(ts), ptr(ty), ptr(tN), ptr(tu), n, int(form), ptr(F),
                                            ptr(g), ptr(H), ptr(ell), _stream_handle(torch)))
    torch.cuda.current_stream().synchronize()
    return F.cpu().numpy(), g.cpu().numpy(), H.cpu().numpy(), ell.cpu().numpy()
