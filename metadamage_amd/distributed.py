"""Taxon sharding across GPUs and the single result gather.

The fit is embarrassingly parallel over taxa (fits.py:428-469 fits one taxon
with no shared state), so the multi-GPU path is: each rank (one process per
GPU, torch.distributed over RCCL) fits a contiguous shard of taxa in df_counts
order, then ONE gather moves every rank's packed result records to rank 0,
which writes the parquet files.  There is no other collective on the data path.

Works with any torch.distributed backend: "nccl" (= RCCL on ROCm, device
tensors) on the GPU box, "gloo" (host tensors) in the CPU tests.
"""

from __future__ import annotations

import os

import numpy as np

from . import _lib

# One gathered per-taxon record (496 bytes): the 25 result columns of out as
# the frames store them -- the 8 count columns (N_z1_*, N_sum_*, y_sum_*) as
# f64 (exact integers up to 2^53; the frames' uint32 range check runs on rank 0)
# and the 17 others rounded to f32 on the device, as downcast_dataframe rounds
# them (utils.py:329-356: make_df_fit_results writes them float32, so the
# frames are bit-identical to a single-process run) -- | pred f32[3*30] |
# status i32.  The record's 7 reserved doubles and its 48 per-sub-fit
# diagnostic doubles stay on the rank that fitted them.
NRES_GATHER = _lib.NRESULT
INT_LO, INT_HI = 7, 15  # result columns N_z1_forward .. y_sum_total (include/mdfit.h: MDFIT_F_N_Z1_FORWARD ..)
FLOAT_COLS = [j for j in range(NRES_GATHER) if not INT_LO <= j < INT_HI]
REC_INT = (INT_HI - INT_LO) * 8
REC_F32 = len(FLOAT_COLS) * 4
REC_PRED = _lib.NPRED * _lib.NPOS * 4
REC_RES = REC_INT + REC_F32
REC_BYTES = REC_RES + REC_PRED + 4
REC_OUT = _lib.NOUT * 8  # the full record the kernel writes (rank-local)
# with_laplace (a "map-laplace" run): one more f32 block [n, 3, NLAPLACE] after
# the status, 96 B per taxon, in the same buffer and the same single gather
REC_LAP = 3 * _lib.NLAPLACE * 4
# with_diag (a "nuts-diag" run; never together with with_laplace): the same for
# the sampling diagnostics, one more f32 block [n, 6, NNUTSDIAG], 288 B per taxon
REC_DIAG = _lib.NSUBFIT * _lib.NNUTSDIAG * 4
# with_summary (a "nuts-summary" run; never together with either): the same for
# the posterior summaries, one more f32 block [n, 6, NNUTSSUMM], 384 B per taxon
REC_SUMM = _lib.NSUBFIT * _lib.NNUTSSUMM * 4
# with_loo (a "nuts-loo" run; never together with any of them): the same for the
# PSIS-LOO records, one more f32 block [n, 7, NNUTSLOO], 224 B per taxon
REC_LOO = _lib.NLOOROW * _lib.NNUTSLOO * 4
# with_psis (a "map-psis" run; never together with any of them): the same for the
# importance-sampled posteriors, one more f32 block [n, 3, NMAPPSIS], 192 B per taxon
REC_PSIS = 3 * _lib.NMAPPSIS * 4
# with_waic (a "map-waic" run; never together with any of them): the same for the
# importance-weighted WAIC records, one more f32 block [n, 7, NMAPWAIC], 224 B per taxon
REC_WAIC = _lib.NWAICROW * _lib.NMAPWAIC * 4
# with_evidence (a "map-evidence" run; never together with any of them): the importance-sampled evidence records
# have the WAIC records' shape, f32 [n, 7, NMAPEVID], and take their place in the layout
REC_EVID = _lib.NEVIDROW * _lib.NMAPEVID * 4
assert REC_EVID == REC_WAIC


def _evidence_as_waic(with_evidence: bool, with_waic: bool, *others: bool) -> bool:
    """The with_waic switch of the layout for a run with the evidence block (its only extra block)."""
    if with_evidence and (with_waic or any(others)):
        raise ValueError("with_evidence, with_ppred, with_auto, with_waic, with_psis, with_loo, with_summary, with_diag "
                         "and with_laplace are mutually exclusive: one extra block per run")
    return bool(with_waic or with_evidence)
# with_auto (an "auto" run; never together with any of them): the same for the
# auto block, one more f32 block [n, NAUTO] = route, sampled, khat_max, ess_min, 16 B per taxon
REC_AUTO = _lib.NAUTO * 4
# with_ppred (a "map-pred" run; never together with any of them): the same for the
# posterior predictive, one more f32 block [n, 106] = ppred [3][30] | rec [NMAPPRED], 424 B per taxon
REC_PPRED = (_lib.NPRED * _lib.NPOS + _lib.NMAPPRED) * 4
# psis_adapt > 0 (with the psis, waic or auto block: with_adapt; with the ppred block: with_ppred_adapt): one more f32
# block [n, 2] behind it, 8 B per taxon
REC_ADAPT = _lib.NADAPTOUT * 4
# auto_pred (with the auto block): one more f32 block [n, NAUTOPRED] = pred_ess_min, pred_distinct_min behind the
# auto block and before the adapt block, 8 B per taxon
REC_AUTO_PRED = _lib.NAUTOPRED * 4


def _check_adapt(with_adapt: bool, with_psis: bool, with_waic: bool, with_auto: bool, with_ppred: bool = False,
                 with_auto_pred: bool = False, with_ppred_adapt: bool = False) -> int:
    """The bytes per taxon behind the run's extra block: the auto-pred block, then the adapt block (with_adapt
    beside the psis, waic or auto block; with_ppred_adapt, its own switch, beside the ppred block)."""
    if with_adapt and not (with_psis or with_waic or with_auto):
        raise ValueError("with_adapt goes with with_psis, with_waic or with_auto")
    if with_ppred_adapt and not with_ppred:
        raise ValueError("with_ppred_adapt goes with with_ppred")
    if with_auto_pred and not with_auto:
        raise ValueError("with_auto_pred goes with with_auto")
    return (REC_AUTO_PRED if with_auto_pred else 0) + (REC_ADAPT if with_adapt or with_ppred_adapt else 0)


def _extra(with_laplace: bool, with_diag: bool, with_summary: bool = False, with_loo: bool = False,
           with_psis: bool = False, with_waic: bool = False, with_auto: bool = False,
           with_ppred: bool = False) -> int:
    if with_ppred:
        if with_laplace or with_diag or with_summary or with_loo or with_psis or with_waic or with_auto:
            raise ValueError("with_ppred, with_auto, with_waic, with_psis, with_loo, with_summary, with_diag and "
                             "with_laplace are mutually exclusive: one extra block per run")
        return REC_PPRED
    if with_auto:
        if with_laplace or with_diag or with_summary or with_loo or with_psis or with_waic:
            raise ValueError("with_auto, with_waic, with_psis, with_loo, with_summary, with_diag and with_laplace "
                             "are mutually exclusive: one extra block per run")
        return REC_AUTO
    if with_waic:
        if with_laplace or with_diag or with_summary or with_loo or with_psis:
            raise ValueError("with_waic, with_psis, with_loo, with_summary, with_diag and with_laplace are mutually "
                             "exclusive: one extra block per run")
        return REC_WAIC
    if with_psis:
        if with_laplace or with_diag or with_summary or with_loo:
            raise ValueError("with_psis, with_loo, with_summary, with_diag and with_laplace are mutually exclusive: "
                             "one extra block per run")
        return REC_PSIS
    if with_laplace and with_diag:
        raise ValueError("with_laplace (MAP) and with_diag (NUTS) are mutually exclusive")
    if with_summary and (with_laplace or with_diag):
        raise ValueError("with_summary, with_diag and with_laplace are mutually exclusive: one extra block per run")
    if with_loo:
        if with_laplace or with_diag or with_summary:
            raise ValueError("with_loo, with_summary, with_diag and with_laplace are mutually exclusive: "
                             "one extra block per run")
        return REC_LOO
    return REC_LAP if with_laplace else (REC_DIAG if with_diag else (REC_SUMM if with_summary else 0))


def shard_range(n_taxa: int, rank: int, world: int) -> tuple[int, int]:
    """Contiguous shard [lo, hi) of rank `rank`: ceil-split so shards differ by
    at most one taxon."""
    if world < 1 or not (0 <= rank < world):
        raise ValueError(f"bad rank/world {rank}/{world}")
    per = -(-n_taxa // world) if n_taxa else 0
    lo = min(rank * per, n_taxa)
    hi = min(lo + per, n_taxa)
    return lo, hi


def shard_capacity(n_taxa: int, world: int) -> int:
    """Padded shard size (every rank gathers the same number of records)."""
    return -(-n_taxa // world) if n_taxa else 0


class Records:
    """Rank-local result buffers of a shard of n taxa: `out` f64[n, NOUT] (the
    kernel's full record), and one uint8 gather buffer `buf` of n * REC_BYTES
    bytes holding ints f64[n, 8] | floats f32[n, 17] | pred f32[n, 3, 30] |
    status i32[n].  The kernel writes pred and status in place; `stage()`
    copies the result columns of out into ints / floats (two strided device
    copies, the second rounding to f32) before the gather.  with_laplace: the
    buffer is n * REC_LAP bytes longer, `lap` f32[n, 3, 8] after the status,
    written in place by the chunked dispatch.  with_diag: likewise n * REC_DIAG
    bytes, `diag` f32[n, 6, 12]; with_summary: n * REC_SUMM bytes, `summ` f32[n,
    6, 16]; with_loo: n * REC_LOO bytes, `loo` f32[n, 7, 8]; with_psis: n *
    REC_PSIS bytes, `psis` f32[n, 3, 16]; with_waic: n * REC_WAIC bytes, `waic`
    f32[n, 7, 8]; with_auto: n * REC_AUTO bytes, `auto` f32[n, 4]; with_ppred: n
    * REC_PPRED bytes, `ppred` f32[n, 106]; with_evidence: n * REC_EVID bytes,
    `evid` f32[n, 7, 8], where with_waic's block would lie.  At most one of the
    nine."""

    def __init__(self, n: int, device, with_laplace: bool = False, with_diag: bool = False,
                 with_summary: bool = False, with_loo: bool = False, with_psis: bool = False,
                 with_waic: bool = False, with_auto: bool = False, with_ppred: bool = False,
                 with_adapt: bool = False, with_auto_pred: bool = False, with_ppred_adapt: bool = False,
                 with_evidence: bool = False):
        import torch

        with_waic = _evidence_as_waic(with_evidence, with_waic, with_laplace, with_diag, with_summary, with_loo,
                                      with_psis, with_auto, with_ppred)
        self.n = n
        self.out = torch.empty((n, _lib.NOUT), dtype=torch.float64, device=device)
        extra = _extra(with_laplace, with_diag, with_summary, with_loo, with_psis, with_waic, with_auto, with_ppred)
        tail = _check_adapt(with_adapt, with_psis, with_waic, with_auto, with_ppred, with_auto_pred, with_ppred_adapt)
        self.buf = torch.empty(n * (REC_BYTES + extra + tail), dtype=torch.uint8, device=device)
        self.lap = self.diag = self.summ = self.loo = self.psis = self.waic = self.auto = self.ppred = None
        self.adapt = self.auto_pred = None
        o5 = n * (REC_BYTES + extra)  # (behind the run's extra block; the views below stop before it)
        if with_auto_pred:
            self.auto_pred = self.buf[o5 : o5 + n * REC_AUTO_PRED].view(dtype=torch.float32).view(n, _lib.NAUTOPRED)
            o5 += n * REC_AUTO_PRED
        if with_adapt or with_ppred_adapt:
            self.adapt = self.buf[o5 : o5 + n * REC_ADAPT].view(dtype=torch.float32).view(n, _lib.NADAPTOUT)
        if with_ppred:
            self.pred, self.status, self.ints, self.floats, self.ppred = packed_views(self.buf, n, with_ppred=True)
        elif with_auto:
            self.pred, self.status, self.ints, self.floats, self.auto = packed_views(self.buf, n, with_auto=True)
        elif with_laplace:
            self.pred, self.status, self.ints, self.floats, self.lap = packed_views(self.buf, n, with_laplace=True)
        elif with_diag:
            self.pred, self.status, self.ints, self.floats, self.diag = packed_views(self.buf, n, with_diag=True)
        elif with_summary:
            self.pred, self.status, self.ints, self.floats, self.summ = packed_views(self.buf, n, with_summary=True)
        elif with_loo:
            self.pred, self.status, self.ints, self.floats, self.loo = packed_views(self.buf, n, with_loo=True)
        elif with_psis:
            self.pred, self.status, self.ints, self.floats, self.psis = packed_views(self.buf, n, with_psis=True)
        elif with_waic:
            self.pred, self.status, self.ints, self.floats, self.waic = packed_views(self.buf, n, with_waic=True)
        else:
            self.pred, self.status, self.ints, self.floats = packed_views(self.buf, n)
        self.evid = None
        if with_evidence:  # (the [n, 7, 8] block is the evidence records')
            self.evid, self.waic = self.waic, None
        self._fidx = torch.as_tensor(FLOAT_COLS, device=device)

    def stage(self):
        self.ints.copy_(self.out[:, INT_LO:INT_HI])
        self.floats.copy_(self.out.index_select(1, self._fidx))  # (f64 -> f32: round to nearest even, as numpy)
        return self.buf


def packed_views(buf, n: int, with_laplace: bool = False, with_diag: bool = False, with_summary: bool = False,
                 with_loo: bool = False, with_psis: bool = False, with_waic: bool = False, with_auto: bool = False,
                 with_ppred: bool = False):
    """Views (pred[n, 3, 30] f32, status[n] i32, ints[n, 8] f64, floats[n, 17]
    f32) into one uint8 gather buffer of n * REC_BYTES bytes laid out ints |
    floats | pred | status (torch tensor; the f64 block first keeps it 8-byte
    aligned for any n).  with_laplace: the buffer holds n * REC_LAP more bytes
    and a fifth view, lap[n, 3, 8] f32, follows the status; with_diag: n *
    REC_DIAG more bytes and the fifth view is diag[n, 6, 12] f32; with_summary: n
    * REC_SUMM more bytes and the fifth view is summ[n, 6, 16] f32; with_loo: n *
    REC_LOO more bytes and the fifth view is loo[n, 7, 8] f32; with_psis: n *
    REC_PSIS more bytes and the fifth view is psis[n, 3, 16] f32; with_waic: n *
    REC_WAIC more bytes and the fifth view is waic[n, 7, 8] f32; with_auto: n *
    REC_AUTO more bytes and the fifth view is auto[n, 4] f32; with_ppred: n *
    REC_PPRED more bytes and the fifth view is ppred[n, 106] f32."""
    _extra(with_laplace, with_diag, with_summary, with_loo, with_psis, with_waic, with_auto, with_ppred)
    o1 = n * REC_INT
    o2 = o1 + n * REC_F32
    o3 = o2 + n * REC_PRED
    ints = buf[:o1].view(dtype=_torch_dtype("float64")).view(n, INT_HI - INT_LO)
    floats = buf[o1:o2].view(dtype=_torch_dtype("float32")).view(n, len(FLOAT_COLS))
    pred = buf[o2:o3].view(dtype=_torch_dtype("float32")).view(n, _lib.NPRED, _lib.NPOS)
    status = buf[o3 : o3 + 4 * n].view(dtype=_torch_dtype("int32"))
    if with_ppred:
        o4 = o3 + 4 * n
        ppred = buf[o4 : o4 + n * REC_PPRED].view(dtype=_torch_dtype("float32")).view(n, REC_PPRED // 4)
        return pred, status, ints, floats, ppred
    if with_auto:
        o4 = o3 + 4 * n
        auto = buf[o4 : o4 + n * REC_AUTO].view(dtype=_torch_dtype("float32")).view(n, _lib.NAUTO)
        return pred, status, ints, floats, auto
    if with_laplace:
        o4 = o3 + 4 * n
        lap = buf[o4 : o4 + n * REC_LAP].view(dtype=_torch_dtype("float32")).view(n, 3, _lib.NLAPLACE)
        return pred, status, ints, floats, lap
    if with_diag:
        o4 = o3 + 4 * n
        diag = buf[o4 : o4 + n * REC_DIAG].view(dtype=_torch_dtype("float32")).view(n, _lib.NSUBFIT, _lib.NNUTSDIAG)
        return pred, status, ints, floats, diag
    if with_summary:
        o4 = o3 + 4 * n
        summ = buf[o4 : o4 + n * REC_SUMM].view(dtype=_torch_dtype("float32")).view(n, _lib.NSUBFIT, _lib.NNUTSSUMM)
        return pred, status, ints, floats, summ
    if with_loo:
        o4 = o3 + 4 * n
        loo = buf[o4 : o4 + n * REC_LOO].view(dtype=_torch_dtype("float32")).view(n, _lib.NLOOROW, _lib.NNUTSLOO)
        return pred, status, ints, floats, loo
    if with_psis:
        o4 = o3 + 4 * n
        psis = buf[o4 : o4 + n * REC_PSIS].view(dtype=_torch_dtype("float32")).view(n, 3, _lib.NMAPPSIS)
        return pred, status, ints, floats, psis
    if with_waic:
        o4 = o3 + 4 * n
        waic = buf[o4 : o4 + n * REC_WAIC].view(dtype=_torch_dtype("float32")).view(n, _lib.NWAICROW, _lib.NMAPWAIC)
        return pred, status, ints, floats, waic
    return pred, status, ints, floats


def round_like_gather(out: np.ndarray) -> np.ndarray:
    """The 25 result columns of host records out[T, >= 25] as the gather
    carries them (the 17 non-count columns rounded to f32), float64[T, 25]."""
    o = np.array(out[:, :NRES_GATHER], dtype=np.float64)
    o[:, FLOAT_COLS] = o[:, FLOAT_COLS].astype(np.float32).astype(np.float64)
    return o


def _torch_dtype(name):
    import torch

    return getattr(torch, name)


def alloc_records(n: int, device, with_laplace: bool = False, with_diag: bool = False,
                  with_summary: bool = False, with_loo: bool = False, with_psis: bool = False,
                  with_waic: bool = False, with_auto: bool = False, with_ppred: bool = False,
                  with_adapt: bool = False, with_auto_pred: bool = False, with_ppred_adapt: bool = False,
                  with_evidence: bool = False) -> Records:
    """with_adapt (psis_adapt > 0, beside with_psis, with_waic or with_auto), or
    with_ppred_adapt (the same beside with_ppred): the buffer is n * REC_ADAPT
    bytes longer, `adapt` f32[n, 2] behind the extra block.  with_auto_pred (beside with_auto): n * REC_AUTO_PRED bytes
    longer, `auto_pred` f32[n, 2] behind the auto block and before `adapt`."""
    return Records(n, device, with_laplace, with_diag, with_summary, with_loo, with_psis, with_waic, with_auto,
                   with_ppred, with_adapt, with_auto_pred, with_ppred_adapt, with_evidence)


def gather_records(buf, n_cap: int, rank: int, world: int, group=None, async_op: bool = False):
    """Gather every rank's staged gather buffer (Records.stage(), n_cap records
    each) to rank 0.
    Returns a list of `world` buffers on rank 0, None elsewhere.  This is the
    one collective of the multi-GPU path (ncclGather semantics).  Under the
    gloo backend (CPU tests, or ranks sharing one GPU in a test) a device
    buffer is staged to host first: gloo gathers host tensors only.

    async_op=True returns (parts, work) instead: the collective is queued
    behind the work already on the current stream and runs on the backend's
    own stream, so the caller can fit the next batch into other buffers while
    it moves; `work.wait()` orders the current stream after it (and must
    precede any reuse of `buf` or any read of `parts`)."""
    import torch.distributed as dist

    if world == 1 and not (dist.is_available() and dist.is_initialized()):
        return ([buf], None) if async_op else [buf]
    if buf.is_cuda and dist.get_backend(group) == "gloo":
        buf = buf.cpu()
    parts = [buf.new_empty(buf.shape) for _ in range(world)] if rank == 0 else None
    work = dist.gather(buf, gather_list=parts, dst=0, group=group, async_op=async_op)
    return (parts, work) if async_op else parts


def all_ranks_agree(flag: bool) -> bool:
    """True iff `flag` is true on every rank (a one-int all-reduce; no process
    group: flag).
    Used so that all ranks take the same branch before a collective (e.g. a
    cache hit must skip the fit on every rank or on none)."""
    import torch
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()):
        return bool(flag)
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else "cpu"
    t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MIN)
    return bool(int(t.item()))


def init_from_env(backend: str | None = None) -> tuple[int, int]:
    """Join the torch.distributed job described by the torchrun environment
    (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*): one process per GPU, the
    rank's GPU selected BEFORE any other device call, backend "nccl" (RCCL
    over xGMI) unless given.  WORLD_SIZE 1 (or unset): nothing to join.
    Returns (rank, world)."""
    rank, local, world = env_rank_world()
    if world <= 1:
        return 0, 1
    import torch
    import torch.distributed as dist

    if dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    backend = backend or "nccl"
    if backend == "nccl":
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        dist.init_process_group(backend)
    return dist.get_rank(), dist.get_world_size()


def shutdown(ok: bool = True) -> None:
    """Leave the process group.  ok=True (the run succeeded on this rank): a
    barrier first, so no rank tears the group down under a peer's last
    collective.  ok=False (this rank raised): no barrier -- an NCCL barrier is
    itself a one-element all-reduce and could pair with a healthy peer's
    agreement all-reduce or result gather, leaving the job hung until the
    collective timeout; the group is torn down (RCCL: the communicator
    aborted) so the peers' pending collectives fail and the job exits."""
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()):
        return
    if ok:
        dist.barrier()
        dist.destroy_process_group()
        return
    from torch.distributed import distributed_c10d as c10d

    abort = getattr(c10d, "_abort_process_group", None)
    if dist.get_backend() == "nccl" and abort is not None:
        abort()  # tears the communicators down without waiting on peers
    if dist.is_initialized():
        dist.destroy_process_group()


def run_distributed(fn, *args, **kwargs):
    """Join the torchrun job (init_from_env), run fn, leave the group: with a
    barrier when fn returned, without one when it raised (shutdown(ok=False)),
    re-raising so the launcher tears the job down."""
    init_from_env()
    try:
        result = fn(*args, **kwargs)
    except BaseException:
        shutdown(ok=False)
        raise
    shutdown(ok=True)
    return result


def unpack_gathered(parts, n_taxa: int, world: int, with_laplace: bool = False, with_diag: bool = False,
                    with_summary: bool = False, with_loo: bool = False, with_psis: bool = False,
                    with_waic: bool = False, with_auto: bool = False, with_ppred: bool = False,
                    with_adapt: bool = False, with_auto_pred: bool = False, with_ppred_adapt: bool = False,
                    with_evidence: bool = False):
    """Concatenate gathered shards back into df_counts order (host numpy);
    the parts may be device (RCCL) or host (gloo) buffers.  with_laplace: the
    parts carry the Laplace block and a fourth array lap[T, 3, 8] f32 is returned;
    with_diag: the diagnostics block, returned as diag[T, 6, 12] f32;
    with_summary: the summaries block, returned as summ[T, 6, 16] f32; with_loo:
    the PSIS-LOO block, returned as loo[T, 7, 8] f32; with_psis: the
    importance-sampled posteriors, returned as psis[T, 3, 16] f32; with_waic: the
    importance-weighted WAIC records, returned as waic[T, 7, 8] f32; with_auto:
    the auto block, returned as auto[T, 4] f32; with_ppred: the posterior
    predictive block, returned as ppred[T, 106] f32.  with_adapt (beside
    with_psis, with_waic or with_auto; with_ppred_adapt beside with_ppred): the
    parts carry the adapt block behind it, returned last as adapt[T, 2] f32.  with_auto_pred (beside
    with_auto): the parts carry the auto-pred block behind the auto block,
    returned behind auto[T, 4] as auto_pred[T, 2] f32.  with_evidence: the
    importance-sampled evidence records in with_waic's place, returned as
    evid[T, 7, 8] f32 (with_adapt goes with it too)."""
    import torch

    with_waic = _evidence_as_waic(with_evidence, with_waic, with_laplace, with_diag, with_summary, with_loo, with_psis,
                                  with_auto, with_ppred)
    outs, preds, sts, laps, adapts, apreds = [], [], [], [], [], []
    rec_extra = _extra(with_laplace, with_diag, with_summary, with_loo, with_psis, with_waic, with_auto, with_ppred)
    rec_bytes = REC_BYTES + rec_extra + _check_adapt(with_adapt, with_psis, with_waic, with_auto, with_ppred,
                                                     with_auto_pred, with_ppred_adapt)
    with_adapt = with_adapt or with_ppred_adapt
    extra = with_laplace or with_diag or with_summary or with_loo or with_psis or with_waic or with_auto or with_ppred
    if parts and parts[0].is_cuda:
        # every part's D2H copy queued at once into one pinned host buffer,
        # then one synchronisation (not a blocking copy per part)
        n = sum(p.numel() for p in parts)
        host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        off = []
        o0 = 0
        for p in parts:
            host[o0 : o0 + p.numel()].copy_(p, non_blocking=True)
            off.append(o0)
            o0 += p.numel()
        torch.cuda.current_stream(parts[0].device).synchronize()
        parts = [host[o : o + p.numel()] for o, p in zip(off, parts)]
    for r, part in enumerate(parts):
        lo, hi = shard_range(n_taxa, r, world)
        n_cap = part.numel() // rec_bytes
        p, s, ints, floats, *rest = packed_views(part, n_cap, with_laplace=with_laplace, with_diag=with_diag,
                                                 with_summary=with_summary, with_loo=with_loo, with_psis=with_psis,
                                                 with_waic=with_waic, with_auto=with_auto,
                                                 with_ppred=with_ppred)
        if extra:
            laps.append(rest[0][: hi - lo].numpy())
        o5 = n_cap * (REC_BYTES + rec_extra)
        if with_auto_pred:
            ap = part[o5 : o5 + n_cap * REC_AUTO_PRED].view(dtype=_torch_dtype("float32")).view(n_cap, _lib.NAUTOPRED)
            apreds.append(ap[: hi - lo].numpy())
            o5 += n_cap * REC_AUTO_PRED
        if with_adapt:
            ad = part[o5 : o5 + n_cap * REC_ADAPT].view(dtype=_torch_dtype("float32")).view(n_cap, _lib.NADAPTOUT)
            adapts.append(ad[: hi - lo].numpy())
        o = np.empty((hi - lo, NRES_GATHER), np.float64)
        o[:, INT_LO:INT_HI] = ints[: hi - lo].numpy()
        o[:, FLOAT_COLS] = floats[: hi - lo].numpy()
        outs.append(o)
        preds.append(p[: hi - lo].numpy())
        sts.append(s[: hi - lo].numpy())
    if with_adapt or with_auto_pred:
        return ((np.concatenate(outs), np.concatenate(preds), np.concatenate(sts), np.concatenate(laps))
                + ((np.concatenate(apreds),) if with_auto_pred else ())
                + ((np.concatenate(adapts),) if with_adapt else ()))
    if extra:
        return np.concatenate(outs), np.concatenate(preds), np.concatenate(sts), np.concatenate(laps)
    return np.concatenate(outs), np.concatenate(preds), np.concatenate(sts)


def env_rank_world() -> tuple[int, int, int]:
    """(rank, local_rank, world_size) from the torch.distributed.run environment."""
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    return rank, local, world
