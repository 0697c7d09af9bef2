"""The drop-in fit boundary: get_fits / compute_fits over the HIP engine.

Mirrors /root/reference/metadamage/fits.py at its operator boundary:

  get_fits(df_counts, cfg)        fits.py:754-807  (cache check, top-N, fit, save)
  get_top_max_fits                fits.py:736-751
  compute_fits(df_counts, cfg)    fits.py:709-730  -> ONE batched device call
  make_df_fit_results_*           fits.py:668-680
  make_df_fit_predictions_*       fits.py:632-665

What changes is the body of compute_fits: instead of a process pool running
numpyro NUTS per taxon (fits.py:477-626), the counts table is packed once into
the dense layout of include/mdfit.h (the batched group_to_numpyro_data,
fits.py:398-419) and fitted by mdfit_fit_batch on the GPU(s); taxa the engine
flags (status != 0) are dropped with a warning, like the reference drops taxa
whose fit timed out (fits.py:520-522, 603-606).
"""

from __future__ import annotations

import logging
import warnings

import numpy as np
import pandas as pd

from . import _lib, blocks, io, utils

logger = logging.getLogger(__name__)

MM_COLUMNS = ["AC", "AG", "AT", "CA", "CG", "CT", "GA", "GC", "GT", "TA", "TC", "TG"]
POSITIONS = np.concatenate([np.arange(1, 16), -np.arange(1, 16)])

# fit_results column order (fits.py:244-293, 317-356, 374-376 + :671)
FIT_RESULT_COLUMNS = (
    ["tax_id", "tax_name", "tax_rank"]
    + _lib.RESULT_FIELDS[:7]
    + ["N_alignments"]
    + _lib.RESULT_FIELDS[7:]
    + ["shortname"]
)
# "map-laplace": the Laplace columns appended after shortname --
# (column, row of the Laplace record: 0 PMD-all, 1 forward, 2 reverse, its field)
LAPLACE_COLUMNS = (
    [(name, 0, f) for name, f in (("D_max_std", "D_max_std"), ("significance", "significance"), ("q_std", "q_std"),
                                   ("A_std", "A_std"), ("c_std", "c_std"), ("concentration_std", "phi_std"),
                                   ("rho_Ac", "rho_Ac"))]
    + [("D_max_std_forward", 1, "D_max_std"), ("q_std_forward", 1, "q_std"),
       ("D_max_std_reverse", 2, "D_max_std"), ("q_std_reverse", 2, "q_std")]
)
# "nuts-diag": the sampling diagnostics appended after shortname,
# float32 -- (column, row of the diag record: 0 PMD-all, 1 null-all, its field);
# n_sigma is a WAIC difference of those two chains
_NUTS_DIAG_PICKS = (
    [(f, 0, f) for f in _lib.NUTSDIAG_FIELDS[:11]]
    + [("ess_q_null", 1, "ess_q"), ("ess_phi_null", 1, "ess_phi"), ("rhat_q_null", 1, "rhat_q"),
       ("rhat_phi_null", 1, "rhat_phi")]
)
# ... then the worst series of all six sub-fits (nanmin / nanmax), then uint32
# divergences (summed over the six chains) and nuts_diag_valid (all six rows valid)
NUTS_DIAG_COLUMNS = [name for name, _, _ in _NUTS_DIAG_PICKS] + ["ess_min", "rhat_max"]
NUTS_DIAG_UINT_COLUMNS = ["divergences", "nuts_diag_valid"]
# "nuts-summary": the posterior summaries appended after shortname (DESIGN.md
# §9.2), float32 -- (column, row of the summary record: 0 PMD-all, 2
# PMD-forward, 3 PMD-reverse, its field).  The first eleven are the
# LAPLACE_COLUMNS' names in their order: downstream code reads one set of names,
# and the metadata's `inference` says which estimate they hold
_NUTS_SUMMARY_PICKS = (
    [("D_max_std", 0, "D_max_std"), ("significance", 0, "significance"), ("q_std", 0, "q_std"),
     ("A_std", 0, "A_std"), ("c_std", 0, "c_std"), ("concentration_std", 0, "phi_std"), ("rho_Ac", 0, "rho_Ac"),
     ("D_max_std_forward", 2, "D_max_std"), ("q_std_forward", 2, "q_std"),
     ("D_max_std_reverse", 3, "D_max_std"), ("q_std_reverse", 3, "q_std"),
     ("D_max_posterior_median", 0, "D_max_median"), ("D_max_posterior_lower_hpdi", 0, "D_max_lo"),
     ("D_max_posterior_upper_hpdi", 0, "D_max_hi"), ("q_median", 0, "q_median"), ("q_lower_hpdi", 0, "q_lo"),
     ("q_upper_hpdi", 0, "q_hi"), ("concentration_median", 0, "phi_median")]
)
NUTS_SUMMARY_COLUMNS = [name for name, _, _ in _NUTS_SUMMARY_PICKS]
# ... then uint32 nuts_summary_valid: the rows 0, 2 and 3 all valid
NUTS_SUMMARY_UINT_COLUMNS = ["nuts_summary_valid"]
_NUTS_SUMMARY_ROWS = (0, 2, 3)
# "nuts-loo": the PSIS-LOO model comparison appended after shortname (DESIGN.md
# §9.3), float32 -- (column, row of the loo record: 0 PMD-all, 1 null-all, 6 the
# comparisons, its field index)
_NUTS_LOO_PICKS = (
    [("elpd_loo", 0, 0), ("p_loo", 0, 1), ("elpd_loo_se", 0, 2), ("pareto_k_max", 0, 3),
     ("elpd_loo_null", 1, 0), ("p_loo_null", 1, 1), ("pareto_k_max_null", 1, 3),
     ("n_sigma_loo", 6, 0), ("n_sigma_loo_forward", 6, 1), ("n_sigma_loo_reverse", 6, 2), ("asymmetry_loo", 6, 3)]
)
NUTS_LOO_COLUMNS = [name for name, _, _ in _NUTS_LOO_PICKS]
# ... then uint32 pareto_k_bad (the points of the six sub-fits with khat above the
# threshold: row 6's count) and nuts_loo_valid (row 6's valid bit: all six rows valid)
NUTS_LOO_UINT_COLUMNS = ["pareto_k_bad", "nuts_loo_valid"]
# "map-psis": the importance-sampled posterior appended after shortname
# (DESIGN.md §3.8), float32 -- (column, row of the record: 0 PMD-all, 1 forward,
# 2 reverse, its field).  The first eleven are the LAPLACE_COLUMNS' names in
# their order, as in "nuts-summary"
_MAP_PSIS_PICKS = (
    [(name, row, f) for name, row, f in LAPLACE_COLUMNS]
    + [("D_max_posterior_mean", 0, "D_max_mean"), ("q_posterior_mean", 0, "q_mean"),
       ("concentration_posterior_mean", 0, "phi_mean"),
       ("D_max_posterior_mean_forward", 1, "D_max_mean"), ("D_max_posterior_mean_reverse", 2, "D_max_mean"),
       ("pareto_k", 0, "khat"), ("pareto_k_forward", 1, "khat"), ("pareto_k_reverse", 2, "khat"),
       ("psis_ess", 0, "ess")]
)
MAP_PSIS_COLUMNS = [name for name, _, _ in _MAP_PSIS_PICKS]
# ... then uint32 map_psis_valid (all three rows valid) and map_psis_reliable
# (valid, and all three khat at or below the threshold)
MAP_PSIS_UINT_COLUMNS = ["map_psis_valid", "map_psis_reliable"]
# "map-psis" with quantiles (mdfit_map_quant, MDFIT-QUANT v1): behind map-psis's columns the weighted
# order statistics of that posterior, float32 -- (column, row of the record, its field).  The first seven are
# "nuts-summary"'s names in its order
_MAP_QUANT_PICKS = [("D_max_posterior_median", 0, "D_max_median"), ("D_max_posterior_lower_hpdi", 0, "D_max_lo"),
                    ("D_max_posterior_upper_hpdi", 0, "D_max_hi"), ("q_median", 0, "q_median"),
                    ("q_lower_hpdi", 0, "q_lo"), ("q_upper_hpdi", 0, "q_hi"),
                    ("concentration_median", 0, "phi_median"), ("A_median", 0, "A_median"),
                    ("c_median", 0, "c_median"), ("D_max_posterior_q05", 0, "D_max_q05"),
                    ("D_max_posterior_q95", 0, "D_max_q95"), ("D_max_prob_above", 0, "D_max_p_above"),
                    ("D_max_posterior_median_forward", 1, "D_max_median"),
                    ("D_max_posterior_median_reverse", 2, "D_max_median")]
MAP_QUANT_COLUMNS = [name for name, _, _ in _MAP_QUANT_PICKS]
# ... then uint32 quant_window_min (the least number of draws in D_max's interval over the three rows; 0 when a row
# has none) and map_quant_valid (all three rows valid)
MAP_QUANT_UINT_COLUMNS = ["quant_window_min", "map_quant_valid"]
# "map-waic": the importance-weighted WAIC comparison appended after shortname
# (DESIGN.md §3.9), float32 -- (column, row of the record: 0 PMD-all, 1 null-all,
# 6 the comparisons, its field index) ...
_MAP_WAIC_PICKS = (
    [("n_sigma_waic", 6, 0), ("n_sigma_waic_forward", 6, 1), ("n_sigma_waic_reverse", 6, 2), ("asymmetry_waic", 6, 3),
     ("p_waic", 0, 1), ("p_waic_null", 1, 1), ("elpd_waic", 0, 0), ("elpd_waic_null", 1, 0),
     ("pareto_k_waic", 6, 4), ("waic_ess_min", 6, 5)]
)
MAP_WAIC_COLUMNS = [name for name, _, _ in _MAP_WAIC_PICKS]
# ... then uint32 map_waic_valid (row 6's bit 0: all six rows valid) and
# map_waic_reliable (its bit 1: valid, and all six khat at or below the threshold)
MAP_WAIC_UINT_COLUMNS = ["map_waic_valid", "map_waic_reliable"]
# "map-evidence": the importance-sampled evidence and Bayes factors appended after shortname,
# float32 -- (column, row of the record: 0 PMD-all, 1 null-all, 6 the comparisons, its field index); between
# log_evidence_null and pareto_k_evidence stands damage_probability = 1 / (1 + exp(-log_bf)), formed in float64 ...
_MAP_EVIDENCE_PICKS = [("log_bf", 6, 0), ("log_bf_forward", 6, 1), ("log_bf_reverse", 6, 2), ("log_bf_asymmetry", 6, 3),
                       ("log_bf_se", 6, 4), ("log_evidence", 0, 0), ("log_evidence_null", 1, 0),
                       ("pareto_k_evidence", 6, 5), ("evidence_ess_min", 6, 6)]
MAP_EVIDENCE_COLUMNS = ([name for name, _, _ in _MAP_EVIDENCE_PICKS[:7]] + ["damage_probability"]
                        + [name for name, _, _ in _MAP_EVIDENCE_PICKS[7:]])
# ... then uint32 map_evidence_valid (row 6's bit 0: all six rows valid) and map_evidence_reliable (its bit 1:
# valid, and all six khat at or below the threshold)
MAP_EVIDENCE_UINT_COLUMNS = ["map_evidence_valid", "map_evidence_reliable"]
# a "map-pred" run (mdfit_map_pred, MDFIT-PPRED v1): the posterior predictive D_max columns from
# importance-weighted draws, their worst k-hat and least ess / distinct draws over the three PMD rows
_MAP_PRED_PICKS = [("D_max_predictive", "D_max"), ("D_max_predictive_lower_hpdi", "D_max_lower_hpdi"),
                   ("D_max_predictive_upper_hpdi", "D_max_upper_hpdi"), ("D_max_predictive_forward", "D_max_forward"),
                   ("D_max_predictive_reverse", "D_max_reverse")]
MAP_PRED_COLUMNS = [name for name, _ in _MAP_PRED_PICKS] + ["pareto_k_pred", "pred_ess_min"]
MAP_PRED_UINT_COLUMNS = ["pred_distinct_min", "map_pred_valid", "map_pred_reliable"]
MAP_PRED_PREDICTION_COLUMNS = ["median_posterior", "hdpi_lower_posterior", "hdpi_upper_posterior"]
# "map-pred" with ppc (mdfit_map_ppc, MDFIT-PPC v1): behind map-pred's columns the posterior
# predictive check of the PMD fit -- the two p-values and the mean observed discrepancies (float32), the reference's
# z (+1..+15, -1..-15; 0: none) of the column with the smallest two-sided mid-p (int8), that mid-p (float32), the
# number of columns where it is below 0.05 (uint8) and the record's valid bit (bool); ppc_p in the predictions frame
_PPC_PICKS = [("ppc_p_outlier", "p_outlier"), ("ppc_p_strand", "p_strand"), ("ppc_t_outlier", "t_outlier"),
              ("ppc_t_strand", "t_strand")]
PPC_COLUMNS = [name for name, _ in _PPC_PICKS] + ["ppc_worst_position", "ppc_p_worst", "ppc_n_low", "ppc_valid"]
PPC_PREDICTION_COLUMNS = ["ppc_p"]
# "auto": the auto block appended after shortname -- uint32
# auto_route (the mdfit_auto_route bits) and auto_sampled (1: the row is the
# sampler's), then float32 pareto_k_max and psis_ess_min (row 6 of the waic
# record: the largest khat and the smallest ess of the six sub-fits)
AUTO_UINT_COLUMNS = ["auto_route", "auto_sampled"]
AUTO_COLUMNS = ["pareto_k_max", "psis_ess_min"]
# "auto" with auto_pred (MDFIT-AUTO v1.1): behind them pred_ess_min (float32) and pred_distinct_min
# (uint32, 0 where the taxon is sampled), the least ess and distinct importance draws over the three PMD rows of the
# predictive the settled taxon's D_max columns and prediction rows come from
AUTO_PRED_COLUMNS = ["pred_ess_min", "pred_distinct_min"]
# psis_adapt > 0 ("map-psis", "map-waic", "map-evidence", "map-pred", "auto"): the last two columns -- the largest round-0 Pareto-k over the PMD
# rows (float32) and the largest best round of MDFIT-ADAPT v1 (uint32)
ADAPT_COLUMNS = ["pareto_k_initial", "psis_adapt_rounds"]
INT_RESULT_FIELDS = {"N_alignments", "N_z1_forward", "N_z1_reverse", "N_sum_forward", "N_sum_reverse",
                     "N_sum_total", "y_sum_forward", "y_sum_reverse", "y_sum_total"}


# --------------------------------------------------------------------------
# packing: df_counts -> dense [T][32] tensors (batched group_to_numpyro_data)
# --------------------------------------------------------------------------
class Packed:
    def __init__(self, tax_id, tax_name, tax_rank, N_alignments, y, N, mm, cats=None, pinned=None):
        self.tax_id = tax_id
        self.tax_name = tax_name
        self.tax_rank = tax_rank
        self.N_alignments = N_alignments
        self.y = y
        self.N = N
        self.mm = mm
        # per-taxon pd.Categorical of tax_id / tax_name / tax_rank when df_counts
        # had them (sorted categories): the frames reuse their order instead of
        # re-sorting a million names
        self.cats = cats or {}
        # the engine.PinnedPack y / N / mm live in (main.main's pipeline), handed
        # back to its pool once the device has them (release_pinned)
        self.pinned = pinned

    def release_pinned(self):
        """Return the pinned buffer set; y / N / mm are gone afterwards."""
        if self.pinned is not None:
            from . import engine

            engine.release_pinned_pack(self.pinned)
            self.pinned = None
            self.y = self.N = self.mm = None

    @property
    def n_taxa(self):
        return len(self.tax_id)


def _as_u32(a: np.ndarray) -> np.ndarray:
    """uint32 view/copy of a count column, with utils.py:338-339's range check."""
    if a.dtype == np.uint32:
        return a
    if a.size and (int(a.max()) > np.iinfo(np.uint32).max or int(a.min()) < 0):
        raise AssertionError("Dataframe contains too large values.")
    return a.astype(np.uint32)


def _interleave(cols, out2d: np.ndarray) -> None:
    """out2d[:, j] = cols[j], natively over row ranges (ingest.interleave:
    numpy's strided column writes take ~0.09 s of the GIL-holding main
    thread on a 2.8 M x 12 table)."""
    from . import ingest

    ingest.interleave(cols, out2d)


def _first_values(s: pd.Series, first: np.ndarray) -> np.ndarray:
    """s.to_numpy()[first] without materialising a categorical column."""
    return np.asarray(s.array[first]) if isinstance(s.dtype, pd.CategoricalDtype) else s.to_numpy()[first]


def _first_categoricals(df: pd.DataFrame, first: np.ndarray) -> dict:
    out = {}
    for c in ("tax_id", "tax_name", "tax_rank"):
        col = df[c]
        if isinstance(col.dtype, pd.CategoricalDtype) and col.cat.categories.is_monotonic_increasing:
            out[c] = col.array[first]
    return out


def pack_counts(df: pd.DataFrame, cfg, pinned: bool = False) -> Packed:
    """Dense y/N (uint32[T][32]) and mismatch counts (uint32[T][30][12]) in
    df order (first appearance of each tax_id, i.e. the N_alignments-desc
    order of sort_by_alignments).  Column i < 15 holds z = i+1 (y = the
    forward substitution, N = its reference-base sum), i >= 15 holds
    z = -(i-14) (reverse substitution) — group_to_numpyro_data, fits.py:398-419.
    Rows are placed by their position value, so missing positions read as
    N = 0 (no information) instead of shifting the others.  The usual table
    (every taxon with its 30 rows in sort_by_alignments order) is packed by
    reshaping; anything else is scattered row by row."""
    fwd, rev = cfg.substitution_bases_forward, cfg.substitution_bases_reverse
    tax = df["tax_id"]
    # rows without a tax_id belong to no taxon: the reference's
    # groupby("tax_id", observed=True) drops missing keys (fits.py:736-744,
    # 398-419), so they are dropped here before any index is formed (a -1
    # index would scatter them onto the last taxon's row)
    missing = tax.isna().to_numpy()
    if missing.any():
        df = df[~missing]
        tax = df["tax_id"]
    codes = tax.cat.codes.to_numpy() if isinstance(tax.dtype, pd.CategoricalDtype) else None

    def packed(first, y, N, mm, pp):
        return Packed(
            tax_id=_first_values(tax, first),
            tax_name=_first_values(df["tax_name"], first),
            tax_rank=_first_values(df["tax_rank"], first),
            N_alignments=df["N_alignments"].to_numpy()[first].astype(np.int64),
            y=y,
            N=N,
            mm=mm,
            cats=_first_categoricals(df, first),
            pinned=pp,
        )

    # the usual table (counts.compute_counts: 30 rows per taxon in z order,
    # uint32 counts): one native pass writes y, N and mm and checks the layout
    pos = df["position"].to_numpy()
    n = len(tax)
    if codes is not None and n and n % _lib.NPOS == 0 and pos.dtype == np.int8 and len(tax.cat.categories) < 2**31:
        cols = [df[c].to_numpy() for c in (*MM_COLUMNS, fwd, rev, fwd[0], rev[0])]
        if all(c.dtype == np.uint32 for c in cols):
            from . import ingest

            T = n // _lib.NPOS
            y, N, mm, pp = _pack_buffers(T, pinned, zero=False)
            T = ingest.pack_dense(np.ascontiguousarray(codes, dtype=np.int32), len(tax.cat.categories), pos,
                                  [np.ascontiguousarray(c) for c in cols], y, N, mm)
            if T >= 0:
                return packed(np.arange(T, dtype=np.int64) * _lib.NPOS, y, N, mm, pp)
            if pp is not None:
                from . import engine

                engine.release_pinned_pack(pp)
    # taxon index in first-appearance order (pd.factorize) and each taxon's first row
    if codes is not None and len(tax.cat.categories) < 2**31:
        from . import ingest

        t, first = ingest.first_index(codes, len(tax.cat.categories))
    else:
        t, _ = pd.factorize(tax.to_numpy())
        t = t.astype(np.int64)
        first = np.flatnonzero(np.r_[True, t[1:] > np.maximum.accumulate(t[:-1])]) if t.size else np.zeros(0, np.int64)
    n = t.size
    T = first.size
    pos_fwd = pos > 0
    yv = _as_u32(np.where(pos_fwd, df[fwd].to_numpy(), df[rev].to_numpy()))
    Nv = _as_u32(np.where(pos_fwd, df[fwd[0]].to_numpy(), df[rev[0]].to_numpy()))
    mm_cols = [_as_u32(df[c].to_numpy()) for c in MM_COLUMNS]
    dense = n == T * _lib.NPOS and np.array_equal(
        pos.reshape(T, _lib.NPOS), np.broadcast_to(POSITIONS.astype(pos.dtype), (T, _lib.NPOS))) and np.array_equal(
        t.reshape(T, _lib.NPOS), np.broadcast_to(np.arange(T)[:, None], (T, _lib.NPOS)))
    y, N, mm, pp = _pack_buffers(T, pinned, zero=True)
    if dense:
        y[:, :_lib.NPOS] = yv.reshape(T, _lib.NPOS)
        N[:, :_lib.NPOS] = Nv.reshape(T, _lib.NPOS)
        _interleave(mm_cols, mm.reshape(-1, _lib.NMM))
    else:
        p64 = pos.astype(np.int64)
        col = np.where(p64 > 0, p64 - 1, 14 - p64)
        ok = (p64 != 0) & (np.abs(p64) <= 15)
        if not ok.all():
            logger.warning(f"{int((~ok).sum())} rows with |position| outside 1..15 ignored")
        y[t[ok], col[ok]] = yv[ok]
        N[t[ok], col[ok]] = Nv[ok]
        mm.fill(0)
        rows = np.empty((n, _lib.NMM), np.uint32)
        _interleave(mm_cols, rows)
        mm.reshape(-1, _lib.NMM)[(t * _lib.NPOS + col)[ok]] = rows[ok]
    return packed(first, y, N, mm, pp)


def _pack_buffers(T: int, pinned: bool, zero: bool):
    """y, N (uint32[T][LD]) and mm (uint32[T][30][12]) for pack_counts, in a
    pinned buffer set when pinned (main.main's reader threads: the device copy
    reads them directly); zero: y and N zero-filled."""
    pp = None
    if pinned and T > 0:
        from . import engine

        pp = engine.acquire_pinned_pack(T)
    if pp is not None:
        y, N, mm = pp.views(T)
        if zero:
            y.fill(0)
            N.fill(0)
    else:
        alloc = np.zeros if zero else np.empty
        y = alloc((T, _lib.LD), np.uint32)
        N = alloc((T, _lib.LD), np.uint32)
        mm = np.empty((T, _lib.NPOS, _lib.NMM), np.uint32)
    return y, N, mm, pp


# --------------------------------------------------------------------------
# the device call (single GPU or sharded over torch.distributed ranks)
# --------------------------------------------------------------------------
def fit_packed(p: Packed, opts=None, shard: bool = True, psis_draws: int = 256, pred_draws: int = 1000,
               psis_adapt: int = 0, auto_pred: bool = False, ppc: bool = False, quantiles: bool = False,
               dmax_threshold: float = 0.01, joint: bool = False, **named):
    """Run mdfit_fit_batch on the packed taxa; returns host (out, pred, status)
    on rank 0 (None elsewhere in a multi-GPU job).  shard=False fits every
    taxon on this rank's GPU (main() shards whole files across ranks).
    named (at most one block of blocks.BLOCKS by its name, e.g. laplace=True):
    the block's launch follows the fit (engine.ChunkedFitter) and a fourth
    array, the block's f32 [T, *shape], is returned; the sampled blocks take
    psis_draws draws per sub-fit, ppred also pred_draws predictive draws per
    job.  auto: the auto inference instead (engine.fit_auto_chunks: the MAP fit,
    its importance-sampled correction and the sampler over the taxa that does
    not settle; opts carries both fits' options); its chunks run one after
    another, with no transfer overlap.
    psis_adapt > 0 (with a sampled block): the importance sampling adapts its
    proposals in at most that many rounds (MDFIT-ADAPT v1) and one more array
    adapt[T, 2] f32 = (largest round-0 khat, largest best round) is returned,
    last.  auto_pred (with auto; MDFIT-AUTO v1.1): a settled taxon's
    predictive columns and prediction rows are the importance-weighted posterior
    predictive from pred_draws draws per job, and auto_pred[T, 2] f32 =
    (pred_ess_min, pred_distinct_min) is returned behind the auto block.  ppc
    (with ppred; MDFIT-PPC v1): mdfit_map_ppc follows each chunk's map_pred
    launch and ppc[T, 42] f32 = ppos | rec is returned directly behind the
    ppred block.  quantiles (with psis; MDFIT-QUANT v1): mdfit_map_quant follows
    each chunk's map_psis launch and quant[T, 48] f32, the three rows of
    _lib.MAPQUANT_FIELDS with P(D_max > dmax_threshold), is returned directly
    behind the psis block.  joint (with waic): each chunk's map_waic launch is
    the fused mdfit_map_joint and joint[T, 104] f32 = evid | psis
    (engine.split_joint) is returned directly behind the waic block."""
    import torch

    from . import engine

    if not torch.cuda.is_available():
        raise _lib.MdfitError("metadamage_amd fits run on MI355X GPUs only (no HIP device visible)")
    import torch.distributed as dist

    # the sharded branch whenever a process group is up (a world of one
    # included: one gather to itself, which is how a one-GPU box runs the
    # RCCL path, tests/test_gpu_distributed.py)
    grouped = shard and dist.is_available() and dist.is_initialized()
    world = dist.get_world_size() if grouped else 1
    rank = dist.get_rank() if grouped else 0
    dev = torch.device("cuda", torch.cuda.current_device())
    # add_noise_estimates (fits.py:359-376) runs in the assembly kernel on the
    # shipped mismatch counts: 1,440 B/taxon of asynchronous PCIe (~0.7 ms per
    # 10k taxa, bench host_to_host) costs no host time, while the host
    # statistics (ingest.noise) take ~1.5 ms of CPU per 10k taxa on the 16-thread
    # share of a multi-file pipeline that is host-bound
    # (the block's mode is checked against opts where the fit is planned: engine.staging)
    tails = {"psis_adapt": psis_adapt, "auto_pred": auto_pred, "ppc": ppc, "quantiles": quantiles, "joint": joint}
    run = blocks.describe(None, tails, check_mode=False, psis_draws=psis_draws, pred_draws=pred_draws,
                          dmax_threshold=dmax_threshold, **{"with_" + name: on for name, on in named.items()})
    try:
        if grouped:
            return _fit_sharded(p, opts, dev, rank, world, run)
        if run.block is not None and not run.block.chunked:
            return engine.fit_auto_chunks(p.y, p.N, p.mm, opts, device=dev, **run.options)
        return engine.fit_batch_host(p.y, p.N, p.mm, opts, pinned=p.pinned, **run.options, **named)
    finally:
        p.release_pinned()  # (the call synchronised, or raised: the pinned set goes back either way)


def _fit_sharded(p: Packed, opts, dev, rank: int, world: int, run: blocks.Run):
    import torch

    from . import engine
    from .distributed import alloc_records, gather_records, shard_capacity, shard_range, unpack_gathered

    lo, hi = shard_range(p.n_taxa, rank, world)
    if opts is not None:  # the sampler's streams are keyed by the global taxon index
        opts = _lib.MdfitOpts.from_buffer_copy(opts)
        opts.index_base = opts.index_base + lo
    cap = shard_capacity(p.n_taxa, world)
    block = run.block
    rec = alloc_records(cap, dev, **run.layout)
    # the rows are written in place into the gather buffers
    dest = engine.FitBatch(rec.out[: hi - lo], rec.pred[: hi - lo], rec.status[: hi - lo],
                           **{part.attr: getattr(rec, part.attr)[: hi - lo] for part in run.parts})
    mm = p.mm[lo:hi] if p.mm is not None else None
    if hi > lo and block is not None and not block.chunked:  # each rank runs auto on its shard
        engine.fit_auto_chunks(p.y[lo:hi], p.N[lo:hi], mm, opts, device=dev, dest=dest, **run.options)
        torch.cuda.synchronize(dev)
    elif hi > lo:  # the shard through the bounded-memory chunked dispatch
        with engine._STAGING_LOCK:
            st = engine.staging(hi - lo, device=dev, opts=opts, with_mm=mm is not None, dest_on_device=True,
                                **run.options, **({block.switch: True} if block is not None else {}))
            st.run_into_device(p.y[lo:hi], p.N[lo:hi], mm, opts, dest)
            torch.cuda.synchronize(dev)  # (the chunks' pinned input staging is reused by the next call)
    p.release_pinned()
    buf = rec.stage()
    torch.cuda.synchronize(dev)
    parts = gather_records(buf, cap, rank, world)
    if rank != 0:
        return None
    return unpack_gathered(parts, p.n_taxa, world, **run.layout)


# --------------------------------------------------------------------------
# frames (fits.py:632-680)
# --------------------------------------------------------------------------
def _category(p: Packed, name: str, keep, repeat: int = 1) -> pd.Categorical:
    """astype("category") of np.repeat(getattr(p, name)[keep], repeat) (keep
    None: every taxon):
    categories = the sorted distinct values.  From the packed categorical when
    there is one (its categories are sorted already), else by factorising the
    per-taxon values once (the predictions repeat each taxon 30 times)."""
    cat = p.cats.get(name)
    if cat is None:
        v = getattr(p, name)
        c = pd.Categorical(v if keep is None else v[keep])
    else:
        # remove_unused_categories by a presence table instead of np.unique's
        # sort (the categories stay in their sorted order)
        codes = cat.codes if keep is None else cat.codes[keep]
        used = np.zeros(len(cat.categories), bool)
        used[codes[codes >= 0]] = True
        if used.all():
            c = pd.Categorical.from_codes(codes, dtype=cat.dtype)
        else:
            remap = (np.cumsum(used) - 1).astype(codes.dtype)
            c = pd.Categorical.from_codes(np.where(codes >= 0, remap[np.maximum(codes, 0)], -1).astype(codes.dtype),
                                          cat.categories[used])
    return pd.Categorical.from_codes(np.repeat(c.codes, repeat), dtype=c.dtype) if repeat != 1 else c


def _const_category(value, n: int) -> pd.Categorical:
    """astype("category") of a column holding one value (no categories when empty)."""
    return pd.Categorical.from_codes(np.zeros(n, np.int8), [value] if n else [])


def _uint32(v: np.ndarray) -> np.ndarray:
    if v.size and int(v.max()) > np.iinfo(np.uint32).max:
        raise AssertionError("Dataframe contains too large values.")  # utils.py:338-339
    return v.astype(np.uint32)


def _record_columns(out, keep, ncol: int, block: int = 2048) -> np.ndarray:
    """The first ncol columns of the kept rows of the row-major record as a
    column-major float64[ncol][n], transposed block by block (a column gathered
    from the 640-B record rows touches one cache line per taxon; a whole-array
    transposed copy ~4x slower than these cache-sized blocks)."""
    idx = None if keep is None else np.flatnonzero(keep)
    n = out.shape[0] if idx is None else idx.size
    cols = np.empty((ncol, n), np.float64)
    for i in range(0, n, block):
        rows = out[i:i + block, :ncol] if idx is None else out[idx[i:i + block], :ncol]
        cols[:, i:i + block] = rows.T
    return cols


def _psis_columns(kp, data) -> list:
    """The MAP_PSIS_COLUMNS and MAP_PSIS_UINT_COLUMNS of the kept psis records kp[n, 3, 16] into data; their names."""
    for name, row, field in _MAP_PSIS_PICKS:
        data[name] = np.ascontiguousarray(kp[:, row, _lib.MAPPSIS_FIELDS.index(field)], dtype=np.float32)
    flags = np.nan_to_num(kp[:, :, _lib.MAPPSIS_FIELDS.index("flags")]).astype(np.int64)
    valid = ((flags & _lib.MAPPSIS_VALID) != 0).all(axis=1)
    data["map_psis_valid"] = valid.astype(np.uint32)
    data["map_psis_reliable"] = (valid & ((flags & _lib.MAPPSIS_RELIABLE) != 0).all(axis=1)).astype(np.uint32)
    return MAP_PSIS_COLUMNS + MAP_PSIS_UINT_COLUMNS


def _evidence_columns(ke, data) -> list:
    """The MAP_EVIDENCE_COLUMNS and MAP_EVIDENCE_UINT_COLUMNS of the kept evidence records ke[n, 7, 8] into data;
    their names."""
    for name, row, field in _MAP_EVIDENCE_PICKS:
        data[name] = np.ascontiguousarray(ke[:, row, field], dtype=np.float32)
    with np.errstate(over="ignore"):  # (exp(-log_bf) = inf: probability 0)
        data["damage_probability"] = (1.0 / (1.0 + np.exp(-ke[:, 6, 0].astype(np.float64)))).astype(np.float32)
    flags = np.nan_to_num(ke[:, 6, _lib.MAPEVID_COMPARE_FIELDS.index("flags")]).astype(np.int64)
    data["map_evidence_valid"] = ((flags & _lib.MAPEVID_VALID) != 0).astype(np.uint32)
    data["map_evidence_reliable"] = ((flags & _lib.MAPEVID_RELIABLE) != 0).astype(np.uint32)
    return MAP_EVIDENCE_COLUMNS + MAP_EVIDENCE_UINT_COLUMNS


def make_df_fit_results(p: Packed, out, keep, cfg, lap=None, diag=None, summ=None, loo=None,
                        psis=None, waic=None, auto=None, ppred=None, adapt=None, auto_pred=None,
                        evid=None, ppc=None, quant=None, joint=None) -> pd.DataFrame:
    """One row per fitted taxon in FIT_RESULT_COLUMNS order with the dtypes of
    downcast_dataframe (fits.py:668-680 + utils.py:329-356): names
    categorical, integer fields uint32, the rest float32.  lap (the Laplace
    records [T, 3, 8] of a "map-laplace" run): the LAPLACE_COLUMNS follow as
    float32, then laplace_valid (uint32: the valid bit of the PMD-all row).
    diag (the sampling diagnostics [T, 6, 12] of a "nuts-diag" run, as
    fit_packed returns them): the NUTS_DIAG_COLUMNS follow as float32, then the
    NUTS_DIAG_UINT_COLUMNS.  summ (the posterior summaries [T, 6, 16] of a
    "nuts-summary" run): the NUTS_SUMMARY_COLUMNS follow as float32, then
    nuts_summary_valid (uint32: the PMD rows 0, 2 and 3 all valid).  loo (the
    PSIS-LOO records [T, 7, 8] of a "nuts-loo" run): the NUTS_LOO_COLUMNS follow
    as float32, then pareto_k_bad and nuts_loo_valid (uint32).  psis (the
    importance-sampled posteriors [T, 3, 16] of a "map-psis" run): the
    MAP_PSIS_COLUMNS follow as float32, then map_psis_valid and
    map_psis_reliable (uint32).  waic (the importance-weighted WAIC records [T,
    7, 8] of a "map-waic" run): the MAP_WAIC_COLUMNS follow as float32, then
    map_waic_valid and map_waic_reliable (uint32).  auto (the auto block [T, 4]
    of an "auto" run): auto_route and auto_sampled (uint32), then pareto_k_max
    and psis_ess_min (float32) follow.  ppred (the posterior predictive block
    [T, 106] of a "map-pred" run): the MAP_PRED_COLUMNS follow as float32, then
    the MAP_PRED_UINT_COLUMNS.  auto_pred (the auto-pred block [T, 2] of an
    "auto" run with auto_pred): pred_ess_min (float32) and pred_distinct_min
    (uint32) follow the auto columns.  ppc (the posterior predictive check's
    block [T, 42] of a "map-pred" run with ppc): the PPC_COLUMNS follow
    map-pred's, in their own dtypes.  quant (the weighted order statistics'
    block [T, 48] of a "map-psis" run with quantiles): the MAP_QUANT_COLUMNS
    follow map-psis's as float32, then the MAP_QUANT_UINT_COLUMNS.  joint (the
    block [T, 104] = evid | psis of a "map-waic" run with joint): behind
    map-waic's columns map-evidence's, then map-psis's, each formed as from
    evid= and psis=.  adapt (the adapt block [T, 2] of a run with
    psis_adapt > 0): pareto_k_initial (float32) and psis_adapt_rounds (uint32)
    are the last two columns."""
    n = int(keep.sum())
    keep = None if n == len(keep) else keep  # (every taxon kept: no row selection)
    data = {
        "tax_id": _category(p, "tax_id", keep),
        "tax_name": _category(p, "tax_name", keep),
        "tax_rank": _category(p, "tax_rank", keep),
    }
    cols = _record_columns(out, keep, _lib.NRESULT)
    for j, name in enumerate(_lib.RESULT_FIELDS):
        v = cols[j]
        data[name] = _uint32(np.rint(v).astype(np.int64)) if name in INT_RESULT_FIELDS else v.astype(np.float32)
    data["N_alignments"] = _uint32(p.N_alignments if keep is None else p.N_alignments[keep])
    data["shortname"] = _const_category(cfg.shortname, n)
    columns = list(FIT_RESULT_COLUMNS)
    if lap is not None:
        kl = np.asarray(lap) if keep is None else np.asarray(lap)[keep]
        for name, row, field in LAPLACE_COLUMNS:
            data[name] = np.ascontiguousarray(kl[:, row, _lib.LAPLACE_FIELDS.index(field)], dtype=np.float32)
        flags = kl[:, 0, _lib.LAPLACE_FIELDS.index("flags")].astype(np.int64)
        data["laplace_valid"] = ((flags & _lib.LAPLACE_VALID) != 0).astype(np.uint32)
        columns += [name for name, _, _ in LAPLACE_COLUMNS] + ["laplace_valid"]
    if diag is not None:
        kd = np.asarray(diag) if keep is None else np.asarray(diag)[keep]
        for name, row, field in _NUTS_DIAG_PICKS:
            data[name] = np.ascontiguousarray(kd[:, row, _lib.NUTSDIAG_FIELDS.index(field)], dtype=np.float32)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # (a row of NaN: NaN)
            data["ess_min"] = np.nanmin(kd[:, :, 0:5].reshape(n, -1), axis=1).astype(np.float32)
            data["rhat_max"] = np.nanmax(kd[:, :, 5:10].reshape(n, -1), axis=1).astype(np.float32)
        flags = np.nan_to_num(kd[:, :, _lib.NUTSDIAG_FIELDS.index("flags")]).astype(np.int64)
        data["divergences"] = _uint32((flags >> 1).sum(axis=1))
        data["nuts_diag_valid"] = ((flags & _lib.NUTSDIAG_VALID) != 0).all(axis=1).astype(np.uint32)
        columns += NUTS_DIAG_COLUMNS + NUTS_DIAG_UINT_COLUMNS
    if summ is not None:
        ks = np.asarray(summ) if keep is None else np.asarray(summ)[keep]
        for name, row, field in _NUTS_SUMMARY_PICKS:
            data[name] = np.ascontiguousarray(ks[:, row, _lib.NUTSSUMM_FIELDS.index(field)], dtype=np.float32)
        flags = np.nan_to_num(ks[:, _NUTS_SUMMARY_ROWS, _lib.NUTSSUMM_FIELDS.index("flags")]).astype(np.int64)
        data["nuts_summary_valid"] = ((flags & _lib.NUTSSUMM_VALID) != 0).all(axis=1).astype(np.uint32)
        columns += NUTS_SUMMARY_COLUMNS + NUTS_SUMMARY_UINT_COLUMNS
    if loo is not None:
        kl = np.asarray(loo) if keep is None else np.asarray(loo)[keep]
        for name, row, field in _NUTS_LOO_PICKS:
            data[name] = np.ascontiguousarray(kl[:, row, field], dtype=np.float32)
        cmp_ = _lib.NUTSLOO_COMPARE_FIELDS.index
        data["pareto_k_bad"] = _uint32(np.nan_to_num(kl[:, 6, cmp_("n_bad")]).astype(np.int64))
        flags = np.nan_to_num(kl[:, 6, cmp_("flags")]).astype(np.int64)
        data["nuts_loo_valid"] = ((flags & _lib.NUTSLOO_VALID) != 0).astype(np.uint32)
        columns += NUTS_LOO_COLUMNS + NUTS_LOO_UINT_COLUMNS
    if psis is not None:
        columns += _psis_columns(np.asarray(psis) if keep is None else np.asarray(psis)[keep], data)
    if quant is not None:
        kq = np.asarray(quant).reshape(-1, 3, _lib.NMAPQUANT)
        kq = kq if keep is None else kq[keep]
        f = _lib.MAPQUANT_FIELDS.index
        for name, row, field in _MAP_QUANT_PICKS:
            data[name] = np.ascontiguousarray(kq[:, row, f(field)], dtype=np.float32)
        data["quant_window_min"] = np.nan_to_num(kq[:, :, f("n_window")], nan=0.0).min(axis=1).astype(np.uint32)
        flags = np.nan_to_num(kq[:, :, f("flags")]).astype(np.int64)
        data["map_quant_valid"] = ((flags & _lib.MAPPSIS_VALID) != 0).all(axis=1).astype(np.uint32)
        columns += MAP_QUANT_COLUMNS + MAP_QUANT_UINT_COLUMNS
    if waic is not None:
        kw = np.asarray(waic) if keep is None else np.asarray(waic)[keep]
        for name, row, field in _MAP_WAIC_PICKS:
            data[name] = np.ascontiguousarray(kw[:, row, field], dtype=np.float32)
        flags = np.nan_to_num(kw[:, 6, _lib.MAPWAIC_COMPARE_FIELDS.index("flags")]).astype(np.int64)
        data["map_waic_valid"] = ((flags & _lib.MAPWAIC_VALID) != 0).astype(np.uint32)
        data["map_waic_reliable"] = ((flags & _lib.MAPWAIC_RELIABLE) != 0).astype(np.uint32)
        columns += MAP_WAIC_COLUMNS + MAP_WAIC_UINT_COLUMNS
    if joint is not None:
        if waic is None or psis is not None or evid is not None:
            raise ValueError("joint goes with waic, and neither psis nor evid beside it")
        kj = np.asarray(joint).reshape(-1, _lib.NJOINTOUT)
        kj = kj if keep is None else kj[keep]
        n_ev = _lib.NEVIDROW * _lib.NMAPEVID
        columns += _evidence_columns(kj[:, :n_ev].reshape(-1, _lib.NEVIDROW, _lib.NMAPEVID), data)
        columns += _psis_columns(kj[:, n_ev:].reshape(-1, 3, _lib.NMAPPSIS), data)
    if evid is not None:
        columns += _evidence_columns(np.asarray(evid) if keep is None else np.asarray(evid)[keep], data)
    if auto is not None:
        ka = np.asarray(auto) if keep is None else np.asarray(auto)[keep]
        data["auto_route"] = _uint32(np.nan_to_num(ka[:, 0]).astype(np.int64))
        data["auto_sampled"] = _uint32(np.nan_to_num(ka[:, 1]).astype(np.int64))
        data["pareto_k_max"] = np.ascontiguousarray(ka[:, 2], dtype=np.float32)
        data["psis_ess_min"] = np.ascontiguousarray(ka[:, 3], dtype=np.float32)
        columns += AUTO_UINT_COLUMNS + AUTO_COLUMNS
    if auto_pred is not None:
        kq = np.asarray(auto_pred) if keep is None else np.asarray(auto_pred)[keep]
        data["pred_ess_min"] = np.ascontiguousarray(kq[:, 0], dtype=np.float32)
        data["pred_distinct_min"] = _uint32(np.nan_to_num(kq[:, 1]).astype(np.int64))
        columns += AUTO_PRED_COLUMNS
    if ppred is not None:
        kr = np.asarray(ppred)[:, _lib.NPRED * _lib.NPOS:]
        kr = kr if keep is None else kr[keep]
        f = _lib.MAPPRED_FIELDS.index
        for name, field in _MAP_PRED_PICKS:
            data[name] = np.ascontiguousarray(kr[:, f(field)], dtype=np.float32)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # (three invalid rows: NaN)
            data["pareto_k_pred"] = np.nanmax(kr[:, f("khat_all"):f("khat_all") + 3], axis=1).astype(np.float32)
            data["pred_ess_min"] = np.nanmin(kr[:, f("ess_all"):f("ess_all") + 3], axis=1).astype(np.float32)
            nd = np.nanmin(kr[:, f("n_distinct_all"):f("n_distinct_all") + 3], axis=1)
        data["pred_distinct_min"] = _uint32(np.nan_to_num(nd).astype(np.int64))
        flags = np.nan_to_num(kr[:, f("flags")]).astype(np.int64)
        data["map_pred_valid"] = ((flags & _lib.MAPPRED_VALID) != 0).astype(np.uint32)
        data["map_pred_reliable"] = ((flags & _lib.MAPPRED_RELIABLE) != 0).astype(np.uint32)
        columns += MAP_PRED_COLUMNS + MAP_PRED_UINT_COLUMNS
    if ppc is not None:
        kc = np.asarray(ppc)[:, _lib.NPOS:]
        kc = kc if keep is None else kc[keep]
        f = _lib.MAPPPC_FIELDS.index
        for name, field in _PPC_PICKS:
            data[name] = np.ascontiguousarray(kc[:, f(field)], dtype=np.float32)
        worst = kc[:, f("worst_pos")]
        col = np.nan_to_num(worst, nan=0.0).astype(np.int64)
        data["ppc_worst_position"] = np.where(np.isnan(worst), 0, POSITIONS[col]).astype(np.int8)
        data["ppc_p_worst"] = np.ascontiguousarray(kc[:, f("p_worst")], dtype=np.float32)
        data["ppc_n_low"] = np.nan_to_num(kc[:, f("n_low")]).astype(np.uint8)
        flags = np.nan_to_num(kc[:, f("flags")]).astype(np.int64)
        data["ppc_valid"] = (flags & _lib.MAPPPC_VALID) != 0
        columns += PPC_COLUMNS
    if adapt is not None:
        kd = np.asarray(adapt) if keep is None else np.asarray(adapt)[keep]
        data["pareto_k_initial"] = np.ascontiguousarray(kd[:, 0], dtype=np.float32)
        data["psis_adapt_rounds"] = _uint32(np.nan_to_num(kd[:, 1]).astype(np.int64))
        columns += ADAPT_COLUMNS
    return pd.DataFrame({c: data[c] for c in columns}, copy=False)


def make_df_fit_predictions(p: Packed, pred, keep, cfg, ppred=None, ppc=None) -> pd.DataFrame:
    """fits.py:632-665: 30 rows per fitted taxon (z = 1..15, -1..-15).  ppred
    (the posterior predictive block [T, 106] of a "map-pred" run): the
    MAP_PRED_PREDICTION_COLUMNS follow as float32.  ppc (the posterior
    predictive check's block [T, 42]): ppc_p, the upper mid-p of the position's
    observed count, follows as float32."""
    n = int(keep.sum())
    kp = pred if n == len(keep) else pred[keep]
    data = {
        "tax_id": _category(p, "tax_id", None if n == len(keep) else keep, _lib.NPOS),
        "position": np.tile(POSITIONS.astype(np.int8), n),
        "median": np.ascontiguousarray(kp[:, 0, :], dtype=np.float32).reshape(-1),
        "hdpi_lower": np.ascontiguousarray(kp[:, 1, :], dtype=np.float32).reshape(-1),
        "hdpi_upper": np.ascontiguousarray(kp[:, 2, :], dtype=np.float32).reshape(-1),
        "shortname": _const_category(cfg.shortname, n * _lib.NPOS),
    }
    if ppred is not None:
        pp = np.asarray(ppred)[:, :_lib.NPRED * _lib.NPOS].reshape(-1, _lib.NPRED, _lib.NPOS)
        pp = pp if n == len(keep) else pp[keep]
        for j, name in enumerate(MAP_PRED_PREDICTION_COLUMNS):
            data[name] = np.ascontiguousarray(pp[:, j, :], dtype=np.float32).reshape(-1)
    if ppc is not None:
        pc = np.asarray(ppc)[:, :_lib.NPOS]
        pc = pc if n == len(keep) else pc[keep]
        data["ppc_p"] = np.ascontiguousarray(pc, dtype=np.float32).reshape(-1)
    return pd.DataFrame(data, copy=False)


def make_opts(cfg, mcmc_kwargs=None):
    """Engine options for cfg.inference: "nuts" (the reference's sampler,
    num_warmup / num_samples from mcmc_kwargs as fits.py:792-799 passes them)
    "nuts-diag" (the same call; wants_diag adds the sampling diagnostics),
    "nuts-summary" (the same call; wants_summary adds the posterior summaries),
    "nuts-loo" (the same call; wants_loo adds the PSIS-LOO model comparison), "map"
    "map-laplace" (the MAP fit; wants_laplace adds the standard errors) or
    "map-psis" (the MAP fit; wants_psis adds the importance-sampled posterior) or
    "map-waic" (the MAP fit; wants_waic adds the importance-weighted WAIC comparison) or
    "map-evidence" (the MAP fit; wants_evidence adds the importance-sampled evidence and Bayes factors) or
    "map-pred" (the MAP fit; wants_pred adds the importance-weighted posterior predictive) or
    "auto" (one option set for the MAP fit and the sampler of engine.fit_auto_device:
    the sampler's mode and lengths, the MAP fit's defaults)."""
    inference = getattr(cfg, "inference", "nuts")
    if mode_of(inference) == _lib.MODE_MAP:
        return _lib.default_opts(mode=_lib.MODE_MAP)
    kw = mcmc_kwargs or {}
    return _lib.default_opts(mode=_lib.MODE_NUTS, num_warmup=int(kw.get("num_warmup", 500)),
                             num_samples=int(kw.get("num_samples", 1000)))


# the engine mode of every --inference value: the plain fits, then each block's ("auto" runs both: its option set is
# the sampler's, engine.auto_opts makes the MAP copy)
_MODE_OF = {"map": _lib.MODE_MAP, "nuts": _lib.MODE_NUTS,
            **{b.inference: _lib.MODE_NUTS if b.mode is None else b.mode for b in blocks.BLOCKS}}


def mode_of(inference: str) -> int:
    """The engine mode of an --inference value: "nuts" and the nuts-* values
    (the sampler), "map" and the map-* values, or "auto" (the sampler's)."""
    if inference not in _MODE_OF:
        raise ValueError("inference must be " + ", ".join(repr(k) for k in _MODE_OF) + f", got {inference!r}")
    return _MODE_OF[inference]


def wants_diag(cfg) -> bool:
    """cfg.inference "nuts-diag": the sampler followed by mdfit_nuts_diag."""
    return getattr(cfg, "inference", "nuts") == "nuts-diag"


def wants_summary(cfg) -> bool:
    """cfg.inference "nuts-summary": the sampler followed by mdfit_nuts_summary."""
    return getattr(cfg, "inference", "nuts") == "nuts-summary"


def wants_loo(cfg) -> bool:
    """cfg.inference "nuts-loo": the sampler followed by mdfit_nuts_loo."""
    return getattr(cfg, "inference", "nuts") == "nuts-loo"


def wants_laplace(cfg) -> bool:
    """cfg.inference "map-laplace": the MAP fit followed by mdfit_map_laplace."""
    return getattr(cfg, "inference", "nuts") == "map-laplace"


def wants_psis(cfg) -> bool:
    """cfg.inference "map-psis": the MAP fit followed by mdfit_map_psis."""
    return getattr(cfg, "inference", "nuts") == "map-psis"


def wants_waic(cfg) -> bool:
    """cfg.inference "map-waic": the MAP fit followed by mdfit_map_waic."""
    return getattr(cfg, "inference", "nuts") == "map-waic"


def wants_evidence(cfg) -> bool:
    """cfg.inference "map-evidence": the MAP fit followed by mdfit_map_evidence."""
    return getattr(cfg, "inference", "nuts") == "map-evidence"


def wants_pred(cfg) -> bool:
    """cfg.inference "map-pred": the MAP fit followed by mdfit_map_pred."""
    return getattr(cfg, "inference", "nuts") == "map-pred"


def pred_draws_of(cfg) -> int:
    """The predictive draws per job of a "map-pred" run (cfg.pred_draws, default 1000)."""
    return int(getattr(cfg, "pred_draws", 1000) or 1000)


def wants_auto(cfg) -> bool:
    """cfg.inference "auto": the MAP fit, its importance-sampled correction and
    the sampler over the taxa it cannot settle (engine.fit_auto_device)."""
    return getattr(cfg, "inference", "nuts") == "auto"


def psis_adapt_of(cfg) -> int:
    """The moment-matched proposal rounds of a "map-psis", "map-waic", "map-pred" or "auto" run (cfg.psis_adapt,
    default 0)."""
    return int(getattr(cfg, "psis_adapt", 0) or 0)


def auto_pred_of(cfg) -> bool:
    """cfg.auto_pred (default False): an "auto" run composes the importance-weighted posterior predictive
    (MDFIT-AUTO v1.1); with any other inference a ValueError naming the option."""
    on = bool(getattr(cfg, "auto_pred", False))
    if on and not wants_auto(cfg):
        raise ValueError("auto_pred goes with inference 'auto'")
    return on


def ppc_of(cfg) -> bool:
    """cfg.ppc (default False): a "map-pred" run adds the posterior predictive check of the PMD fit (MDFIT-PPC v1);
    with any other inference a ValueError naming the option."""
    on = bool(getattr(cfg, "ppc", False))
    if on and not wants_pred(cfg):
        raise ValueError("ppc goes with inference 'map-pred'")
    return on


def quantiles_of(cfg) -> bool:
    """cfg.quantiles (default False): a "map-psis" run adds the weighted median, 68 % HPDI and quantiles of its
    posterior (MDFIT-QUANT v1); with any other inference a ValueError naming the option."""
    on = bool(getattr(cfg, "quantiles", False))
    if on and not wants_psis(cfg):
        raise ValueError("quantiles goes with inference 'map-psis'")
    return on


def joint_of(cfg) -> bool:
    """cfg.joint (default False): a "map-waic" run forms the evidence and the posterior from the same weights in the
    same launch (mdfit_map_joint) and adds map-evidence's and map-psis's columns; with any other inference a
    ValueError naming the option."""
    on = bool(getattr(cfg, "joint", False))
    if on and not wants_waic(cfg):
        raise ValueError("joint goes with inference 'map-waic'")
    return on


def dmax_threshold_of(cfg) -> float:
    """The threshold d0 of D_max_prob_above = P(D_max > d0) of a run with quantiles (cfg.dmax_threshold, default
    0.01)."""
    v = getattr(cfg, "dmax_threshold", 0.01)
    return 0.01 if v is None else float(v)


def _split_rest(cfg, rest):
    """The optional arrays behind (out, pred, status) of fit_packed: (the run's extra block or None, auto_pred or
    None, adapt or None) -- the auto-pred block follows the extra block, the adapt block is last."""
    rest = list(rest)
    adapt = rest.pop() if psis_adapt_of(cfg) > 0 else None
    auto_pred = rest.pop() if auto_pred_of(cfg) else None
    return (rest[0] if rest else None), auto_pred, adapt


def psis_draws_of(cfg) -> int:
    """The draws per sub-fit of a "map-psis", "map-waic", "map-pred" or "auto" run (cfg.psis_draws, default 256)."""
    return int(getattr(cfg, "psis_draws", 256) or 256)


def _fit_for_frames(p: Packed, cfg, opts, shard: bool):
    """fit_packed as cfg asks: None on a non-zero rank of a multi-GPU job, else
    (out, pred, keep, kw) -- keep the taxa that fitted (the others warned
    about), kw the optional arrays under make_df_fit_results' keywords."""
    inference = getattr(cfg, "inference", "nuts")
    block = next((b for b in blocks.BLOCKS if b.inference == inference), None)
    # every tail's option has its reader above, <option>_of(cfg)
    tails = {t.option: globals()[t.option + "_of"](cfg) for t in blocks.TAILS}
    draws = dict(psis_draws=psis_draws_of(cfg), pred_draws=pred_draws_of(cfg), dmax_threshold=dmax_threshold_of(cfg))
    res = fit_packed(p, opts, shard=shard, **draws, **tails, **({block.name: True} if block is not None else {}))
    if res is None:
        return None
    out, pred, status, *rest = res
    # the arrays behind (out, pred, status) are the run's block and tails in the record's order
    run = blocks.describe(None, tails, check_mode=False, **draws,
                          **({block.switch: True} if block is not None else {}))
    kw = {part.attr: a for part, a in zip(run.parts, rest, strict=True)}
    keep = status == _lib.OK
    for t in np.where(~keep)[0]:
        logger.warning(f"Fit: tax_id {p.tax_id[t]} failed (status {int(status[t])}). Skipping.")
    return out, pred, keep, kw


def compute_fits(df_counts, cfg, mcmc_kwargs=None, opts=None, shard=True):
    """fits.py:709-730: (df_fit_results, df_fit_predictions) for every taxon of
    df_counts, in df_counts order, by the sampler (cfg.inference "nuts", the
    reference's NUTS with mcmc_kwargs' warmup / samples) or the MAP fit
    ("map-laplace": with the Laplace columns in df_fit_results)."""
    if opts is None:
        opts = make_opts(cfg, mcmc_kwargs)
    p = pack_counts(df_counts, cfg)
    res = _fit_for_frames(p, cfg, opts, shard)
    if res is None:  # non-zero rank of a multi-GPU job
        return None, None
    out, pred, keep, kw = res
    return (make_df_fit_results(p, out, keep, cfg, **kw),
            make_df_fit_predictions(p, pred, keep, cfg, ppred=kw.get("ppred"), ppc=kw.get("ppc")))


def extract_top_max_fits(df_counts, max_fits):
    """fits.py:736-744: taxa with the largest summed N_alignments (ties: first
    in groupby order, i.e. ascending tax_id).

    A categorical tax_id (every counts table of counts.compute_counts) is
    summed per category code with bincount and the winners picked by a stable
    sort -- the set nlargest(keep="first") picks, ties broken by group order --
    and a selection of every taxon returns the table itself (the common case:
    max_fits unset; the groupby + isin + row copy cost ~0.15 s of the driver's
    main thread per 100k-taxon file)."""
    tax = df_counts["tax_id"]
    if isinstance(tax.dtype, pd.CategoricalDtype) and len(df_counts):
        codes = tax.cat.codes.to_numpy()
        n_cat = len(tax.cat.categories)
        from . import ingest

        used, n_missing = ingest.used_codes(codes, n_cat) if n_cat < 2**31 else (None, 1)
        if n_missing == 0:
            present = np.flatnonzero(used)
            if max_fits >= len(present):
                return df_counts
            sums = np.bincount(codes, weights=df_counts["N_alignments"].to_numpy(np.float64), minlength=n_cat)
            # groupby(observed=True) orders the groups by category code
            order = np.argsort(-sums[present], kind="stable")
            chosen = np.zeros(n_cat, bool)
            chosen[present[order[:max_fits]]] = True
            return df_counts[chosen[codes]]
    top = df_counts.groupby("tax_id", observed=True)["N_alignments"].sum().nlargest(max_fits).index
    return df_counts[df_counts["tax_id"].isin(top)]


def get_top_max_fits(df_counts, N_fits):
    if N_fits is not None and N_fits > 0:
        return extract_top_max_fits(df_counts, N_fits)
    return df_counts


def _rank() -> int:
    import torch.distributed as dist

    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


CACHE_KEYS = ["min_alignments", "min_y_sum", "substitution_bases_forward", "substitution_bases_reverse",
              "N_fits", "shortname", "filename", "inference", "psis_draws", "pred_draws", "psis_adapt", "auto_pred",
              "ppc", "quantiles", "dmax_threshold", "joint"]


def _cache_hit(cfg) -> bool:
    """This rank's fit cache check (fits.py:767-783): both parquets exist (and
    --forced is off) with metadata equal on CACHE_KEYS."""
    parquet_fit_results = io.Parquet(cfg.filename_fit_results)
    parquet_fit_predictions = io.Parquet(cfg.filename_fit_predictions)
    if not (parquet_fit_results.exists(cfg.forced) and parquet_fit_predictions.exists(cfg.forced)):
        return False
    metadata_cfg = cfg.to_dict()
    return utils.metadata_is_similar(parquet_fit_results.load_metadata(), metadata_cfg, include=CACHE_KEYS) and \
        utils.metadata_is_similar(parquet_fit_predictions.load_metadata(), metadata_cfg, include=CACHE_KEYS)


def prepare_fits(df_counts, cfg):
    """The host work of get_fits ahead of the device call -- the top-N cut and
    the packing -- for a reader thread (main.main runs it beside the previous
    file's fit); None when this rank's fit cache is a hit (get_fits decides)."""
    if _cache_hit(cfg):
        return None
    return pack_counts(get_top_max_fits(df_counts, cfg.N_fits), cfg, pinned=True)


def get_fits(df_counts, cfg, opts=None, shard=True, writer=None, packed=None, deferred=False):
    """fits.py:754-807.  shard: split the taxa over the torch.distributed ranks
    (rank 0 gathers and saves); writer: an executor for the parquet saves;
    packed: prepare_fits(df_counts, cfg) when it ran already.  deferred: return
    a callable that builds the two frames and submits their saves (main.main
    runs it on a writer thread while the next file fits) instead of the
    frames, once the device results are on the host."""
    from .distributed import all_ranks_agree

    parquet_fit_results = io.Parquet(cfg.filename_fit_results)
    parquet_fit_predictions = io.Parquet(cfg.filename_fit_predictions)
    hit = _cache_hit(cfg)
    if shard:  # a taxon-sharded fit is collective: every rank reuses the cache or none does
        hit = all_ranks_agree(hit)
    if hit:
        if shard and _rank() != 0:
            return None, None
        logger.info("Fit: Loading fits from parquet-file.")
        return parquet_fit_results.load(), parquet_fit_predictions.load()
    logger.info("Fit: Generating fits and saving to file.")
    p = packed if packed is not None else pack_counts(get_top_max_fits(df_counts, cfg.N_fits), cfg)
    # fits.py:792-799
    mcmc_kwargs = dict(progress_bar=False, num_warmup=500, num_samples=1000, num_chains=1, chain_method="sequential")
    res = _fit_for_frames(p, cfg, opts if opts is not None else make_opts(cfg, mcmc_kwargs), shard)
    if res is None:  # non-zero rank of a multi-GPU job
        return None, None
    out, pred, keep, kw = res

    def finish():
        from .counts import _save

        df_fit_results = make_df_fit_results(p, out, keep, cfg, **kw)
        df_fit_predictions = make_df_fit_predictions(p, pred, keep, cfg, ppred=kw.get("ppred"), ppc=kw.get("ppc"))
        _save(writer, parquet_fit_results, df_fit_results, cfg.to_dict())
        _save(writer, parquet_fit_predictions, df_fit_predictions, cfg.to_dict())
        return df_fit_results, df_fit_predictions

    return finish if deferred else finish()
