"""ctypes binding of the engine's C-ABI (include/mdfit.h, libmdfit.so).

The shared library is built in-tree by __graft_entry__.build() (hipcc, gfx950)
and loaded from this package directory.  There is no fallback: if the library
or a GPU is missing, the product path raises.
"""

from __future__ import annotations

import ctypes
import os
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "libmdfit.so"

# mirrors of include/mdfit.h
ABI_VERSION = 3
NPOS = 30
NHALF = 15
LD = 32
NMM = 12
NPRED = 3
MODE_MAP = 0  # (MODE_NUTS below)
OK, MAXITER, NONFINITE, INVALID = 0, 1, 2, 3
NRESULT = 25
F_DIAG = 32
NOUT = 80
NSUBFIT = 6
DIAG_STRIDE = 8
NLAPLACE = 8
NNUTSDIAG = 12
NNUTSSUMM = 16
NNUTSLOO = 8
NMAPPSIS = 16
NMAPWAIC = 8
NMAPPRED = 16
NLOOROW = 7  # rows of a PSIS-LOO record: the six sub-fits, then the comparisons

# output record field order (enum mdfit_field) == fit_results numeric columns
RESULT_FIELDS = [
    "D_max",
    "n_sigma",
    "D_max_lower_hpdi",
    "D_max_upper_hpdi",
    "q_mean",
    "concentration_mean",
    "D_max_marginalized_mean",
    "N_z1_forward",
    "N_z1_reverse",
    "N_sum_forward",
    "N_sum_reverse",
    "N_sum_total",
    "y_sum_forward",
    "y_sum_reverse",
    "y_sum_total",
    "n_sigma_forward",
    "D_max_forward",
    "q_mean_forward",
    "n_sigma_reverse",
    "D_max_reverse",
    "q_mean_reverse",
    "asymmetry",
    "normalized_noise",
    "normalized_noise_forward",
    "normalized_noise_reverse",
]
SUBFITS = ["PMD", "null", "PMD_forward", "PMD_reverse", "null_forward", "null_reverse"]
DIAG_FIELDS = ["q", "A", "c", "phi", "objective", "evals", "status"]
# Laplace record (mdfit_map_laplace): float64 [T][3][NLAPLACE], rows PMD-all, PMD-forward, PMD-reverse
LAPLACE_FIELDS = ["q_std", "A_std", "c_std", "phi_std", "D_max_std", "rho_Ac", "significance", "flags"]
LAPLACE_VALID = 16  # flags: bits 0..3 coordinate (q, A, c, phi) free, bit 4 valid
# sampling diagnostics record (mdfit_nuts_diag): float64 [T][6][NNUTSDIAG], rows in SUBFITS order
NUTSDIAG_FIELDS = ["ess_q", "ess_A", "ess_c", "ess_phi", "ess_D_max", "rhat_q", "rhat_A", "rhat_c", "rhat_phi",
                   "rhat_D_max", "mcse_D_max", "flags"]
NUTSDIAG_VALID = 1  # flags: bit 0 valid
# posterior summary record (mdfit_nuts_summary): float64 [T][6][NNUTSSUMM], rows in SUBFITS order
NUTSSUMM_FIELDS = ["q_std", "A_std", "c_std", "phi_std", "D_max_std", "D_max_mean", "D_max_median", "D_max_lo",
                   "D_max_hi", "q_median", "q_lo", "q_hi", "phi_median", "rho_Ac", "significance", "flags"]
NUTSSUMM_VALID = 1  # flags: bit 0 valid
# PSIS-LOO record (mdfit_nuts_loo): float64 [T][NLOOROW][NNUTSLOO], rows 0..5 in SUBFITS order ...
NUTSLOO_FIELDS = ["elpd_loo", "p_loo", "elpd_se", "khat_max", "khat_argmax", "n_bad", "lppd", "flags"]
# ... and row 6, the comparisons
NUTSLOO_COMPARE_FIELDS = ["n_sigma_loo", "n_sigma_loo_forward", "n_sigma_loo_reverse", "asymmetry_loo", "khat_max",
                          "n_bad", "reserved", "flags"]
NUTSLOO_VALID = 1  # flags: bit 0 valid

# importance-sampled posterior record (mdfit_map_psis): float64 [T][3][NMAPPSIS], rows PMD-all, -forward, -reverse
MAPPSIS_FIELDS = ["q_mean", "A_mean", "c_mean", "phi_mean", "D_max_mean", "q_std", "A_std", "c_std", "phi_std",
                  "D_max_std", "rho_Ac", "significance", "khat", "ess", "n_infeasible", "flags"]
MAPPSIS_VALID, MAPPSIS_RELIABLE = 1, 2  # flags: bit 0 valid, bit 1 khat <= threshold, bits 2..5 coordinate free

# adapt record (mdfit_map_psis_adapt, mdfit_map_waic_adapt): float64 [T][3][NMAPADAPT], rows as the psis record's
NMAPADAPT = 4
MAPADAPT_FIELDS = ["khat_initial", "ess_initial", "best_round", "rounds_tried"]
MAPPSIS_ADAPTED = 64  # flags bit 6 of a PMD row of the psis and waic records: the best round is > 0
ADAPT_MAX_ROUNDS = 4
# the adapt block that leaves the device (ChunkedFitter psis_adapt): float32 [T][NADAPTOUT]
NADAPTOUT = 2
ADAPTOUT_FIELDS = ["khat_initial_max", "best_round_max"]

# importance-weighted WAIC record (mdfit_map_waic): float64 [T][NWAICROW][NMAPWAIC], rows 0..5 in SUBFITS order ...
NWAICROW = 7
MAPWAIC_FIELDS = ["elpd_waic", "p_waic", "lppd", "khat", "ess", "n_infeasible", "p_waic_max", "flags"]
# ... and row 6, the comparisons
MAPWAIC_COMPARE_FIELDS = ["n_sigma_waic", "n_sigma_waic_forward", "n_sigma_waic_reverse", "asymmetry_waic", "khat_max",
                          "ess_min", "reserved", "flags"]
MAPWAIC_VALID, MAPWAIC_RELIABLE = 1, 2  # flags: bit 0 valid, bit 1 khat <= threshold; rows 0..5: bits 2..5 free

# importance-sampled evidence record (mdfit_map_evidence): float64 [T][NEVIDROW][NMAPEVID], rows 0..5 in SUBFITS order ...
NMAPEVID = 8
NEVIDROW = 7
MAPEVID_FIELDS = ["log_evidence", "se", "khat", "ess", "n_infeasible", "log_w_max", "best_round", "flags"]
# ... and row 6, the comparisons
MAPEVID_COMPARE_FIELDS = ["log_bf", "log_bf_forward", "log_bf_reverse", "log_bf_asymmetry", "log_bf_se", "khat_max",
                          "ess_min", "flags"]
MAPEVID_VALID, MAPEVID_RELIABLE = 1, 2  # flags: bit 0 valid, bit 1 khat <= threshold; rows 0..5: bits 2..5 free, bit 6 adapted

# route bits of mdfit_auto_route (MDFIT_ROUTE_*): the taxon is sampled iff route & ROUTE_SAMPLE
ROUTE_WAIC, ROUTE_PSIS, ROUTE_STATUS, ROUTE_INVALID, ROUTE_SAMPLE = 1, 2, 4, 8, 7
# the nine result columns mdfit_auto_route composes for a taxon with route 0
AUTO_COMPOSED_FIELDS = ["q_mean", "concentration_mean", "D_max_marginalized_mean", "q_mean_forward",
                        "q_mean_reverse", "n_sigma", "n_sigma_forward", "n_sigma_reverse", "asymmetry"]
# mdfit_auto_route_pred: one more cause, and the sampled set's mask with it
ROUTE_PRED, ROUTE_SAMPLE_PRED = 16, 23
# the five predictive columns mdfit_auto_route_pred composes beside the nine above
AUTO_PRED_COMPOSED_FIELDS = ["D_max", "D_max_lower_hpdi", "D_max_upper_hpdi", "D_max_forward", "D_max_reverse"]
# the auto-pred block that leaves the device (engine.fit_auto_device auto_pred): float32 [T][NAUTOPRED]
NAUTOPRED = 2
AUTOPRED_FIELDS = ["pred_ess_min", "pred_distinct_min"]
# the auto block that leaves the device (engine.fit_auto_device): float32 [T][NAUTO]
NAUTO = 4
AUTO_FIELDS = ["route", "sampled", "khat_max", "ess_min"]

# importance-weighted posterior predictive record (mdfit_map_pred): float64 [T][NMAPPRED]
MAPPRED_FIELDS = ["D_max", "D_max_lower_hpdi", "D_max_upper_hpdi", "D_max_forward", "D_max_reverse", "khat_all",
                  "khat_forward", "khat_reverse", "ess_all", "ess_forward", "ess_reverse", "n_distinct_all",
                  "n_distinct_forward", "n_distinct_reverse", "n_noncount_jobs", "flags"]
MAPPRED_VALID, MAPPRED_RELIABLE = 1, 2  # flags: bit 0 all rows valid, bit 1 and every khat <= threshold, bits 2..4 row valid
NPREDJOB = 32  # the sampler's predictive jobs: columns 0..29 of PMD-all, column 0 under PMD-forward and PMD-reverse
PRED_DRAWS_MIN, PRED_DRAWS_MAX = 25, 1024

# posterior predictive check record (mdfit_map_ppc): float64 [T][NMAPPPC]; worst_pos is a column 0..29
NMAPPPC = 12
MAPPPC_FIELDS = ["p_outlier", "p_strand", "t_outlier", "t_strand", "worst_pos", "p_worst", "n_low", "n_points", "khat",
                 "ess", "n_distinct", "flags"]
# flags: bit 0 valid, bit 1 khat <= threshold, bit 3 some replicated draw was no count (then bit 0 is clear), bit 6
# (MAPPSIS_ADAPTED) the best round is > 0
MAPPPC_VALID, MAPPPC_RELIABLE, MAPPPC_NONCOUNT = 1, 2, 8
# the ppc block that leaves the device (ChunkedFitter ppc): float32 [T][NPPCOUT] = ppos[30] | rec[NMAPPPC]
NPPCOUT = 30 + NMAPPPC

# weighted order statistics record (mdfit_map_quant): float64 [T][3][NMAPQUANT], rows PMD-all, forward, reverse;
# khat, ess and flags are the psis record's (MAPPSIS_* bits)
NMAPQUANT = 16
MAPQUANT_FIELDS = ["D_max_median", "D_max_lo", "D_max_hi", "D_max_q05", "D_max_q95", "D_max_p_above", "q_median",
                   "q_lo", "q_hi", "A_median", "c_median", "phi_median", "khat", "ess", "n_window", "flags"]
# the quant block that leaves the device (ChunkedFitter quantiles): float32 [T][NQUANTOUT] = the three rows
NQUANTOUT = 3 * NMAPQUANT
NQUANTRES = 8  # mdfit_weighted_order_stats: median, lo, hi, q05, q95, p_above, n_window, ok

# the joint block that leaves the device (ChunkedFitter joint, mdfit_map_joint): float32 [T][NJOINTOUT] = the seven
# rows of the evidence record | the three rows of the psis record
NJOINTOUT = NEVIDROW * NMAPEVID + 3 * NMAPPSIS

# C-ABI symbols declared in include/mdfit.h
EXPORTED_SYMBOLS = [
    "mdfit_default_opts",
    "mdfit_fit_batch",
    "mdfit_fit_batch_indexed",
    "mdfit_auto_route",
    "mdfit_auto_route_pred",
    "mdfit_workspace_bytes",
    "mdfit_noise",
    "mdfit_map_laplace",
    "mdfit_map_laplace_u",
    "mdfit_nuts_diag",
    "mdfit_nuts_summary",
    "mdfit_nuts_loo",
    "mdfit_nuts_post",
    "mdfit_psis",
    "mdfit_map_psis",
    "mdfit_psis_weights",
    "mdfit_map_waic",
    "mdfit_map_psis_adapt",
    "mdfit_map_waic_adapt",
    "mdfit_map_evidence",
    "mdfit_map_evidence_adapt",
    "mdfit_log_mean_weight",
    "mdfit_adapt_proposal",
    "mdfit_map_pred",
    "mdfit_map_pred_adapt",
    "mdfit_map_ppc",
    "mdfit_map_ppc_adapt",
    "mdfit_map_quant",
    "mdfit_map_quant_adapt",
    "mdfit_weighted_order_stats",
    "mdfit_map_joint",
    "mdfit_map_joint_adapt",
    "mdfit_resample",
    "mdfit_betabinom_logpmf",
    "mdfit_special",
    "mdfit_primitive",
    "mdfit_hpdi68",
    "mdfit_peak_probe",
    "mdfit_nuts_peak_probe",
    "mdfit_poison_lds",
    "mdfit_objective",
    "mdfit_objective_form",
    "mdfit_nuts_potential",
    "mdfit_profile_enable",
    "mdfit_profile_read",
    "mdfit_last_error",
    "mdfit_abi_version",
]


class MdfitOpts(ctypes.Structure):
    _fields_ = [
        ("mode", ctypes.c_int32),
        ("max_iter", ctypes.c_int32),
        ("tol_step", ctypes.c_double),
        ("seed", ctypes.c_uint64),
        ("num_warmup", ctypes.c_int32),
        ("num_samples", ctypes.c_int32),
        ("index_base", ctypes.c_int64),
    ]


MODE_MAP, MODE_NUTS = 0, 1
# MAP: below this many taxa per call the predictive HPDI streams beside the fit
# kernel; from it the workspace also holds the wide-window records
# (kStreamMaxTaxa, csrc/mdfit.hip)
STREAM_MAX_TAXA = 60_000
SAMPLES_OFFSET = 256  # NUTS workspace: double[T][6][S][4] draws after the queue counters


class MdfitError(RuntimeError):
    pass


_LIB = None


def load(path: str | os.PathLike | None = None) -> ctypes.CDLL:
    """Load libmdfit.so (in-tree) and declare the C-ABI signatures."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = Path(path) if path is not None else LIB_PATH
    if not p.exists():
        raise MdfitError(
            f"{p} not found: build the HIP extension first (python -c "
            "'import __graft_entry__ as g; g.build()')"
        )
    lib = ctypes.CDLL(str(p))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.mdfit_default_opts.argtypes = [ctypes.POINTER(MdfitOpts)]
    lib.mdfit_default_opts.restype = None
    lib.mdfit_fit_batch.argtypes = [vp, vp, vp, i64, ctypes.POINTER(MdfitOpts), vp, vp, vp, vp, vp]
    lib.mdfit_fit_batch.restype = ctypes.c_int
    lib.mdfit_fit_batch_indexed.argtypes = [vp, vp, vp, i64, vp, ctypes.POINTER(MdfitOpts), vp, vp, vp, vp, vp]
    lib.mdfit_fit_batch_indexed.restype = ctypes.c_int
    lib.mdfit_auto_route.argtypes = [vp, vp, vp, i64, vp, vp, vp]
    lib.mdfit_auto_route.restype = ctypes.c_int
    lib.mdfit_workspace_bytes.argtypes = [i64, ctypes.c_void_p]
    if hasattr(lib, "mdfit_nuts_potential"):
        lib.mdfit_nuts_potential.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, vp]
        lib.mdfit_nuts_potential.restype = ctypes.c_int
    if hasattr(lib, "mdfit_profile_enable"):  # (absent from older dev builds loaded by tools/)
        lib.mdfit_profile_enable.argtypes = [ctypes.c_int]
        lib.mdfit_profile_enable.restype = ctypes.c_int
        lib.mdfit_profile_read.argtypes = [vp, vp, vp]
        lib.mdfit_profile_read.restype = ctypes.c_int
    lib.mdfit_workspace_bytes.restype = i64
    lib.mdfit_noise.argtypes = [vp, vp, vp, i64, vp, vp]
    lib.mdfit_noise.restype = ctypes.c_int
    lib.mdfit_map_laplace.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp]
    lib.mdfit_map_laplace.restype = ctypes.c_int
    lib.mdfit_map_laplace_u.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, vp]
    lib.mdfit_map_laplace_u.restype = ctypes.c_int
    lib.mdfit_nuts_diag.argtypes = [vp, vp, i64, ctypes.POINTER(MdfitOpts), vp, vp]
    lib.mdfit_nuts_diag.restype = ctypes.c_int
    lib.mdfit_nuts_summary.argtypes = [vp, vp, i64, ctypes.POINTER(MdfitOpts), vp, vp]
    lib.mdfit_nuts_summary.restype = ctypes.c_int
    lib.mdfit_nuts_loo.argtypes = [vp, vp, vp, vp, i64, ctypes.POINTER(MdfitOpts), vp, vp, vp]
    lib.mdfit_nuts_loo.restype = ctypes.c_int
    lib.mdfit_nuts_post.argtypes = [vp, vp, vp, i64, ctypes.POINTER(MdfitOpts), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.mdfit_nuts_post.restype = ctypes.c_int
    lib.mdfit_psis.argtypes = [vp, i64, i32, vp, vp, vp]
    lib.mdfit_psis.restype = ctypes.c_int
    lib.mdfit_map_psis.argtypes = [vp, vp, vp, vp, i64, i32, ctypes.c_uint64, i64, vp, vp, vp]
    lib.mdfit_map_psis.restype = ctypes.c_int
    lib.mdfit_map_waic.argtypes = [vp, vp, vp, vp, i64, i32, ctypes.c_uint64, i64, vp, vp, vp, vp]
    lib.mdfit_map_waic.restype = ctypes.c_int
    lib.mdfit_map_psis_adapt.argtypes = [vp, vp, vp, vp, i64, i32, i32, ctypes.c_uint64, i64, vp, vp, vp, vp]
    lib.mdfit_map_psis_adapt.restype = ctypes.c_int
    lib.mdfit_map_waic_adapt.argtypes = [vp, vp, vp, vp, i64, i32, i32, ctypes.c_uint64, i64, vp, vp, vp, vp, vp]
    lib.mdfit_map_waic_adapt.restype = ctypes.c_int
    lib.mdfit_map_evidence.argtypes = [vp, vp, vp, vp, i64, i32, ctypes.c_uint64, i64, vp, vp, vp]
    lib.mdfit_map_evidence.restype = ctypes.c_int
    lib.mdfit_map_evidence_adapt.argtypes = [vp, vp, vp, vp, i64, i32, i32, ctypes.c_uint64, i64, vp, vp, vp, vp]
    lib.mdfit_map_evidence_adapt.restype = ctypes.c_int
    lib.mdfit_log_mean_weight.argtypes = [vp, i64, i32, vp, vp, vp, vp]
    lib.mdfit_log_mean_weight.restype = ctypes.c_int
    lib.mdfit_adapt_proposal.argtypes = [vp, vp, vp, vp, vp, i64, i32, vp, vp, vp]
    lib.mdfit_adapt_proposal.restype = ctypes.c_int
    lib.mdfit_map_pred.argtypes = [vp, vp, vp, vp, i64, i32, i32, ctypes.c_uint64, i64, vp, vp, vp, vp, vp]
    lib.mdfit_map_pred.restype = ctypes.c_int
    if hasattr(lib, "mdfit_map_pred_adapt"):  # (absent from the parent builds loaded by tools/ for A/B)
        lib.mdfit_map_pred_adapt.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, ctypes.c_uint64, i64, vp, vp, vp, vp,
                                             vp, vp]
        lib.mdfit_map_pred_adapt.restype = ctypes.c_int
        lib.mdfit_auto_route_pred.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]
        lib.mdfit_auto_route_pred.restype = ctypes.c_int
    if hasattr(lib, "mdfit_map_ppc"):  # (absent from the parent builds loaded by tools/ for A/B)
        lib.mdfit_map_ppc.argtypes = [vp, vp, vp, vp, i64, i32, i32, ctypes.c_uint64, i64, vp, vp, vp, vp, vp, vp]
        lib.mdfit_map_ppc.restype = ctypes.c_int
        lib.mdfit_map_ppc_adapt.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, ctypes.c_uint64, i64, vp, vp, vp, vp,
                                            vp, vp, vp]
        lib.mdfit_map_ppc_adapt.restype = ctypes.c_int
    if hasattr(lib, "mdfit_map_quant"):  # (absent from the parent builds loaded by tools/ for A/B)
        f64 = ctypes.c_double
        lib.mdfit_map_quant.argtypes = [vp, vp, vp, vp, i64, i32, ctypes.c_uint64, i64, f64, vp, vp, vp]
        lib.mdfit_map_quant.restype = ctypes.c_int
        lib.mdfit_map_quant_adapt.argtypes = [vp, vp, vp, vp, i64, i32, i32, ctypes.c_uint64, i64, f64, vp, vp, vp, vp]
        lib.mdfit_map_quant_adapt.restype = ctypes.c_int
        lib.mdfit_weighted_order_stats.argtypes = [vp, vp, i64, i32, f64, vp, vp]
        lib.mdfit_weighted_order_stats.restype = ctypes.c_int
    if hasattr(lib, "mdfit_map_joint"):  # (absent from the parent builds loaded by tools/ for A/B)
        lib.mdfit_map_joint.argtypes = [vp, vp, vp, vp, i64, i32, ctypes.c_uint64, i64, vp, vp, vp, vp, vp, vp]
        lib.mdfit_map_joint.restype = ctypes.c_int
        lib.mdfit_map_joint_adapt.argtypes = [vp, vp, vp, vp, i64, i32, i32, ctypes.c_uint64, i64, vp, vp, vp, vp, vp,
                                              vp, vp]
        lib.mdfit_map_joint_adapt.restype = ctypes.c_int
    lib.mdfit_resample.argtypes = [vp, i64, i32, i32, vp, vp, vp]
    lib.mdfit_resample.restype = ctypes.c_int
    lib.mdfit_psis_weights.argtypes = [vp, i64, i32, vp, vp, vp]
    lib.mdfit_psis_weights.restype = ctypes.c_int
    lib.mdfit_betabinom_logpmf.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp]
    lib.mdfit_betabinom_logpmf.restype = ctypes.c_int
    lib.mdfit_special.argtypes = [vp, i64, vp, vp]
    lib.mdfit_special.restype = ctypes.c_int
    lib.mdfit_primitive.argtypes = [i32, vp, vp, i64, vp, vp]
    lib.mdfit_primitive.restype = ctypes.c_int
    lib.mdfit_hpdi68.argtypes = [vp, vp, vp, i64, vp, vp, vp]
    lib.mdfit_hpdi68.restype = ctypes.c_int
    lib.mdfit_peak_probe.argtypes = [i64, i32, vp, vp]
    lib.mdfit_peak_probe.restype = ctypes.c_int
    if hasattr(lib, "mdfit_poison_lds"):
        lib.mdfit_poison_lds.argtypes = [vp]
        lib.mdfit_poison_lds.restype = ctypes.c_int
    if hasattr(lib, "mdfit_nuts_peak_probe"):  # (absent from round-3 builds loaded by tools/ for A/B)
        lib.mdfit_nuts_peak_probe.argtypes = [i64, i32, vp, vp]
        lib.mdfit_nuts_peak_probe.restype = ctypes.c_int
    lib.mdfit_objective.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp]
    lib.mdfit_objective.restype = ctypes.c_int
    lib.mdfit_objective_form.argtypes = [vp, vp, vp, vp, vp, i64, ctypes.c_int32, vp, vp, vp, vp, vp]
    lib.mdfit_objective_form.restype = ctypes.c_int
    lib.mdfit_last_error.argtypes = []
    lib.mdfit_last_error.restype = ctypes.c_char_p
    lib.mdfit_abi_version.argtypes = []
    lib.mdfit_abi_version.restype = ctypes.c_int
    if lib.mdfit_abi_version() != ABI_VERSION:
        raise MdfitError(f"ABI mismatch: library {lib.mdfit_abi_version()} != {ABI_VERSION}")
    if path is None:
        _LIB = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().mdfit_last_error().decode(errors="replace")
        raise MdfitError(f"mdfit call failed (rc={rc}): {msg}")


def default_opts(**overrides) -> MdfitOpts:
    o = MdfitOpts()
    load().mdfit_default_opts(ctypes.byref(o))
    for k, v in overrides.items():
        setattr(o, k, v)
    return o
