/*
 * mdfit.h — C-ABI of the MI355X-native per-TaxID ancient-DNA damage-fit engine.
 *
 * This is the drop-in boundary for the hot path of metadamage's fits.py
 * (reference: /root/reference/metadamage/fits.py).  The reference has no FFI;
 * its operator boundary is the per-taxon numpyro call chain
 *
 *     fit_single_group_without_timeout(group, cfg, ...)   fits.py:428-469
 *       group_to_numpyro_data                              fits.py:398-419
 *       fit_mcmc(mcmc_PMD / mcmc_null, data)               fits.py:382-387, 438-439
 *       compute_fit_results                                fits.py:230-295
 *         add_assymetry_results_to_fit_results             fits.py:298-356
 *         add_noise_estimates                              fits.py:359-376
 *
 * dispatched by compute_fits (fits.py:709-730).  mdfit_fit_batch replaces the
 * whole chain for a batch of taxa in one stream-ordered launch: one call per
 * device, outputs in input order (so the reference's reorder step,
 * fits.py:422-425, is a no-op).
 *
 * Conventions
 *  - Every pointer argument of mdfit_fit_batch is a DEVICE pointer (HBM); the
 *    caller owns all buffers (PyTorch tensors in the Python host).  The library
 *    allocates no persistent device memory.
 *  - The call is asynchronous on `hip_stream` (a hipStream_t, NULL = default
 *    stream) and never synchronises the host.
 *  - Return value: 0 on success, otherwise a negative MDFIT_E* code or a
 *    positive hipError_t; mdfit_last_error() gives a message (thread-local).
 *  - Per-taxon failures are reported in status[] and never abort the batch.
 */
#ifndef MDFIT_H
#define MDFIT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDFIT_ABI_VERSION 3

/* Dense count layout: one row of MDFIT_LD uint32 per taxon.
 * Column i < 15 is forward position z = i+1 (y = CT, N = C by default);
 * column 15 <= i < 30 is reverse position z = -(i-14) (y = GA, N = G).
 * Columns 30, 31 are padding (ignored).  This is group_to_numpyro_data
 * (fits.py:398-419) packed for a whole batch. */
#define MDFIT_NPOS 30
#define MDFIT_NHALF 15
#define MDFIT_LD 32

/* Mismatch counts for the noise estimate (fits.py:359-376): uint32
 * mm[T][30][12], columns in the reference order AC AG AT CA CG CT GA GC GT TA TC TG. */
#define MDFIT_NMM 12

/* Fit modes. */
#define MDFIT_MODE_MAP 0  /* maximum a posteriori of model_PMD / model_null (fits.py:43-67) */
#define MDFIT_MODE_NUTS 1 /* NUTS posterior sampling as fits.py:382-387 (MDFIT-NUTS v1) */

/* Per-taxon status codes (status[t]). */
#define MDFIT_OK 0
#define MDFIT_MAXITER 1   /* a sub-fit hit max_iter before converging */
#define MDFIT_NONFINITE 2 /* non-finite objective at the returned point */
#define MDFIT_INVALID 3   /* invalid input (y > N somewhere) */

/* Error codes (return values). */
#define MDFIT_E_ARG (-1)
#define MDFIT_E_HIP (-2)

/* Output record: double out[T][MDFIT_NOUT].  Fields 0..24 are the numeric
 * columns of fit_results (fits.py:244-293, 317-356, 374-376) in the reference
 * column order; the rest are per-sub-fit diagnostics. */
enum mdfit_field {
  MDFIT_F_D_MAX = 0,
  MDFIT_F_N_SIGMA,
  MDFIT_F_D_MAX_LOWER_HPDI,
  MDFIT_F_D_MAX_UPPER_HPDI,
  MDFIT_F_Q_MEAN,
  MDFIT_F_CONCENTRATION_MEAN,
  MDFIT_F_D_MAX_MARGINALIZED_MEAN,
  MDFIT_F_N_Z1_FORWARD,
  MDFIT_F_N_Z1_REVERSE,
  MDFIT_F_N_SUM_FORWARD,
  MDFIT_F_N_SUM_REVERSE,
  MDFIT_F_N_SUM_TOTAL,
  MDFIT_F_Y_SUM_FORWARD,
  MDFIT_F_Y_SUM_REVERSE,
  MDFIT_F_Y_SUM_TOTAL,
  MDFIT_F_N_SIGMA_FORWARD,
  MDFIT_F_D_MAX_FORWARD,
  MDFIT_F_Q_MEAN_FORWARD,
  MDFIT_F_N_SIGMA_REVERSE,
  MDFIT_F_D_MAX_REVERSE,
  MDFIT_F_Q_MEAN_REVERSE,
  MDFIT_F_ASYMMETRY,
  MDFIT_F_NORMALIZED_NOISE,
  MDFIT_F_NORMALIZED_NOISE_FORWARD,
  MDFIT_F_NORMALIZED_NOISE_REVERSE,
  MDFIT_NRESULT, /* = 25 result columns */
  /* diagnostics: sub-fit k in {0 PMD-all, 1 null-all, 2 PMD-fwd, 3 PMD-rev,
   * 4 null-fwd, 5 null-rev} occupies MDFIT_F_DIAG + 8*k + {q, A, c, phi,
   * objective, evaluations, status, polished}.  Null sub-fits store A = c = 0.
   * MAP: `polished` = 1 when the fit entered its polish phase (DESIGN.md
   * §3.4); its objective is then the cancellation-free form (the full log-pmf,
   * log C(N,y) included), else the lnGamma-sum form.  After the MDFIT-MAP
 * v1.1 quadratic-contraction stop the returned point is u + d
 * (the last Newton step taken without evaluating its end) while `objective`
 * holds F at the last EVALUATED point u: it exceeds F(u + d) by O(|g.d|) <=
 * ~1e-9 relative (the oracle stores the same).  NUTS: {posterior means
   * of q, A, c, phi, adapted step size, leapfrogs per draw, status,
   * divergences}. */
  MDFIT_F_DIAG = 32,
  MDFIT_NOUT = 80
};

#define MDFIT_NSUBFIT 6
#define MDFIT_DIAG_STRIDE 8

/* Prediction record: float pred[T][3][30] = (median, hdpi_lower, hdpi_upper)
 * per position, the payload of fit_predictions (fits.py:632-665). */
#define MDFIT_NPRED 3

typedef struct mdfit_opts {
  int32_t mode;       /* MDFIT_MODE_MAP or MDFIT_MODE_NUTS */
  int32_t max_iter;   /* MAP: objective evaluations per sub-fit (default 200) */
  double tol_step;    /* MAP: convergence, max |Newton step| in unconstrained units (default 1e-9) */
  uint64_t seed;      /* NUTS: key of the Philox streams (default 0, the reference's Key(0)) */
  int32_t num_warmup; /* NUTS: adaptation iterations (default 500, fits.py:792-799) */
  int32_t num_samples;/* NUTS: kept iterations (default 1000) */
  int64_t index_base; /* NUTS: global index of taxon 0 of this call -- the random streams are keyed
                         by it, so a sharded run draws the same numbers as one call (default 0) */
} mdfit_opts;

/* Fill `opts` with defaults. */
void mdfit_default_opts(mdfit_opts* opts);

/*
 * Fit a batch of taxa.
 *   y, N      : const uint32_t[n_taxa][MDFIT_LD]           (device)
 *   mm        : const uint32_t[n_taxa][30][MDFIT_NMM] or NULL (device; NULL -> noise columns NaN)
 *   out       : double[n_taxa][MDFIT_NOUT]                  (device)
 *   pred      : float[n_taxa][MDFIT_NPRED][MDFIT_NPOS] or NULL (device)
 *   status    : int32_t[n_taxa]                             (device)
 *   workspace : device buffer of mdfit_workspace_bytes(n_taxa) bytes (work
 *               queues, the PMD-all mode for the HPDI, the wide-window list:
 *               MAP 256 B + 48 B per taxon below 60k taxa, + 4,800 B more
 *               per taxon from 60k (160 B per position's wide-window record),
 *               + the HPDI stream's defer list: min(120 B per taxon, 512 KB);
 *               NUTS 256 B + 6 x num_samples x 32 B per taxon, the draws)
 *   hip_stream: hipStream_t or NULL.  MAP: parts of the call run on two
 *               library-owned side streams (one set per device, created once),
 *               forked from and joined back into hip_stream by events on every
 *               return path, so the call stays ordered on hip_stream and
 *               capturable in a graph: below 60k taxa the early HPDI launch
 *               beside the fit kernel and the late HPDI launch beside the
 *               record assembly (which follows the fit on hip_stream); from
 *               60k taxa the record assembly beside the HPDI launches (which
 *               stay on hip_stream).  MAP below 60k taxa: the predictive
 *               HPDI kernel runs beside the fit kernel and waits for modes
 *               the fit kernel's waves publish (relaxed, order-free: each
 *               field of a ready-list entry is written once as the bit
 *               complement of its value into a list the call zeroed, and an
 *               entry is taken when every field reads non-zero -- no fence,
 *               DESIGN.md §4); the two grids are sized to be co-resident on
 *               an otherwise idle device.
 *               The waits are bounded: a wave that makes no progress for 1 ms
 *               hands its items to the HPDI launch after the fit and exits, so
 *               concurrent calls or other kernels on the device (e.g. an RCCL
 *               collective) cost time, never a hang.  Fastest when calls on
 *               one device run one after another.
 *   n_taxa    : at most 2^25 per call (MAP: int32 position indices)
 * Replaces compute_fits' per-taxon loop (fits.py:477-526, 569-626, 709-730).
 */
int mdfit_fit_batch(const uint32_t* y, const uint32_t* N, const uint32_t* mm,
                    int64_t n_taxa, const mdfit_opts* opts, double* out,
                    float* pred, int32_t* status, void* workspace,
                    void* hip_stream);

/* Bytes of device workspace mdfit_fit_batch needs for n_taxa taxa under
 * `opts` (NULL = defaults; NUTS keeps every chain's samples there:
 * 6 x num_samples x 4 doubles per taxon). */
int64_t mdfit_workspace_bytes(int64_t n_taxa, const mdfit_opts* opts);

/*
 * mdfit_fit_batch in MDFIT_MODE_NUTS with the random streams of each row keyed
 * by a global taxon index the caller gives (MDFIT-AUTO v1):
 *   taxon_index : const int64_t[n_taxa], every entry >= 0 (device), or NULL
 * Row t's Philox streams -- the chain's, at its start, and the predictive
 * draws' of the record assembly -- are keyed by opts->index_base +
 * taxon_index[t] instead of opts->index_base + t.  Everything else is row t's:
 * the rows of y, N, mm, out, pred, status, the draws in the workspace
 * (mdfit_workspace_bytes(n_taxa, opts) bytes) and the work queues.  So fitting
 * the rows idx of a batch with taxon_index = idx gives the rows idx of the full
 * call bit for bit -- record, predictions, status and draws.  Duplicate
 * indices are allowed and draw the same numbers.  taxon_index == NULL is
 * exactly mdfit_fit_batch (which launches the same kernels as it always did);
 * MDFIT_MODE_MAP with a non-NULL index returns MDFIT_E_ARG (the MAP fit draws
 * nothing).  The index is read once per chain start and once per taxon of the
 * record assembly; the sampler's inner loop is the plain call's.
 * mdfit_nuts_diag, mdfit_nuts_summary and mdfit_nuts_loo draw nothing: they
 * work on the workspace and records of an indexed call unchanged, row by row.
 */
int mdfit_fit_batch_indexed(const uint32_t* y, const uint32_t* N, const uint32_t* mm, int64_t n_taxa,
                            const int64_t* taxon_index, const mdfit_opts* opts, double* out, float* pred,
                            int32_t* status, void* workspace, void* hip_stream);

/* Route bits of mdfit_auto_route (route[t]); the taxon goes to the sampler iff
 * route & MDFIT_ROUTE_SAMPLE is non-zero. */
#define MDFIT_ROUTE_WAIC 1    /* row 6 of the waic record lacks bit 1 (not all six rows valid and reliable) */
#define MDFIT_ROUTE_PSIS 2    /* some row 0..2 of the psis record lacks bit 0 or bit 1 */
#define MDFIT_ROUTE_STATUS 4  /* status[t] is MDFIT_MAXITER or MDFIT_NONFINITE */
#define MDFIT_ROUTE_INVALID 8 /* status[t] == MDFIT_INVALID: not sampled, its NaN record left alone, no other bit */
#define MDFIT_ROUTE_SAMPLE 7

/*
 * The routing rule of the auto inference (MDFIT-AUTO v1): which
 * taxa of a finished MODE_MAP call the importance sampling settles, and their
 * record.
 *   status, psis, waic : that call's status[n_taxa], its mdfit_map_psis records
 *                [n_taxa][3][MDFIT_NMAPPSIS] and its mdfit_map_waic records
 *                [n_taxa][7][MDFIT_NMAPWAIC], the two from the same num_draws,
 *                seed and index_base (device; read only)
 *   out        : that call's records double[n_taxa][MDFIT_NOUT] (device).  For a
 *                taxon with route 0 nine result columns are overwritten with the
 *                importance-sampled posterior statistics, copied exactly:
 *                q_mean, concentration_mean, D_max_marginalized_mean <- psis
 *                row 0 q_mean, phi_mean, D_max_mean; q_mean_forward,
 *                q_mean_reverse <- psis rows 1, 2 q_mean; n_sigma,
 *                n_sigma_forward, n_sigma_reverse, asymmetry <- waic row 6
 *                fields 0..3.  Every other field, and every field of a taxon
 *                with route != 0, is left as the MAP call wrote it (D_max, its
 *                HPDI bounds, D_max_forward / _reverse and pred are predictive
 *                quantities, exact at the mode).
 *   route      : int32_t[n_taxa], the MDFIT_ROUTE_* bits             (device)
 * By the bit-for-bit identity of the PMD rows of the two records,
 * MDFIT_ROUTE_PSIS is never set without MDFIT_ROUTE_WAIC on records of one
 * call; the rule checks it regardless.  One launch on hip_stream, one thread
 * per taxon; no workspace, no atomics, no host synchronisation.  n_taxa: at
 * most 2^25 per call.
 */
int mdfit_auto_route(const int32_t* status, const double* psis, const double* waic, int64_t n_taxa,
                     double* out, int32_t* route, void* hip_stream);

/* Route bit of mdfit_auto_route_pred beside the four above; the taxon goes to
 * the sampler iff route & MDFIT_ROUTE_SAMPLE_PRED is non-zero. */
#define MDFIT_ROUTE_PRED 16        /* the pred record lacks flags bit 1, or counts a job made NaN by a draw that is no count */
#define MDFIT_ROUTE_SAMPLE_PRED 23 /* MDFIT_ROUTE_SAMPLE | MDFIT_ROUTE_PRED */

/*
 * mdfit_auto_route with the importance-weighted posterior predictive
 * (MDFIT-AUTO v1.1).  route[t] is mdfit_auto_route's, plus
 * MDFIT_ROUTE_PRED when flags of prec[t] lacks bit 1 or its n_noncount field is
 * not 0 (a NaN counts as not 0); a taxon with MDFIT_INVALID gets
 * MDFIT_ROUTE_INVALID alone.
 *   status, psis, waic : as mdfit_auto_route's
 *   prec, ppred : the records double[n_taxa][MDFIT_NMAPPRED] and float[n_taxa]
 *                [MDFIT_NPRED][30] of mdfit_map_pred_adapt (or mdfit_map_pred)
 *                from the same num_draws, adapt_rounds, seed and index_base as
 *                psis and waic (device; read only)
 *   out        : for a taxon with route 0 the nine columns of mdfit_auto_route
 *                and D_max, D_max_lower_hpdi, D_max_upper_hpdi, D_max_forward,
 *                D_max_reverse <- prec fields 0..4, copied exactly; every other
 *                field, and every field of a taxon with route != 0, is left as
 *                the MAP call wrote it                               (device)
 *   pred       : the MAP call's float[n_taxa][MDFIT_NPRED][30], or NULL; for a
 *                taxon with route 0 its 90 floats <- ppred's         (device)
 *   route      : int32_t[n_taxa]                                     (device)
 * By the bit-for-bit identity of khat and the valid / reliable bits of the pred
 * and psis records of one call, the flags half of MDFIT_ROUTE_PRED is never set
 * without MDFIT_ROUTE_PSIS; the rule checks it regardless.  One launch on
 * hip_stream, one thread per taxon; no workspace, no atomics, no host
 * synchronisation.  n_taxa: at most 2^25 per call.
 */
int mdfit_auto_route_pred(const int32_t* status, const double* psis, const double* waic, const double* prec,
                          const float* ppred, int64_t n_taxa, double* out, float* pred, int32_t* route,
                          void* hip_stream);

/*
 * Noise columns of records fitted with mm = NULL (both modes): the three
 * normalized_noise columns of out[n_taxa][MDFIT_NOUT] from the mismatch counts
 * mm[n_taxa][30][12] (add_noise_estimates, fits.py:359-376) -- the values a
 * call with mm writes, bit for bit; taxa with y > N (status 3, NaN record) are
 * left alone.  Device pointers, stream-ordered.  Lets a host ship the 1,440 B
 * per taxon of mismatch counts while the fit runs (engine.ChunkedFitter).
 */
int mdfit_noise(const uint32_t* y, const uint32_t* N, const uint32_t* mm, int64_t n_taxa, double* out,
                void* hip_stream);

/* Laplace record: double lap[T][3][MDFIT_NLAPLACE], one row per PMD sub-fit
 * (0 all positions, 1 forward, 2 reverse): q_std, A_std, c_std, phi_std,
 * D_max_std, rho_Ac, significance, flags.  flags (an integer stored as double):
 * bit j (1, 2, 4, 8) coordinate j of (q, A, c, phi) is free, bit 4 (16) the
 * row is valid. */
#define MDFIT_NLAPLACE 8

/*
 * Laplace standard errors of finished MAP records: per PMD
 * sub-fit one evaluation of the objective's Hessian at the mode -- the fit
 * kernel's own code, at u = (logit q, logit A, c, log(phi - 2)) rebuilt from
 * the record's diagnostic slots -- the inverse of its block over the
 * coordinates the optimiser's binding rule does not hold on a box bound, and
 * the delta method to (q, A, c, phi) and D_max = A + c:
 *   std_j = J_j sqrt(C_jj), J = (q(1-q), A(1-A), 1, phi - 2); 0 for a held j
 *   D_max_std = sqrt(J_A^2 C_AA + C_cc + 2 J_A C_Ac)
 *   rho_Ac = C_Ac / sqrt(C_AA C_cc)   (NaN when A or c is held)
 *   significance = (A + c) / D_max_std (NaN when D_max_std = 0)
 * The Hessian includes the priors: these are posterior-mode standard errors,
 * not likelihood-only ones.  A row is valid when status[t] == 0, at least one
 * coordinate is free, every free H_jj > 0 and every pivot of the Cholesky of
 * the Jacobi-scaled free block exceeds 1e-8; otherwise its seven statistics
 * are NaN and bit 4 of flags is clear (status[t] != 0: flags 0).
 *   y, N, out, status : the inputs and results of a finished MODE_MAP
 *                       mdfit_fit_batch call (device; read only -- records of a
 *                       MODE_NUTS call hold posterior means, not modes, and give
 *                       meaningless numbers)
 *   lap               : double[n_taxa][3][MDFIT_NLAPLACE]       (device)
 *   gh                : double[n_taxa][3][20] or NULL (device): the gradient
 *                       g[4], then the Hessian H[4][4], at the rebuilt u (parity
 *                       tests)
 * One launch on hip_stream, one wave per taxon; no workspace, no side stream,
 * no host synchronisation.  n_taxa: at most 2^25 per call.
 */
int mdfit_map_laplace(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                      int64_t n_taxa, double* lap, double* gh, void* hip_stream);

/* The same launch (the same kernel), which also writes the rebuilt modes it
 * evaluates at: u double[n_taxa][3][4] or NULL (device; NaN where status[t]
 * != 0).  For parity tests: g and H of `gh` are those of mdfit_objective at
 * exactly these u. */
int mdfit_map_laplace_u(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                        int64_t n_taxa, double* lap, double* gh, double* u, void* hip_stream);

/* Sampling diagnostics record: double diag[T][6][MDFIT_NNUTSDIAG], one row per
 * sub-fit in the order of the diagnostic slots: ess(q, A, c, phi, D_max),
 * rhat(q, A, c, phi, D_max), mcse(D_max), flags (an integer stored as double:
 * bit 0 the row is valid). */
#define MDFIT_NNUTSDIAG 12

/*
 * Convergence diagnostics of the chains of a finished MODE_NUTS call
 * (MDFIT-DIAG v1): per sub-fit and per series -- q, A, c, phi
 * and D_max (A + c of a PMD sub-fit, q of a null one) -- the effective sample
 * size by Geyer's initial monotone sequence, capped at S log10 S, the split
 * R-hat of the chain's two halves, and for D_max the Monte Carlo standard
 * error sqrt(var / ess); what numpyro's print_summary shows as n_eff and r_hat
 * for the reference's MCMC objects (fits.py:440), in the single-chain case.  A
 * constant series (a null sub-fit's A and c) gives NaN.  A row is valid when
 * the chain's status slot (MDFIT_F_DIAG + 8k + 6) is 0 and every draw of the
 * sub-fit is finite; otherwise its eleven statistics are NaN and flags is 0.
 *   workspace : the workspace of that call (device; read only): the draws
 *               double[n_taxa][6][num_samples][4] behind its first 256 bytes,
 *               intact until the next mdfit_fit_batch on it
 *   out       : its records (device; read only)
 *   opts      : the options of that call: mode MDFIT_MODE_NUTS, num_samples in
 *               [2, 4096] (else MDFIT_E_ARG)
 *   diag      : double[n_taxa][6][MDFIT_NNUTSDIAG]                (device)
 * One launch on hip_stream, one wave per sub-fit; no allocation, no side
 * stream, no host synchronisation.  n_taxa: at most 2^25 per call.
 */
int mdfit_nuts_diag(const void* workspace, const double* out, int64_t n_taxa,
                    const mdfit_opts* opts, double* diag, void* hip_stream);

/* Posterior summary record: double summ[T][6][MDFIT_NNUTSSUMM], one row per
 * sub-fit in the order of the diagnostic slots: std(q, A, c, phi, D_max) with
 * ddof 1, D_max_mean, D_max (median, lo, hi), q (median, lo, hi), phi_median,
 * rho_Ac, significance, flags (an integer stored as double: bit 0 the row is
 * valid). */
#define MDFIT_NNUTSSUMM 16

/*
 * Posterior summary of the chains of a finished MODE_NUTS call (MDFIT-SUMM v1,
 * DESIGN.md §9.2): per sub-fit the standard deviations (ddof 1) of q, A, c,
 * phi and D_max (A + c of a PMD sub-fit, q of a null one), the mean of D_max,
 * the median (np.median) and the 68 % highest-posterior-density interval
 * (numpyro's hpdi: the narrowest window of int(0.68 S) + 1 sorted draws, the
 * lowest index among equal widths) of D_max, q and phi's median, the Pearson
 * correlation of A and c, and significance = D_max_mean / D_max_std; what the
 * reference's user computes from the MCMC objects kept at fits.py:440.  A
 * constant series has std 0; rho_Ac is NaN when A or c is constant (a null
 * sub-fit), significance when D_max_std is 0.  The order statistics are draws
 * or one subtraction of two: exact.  A row is valid when the chain's status
 * slot (MDFIT_F_DIAG + 8k + 6) is 0 and every draw of the sub-fit is finite;
 * otherwise its fifteen statistics are NaN and flags is 0.
 *   workspace : the workspace of that call (device; read only): the draws
 *               double[n_taxa][6][num_samples][4] behind its first 256 bytes,
 *               intact until the next mdfit_fit_batch on it
 *   out       : its records (device; read only)
 *   opts      : the options of that call: mode MDFIT_MODE_NUTS, num_samples in
 *               [2, 4096] (else MDFIT_E_ARG)
 *   summ      : double[n_taxa][6][MDFIT_NNUTSSUMM]                (device)
 * One launch on hip_stream, one wave per sub-fit; no allocation, no side
 * stream, no host synchronisation.  n_taxa: at most 2^25 per call.
 * Independent of mdfit_nuts_diag: both may run on one finished call's
 * workspace, in either order.
 */
int mdfit_nuts_summary(const void* workspace, const double* out, int64_t n_taxa,
                       const mdfit_opts* opts, double* summ, void* hip_stream);

/* PSIS-LOO record: double loo[T][7][MDFIT_NNUTSLOO].  Rows 0..5, one per
 * sub-fit in the order of the diagnostic slots: elpd_loo, p_loo, elpd_se,
 * khat_max, khat_argmax (the point's column 0..29, the lowest on ties), n_bad
 * (points with khat > min(1 - 1 / log10 S, 0.7)), lppd, flags (an integer stored
 * as double: bit 0 the row is valid).  Row 6, the comparisons: n_sigma_loo,
 * n_sigma_loo_forward, n_sigma_loo_reverse, asymmetry_loo, khat_max and n_bad
 * over the six rows, 0, flags (valid when all six rows are). */
#define MDFIT_NNUTSLOO 8

/*
 * Pareto-smoothed importance-sampling leave-one-out of the chains of a finished
 * MODE_NUTS call (MDFIT-LOO v1): per sub-fit and point the
 * pointwise log-likelihood of every draw (the full beta-binomial log-pmf, as
 * the record's WAIC forms it), the generalised Pareto fit of the top M =
 * min(S / 5, ceil(3 sqrt S)) importance ratios (Zhang & Stephens 2009 with
 * loo's priors) giving the point's shape khat, the smoothed tail and elpd_i;
 * per sub-fit their sums and khat's maximum; in row 6 the reference's n_sigma
 * comparisons (fits.py:194-227) on looic_i = -2 elpd_i in place of waic_i.
 * khat is +inf when S < 25 and 0 when the tail is constant (a position with N
 * = 0); neither is smoothed.  A row is valid when the chain's status slot is
 * 0 and every pointwise log-likelihood of the sub-fit is finite; otherwise
 * its seven statistics are NaN and flags is 0, as are all seven rows of a taxon
 * with some y > N.
 *   y, N      : the counts of that call, uint32[n_taxa][MDFIT_LD] (device; read only)
 *   workspace : the workspace of that call (device; read only)
 *   out       : its records (device; read only)
 *   opts      : the options of that call: mode MDFIT_MODE_NUTS, num_samples in
 *               [2, 4096] (else MDFIT_E_ARG)
 *   loo       : double[n_taxa][7][MDFIT_NNUTSLOO]                  (device)
 *   pointwise : double[n_taxa][6][30][2] = (elpd_i, khat_i), NaN outside a
 *               sub-fit's points and in an invalid row, or NULL    (device)
 * One launch on hip_stream, one wave per taxon; no allocation, no side stream,
 * no host synchronisation, no atomics.  n_taxa: at most 2^25 per call.
 * Independent of mdfit_nuts_diag and mdfit_nuts_summary: all may run on one
 * finished call's workspace, in any order.
 */
int mdfit_nuts_loo(const uint32_t* y, const uint32_t* N, const void* workspace, const double* out,
                   int64_t n_taxa, const mdfit_opts* opts, double* loo, double* pointwise,
                   void* hip_stream);

/*
 * Test helper: the record assembly of a MODE_NUTS call (its post kernel, the
 * same source lines as the product's launch) alone, on draws and chain
 * diagnostics the caller chose.  What mdfit_fit_batch's second kernel does
 * after the chains: the posterior means, waic_i per sub-fit and point, n_sigma
 * x3 and asymmetry, the predictive median and 68 % HPDI, the sums and the
 * noise.  tests/test_gpu_nuts_post.py pins it on crafted draws.
 *   y, N, mm  : as for mdfit_fit_batch (device; read only); mm may be NULL
 *   opts      : mode MDFIT_MODE_NUTS, num_samples in [2, 4096] (else
 *               MDFIT_E_ARG); seed and index_base key the predictive streams
 *   workspace : mdfit_workspace_bytes() bytes whose draws
 *               double[n_taxa][6][num_samples][4] behind the first 256 bytes
 *               the caller wrote (device; read only)
 *   out       : double[n_taxa][MDFIT_NOUT]; on entry the chain diag slots 4..7
 *               of each sub-fit (MDFIT_F_DIAG + 8k + 4..7: step, leapfrogs,
 *               status, divergences) as the chains would have left them, the
 *               rest zero (as mdfit_fit_batch clears it); on return the
 *               record                                            (device)
 *   pred      : float[n_taxa][MDFIT_NPRED][30], or NULL           (device)
 *   status    : int32[n_taxa]                                     (device)
 * Two taps of what the kernel forms on the way, each NULL or:
 *   waic      : double[n_taxa][6][30], waic_i of sub-fit k at column i; NaN
 *               where the kernel forms none (columns outside a forward /
 *               reverse sub-fit, a taxon with y > N or a failed chain)
 *   counts    : uint32[n_taxa][32][num_samples], the unsorted predictive
 *               counts of job j: 0..29 the columns under the PMD-all chain, 30
 *               and 31 column 0 under the forward and the reverse PMD chain;
 *               0xFFFFFFFF where the draw was no count in [0, N] and in a job
 *               that was not run
 *   count_flags : uint8[n_taxa][32] per job: 0 every draw a count, 1 some
 *               draw was none (the job's median and HPDI are NaN), 2 skipped
 *               for N = 0, 0xFF not reached (y > N or a failed chain); tells
 *               0xFFFFFFFF the count (N = 4294967295) from the marker
 * The taps are first filled with 0xFF bytes on hip_stream, then one launch,
 * one wave per taxon; no allocation, no host synchronisation.  n_taxa: at most
 * 2^25 per call.
 */
int mdfit_nuts_post(const uint32_t* y, const uint32_t* N, const uint32_t* mm, int64_t n_taxa,
                    const mdfit_opts* opts, const void* workspace, double* out, float* pred,
                    int32_t* status, double* waic, uint32_t* counts, uint8_t* count_flags,
                    void* hip_stream);

/*
 * Test helper: the estimator of mdfit_nuts_loo (its device function) on given
 * pointwise log-likelihood series ll[n_series][S], one wave per series:
 * elpd[i] and khat[i]; NaN for a series with a value that is not finite.  S in
 * [2, 4096] (else MDFIT_E_ARG); n_series at most 2^25.  Device pointers.
 */
int mdfit_psis(const double* ll, int64_t n_series, int32_t S, double* elpd, double* khat,
               void* hip_stream);

/* Importance-sampled posterior record: double psis[T][3][MDFIT_NMAPPSIS], rows
 * PMD-all, PMD-forward, PMD-reverse: q_mean A_mean c_mean phi_mean D_max_mean,
 * q_std A_std c_std phi_std D_max_std, rho_Ac, significance, khat, ess,
 * n_infeasible, flags (an integer stored as double: bit 0 the row is valid,
 * bit 1 khat <= min(1 - 1 / log10 S, 0.7), bits 2..5 coordinate (q, A, c, phi)
 * free). */
#define MDFIT_NMAPPSIS 16

/*
 * Importance-sampled posterior of the PMD sub-fits of a finished MODE_MAP call
 * (MDFIT-PSIS v1).  Per sub-fit: num_draws points from a
 * multivariate Student-t (nu = 4) centred on the mode with the Laplace
 * covariance of mdfit_map_laplace (its held set and factorisation, bit for
 * bit; a c held on 0 is drawn from the exponential of its gradient and moves
 * the centre of the free block), each weighted by the density the sampling
 * mode draws from -- the full beta-binomial log-pmf, the priors and the
 * Jacobian of u = (logit q, logit A, c, log delta) -- over the proposal's.  A
 * draw with c < 0 or A + c >= 1 is infeasible: weight 0.  The weights are
 * Pareto-smoothed (the top M = min(S / 5, ceil(3 sqrt S)) by rank, ties by draw
 * index, take the quantiles of the generalised Pareto fit of mdfit_nuts_loo)
 * and normalised; the record holds the weighted means and standard deviations
 * of q, A, c, phi and D_max = A + c, the weighted A-c correlation,
 * significance = D_max_mean / D_max_std, the fit's shape khat, ess = 1 / sum
 * w^2 and the number of infeasible draws.  khat above the threshold of bit 1
 * says that the estimates cannot be trusted and the taxon needs the sampling
 * mode.  A row is invalid -- NaN statistics, the free bits alone in flags --
 * when q, A or phi is held or c is held elsewhere than on 0, when the Laplace
 * row is invalid, when a log-weight is NaN or +inf, or when the draw that sets
 * the tail's cut-off is infeasible.  A taxon with status != MDFIT_OK gets NaN
 * statistics and flags 0.
 *   y, N, out, status : those of the MODE_MAP call (device; read only)
 *   num_draws  : S in [25, 1024] (else MDFIT_E_ARG): 25 is the smallest S with
 *                a five-draw tail; at 1024 a wave takes 22,016 B of LDS, so six
 *                blocks still share a CU's 160 KB
 *   seed, index_base : the Philox streams are keyed by (seed, index_base +
 *                taxon, sub-fit): a chunked or sharded run draws what one call
 *                draws
 *   psis       : double[n_taxa][3][MDFIT_NMAPPSIS]                 (device)
 *   draws      : double[n_taxa][3][num_draws][6] = u[4], the raw log-weight,
 *                the weight; NaN in an invalid row; or NULL         (device)
 * One launch on hip_stream, one wave per taxon; no workspace, no allocation,
 * no side stream, no host synchronisation, no atomics; capturable in a graph.
 * n_taxa: at most 2^25 per call.
 */
int mdfit_map_psis(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                   int64_t n_taxa, int32_t num_draws, uint64_t seed, int64_t index_base,
                   double* psis, double* draws, void* hip_stream);

/*
 * Test helper: the smoothing of mdfit_map_psis (its device function) on given
 * log-weight series lw[n_series][S], one wave per series: the normalised
 * weights w[n_series][S] and khat[i]; -inf is an infeasible draw; NaN for a
 * series with a NaN or +inf or an infeasible cut-off draw.  S in [25, 1024]
 * (else MDFIT_E_ARG); n_series at most 2^25.  Device pointers.
 */
int mdfit_psis_weights(const double* lw, int64_t n_series, int32_t S, double* w, double* khat,
                       void* hip_stream);

/* Importance-weighted WAIC record: double waic[T][7][MDFIT_NMAPWAIC].  Rows
 * 0..5, one per sub-fit in diagnostic-slot order (PMD-all, null-all, PMD-fwd,
 * PMD-rev, null-fwd, null-rev): elpd_waic = sum_i (lppd_i - p_i), p_waic =
 * sum_i p_i, lppd, khat, ess = 1 / sum w^2, n_infeasible, p_waic_max = max_i
 * p_i, flags (an integer stored as double: bit 0 the row is valid, bit 1 khat
 * <= min(1 - 1 / log10 S, 0.7), bits 2..5 coordinate (q, A, c, phi) free).
 * Row 6, the comparisons: n_sigma_waic, n_sigma_waic_forward,
 * n_sigma_waic_reverse, asymmetry_waic, khat_max and ess_min over the valid
 * rows, 0, flags (bit 0 all six rows valid, bit 1 all six valid and at or
 * under the khat threshold). */
#define MDFIT_NMAPWAIC 8

/*
 * Importance-weighted WAIC of the six sub-fits of a finished MODE_MAP call and
 * the reference's comparisons on it (MDFIT-WAIC v1, DESIGN.md §3.9;
 * fits.py:147-227).  The PMD rows are importance-sampled as mdfit_map_psis
 * does it: the same proposal, Philox stream (sub-fit 0 / 2 / 3), target,
 * smoothing and validity rule, so khat, ess, n_infeasible and the free bits of
 * rows 0, 2, 3 are mdfit_map_psis's bit for bit.  A null row (stream sub-fit
 * 1 / 4 / 5, the same domain and block layout) draws (logit q, log delta) from
 * a bivariate Student-t (nu = 4) on the Laplace fit of the null objective at
 * its mode and weighs it by the null model's log-pmf, priors and Jacobian; it
 * is valid when q and delta are free, both diagonal entries of H are positive
 * and the Jacobi-scaled 2x2 Cholesky's pivots exceed 1e-8.  For a valid row,
 * with the smoothed, normalised weights w_s and l_si the full beta-binomial
 * log-pmf of draw s at point i of the row's 15 or 30 columns: lppd_i = log
 * sum_s w_s exp(l_si), p_i = sum_s w_s (l_si - sum_s w_s l_si)^2, waic_i = -2
 * (lppd_i - p_i); a point with N_i = 0 has lppd_i = p_i = 0 exactly.  Row 6 is
 * the reference's n_sigma of the waic_i columns: n_sigma_waic needs rows 0 and
 * 1, forward rows 2 and 4, reverse rows 3 and 5, asymmetry rows 0, 2 and 3;
 * NaN when one of them is invalid.  An invalid row has NaN statistics and only
 * its free bits in flags; a taxon with status != MDFIT_OK NaN statistics and
 * flags 0 in all seven rows.
 *   y, N, out, status : those of the MODE_MAP call (device; read only)
 *   num_draws  : S in [25, 1024] (else MDFIT_E_ARG)
 *   seed, index_base : the Philox streams are keyed by (seed, index_base +
 *                taxon, sub-fit), as mdfit_map_psis's
 *   waic       : double[n_taxa][7][MDFIT_NMAPWAIC]                 (device)
 *   pointwise  : double[n_taxa][6][30][2] = (lppd_i, p_i); NaN outside a
 *                sub-fit's columns and in an invalid row; or NULL   (device)
 *   draws      : double[n_taxa][6][num_draws][6] = u[4] (a null row: u[1] = u[2]
 *                = 0), the raw log-weight, the weight; NaN in an invalid row;
 *                or NULL (parity tests)                             (device)
 * One launch on hip_stream, one wave per taxon; no workspace, no allocation,
 * no side stream, no host synchronisation, no atomics; capturable in a graph.
 * n_taxa: at most 2^25 per call.
 */
int mdfit_map_waic(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                   int64_t n_taxa, int32_t num_draws, uint64_t seed, int64_t index_base,
                   double* waic, double* pointwise, double* draws, void* hip_stream);

/* Adapt record: double adapt[T][3][MDFIT_NMAPADAPT], rows PMD-all, PMD-forward,
 * PMD-reverse: khat of round 0, ess of round 0, the best round, the rounds
 * tried (redrawn and smoothed).  NaN in a row that is invalid in round 0 and
 * for a taxon with status != MDFIT_OK. */
#define MDFIT_NMAPADAPT 4
#define MDFIT_ADAPT_MAX_ROUNDS 4
/* flags bit 6 of a PMD row of the psis and waic records written by the two
 * entries below: the best round is > 0 (the proposal was refitted). */
#define MDFIT_FLAG_ADAPTED 64

/*
 * mdfit_map_psis with moment-matched proposal rounds (MDFIT-ADAPT v1, DESIGN.md
 * §3.12; importance-weighted moment matching, Paananen et al. 2021).  Round 0
 * is mdfit_map_psis exactly; a row invalid there stays invalid.  While the best
 * round's khat is over the threshold of flags bit 1 and fewer than
 * adapt_rounds rounds have run, the Student-t proposal is refitted to the best
 * round's smoothed weights w: with rho_j = u_j - K_j c_s the residual of free
 * coordinate j (K the shift of the centre with a held c, zero when c is free),
 * the new centre is m_j = sum w rho_j (+ K_j c_s), the new scale the weighted
 * covariance C of rho -- d_j = sqrt(C_jj) and the upper-triangular factor F of
 * C_jm / (d_j d_m) = (F F')_jm -- and, with c held on 0, the exponential's new
 * rate 1 / sum w c_s.  All num_draws draws are redrawn from the same Philox
 * blocks, weighted and smoothed again; the round becomes the best one when it
 * is valid and its khat is finite and below the best one's, and ends the loop
 * otherwise, as do a C_jj that is not > 0, a pivot of the factor <= 1e-8, a
 * mean held c that is not > 0 and anything non-finite.  The record is that of
 * the best round, with MDFIT_FLAG_ADAPTED in flags when that is not round 0.
 * With adapt_rounds = 0 psis and draws are mdfit_map_psis's bit for bit and
 * adapt reads (khat, ess, 0, 0).
 *   adapt_rounds : R in [0, MDFIT_ADAPT_MAX_ROUNDS] (else MDFIT_E_ARG)
 *   adapt      : double[n_taxa][3][MDFIT_NMAPADAPT], or NULL       (device)
 *   draws      : as mdfit_map_psis's, of the best round.  The constants dropped
 *                from log g differ from round to round, so raw log-weights
 *                compare within a round only; the weights are normalised
 * The other arguments, the launch and its guarantees are mdfit_map_psis's; the
 * records do not depend on the grid, the chunking or index_base's split.
 */
int mdfit_map_psis_adapt(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                         int64_t n_taxa, int32_t num_draws, int32_t adapt_rounds, uint64_t seed,
                         int64_t index_base, double* psis, double* adapt, double* draws, void* hip_stream);

/*
 * mdfit_map_waic with the rounds of mdfit_map_psis_adapt on its PMD rows (0, 2,
 * 3): their khat, ess, n_infeasible, flags and adapt rows are
 * mdfit_map_psis_adapt's bit for bit, and their WAIC statistics those of the
 * best round's weights.  The null rows (1, 4, 5) are not adapted: they are
 * mdfit_map_waic's bit for bit.  With adapt_rounds = 0 waic, pointwise and
 * draws are mdfit_map_waic's bit for bit.
 *   adapt      : double[n_taxa][3][MDFIT_NMAPADAPT] (rows PMD-all, PMD-forward,
 *                PMD-reverse), or NULL                              (device)
 */
int mdfit_map_waic_adapt(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                         int64_t n_taxa, int32_t num_draws, int32_t adapt_rounds, uint64_t seed,
                         int64_t index_base, double* waic, double* adapt, double* pointwise, double* draws,
                         void* hip_stream);

/* Importance-sampled evidence record: double evid[T][7][MDFIT_NMAPEVID].  Rows
 * 0..5, one per sub-fit in diagnostic-slot order (PMD-all, null-all, PMD-fwd,
 * PMD-rev, null-fwd, null-rev): log_evidence, se, khat, ess = 1 / sum w^2,
 * n_infeasible, log_w_max = K_prior - K_prop + max lw, the best adapt round (0
 * without rounds and in a null row), flags (an integer stored as double: bit 0
 * the row is valid, bit 1 khat <= min(1 - 1 / log10 S, 0.7), bits 2..5
 * coordinate (q, A, c, phi) free, bit 6 MDFIT_FLAG_ADAPTED).  Row 6, the
 * comparisons: log_bf = lZ_0 - lZ_1, log_bf_forward = lZ_2 - lZ_4,
 * log_bf_reverse = lZ_3 - lZ_5, log_bf_asymmetry = lZ_0 - (lZ_2 + lZ_3) (the
 * sign of the reference's asymmetry: positive favours one decay for both
 * strands), log_bf_se = sqrt(se_0^2 + se_1^2), khat_max and ess_min over the
 * valid rows, flags (bit 0 all six rows valid, bit 1 all six valid and at or
 * under the khat threshold). */
#define MDFIT_NMAPEVID 8

/*
 * Importance-sampled marginal likelihood (evidence) of the six sub-fits of a
 * finished MODE_MAP call and the Bayes factors PMD : null on it (MDFIT-EVID v1,
 * DESIGN.md §3.14).  Per sub-fit the raw log-weights lw_t are mdfit_map_waic's
 * exactly -- the same proposal, Philox stream (sub-fit index = row), target,
 * feasibility rule and dropped constants -- and are smoothed as there.  With c
 * the largest finite lw_t, tot the sum of the smoothed weights exp(lw_t - c)
 * (an infeasible draw adds 0 and still counts in S) and w the normalised ones,
 *   log_evidence = K_prior - K_prop + c + log(tot / S),
 *   se           = sqrt(sum_t (w_t - 1/S)^2)   (= sqrt(1/ess - 1/S)),
 * the delta-method standard error of the log of the mean weight.  K_prior, the
 * constants left out of the log prior: PMD log 12 + log 12 + log 9 + log
 * (1/1000) (Beta(2,3) on q and A, Beta(1,9) on c, Exponential(rate 1/1000) on
 * delta), null log 12 + log(1/1000).  K_prop, those left out of the log
 * proposal density, with d free Student-t coordinates (nu = 4): lgamma((4 + d)
 * / 2) - lgamma(2) - (d / 2) log(4 pi) - sum over free j of [log scale_j + log
 * factor_jj], the log determinant of the map from the unit-scale t to u, plus
 * log rate of the exponential when c is held on 0; a refitted proposal brings
 * its own constant.  The prior is not renormalised for the region A + c >= 1 (a
 * draw there has weight 0): the evidence is that of the density the sampling
 * mode draws from.  khat says whether the estimate can be trusted, with the
 * threshold of flags bit 1: the estimate is a plain mean of the weights.  A
 * comparison of row 6 is NaN when a row it needs is invalid; a row's validity
 * is exactly mdfit_map_waic's; an invalid row has NaN statistics and only its
 * free bits in flags; a taxon with status != MDFIT_OK NaN statistics and flags
 * 0 in all seven rows.
 *   y, N, out, status : those of the MODE_MAP call (device; read only)
 *   num_draws  : S in [25, 1024] (else MDFIT_E_ARG, before any device call)
 *   seed, index_base : the Philox streams are keyed by (seed, index_base +
 *                taxon, sub-fit), as mdfit_map_psis's
 *   evid       : double[n_taxa][7][MDFIT_NMAPEVID]                 (device)
 *   draws      : double[n_taxa][6][num_draws][6], as mdfit_map_waic's, or NULL
 * khat, ess, n_infeasible, the valid / reliable / free bits of rows 0..5 and
 * draws are mdfit_map_waic's bit for bit for the same num_draws, seed and
 * index_base (rows 0, 2, 3 therefore mdfit_map_psis's).
 * One launch on hip_stream, one wave per taxon; no workspace, no allocation,
 * no side stream, no host synchronisation, no atomics; capturable in a graph.
 * The records do not depend on the grid, the chunking or index_base's split.
 * n_taxa: at most 2^25 per call.
 */
int mdfit_map_evidence(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                       int64_t n_taxa, int32_t num_draws, uint64_t seed, int64_t index_base,
                       double* evid, double* draws, void* hip_stream);

/*
 * mdfit_map_evidence with the rounds of mdfit_map_psis_adapt on its PMD rows
 * (0, 2, 3): khat, ess, n_infeasible, the valid / reliable / free / adapted
 * bits of rows 0..5, the adapt record and draws are mdfit_map_waic_adapt's bit
 * for bit for the same num_draws, adapt_rounds, seed and index_base (rows 0,
 * 2, 3 therefore mdfit_map_psis_adapt's); the evidence is that of the best
 * round's weights with that round's K_prop, and field 6 holds the best round.
 * The null rows (1, 4, 5) are not adapted.  With adapt_rounds = 0 evid and
 * draws are mdfit_map_evidence's bit for bit.
 *   adapt_rounds : R in [0, MDFIT_ADAPT_MAX_ROUNDS] (else MDFIT_E_ARG, before
 *                any device call)
 *   adapt      : double[n_taxa][3][MDFIT_NMAPADAPT] (rows PMD-all, PMD-forward,
 *                PMD-reverse), or NULL                              (device)
 * The other arguments, the launch and its guarantees are mdfit_map_evidence's.
 */
int mdfit_map_evidence_adapt(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                             int64_t n_taxa, int32_t num_draws, int32_t adapt_rounds, uint64_t seed,
                             int64_t index_base, double* evid, double* adapt, double* draws, void* hip_stream);

/*
 * Test helper: the log of the mean weight of mdfit_map_evidence (its device
 * functions) on given log-weight series lw[n_series][S], one wave per series,
 * as mdfit_psis_weights: logz[i] = c + log(tot / S), se[i] and khat[i]; NaN
 * where the smoothing refuses the series (a NaN or +inf, or an infeasible
 * cut-off draw).  S in [25, 1024] (else MDFIT_E_ARG); n_series at most 2^25.
 * Device pointers.
 */
int mdfit_log_mean_weight(const double* lw, int64_t n_series, int32_t S, double* logz, double* se,
                          double* khat, void* hip_stream);

/*
 * Test helper: the refit of one round of mdfit_map_psis_adapt (its device
 * function) on given series, one wave per series: from draws u[n_series][S][4]
 * = (logit q, logit A, c, log delta), normalised weights w[n_series][S] (a draw
 * of weight 0 takes no part and may hold anything), the free mask[i] (bit j:
 * coordinate j free), c_held[i] (non-zero: c is held on 0 and u[2] its
 * exponential draw) and the shift K[n_series][4], prop[n_series][25] = m[4],
 * d[4], F[4][4] (row-major, F[j][p], p >= j; a held coordinate: m = 0, d = 1,
 * the identity's row and column), the exponential's rate (0 with c free); and
 * ok[i] = 1, or 0 and NaN where the round stops.  S in [25, 1024] (else
 * MDFIT_E_ARG); n_series at most 2^25.  Device pointers.
 */
int mdfit_adapt_proposal(const double* u, const double* w, const int32_t* mask, const int32_t* c_held,
                         const double* K, int64_t n_series, int32_t S, double* prop, int32_t* ok,
                         void* hip_stream);

/* Importance-weighted posterior predictive record: double rec[T][MDFIT_NMAPPRED]:
 * D_max, D_max_lower_hpdi, D_max_upper_hpdi (job 0), D_max_forward (job 30),
 * D_max_reverse (job 31), khat of rows 0..2 (PMD-all, PMD-forward,
 * PMD-reverse), ess = 1 / sum w^2 of rows 0..2, n_distinct of rows 0..2 (the
 * importance draws the resampling took), the number of jobs made NaN by a
 * draw that is no count, flags (an integer stored as double: bit 0 all three
 * rows valid, bit 1 all valid and every khat <= min(1 - 1 / log10 S, 0.7),
 * bits 2..4 row 0..2 valid). */
#define MDFIT_NMAPPRED 16

/*
 * The reference's posterior predictive (fits.py:89-120) of a finished MODE_MAP
 * call from importance-weighted draws (MDFIT-PPRED v1).  Each
 * PMD row (stream sub-fit 0 / 2 / 3) is importance-sampled as mdfit_map_psis
 * does it: the same proposal, Philox stream, target, smoothing and validity
 * rule, so khat, ess and the valid / reliable bits are mdfit_map_psis's bit
 * for bit.  The smoothed weights w_s are resampled without a random number:
 * c_s = c_{s-1} + w_s in ascending s, p_r = (r + 0.5) c_{S-1} / R, s(r) the
 * least s with c_s > p_r (a draw of weight 0 is never taken).  Draw r of job j
 * of the sampler's 32 predictive jobs (jobs 0..29: row 0 at column j, N[j];
 * job 30: row 1 at column 0; job 31: row 2 at column 0 of data_forward, N[0])
 * is the sampler's predictive Beta-Binomial draw r (counter word 2 = 0xFFFD0000
 * + r, word 3 = column << 16 counting up) of the row's stream at theta = (q, A,
 * c, phi) of importance draw s(r); a job's summary is np.median and numpyro's
 * hpdi(0.68) of count / N.  N = 0, a draw that is no count in [0, N], or an
 * invalid row give NaN in the job; a taxon with status != MDFIT_OK NaN
 * everywhere and flags 0.
 *   y, N, out, status : those of the MODE_MAP call (device; read only)
 *   num_draws  : S in [25, 1024] (else MDFIT_E_ARG)
 *   num_pred   : R in [25, 1024] (else MDFIT_E_ARG); the reference draws 1000
 *   seed, index_base : the Philox streams are keyed by (seed, index_base +
 *                taxon, sub-fit), as mdfit_map_psis's and the sampler's
 *   ppred      : float[n_taxa][MDFIT_NPRED][30] = median, lower, upper of
 *                jobs 0..29, in pred's layout                       (device)
 *   rec        : double[n_taxa][MDFIT_NMAPPRED]                     (device)
 *   index      : int32[n_taxa][3][num_pred] = s(r) of each row, -1 in an
 *                invalid row or a taxon with status != MDFIT_OK; or NULL
 *                (parity tests)                                     (device)
 *   counts     : uint32[n_taxa][32][num_pred], the unsorted counts of each
 *                job, 0xFFFFFFFF for no count or a job not run; or NULL
 *                (parity tests)                                     (device)
 * One launch on hip_stream, one wave per taxon; no workspace, no allocation,
 * no side stream, no host synchronisation, no atomics; capturable in a graph.
 * n_taxa: at most 2^25 per call.
 */
int mdfit_map_pred(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                   int64_t n_taxa, int32_t num_draws, int32_t num_pred, uint64_t seed, int64_t index_base,
                   float* ppred, double* rec, int32_t* index, uint32_t* counts, void* hip_stream);

/*
 * mdfit_map_pred with the moment-matched proposal rounds of
 * mdfit_map_psis_adapt on each PMD row (MDFIT-AUTO v1.1): per
 * row, khat, ess and the valid / reliable bits of rec are mdfit_map_psis_adapt's
 * bit for bit for the same num_draws, adapt_rounds, seed and index_base, and so
 * is adapt; the resampling, the regenerated theta and the predictive draws are
 * those of the best round's proposal and weights.  flags of rec gains
 * MDFIT_FLAG_ADAPTED (64) when some valid row's best round is > 0.  With
 * adapt_rounds = 0, ppred, rec, index and counts are mdfit_map_pred's bit for
 * bit and adapt reads (khat, ess, 0, 0).
 *   adapt_rounds : R in [0, MDFIT_ADAPT_MAX_ROUNDS] (else MDFIT_E_ARG)
 *   adapt      : double[n_taxa][3][MDFIT_NMAPADAPT], or NULL       (device)
 * The other arguments, the launch and its guarantees are mdfit_map_pred's: one
 * wave per taxon, no workspace, no atomics, no side stream, capturable in a
 * graph; the records do not depend on the grid, the chunking or index_base's
 * split.
 */
int mdfit_map_pred_adapt(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                         int64_t n_taxa, int32_t num_draws, int32_t num_pred, int32_t adapt_rounds,
                         uint64_t seed, int64_t index_base, float* ppred, double* rec, double* adapt,
                         int32_t* index, uint32_t* counts, void* hip_stream);

/* Posterior predictive check record: double rec[T][MDFIT_NMAPPPC]: p_outlier,
 * p_strand, t_outlier, t_strand, worst_pos (column 0..29), p_worst, n_low,
 * n_points, khat, ess, n_distinct, flags (an integer stored as double: bit 0
 * valid, bit 1 khat <= min(1 - 1 / log10 S, 0.7), bit 3 some replicated draw
 * was no count, MDFIT_FLAG_ADAPTED as in the sibling records). */
#define MDFIT_NMAPPPC 12
#define MDFIT_PPC_VALID 1
#define MDFIT_PPC_RELIABLE 2
#define MDFIT_PPC_NONCOUNT 8

/*
 * Posterior predictive check of the PMD fit on all positions of a finished
 * MODE_MAP call (MDFIT-PPC v1).  Row 0 (stream sub-fit 0) is
 * importance-sampled and resampled exactly as mdfit_map_pred does it, so
 * khat, ess, n_distinct, index and the counts of jobs 0..29 are that entry's
 * row-0 bits at the same (seed, index_base + taxon, num_draws, num_pred).
 * Draw r holds the observed count y_i and the replicated count of every column
 * i with N_i > 0 against theta = (q, A, c, phi) of importance draw s(r): D =
 * clamp(A (1 - q)^k + c, 0, 1), mu = N D, v = N D (1 - D)(phi + N) / (phi + 1),
 * residual (count - mu) / sqrt(v), a column with v not > 0 skipped on both
 * sides.  T_out = max_i r_i^2 (0 without a column), T_str = sum_{i<15} r_i -
 * sum_{i>=15} r_i.  p_outlier = #{T_out(rep) >= T_out(obs)} / R, p_strand =
 * #{|T_str(rep)| >= |T_str(obs)|} / R (NaN when a strand has no column with
 * N > 0), t_outlier and t_strand the means over r of T_out(obs) and the signed
 * T_str(obs).  ppos[i] = (2 #{rep_i > y_i} + #{rep_i = y_i}) / (2 R), the upper
 * mid-p, NaN where N_i = 0; worst_pos the column with the smallest 2 min(p, 1 -
 * p) (the lowest index among equals), p_worst that value, n_low the number of
 * columns where it is < 0.05, n_points the number of columns with N > 0.  When
 * a replicated draw is no count in [0, N], bit 3 is set, bit 0 is clear and
 * p_outlier, p_strand, worst_pos, p_worst, n_low and ppos are NaN.  A row with
 * no valid proposal or no weights, or a taxon with status != MDFIT_OK, gives
 * NaN everywhere and flags 0.
 *   y, N, out, status : those of the MODE_MAP call (device; read only)
 *   num_draws  : S in [25, 1024] (else MDFIT_E_ARG)
 *   num_pred   : R in [25, 1024] (else MDFIT_E_ARG)
 *   seed, index_base : as mdfit_map_pred's
 *   ppos       : float[n_taxa][30]                                  (device)
 *   rec        : double[n_taxa][MDFIT_NMAPPPC]                      (device)
 *   index      : int32[n_taxa][num_pred] = s(r), -1 where the taxon has no
 *                weights; or NULL (parity tests)                    (device)
 *   counts     : uint32[n_taxa][30][num_pred], the replicated counts,
 *                0xFFFFFFFF for no count or a column not run; or NULL (device)
 *   disc       : double[n_taxa][num_pred][4] = T_out(obs), T_out(rep),
 *                T_str(obs), T_str(rep) of each draw, NaN where the taxon has
 *                no weights; or NULL (parity tests)                 (device)
 * One launch on hip_stream, one wave per taxon; no workspace, no allocation,
 * no side stream, no host synchronisation, no atomics; capturable in a graph.
 * Every count is an integer count, so the records do not depend on the grid,
 * the chunking or index_base's split.  n_taxa: at most 2^25 per call.
 */
int mdfit_map_ppc(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                  int64_t n_taxa, int32_t num_draws, int32_t num_pred, uint64_t seed, int64_t index_base,
                  float* ppos, double* rec, int32_t* index, uint32_t* counts, double* disc, void* hip_stream);

/*
 * mdfit_map_ppc with the moment-matched proposal rounds of mdfit_map_psis_adapt
 * on row 0 (as mdfit_map_pred_adapt): khat, ess, the flag bits and row 0 of
 * adapt are mdfit_map_pred_adapt's bit for bit; rows 1 and 2 of adapt, which
 * the check does not run, are NaN.  With adapt_rounds = 0 every output is
 * mdfit_map_ppc's bit for bit.
 *   adapt_rounds : in [0, MDFIT_ADAPT_MAX_ROUNDS] (else MDFIT_E_ARG)
 *   adapt      : double[n_taxa][3][MDFIT_NMAPADAPT], or NULL       (device)
 */
int mdfit_map_ppc_adapt(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                        int64_t n_taxa, int32_t num_draws, int32_t num_pred, int32_t adapt_rounds,
                        uint64_t seed, int64_t index_base, float* ppos, double* rec, double* adapt,
                        int32_t* index, uint32_t* counts, double* disc, void* hip_stream);

/* Weighted order statistics record: double quant[T][3][MDFIT_NMAPQUANT], rows
 * PMD-all, forward, reverse: D_max_median, D_max_lo, D_max_hi, D_max_q05,
 * D_max_q95, D_max_p_above, q_median, q_lo, q_hi, A_median, c_median,
 * phi_median, khat, ess, n_window (of D_max), flags (mdfit_map_psis's: an
 * integer stored as double, MDFIT_PSIS_* and MDFIT_FLAG_ADAPTED). */
#define MDFIT_NMAPQUANT 16

/*
 * The median, 68 % highest-posterior-density interval and quantiles of the
 * importance-weighted posterior of a finished MODE_MAP call (MDFIT-QUANT v1,
 * DESIGN.md §3.17).  Each PMD sub-fit is drawn, weighted and smoothed exactly
 * as mdfit_map_psis does it, so khat, ess and flags are that entry's bit for
 * bit at the same (seed, index_base + taxon, num_draws).  The smoothed weight
 * w_s of draw s becomes the integer mass k_s = rint(w_s 2^52), K = sum k_s;
 * a draw with k_s = 0 takes no part.  The draws are ordered ascending by
 * (value, draw index) and cum_j is the mass up to sorted draw j; every
 * comparison of masses is an integer comparison:
 *   median  : the mean of the first draw with 2 cum_j >= K and the first with
 *             2 cum_j > K
 *   q05, q95: the first draw with 100 cum_j >= 5 K, >= 95 K
 *   lo, hi  : over every first draw i, the window [i, j(i)] ending at the
 *             first j >= i with 100 (cum_j - cum_{i-1}) > 68 K; the narrowest
 *             window hi - lo, the lowest i among equals; n_window its draws
 *   p_above : sum of k_s over the draws with value > d0 (strictly), over K
 * With equal weights these are mdfit_nuts_summary's median and window of
 * int(0.68 S) + 1 sorted draws.  D_max = A + c gets all of them, q its median
 * and interval, A, c and phi their medians.  A row that mdfit_map_psis gives
 * as invalid is NaN with the free bits alone in flags; a taxon with status !=
 * MDFIT_OK is NaN with flags 0.
 *   y, N, out, status : those of the MODE_MAP call (device; read only)
 *   num_draws  : S in [25, 1024] (else MDFIT_E_ARG)
 *   seed, index_base : as mdfit_map_psis's
 *   d0         : the threshold of p_above; finite and in [0, 1] (else
 *                MDFIT_E_ARG)
 *   quant      : double[n_taxa][3][MDFIT_NMAPQUANT]                (device)
 *   values     : double[n_taxa][3][num_draws][6] = D_max, q, A, c, phi of draw
 *                s and its smoothed weight, NaN in an invalid row; or NULL
 *                (parity tests)                                    (device)
 * One launch on hip_stream, one wave per taxon; no workspace, no allocation,
 * no side stream, no host synchronisation, no atomics; capturable in a graph.
 * The records do not depend on the grid, the chunking or index_base's split.
 * n_taxa: at most 2^25 per call.
 */
int mdfit_map_quant(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                    int64_t n_taxa, int32_t num_draws, uint64_t seed, int64_t index_base, double d0,
                    double* quant, double* values, void* hip_stream);

/*
 * mdfit_map_quant with the moment-matched proposal rounds of
 * mdfit_map_psis_adapt: khat, ess, flags (MDFIT_FLAG_ADAPTED included) and
 * adapt are that entry's bit for bit, and the statistics are those of the best
 * round's draws and weights.  With adapt_rounds = 0 every output is
 * mdfit_map_quant's bit for bit.
 *   adapt_rounds : in [0, MDFIT_ADAPT_MAX_ROUNDS] (else MDFIT_E_ARG)
 *   adapt      : double[n_taxa][3][MDFIT_NMAPADAPT], or NULL       (device)
 */
int mdfit_map_quant_adapt(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                          int64_t n_taxa, int32_t num_draws, int32_t adapt_rounds, uint64_t seed,
                          int64_t index_base, double d0, double* quant, double* adapt, double* values,
                          void* hip_stream);

/* Test helper: the weighted order statistics of MDFIT-QUANT v1 on given
 * series v[n_series][S] and weights w[n_series][S] (each in [0, 1]), one wave
 * per series: res[n_series][8] = median, lo, hi, q05, q95, p_above, n_window,
 * ok (device pointers).  ok = 0 and NaN statistics when the masses sum to 0,
 * when a draw with mass is not finite, or when a weight is NaN or outside
 * [0, 1].  S in [25, 1024]; d0 finite and in [0, 1]. */
int mdfit_weighted_order_stats(const double* v, const double* w, int64_t n_series, int32_t S, double d0,
                               double* res, void* hip_stream);

/*
 * The WAIC comparison, the evidence and the posterior of a finished MODE_MAP
 * call from one launch.  Per sub-fit the proposal, draws,
 * raw log-weights and Pareto smoothing are formed once, as mdfit_map_waic forms
 * them, and the three records are taken from those weights by the row
 * functions of the three entries.  At equal num_draws, seed and index_base
 *   waic, pointwise and draws are mdfit_map_waic's,
 *   evid is mdfit_map_evidence's,
 *   psis is mdfit_map_psis's (rows PMD-all, PMD-forward, PMD-reverse from the
 *        sub-fits 0, 2 and 3)
 * bit for bit, NaN rows and flags included.
 *   y, N, out, status : those of the MODE_MAP call (device; read only)
 *   num_draws  : S in [25, 1024] (else MDFIT_E_ARG)
 *   waic       : double[n_taxa][7][MDFIT_NMAPWAIC]                 (device)
 *   evid       : double[n_taxa][7][MDFIT_NMAPEVID]                 (device)
 *   psis       : double[n_taxa][3][MDFIT_NMAPPSIS]                 (device)
 *   pointwise  : as mdfit_map_waic's, or NULL                      (device)
 *   draws      : as mdfit_map_waic's, or NULL                      (device)
 * One launch on hip_stream, one wave per taxon; no workspace, no allocation,
 * no side stream, no host synchronisation, no atomics; capturable in a graph.
 * n_taxa: at most 2^25 per call.
 */
int mdfit_map_joint(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                    int64_t n_taxa, int32_t num_draws, uint64_t seed, int64_t index_base, double* waic,
                    double* evid, double* psis, double* pointwise, double* draws, void* hip_stream);

/*
 * mdfit_map_joint with the rounds of mdfit_map_psis_adapt on the PMD rows: at
 * equal num_draws, adapt_rounds, seed and index_base waic, pointwise, draws and
 * adapt are mdfit_map_waic_adapt's, evid is mdfit_map_evidence_adapt's and psis
 * is mdfit_map_psis_adapt's bit for bit.  With adapt_rounds = 0 the records are
 * mdfit_map_joint's bit for bit.
 *   adapt_rounds : R in [0, MDFIT_ADAPT_MAX_ROUNDS] (else MDFIT_E_ARG)
 *   adapt      : double[n_taxa][3][MDFIT_NMAPADAPT], or NULL       (device)
 */
int mdfit_map_joint_adapt(const uint32_t* y, const uint32_t* N, const double* out, const int32_t* status,
                          int64_t n_taxa, int32_t num_draws, int32_t adapt_rounds, uint64_t seed,
                          int64_t index_base, double* waic, double* evid, double* psis, double* adapt,
                          double* pointwise, double* draws, void* hip_stream);

/* Test helper: mdfit_map_pred's resampling of given weights w[n_series][S]
 * (>= 0, not all 0), one wave per series: idx[n_series][R] = s(r) and
 * n_distinct[n_series] (device pointers).  S, R in [25, 1024]. */
int mdfit_resample(const double* w, int64_t n_series, int32_t S, int32_t R, int32_t* idx, int32_t* n_distinct,
                   void* hip_stream);

/*
 * Pointwise beta-binomial log-pmf (numpyro BetaBinomial.log_prob, used by
 * fits.py:59,67 and log_likelihood fits.py:126-133):
 *   out[i] = log C(N,y) + lnB(y+alpha, N-y+beta) - lnB(alpha, beta)
 * plus d/dalpha, d/dbeta (grad[i][2]).  Device pointers; for parity tests.
 * The value is computed in the cancellation-free form the record assembly
 * uses for its pointwise log-likelihoods (rising-factorial ratios).
 */
int mdfit_betabinom_logpmf(const double* y, const double* N, const double* alpha,
                           const double* beta, int64_t n, double* out,
                           double* grad, void* hip_stream);

/*
 * Device special functions on an array (parity tests): out[i] =
 * (lgamma(x), digamma(x), trigamma(x)) for x[i] > 0.  Device pointers.
 */
int mdfit_special(const double* x, int64_t n, double* out3, void* hip_stream);

/* The device primitives of csrc/mdfit_special.h that mdfit_primitive evaluates. */
enum mdfit_primitive_id {
  MDFIT_P_RCP = 1,           /* rcp(x): reciprocal, two Newton steps */
  MDFIT_P_RCP1 = 2,          /* rcp1(x): one Newton step */
  MDFIT_P_FLOG = 3,          /* flog(x) */
  MDFIT_P_FLOG_T = 4,        /* flog_t<false>(x): table log, normal x > 0 */
  MDFIT_P_FLOG_T_ZERO = 5,   /* flog_t<true>(x): also 0 and subnormals */
  MDFIT_P_FLOG1P = 6,        /* flog1p(x) */
  MDFIT_P_FEXP = 7,          /* fexp(x) */
  MDFIT_P_FEXP_T = 8,        /* fexp_t(x): table exp */
  MDFIT_P_LG3_L = 9,         /* lg3<true, false>(x).l: lnGamma, the accurate form */
  MDFIT_P_LG3_P = 10,        /* lg3<true, false>(x).p: digamma */
  MDFIT_P_LG3_Q = 11,        /* lg3<true, false>(x).q: trigamma */
  MDFIT_P_LG3_FAST_L = 12,   /* lg3<false, true>(x).l: the sampler's fast form */
  MDFIT_P_LG3_FAST_P = 13,   /* lg3<false, true>(x).p */
  MDFIT_P_STIRLING_REM = 14, /* stirling_rem(x), x >= 10 */
  MDFIT_P_LGDIFF = 15,       /* lgdiff(x, x2) = lnGamma(x + x2) - lnGamma(x) */
  MDFIT_P_LRISE = 16,        /* lrise(x, x2) = ln((x2)_x / x!) */
  MDFIT_P_COUNT = 17
};

/*
 * Test helper: out[i] = the device primitive `which` (enum mdfit_primitive_id)
 * at x[i], or at (x[i], x2[i]) for the two binary ones; one thread per element,
 * one launch on hip_stream.  Device pointers; x2 may be NULL for a unary
 * primitive.  which outside [1, MDFIT_P_COUNT), n < 0 or above 2^31, or a NULL
 * x / out (x2 for a binary primitive) with n > 0: MDFIT_E_ARG before any device call;
 * n == 0 returns 0.  tests/test_gpu_special.py holds every primitive to its
 * derived error bar with it.
 */
int mdfit_primitive(int32_t which, const double* x, const double* x2, int64_t n, double* out,
                    void* hip_stream);

/*
 * Test helper: fills every CU's LDS with NaN (one launch of blocks holding the
 * largest LDS a block may take, several per CU), so that a kernel launched after
 * it on the stream that reads LDS it did not write sees NaN there.  The library's
 * kernels never do; tests/test_gpu_paths.py checks that records are bit-identical
 * after a poisoning.
 */
int mdfit_poison_lds(void* hip_stream);

/*
 * MAP predictive HPDI (MDFIT-HPDI v2): the 68 % highest-
 * probability window [lo, hi] (integer counts, returned as double) of
 * BetaBinomial(alpha, beta, N), the population form of numpyro's
 * hpdi(obs/N, 0.68) over predictive draws (fits.py:112-120, 260-261).  The
 * fit's D_max_{lower,upper}_hpdi and the pred bounds are lo/N, hi/N at the
 * PMD-all mode.  Device pointers; N[i] = 0 -> NaN.  For parity tests.
 */
int mdfit_hpdi68(const double* N, const double* alpha, const double* beta, int64_t n, double* lo,
                 double* hi, void* hip_stream);

/*
 * Objective of one sub-fit at given unconstrained parameters, evaluated by
 * the fit kernel's own lane layout and code (parity tests).  Per item i:
 * model[i] (0 PMD, 1 null), subset[i] (0 all, 1 forward, 2 reverse),
 * y/N rows [n][MDFIT_LD], u[n][4] = (logit q, logit A, c, log delta) -- c on
 * its own scale (MDFIT-MAP v1; the sampler uses logit c).
 * Outputs F[n] = -(sum ell + log prior), g[n][4], H[n][4][4] (d/du),
 * ell[n][30] (pointwise log-lik without log C(N,y); 0 outside the subset).
 */
int mdfit_objective(const int32_t* model, const int32_t* subset, const uint32_t* y,
                    const uint32_t* N, const double* u, int64_t n, double* F, double* g,
                    double* H, double* ell, void* hip_stream);

/*
 * The same kernel layout and outputs with the point evaluation's other forms
 * (the ones the fit kernel takes by wave: tests/test_gpu_map_objective.py).
 * `form` is a sum of the bits below; each applies to the items whose layout has
 * it and leaves the others in the plain form.  g and H are the plain form's in
 * every form; so are F and ell without MDFIT_FORM_ACCF.  Unknown bits: an
 * argument error, nothing launched.
 */
#define MDFIT_FORM_ACCF 1       /* the polish phase's value term: F and ell are the full log-pmf
                                 * (ln C(N,y) included) in the cancellation-free form */
#define MDFIT_FORM_NULL_ROW 2   /* model_null items: lg3(a), lg3(b) from the row's pad lane */
#define MDFIT_FORM_WHOLE_PAIR 4 /* all-position items: lg3(a), lg3(b) shared by the lanes 16 apart */
int mdfit_objective_form(const int32_t* model, const int32_t* subset, const uint32_t* y,
                         const uint32_t* N, const double* u, int64_t n, int32_t form, double* F,
                         double* g, double* H, double* ell, void* hip_stream);

/*
 * Register-only throughput probe of the per-point evaluation the fit kernel
 * runs (value + gradient + Hessian of one beta-binomial point): launches
 * `n_waves` waves that each do `iters` evaluations; `sink` is a device
 * double[n_waves*64].  Used by bench.py for the compute roofline.
 */
int mdfit_peak_probe(int64_t n_waves, int32_t iters, double* sink, void* hip_stream);

/*
 * The same for the sampling mode: the chain kernel's potential evaluation
 * (value + gradient of 15 beta-binomial points per 16-lane chain slot, the
 * unconstrained transform, the row sums) at the chain kernel's occupancy;
 * 60 point-evaluations per wave-iteration.  bench.py's NUTS compute roofline.
 */
int mdfit_nuts_peak_probe(int64_t n_waves, int32_t iters, double* sink, void* hip_stream);

/*
 * Sampling-mode potential -(log density + log|J|) and its gradient in the
 * unconstrained v = (logit q, logit A, logit c, log delta) (numpyro's
 * potential of model_PMD / model_null, fits.py:43-67), evaluated by the chain
 * kernel's own lane layout and code (parity tests).  Per item i: model[i]
 * (0 PMD, 1 null), subset[i] (0 all, 1 forward, 2 reverse), y/N rows
 * [n][MDFIT_LD], v[n][4] -> U[n], g[n][4]; infeasible -> U = +inf, g = 0.
 */
int mdfit_nuts_potential(const int32_t* model, const int32_t* subset, const uint32_t* y,
                         const uint32_t* N, const double* v, int64_t n, double* U, double* g,
                         void* hip_stream);

/* Profiling hooks (bench / roofline): while enabled, every mdfit_fit_batch
 * records HIP events on its stream around the whole call and around the fit
 * kernel (up to 256 calls); on = 2 records only the two events around the fit
 * kernel (call_ms then reads -1).  mdfit_profile_read synchronises on them and
 * returns the summed milliseconds and the number of calls, then resets. */
int mdfit_profile_enable(int on);
int mdfit_profile_read(double* call_ms, double* fit_ms, int32_t* n_calls);

const char* mdfit_last_error(void);
int mdfit_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* MDFIT_H */
