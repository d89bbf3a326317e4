/*
 * dfm.h — C ABI of libdfm, the MI355X-native engine for the data-parallel core
 * of DynamicFactorModels.jl (joidegn/DynamicFactorModels.jl).
 *
 * The reference has no FFI: its boundary is the exported Julia API
 * (src/DynamicFactorModels.jl:16-20).  Each entry point below replaces the
 * reference function cited next to it; the Julia `ccall` shim and the Python
 * ctypes mirror that bind them are shown in INTEGRATION.md.
 *
 * Conventions
 *   - Return codes: 0 ok; <0 invalid argument / shape; >0 HIP or numerical
 *     error (singular design, eigensolver not converged).  No exception,
 *     abort or exit crosses the ABI; dfm_last_error() has the message.
 *   - Host arrays are caller-owned; the library copies in/out and never
 *     retains host pointers.  Matrices passed from the host are COLUMN-major
 *     (Julia) with a leading dimension; vectors are contiguous.
 *   - *_dev entry points take DEVICE pointers on the context's device and run
 *     on the context's stream (dfm_ctx_set_stream lets the caller supply its
 *     own, e.g. PyTorch's current stream).  They never synchronise the host
 *     except where a convergence poll needs a 4-byte read-back.
 *   - Indices are 0-based int32 (the Julia shim subtracts 1).
 *   - One context per GPU, used by one host thread at a time.  Different
 *     contexts (of one device or several) may be used from different threads
 *     at once, except that the lasso path (dfm_targeted_soft, dfm_lasso_path)
 *     runs alone on its device: it waits for every other libdfm call on that
 *     device to return, drains the device, and holds new calls off until it
 *     is done (its grid must own every CU).  Called from inside another
 *     libdfm call on the same device it fails instead of waiting.
 */
#ifndef DFM_H
#define DFM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct dfm_ctx dfm_ctx;
typedef struct dfm_model dfm_model; /* a fitted base model resident in HBM */

/* Information criteria, src/criteria.jl:17-53 (name-based dispatch at
 * src/DynamicFactorModel.jl:138 becomes this code). */
enum dfm_criterion {
  DFM_CRIT_NONE = -1,
  DFM_CRIT_PCP1 = 0, DFM_CRIT_PCP2 = 1, DFM_CRIT_PCP3 = 2,
  DFM_CRIT_ICP1 = 3, DFM_CRIT_ICP2 = 4, DFM_CRIT_ICP3 = 5,
  DFM_CRIT_BIC = 6
};

/* Replicate statistics.  The reference's `stat::Function` callback
 * (src/bootstrap.jl:21, :41) cannot run on the device, so it is this fixed
 * menu.  Each dfm_stat yields ONE double per replicate, except the *_ALL
 * kinds (N doubles, one per variable), FACTORS (T r) and LOADINGS (N r):
 * with those (plus COEF/TSTAT/EIGVAL) a host binding rebuilds each
 * replicate's fit and runs an arbitrary closure on it. */
enum dfm_stat_kind {
  DFM_STAT_V = 0,          /* factor_residual_variance, src/criteria.jl:5       */
  DFM_STAT_CRIT = 1,       /* criterion value (arg0 = dfm_criterion code)       */
  DFM_STAT_EIGVAL = 2,     /* eigenvalue arg0 (0-based, descending)             */
  DFM_STAT_COEF = 3,       /* OLS coefficient arg0, src/DynamicFactorModel.jl:41 */
  DFM_STAT_TSTAT = 4,      /* HC2 t-stat arg0, src/DynamicFactorModel.jl:48     */
  DFM_STAT_TRACE = 5,      /* trace of the Gram (= ||X*||_F^2)                  */
  DFM_STAT_LR = 6,         /* LR_test(dfm, bp=arg0, i=arg1), src/chowtest.jl:19 */
  DFM_STAT_LM = 7,         /* LM_test, src/chowtest.jl:35                       */
  DFM_STAT_WALD = 8,       /* Wald_test, src/chowtest.jl:25                     */
  DFM_STAT_LR_ALL = 9,     /* LR for every variable i (N values), bp = arg0     */
  DFM_STAT_LM_ALL = 10,
  DFM_STAT_WALD_ALL = 11,
  DFM_STAT_ITERS = 12,     /* diagnostic: Rayleigh-Ritz steps of the replicate's eigensolve
                              (NaN on the dense path); an eigenvalue-only stat */
  DFM_STAT_FACTORS = 13,   /* the replicate's factors vcat(F_j) (T x r row-major: T r values),
                              src/DynamicFactorModel.jl:18, :131 — the fields a host-side
                              stat::Function closure reads (src/bootstrap.jl:21, :41) */
  DFM_STAT_LOADINGS = 14,  /* break block arg0's loadings L_j (N x r row-major: N r values), :19 */
  DFM_STAT_SUPLR_ALL = 15, /* max over bp = arg0..arg1 (inclusive) of LR for every variable (N   */
  DFM_STAT_SUPLM_ALL = 16, /* values): the sup-Chow statistics of an unknown break date          */
  DFM_STAT_SUPWALD_ALL = 17 /* (dfm_chow_sweep).  All sup stats of a call share one range        */
};
typedef struct dfm_stat { int32_t kind, arg0, arg1, pad; } dfm_stat;

enum dfm_boot_kind { DFM_BOOT_WILD = 0, DFM_BOOT_RESIDUAL = 1 };
enum dfm_tp_mode { DFM_TP_JOINT = 0, DFM_TP_PER_CANDIDATE = 1 };

/* ---------------------------------------------------------------- context */
int dfm_ctx_create(int device, dfm_ctx **out);
int dfm_ctx_destroy(dfm_ctx *ctx);
const char *dfm_last_error(const dfm_ctx *ctx);
int dfm_ctx_set_stream(dfm_ctx *ctx, void *hip_stream); /* NULL = own stream */
int dfm_ctx_synchronize(dfm_ctx *ctx);
/* Eigensolver controls: relative residual tolerance (default 1e-12), maximum
 * subspace iterations (default 400), block width (0 = auto; a block below
 * r + 1 is raised to r + 1: the filtered subspace iteration needs a guard
 * vector beyond the r wanted ones). */
int dfm_ctx_set_eig_params(dfm_ctx *ctx, double tol, int max_iter, int block);
/* Per-kernel HIP-event timing on the context stream (bench/roofline use). */
/* Bootstrap calls whose statistics are all eigenvalue functions (V, CRIT,
   EIGVAL, TRACE) stop the eigensolver when every returned eigenvalue and the
   residual energy trace - sum(theta) are within `tol` relative by the
   Kato-Temple bound (default 1e-12); tol <= 0 always uses the eigenvector
   residual rule of dfm_ctx_set_eig_params. */
int dfm_ctx_set_value_tol(dfm_ctx *ctx, double tol);
int dfm_ctx_enable_timing(dfm_ctx *ctx, int enable);
/* ms accumulated per kernel class (see DFM_KCLASS_* in the implementation);
 * returns the number of classes written into ms_out/launches_out. */
int dfm_ctx_read_timing(dfm_ctx *ctx, double *ms_out, int64_t *launches_out, int cap);
int dfm_ctx_reset_timing(dfm_ctx *ctx);
/* Eigensolver statistics since the last reset: batches solved, total and
 * maximum subspace iterations per batch. */
int dfm_ctx_eig_stats(dfm_ctx *ctx, int64_t *batches, int64_t *iters_total, int64_t *iters_max);
/* Replicate-iterations of the eigensolver's dominant product (the H.Z GEMM in
   the factored bootstrap, G.Q otherwise) summed over the calls since the last
   dfm_ctx_reset_timing: each counts one unconverged replicate in one
   iteration (2 m^2 P flop).  Instrumentation for the roofline figure. */
/* Replicate-products H . Z run by the factored bootstrap's GEMMs since the
 * last reset (two per Rayleigh-Ritz iteration with the Chebyshev filter):
 * the GEMM's algorithmic work is 2 T^2 p per product. */
int dfm_ctx_gemm_products(dfm_ctx *ctx, int64_t *products);
/* Of those replicate-products, the ones run in fp32: the middle products of a
 * warm eigenvalue-rule solve's filter-only first step ((d0 - 1) nb per solve;
 * 0 under the strict rule or with DFM_FACT_F32=0). */
int dfm_ctx_gemm_products_f32(dfm_ctx *ctx, int64_t *products);
/* The last products of those filters run as six bf16 terms with an fp64 store
 * (nb per such solve; 0 under the strict rule, with DFM_FACT_F32=0,
 * DFM_FACT_SPLIT=0 or DFM_FACT_SPLIT_LAST=0).  Not part of the fp32 count. */
int dfm_ctx_gemm_products_split_last(dfm_ctx *ctx, int64_t *products);
/* Of the gemm_products_f32 products, those run as three bf16 terms on two
 * planes: the split products two or more short of the filter's last
 * ((d0 - 2) nb per such solve; 0 with DFM_FACT_SPLIT3=0, DFM_FACT_SPLIT=0 or
 * DFM_FACT_F32=0, or under the strict rule). */
int dfm_ctx_gemm_products_split3(dfm_ctx *ctx, int64_t *products);
int dfm_ctx_rep_iters(dfm_ctx *ctx, int64_t *rep_iters);
const char *dfm_kernel_class_name(int cls);

/* ------------------------------------------------ principal components
 * principal_components (src/DynamicFactorModel.jl:75-95), no breaks:
 *   T >= N: G = X'X, L = sqrt(N) V, F = X L / N
 *   N >  T: G = XX', F = sqrt(T) U, L = X' F / T
 * Top-k eigenpairs only (the reference consumes [:,1:r]; :33, :131).
 * X column-major T x N (ldx >= T).  Outputs: eigvals[k] descending,
 * F (T x k, col-major, ld T), L (N x k, col-major, ld N), trace_G (may be NULL).
 * Eigenvectors are sign-canonicalised (largest-|.| entry positive). */
int dfm_pca(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx,
            int k, double *eigvals, double *F, double *L, double *trace_G);

/* Full spectrum of the Gram (eigenvalues only, descending) for
 * min(T,N) <= dfm_full_spectrum_max(); used by PCp's unrestricted sigma^2
 * (src/criteria.jl:18) and full IC sweeps. */
int dfm_full_spectrum_max(void);
int dfm_gram_spectrum(dfm_ctx *ctx, const double *X, int64_t T, int64_t N,
                      int64_t ldx, double *eigvals_m, double *trace_G);

/* normalize (src/utils.jl:33): out = (X .- mean(X, 1)) ./ std(X, 1), the
 * column z-score with the sample (n - 1) std.  X and out column-major T x N
 * (ldx, ldo >= T); out may alias X.  dfm_normalize_dev: both on the device,
 * asynchronous on the context stream. */
int dfm_normalize(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, double *out, int64_t ldo);
int dfm_normalize_dev(dfm_ctx *ctx, const double *X_dev, int64_t T, int64_t N, int64_t ldx, double *out_dev,
                      int64_t ldo);

/* ----------------------------------------------------- IC sweep (host math)
 * Criteria for k = 1..kmax from the eigenvalues (identity ||E_k||_F^2 =
 * trace(G) - sum_{j<=k} lambda_j).  sigma2 < 0 means "compute
 * V(ceil(m/2)) from eigvals" (needs ceil(m/2) eigenvalues).  crit_out is
 * 7 x kmax row-major in dfm_criterion order.  Pure arithmetic; no device. */
int dfm_ic_sweep(const double *eigvals, int n_eig, int kmax, double trace_G,
                 int64_t T, int64_t N, double sigma2, double *crit_out);

/* ------------------------------------------------------------ model fit
 * Workhorse constructor (src/DynamicFactorModel.jl:28-51) at fixed r, and
 * the IC-sweep constructor (:53-66) when r <= 0: r is then chosen by
 * criterion `crit` over k = 1..kmax (kmax <= 0 -> ceil(m/2), defect D11).
 * y (T), w (T x q col-major, ldw >= T), X (T x N col-major).  The fitted
 * model (factors, loadings, common component, factor residuals) stays in HBM
 * for the bootstrap and Chow entry points. */
int dfm_model_fit(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw,
                  const double *X, int64_t T, int64_t N, int64_t ldx,
                  int r, int crit, int kmax, dfm_model **out);
/* The same with structural breaks (src/DynamicFactorModel.jl:73, :98): the
 * rows split into blocks at `breaks` (0-based first rows of blocks 2..nbreaks+1,
 * strictly increasing inside 1..T-1 — the reference's 1-based break_indices
 * minus 1).  Each block gets its own principal components with the FULL-sample
 * T, N for branch choice and scaling (:72, defect D7); E = X - vcat(F_j L_j')
 * (:33); the design matrix stacks the blocks' factors (:131).  The IC sweep
 * reads V(k) = (sum_j trace G_j - sum_j sum_{i<=k} lambda_{j,i}) / (N T); PCp's
 * sigma^2 is the no-break unrestricted fit (src/criteria.jl:18).  A block needs
 * at least r (sweep: kmax) eigenpairs: -9 otherwise (the reference's
 * F_j[:, 1:r] would raise).  Reported eigenvalue i is sum_j lambda_{j,i};
 * per-block values and loadings via dfm_model_block.  nbreaks = 0 is
 * dfm_model_fit. */
int dfm_model_fit_breaks(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw,
                         const double *X, int64_t T, int64_t N, int64_t ldx, int r, int crit,
                         int kmax, const int64_t *breaks, int nbreaks, dfm_model **out);
int dfm_model_destroy(dfm_model *m);
/* Number of break blocks (1 without breaks), and block j's first row, rows,
 * top-r eigenvalues (r) and loadings L_j (N x r col-major); NULL skips. */
int dfm_model_blocks(const dfm_model *m);
int dfm_model_block(const dfm_model *m, int j, int64_t *row0, int64_t *rows, double *eigvals,
                    double *L);
/* Sizes of the arrays dfm_model_read fills: r, the IC-sweep kmax (0 when r was
 * given), n_eig = number of eigenvalues returned (max(r, kmax)). */
int dfm_model_dims(const dfm_model *m, int64_t *r, int64_t *kmax, int64_t *n_eig);
/* Scalars: [r, V(r), criterion value, trace_G]. */
int dfm_model_scalars(const dfm_model *m, int64_t *r_out, double *V, double *crit_value,
                      double *trace_G);
/* Host copies (any pointer may be NULL): eigvals (kmax), coefficients and
 * t-stats (q+r), coefficient covariance ((q+r)^2 col-major), OLS residuals
 * (T), F (T x r col-major), L (N x r col-major), factor residuals E (T x N
 * col-major, ld T), criteria for k=1..kmax (7 x kmax, row-major) when the IC
 * sweep ran.  eigvals holds n_eig values (dfm_model_dims). */
int dfm_model_read(const dfm_model *m, double *eigvals, double *coef, double *tstat,
                   double *coef_cov, double *ols_resid, double *F, double *L,
                   double *E, double *ic_values);

/* get_factors (src/DynamicFactorModel.jl:125-128) and predict (:152-155) of a
 * fitted model on n_new new rows, defect D4 repaired: rotation = L (L'L)^-1 of
 * the first break block's loadings (D1), first r columns ("active"); the new
 * rows normalised by the scalar mean and sample std of all T N entries of the
 * fitted x (:127).  x_new: n_new x N column-major (ldx >= n_new), w_new: n_new x q
 * column-major (ldw >= n_new; unused when q = 0); host or device memory.
 * F_out: n_new x r column-major (host); out: n_new predictions (host). */
int dfm_get_factors(dfm_model *m, int64_t n_new, const double *x_new, int64_t ldx, double *F_out);
int dfm_predict(dfm_model *m, int64_t n_new, const double *w_new, int64_t ldw, const double *x_new, int64_t ldx,
                double *out);

/* ------------------------------------------------------------- bootstrap
 * wild_bootstrap (src/bootstrap.jl:41-51) / residual_bootstrap (:21-39):
 * for b < B: X*_b = F_r L_r' + diag(eta_b) E[idx_b, :]  (eta == NULL for
 * RESIDUAL), refit at the model's r and criterion, emit the stats.  A model
 * fitted with breaks refits per break block (:36, :48 pass break_indices);
 * the common component is the blockwise vcat(F_j L_j'); the residual
 * bootstrap's block-wise draws (:23-28) are the caller's idx.  Chow stats of
 * such models read F = vcat(F_j) and the blockwise factor residuals (D1).
 * idx: B x T int32 (row-major, 0-based), eta: B x T.  out: B rows of
 * sum(width(stat)) doubles (row-major). */
int dfm_bootstrap(dfm_model *m, int kind, int64_t B, const int32_t *idx,
                  const double *eta, const dfm_stat *stats, int nstats, double *out);
/* Same, all pointers on the device (inputs resident in HBM). */
int dfm_bootstrap_dev(dfm_model *m, int kind, int64_t B, const int32_t *idx_dev,
                      const double *eta_dev, const dfm_stat *stats, int nstats,
                      double *out_dev);
/* The replicate loop (src/bootstrap.jl:43) sharded over n models, one per
 * context (typically one per GPU; contexts must be distinct), each a
 * dfm_model_clone of the same fit: replicate b runs on model floor(b n / B)
 * (contiguous shards), every shard on its own host thread and stream, rows
 * written in order into the caller's out (B x width, host).  Same arguments and
 * results as dfm_bootstrap: rows are bit-identical to a one-model call. */
int dfm_bootstrap_multi(dfm_model *const *models, int n, int kind, int64_t B, const int32_t *idx,
                        const double *eta, const dfm_stat *stats, int nstats, double *out);
/* Copy of a fitted model on another context (device buffers and host fields),
 * for dfm_bootstrap_multi.  Destroy it with dfm_model_destroy. */
int dfm_model_clone(const dfm_model *m, dfm_ctx *ctx, dfm_model **out);
/* Width of one replicate's output row for a stat list. */
int64_t dfm_stats_width(const dfm_model *m, const dfm_stat *stats, int nstats);
/* Replicates per device batch (0 = auto). */
int dfm_model_set_batch(dfm_model *m, int64_t batch);
/* Bootstrap algorithm for N > T panels: 0 auto (= factored), 1 direct (per-
 * replicate fused-gather Gram + eigensolver on it), 2 factored (the replicate
 * Gram is never formed: every eigen-iteration is one MFMA GEMM of the shared
 * H = E E' against the batch's iterates).  Results agree to rounding. */
int dfm_model_set_mode(dfm_model *m, int mode);
/* Block of the factored bootstrap solver for this model: p eigen-iterate
 * columns per replicate, pz = p rounded up to even = the columns each
 * replicate contributes to the batched H.Z GEMM (its flop per
 * replicate-product is 2 T^2 pz).  Returns 0, or 1 (p = pz = 0) when the
 * model's bootstrap never takes the factored path (T >= N, breaks, r > 16).
 * The answer ignores the statistics of a particular call: a stat list with a
 * PCp criterion (which reads each replicate's full spectrum) or mode 1 sends
 * that call down the direct path even when this returns 0. */
int dfm_model_fact_block(const dfm_model *m, int *p, int *pz);

/* ------------------------------------------------------------ Chow tests
 * LR_test / LM_test / Wald_test (src/chowtest.jl:19-42) for EVERY variable
 * i = 0..N-1 of the fitted model at break period bp (rows 0..bp-1 | bp..T-1).
 * Any output pointer may be NULL. */
int dfm_chow_all(dfm_model *m, int64_t bp, double *LR, double *LM, double *Wald);

/* One variable's LR_test / LM_test / Wald_test (src/chowtest.jl:19-42), i
 * 0-based.  The model keeps the all-variables results of the last break
 * period asked for, so a loop over i = 0..N-1 costs one dfm_chow_all. */
int dfm_chow(dfm_model *m, int64_t bp, int64_t i, double *LR, double *LM, double *Wald);

/* LR/LM/Wald (src/chowtest.jl:19-42) of every variable at every break period
 * bp_lo..bp_hi (inclusive; each within dfm_chow_all's bounds r..T-r).
 * curves: LR/LM/Wald, (bp_hi-bp_lo+1) x N row-major; sup: 3 x N (LR, LM, Wald);
 * argsup: 3 x N break periods (0-based, the first maximum on ties).  Any
 * pointer may be NULL; a statistic none of whose outputs is wanted is not
 * computed.  `stats` selects what sup / argsup hold: a bit mask of 1 (LR),
 * 2 (LM), 4 (Wald), 0 meaning all three; a statistic with its curve pointer
 * set is computed whatever the mask.  Rows of sup / argsup of a statistic that
 * was not computed are NaN / -1.  One device pass: the sup-LM alone costs no
 * Wald work.  Models with r <= 16 fitted without breaks; -7 otherwise and for
 * a bad range. */
int dfm_chow_sweep(dfm_model *m, int64_t bp_lo, int64_t bp_hi, int stats, double *LR, double *LM,
                   double *Wald, double *sup, int64_t *argsup);

/* criterion_<name>(dfm) (src/criteria.jl:17-53) of a fitted model at its r,
 * for any criterion code (not only the one it was fitted with).  PCp's sigma^2
 * = V(ceil(m/2)) of the unrestricted fit DynamicFactorModel(y, w, x)
 * (:18, :23, :28) comes from the resident panel's full spectrum (min(T,N) <=
 * dfm_full_spectrum_max()), computed once per model. */
int dfm_model_criterion(dfm_model *m, int crit, double *value);

/* ---------------------------------------------------- expanding windows
 * The refits of pseudo_out_of_sample_forecasts (src/utils.jl:54-72): window
 * w = 0..P-1 refits the IC-sweep constructor (src/DynamicFactorModel.jl:53)
 * on rows 0..T-P+w-1 with criterion crit (any of the 7) over k = 1..kmax_w,
 * kmax_w = ceil(min(T-P+w, N)/2) (the constructor's default, :54), capped by
 * kmax when kmax > 0 (D11).  N > T uses the prefix-Gram identity (one Gram for
 * all windows).  Outputs per window: r (P), V(r) (P), criterion value (P),
 * eigenvalues (P x K, row-major), OLS coefficients and HC2 t-stats
 * (P x (q + K), row-major, NaN past q + r), K = kmax_{P-1} =
 * min(kmax, ceil(min(T-1, N)/2)) (kmax <= 0: no cap).  The forecast step:
 * dfm_windows_forecast. */
int dfm_windows(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw,
                const double *X, int64_t T, int64_t N, int64_t ldx, int P, int crit,
                int kmax, int64_t *r_out, double *V_out, double *crit_out, double *eig_out,
                double *coef_out, double *tstat_out);

/* pseudo_out_of_sample_forecasts (src/utils.jl:54-72) in full: the refits of
 * dfm_windows, then window w predicts row n = T-P+w from its own fit:
 * predict (src/DynamicFactorModel.jl:152-155) with get_factors repaired
 * (defect D4: rotation = L (L'L)^-1 of :126, L = the window's loadings; the
 * new row normalised by the scalar mean / sample std of the window's X).
 * Outputs per window: r (P), prediction (P), true value y[n] (P). */
int dfm_windows_forecast(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw,
                         const double *X, int64_t T, int64_t N, int64_t ldx, int P, int crit,
                         int kmax, int64_t *r_out, double *pred_out, double *true_out);
/* dfm_windows with the inputs already resident in HBM (y_dev: T, w_dev: ldw x q
 * column-major, X_dev: column-major T x N with leading dimension ldx, all on the
 * context's device); outputs as dfm_windows, in host memory (a few hundred
 * bytes per window).  A multi-GPU caller shards the windows by truncating the
 * panel: windows [w0, w1) of (T, P) are windows 0..w1-w0-1 of the leading
 * T - P + w1 rows with P' = w1 - w0 (window w only reads rows < T - P + w). */
int dfm_windows_dev(dfm_ctx *ctx, const double *y_dev, const double *w_dev, int q, int64_t ldw,
                    const double *X_dev, int64_t T, int64_t N, int64_t ldx, int P, int crit,
                    int kmax, int64_t *r_out, double *V_out, double *crit_out, double *eig_out,
                    double *coef_out, double *tstat_out);

/* pseudo_out_of_sample_forecasts(model, y, w, x, model_args...) (src/utils.jl:54-72)
 * for every model_args form of the DynamicFactorModel constructors, and rolling
 * windows (BASELINE configs[4]: "rolling-window factor re-estimation").
 *   kind DFM_WIN_EXPANDING: window w = rows 0 .. T-P+w-1 (the reference's loop);
 *   kind DFM_WIN_ROLLING:   window w = the `length` rows T-P+w-length .. T-P+w-1.
 *   r > 0:  the workhorse constructor at fixed r (src/DynamicFactorModel.jl:28),
 *           r_w = min(r, ceil(m_w/2)) (:116-119), criterion value of crit at r_w
 *           (crit = DFM_CRIT_NONE: NaN, D3);
 *   r == 0: the IC-sweep constructor (:53-66) by crit over k = 1..kmax_w (as dfm_windows);
 *   r < 0:  the 3-arg constructor's default r_w = ceil(m_w/2) (D2).
 *   breaks (nbreaks > 0, expanding windows only): model_args' break_indices
 *           (0-based first rows of blocks 2..; all inside the first window), the
 *           same rows in every refit; each window is then a break-aware fit
 *           (dfm_model_fit_breaks on its rows, D7) and forecasts through dfm_predict.
 * dev != 0: y, w, X are device pointers (as dfm_windows_dev).  Outputs as
 * dfm_windows with K = the widest window's r_w bound; pred_out / true_out (P
 * each, both or neither) add the forecast step (as dfm_windows_forecast). */
enum dfm_window_kind { DFM_WIN_EXPANDING = 0, DFM_WIN_ROLLING = 1 };
typedef struct dfm_window_spec {
  int32_t kind, length, r, crit, kmax, nbreaks;
  const int64_t *breaks;
} dfm_window_spec;
int dfm_windows_ex(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw,
                   const double *X, int64_t T, int64_t N, int64_t ldx, int P,
                   const dfm_window_spec *spec, int dev, int64_t *r_out, double *V_out,
                   double *crit_out, double *eig_out, double *coef_out, double *tstat_out,
                   double *pred_out, double *true_out);

/* --------------------------------------------------- Monte-Carlo batches
 * M independent panels of one shape fitted and tested in one pass: the loop of
 * the reference's driver script (src/Bai_Ng.jl:12-39: per (T, N, r) tuple and
 * repetition factor_model_DGP -> normalize -> the IC-sweep constructor ->
 * number_of_factors) and of the size / power tables of the Chow tests.  Per
 * panel: the z-score (optional), the Gram, its spectrum, the seven criteria
 * for k = 1..kmax with their first arg-mins, and — when statistics are asked
 * for — the principal-components fit at the panel's r with the statistics of
 * the dfm_bootstrap menu that need no y / w.  No OLS is run.
 *
 * Statistics (meaning and 0-based arguments as in dfm_bootstrap): V,
 * CRIT(code; < 0: spec->crit), EIGVAL(j), TRACE, LR / LM / WALD(bp, i),
 * LR_ALL / LM_ALL / WALD_ALL(bp) (one bp per call), SUPLR_ALL / SUPLM_ALL /
 * SUPWALD_ALL(lo, hi) (one range per call).  COEF, TSTAT, ITERS, FACTORS and
 * LOADINGS return -6.  With r == 0 EIGVAL(j) of a panel whose r^ <= j is NaN.
 *
 * Checked before any device work: break periods and sup ranges against
 * dfm_chow_all's bounds rmax..T-rmax for the largest r a panel can get
 * (rmax = r, or kmax when r == 0): -7; a fixed r above the fit stage's limit
 * (32; 16 with a sup statistic) with statistics asked for: -7; min(T, N) <=
 * dfm_full_spectrum_max(): -31.  After the sweep: a panel whose r^ exceeds
 * that limit while statistics are asked for fails the call with -7 (the
 * message names the panel).  M == 0 is a no-op. */
typedef struct dfm_mc_spec {
  int32_t r;         /* > 0: every panel is fitted at r (clamped to ceil(m/2), :116-119);
                        0: each panel at its own r^ = first arg-min of `crit` over k = 1..kmax */
  int32_t crit;      /* dfm_criterion: selects r^ when r == 0; DFM_STAT_CRIT's default code */
  int32_t kmax;      /* sweep bound; <= 0: ceil(min(T,N)/2) (D11); larger values are cut to that */
  int32_t normalize; /* != 0: z-score every panel's columns first (src/utils.jl:33, Bai_Ng.jl:23) */
  int32_t batch;     /* panels per device pass; 0 = auto (bounded workspace) */
  int32_t dev;       /* != 0: X is a device pointer on the context's device */
} dfm_mc_spec;

/* X: M panels, panel b column-major T x N at X + b*stride (ldx >= T, stride >= ldx*N).
 * r_hat: M x 7 (r^ by each criterion, dfm_criterion order); ic: M x 7 x kmax;
 * eig: M x kmax (descending); out: M rows of dfm_mc_stats_width doubles.
 * (kmax: the effective bound, min(spec->kmax or ceil(m/2), ceil(m/2)).)
 * All outputs are host memory, all are optional (NULL skips), rows are in panel order. */
int dfm_mc(dfm_ctx *ctx, const double *X, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
           const dfm_mc_spec *spec, const dfm_stat *stats, int nstats,
           int64_t *r_hat, double *ic, double *eig, double *out);
/* Width of one panel's output row; < 0 for a statistic dfm_mc does not serve.  Pure arithmetic. */
int64_t dfm_mc_stats_width(int64_t N, const dfm_stat *stats, int nstats);

/* ------------------------------------- missing observations (EM, dfm_em.hip)
 * Principal components of a panel with missing entries (NaN) by the EM
 * iteration of Stock & Watson (2002) as McCracken & Ng (2016) run it for
 * FRED-MD (factors_em, DEMEAN = 2), obs = !isnan(X):
 *   X2 = X, missing := the mean of the column's observed entries
 *   (mu, sd) = column mean and sample (n-1) std of X2;  Z = (X2 - mu) / sd
 *   r fixed, or the first arg-min of `crit` over k = 1..kmax on Z
 *   (F, L) = principal_components(Z)[:, 1:r];  C = F L'
 *   it = 0; err = +inf
 *   while err > tol and it < max_iter:
 *     it += 1;  X2 = obs ? X : C * sd + mu  (the mu, sd that produced C)
 *     (mu, sd), Z from the new X2;  r re-selected when it is not fixed
 *     (F, L) again;  Cnew = F L';  err = ||Cnew - C||_F^2 / ||C||_F^2;  C = Cnew
 *   converged = (err <= tol)
 * The loop runs on the device; per iteration only the two sums, two flags and
 * (when r is selected) kmax eigenvalues and the trace reach the host.  The PCA
 * is the library's own (X'X for T >= N, XX' for N > T), warm-started from the
 * previous iteration.  A row with no observed entry is legal.
 *
 * Return codes: -8 a column with fewer than 2 observed entries, or a zero std
 * of a column when standardising (the message names the column, 0-based);
 * -3 selecting r by a PCp criterion (it needs the full spectrum in every
 * iteration: use ICp1-3 or BIC) or without one; -7 kmax / r beyond the
 * eigensolver's subspace block; -2 NaN in y or w (dfm_model_fit_em).  Reaching
 * max_iter is not an error: converged = 0 says so. */
typedef struct dfm_em_spec {
  int32_t r;            /* > 0 fixed; 0: re-selected every iteration by crit over 1..kmax */
  int32_t crit, kmax;   /* as dfm_model_fit; kmax <= 0 -> min(ceil(m/2), solver limit) */
  int32_t standardize;  /* 1 (default): z-score every iteration; 0: panel as given */
  int32_t max_iter;     /* <= 0 -> 50 */
  int32_t dev;          /* != 0: X is a device pointer */
  double  tol;          /* < 0 -> 1e-6; 0 runs exactly max_iter iterations */
} dfm_em_spec;
typedef struct dfm_em_info { int32_t iterations, converged, r, pad; double err; int64_t n_missing; } dfm_em_info;

/* X column-major T x N (ldx >= T).  Outputs host, column-major, any may be NULL:
 * Z (T x N standardised completed panel), X2 (T x N completed, original units),
 * mu (N), sd (N), F (T x r), L (N x r), eigvals (r) — r = info->r; size F, L
 * and eigvals for spec->r, or for kmax (at most 32) when r is selected. */
int dfm_em(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *spec,
           double *Z, double *X2, double *mu, double *sd, double *F, double *L, double *eigvals,
           dfm_em_info *info);
/* dfm_em, then the workhorse fit of (y, w, Z) at the final r: a normal
 * dfm_model — equal to dfm_model_fit(y, w, Z, r, crit, kmax) bit for bit — so
 * the bootstrap, Chow, sup-Chow, criterion and predict entry points serve it
 * unchanged.  y and w are host memory. */
int dfm_model_fit_em(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw, const double *X,
                     int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *spec, dfm_model **out,
                     dfm_em_info *info);
/* The completed panel X2 (T x N column-major, original units) and the last
 * z-score's mu (N), sd (N) of a dfm_model_fit_em model; -1 for any other model. */
int dfm_model_em_read(const dfm_model *m, double *X2, double *mu, double *sd);

/* ---------- state-space factor model (dfm_ss.hip, dfm_ss_em.hip, dfm_ss_fit.hip)
 * The factors as a VAR(p), smoothed over the observed entries of a panel
 * (NaN = missing, m_ti = !isnan(x_ti)):
 *   x_t = Lambda f_t + e_t,  e_t ~ N(0, diag(sigma^2)),  Lambda N x r
 *   f_t = A_1 f_{t-1} + ... + A_p f_{t-p} + u_t,  u_t ~ N(0, Q)
 *   state alpha_t = (f_t, ..., f_{t-p+1}), s = r p; companion matrix Tm: A =
 *   [A_1 ... A_p] (r x rp) in its first r rows, the identity shift below;
 *   Qs: Q in the top-left r x r block, zero elsewhere.
 * Limits: 1 <= r <= 16, 1 <= p <= 8, s <= 32 (-7 beyond).
 *
 * Collapse (parallel over t, one read of the panel): for every row t
 *   C_t = sum_i m_ti lambda_i lambda_i' / sigma^2_i      (r x r)
 *   b_t = sum_i m_ti lambda_i x_ti / sigma^2_i           (r)
 *   q_t = sum_i m_ti x_ti^2 / sigma^2_i,  n_t = sum_i m_ti,
 *   l_t = sum_i m_ti log sigma^2_i.
 * Recursion (sequential in t, one workgroup per panel), from a = a0, P = P0
 * (the moments of alpha_1 before any data); Pff = P[:r,:r], Pf = P[:, :r],
 * a_f = a[:r], G = I_r + C_t Pff.  For a row with n_t > 0:
 *   K = Pf G^-1;  d = b_t - C_t a_f;  a <- a + K d
 *   P <- P - K C_t Pf', then P <- (P + P') / 2
 *   loglik -= 1/2 [ n_t log 2 pi + l_t + log det G + q_t - 2 b_t'a_f
 *                   + a_f' C_t a_f - d' Pff G^-1 d ]   (a_f, Pff from before the update)
 * a row with n_t = 0 leaves a and P as they are; then for every row
 *   a <- Tm a;  P <- Tm P Tm' + Qs.
 * Backwards (Rauch-Tung-Striebel):
 *   J_t = P_t|t Tm' P_{t+1|t}^-1
 *   a_t|T = a_t|t + J_t (a_{t+1|T} - a_{t+1|t})
 *   P_t|T = P_t|t + J_t (P_{t+1|T} - P_{t+1|t}) J_t'.
 * A forecast horizon h is h rows without an observed entry appended: outputs
 * have T + h rows.  The batch is M panels of one shape sharing the parameters,
 * each with its own NaN pattern (layout of dfm_mc); results are bit-identical
 * run to run, and panel b of a batch is bit-identical to a call on panel b.
 *
 * Two-step fit (Doz, Giannone & Reichlin 2011), dfm_ss_fit:
 *   1. dfm_em on the panel (spec passed through): Z, F, L, mu, sd
 *   2. sigma^2_i = sum_t m_ti (Z_ti - f_t' lambda_i)^2 / n_i, n_i = column i's observed count
 *   3. VAR(p) on F by OLS without intercept: Y = F[p:], Xl = [F[p-1:T-1], ...,
 *      F[0:T-p]], A' = (Xl'Xl)^-1 Xl'Y, U = Y - Xl A', Q = U'U / (T - p)
 *   4. a0 = 0; P0 solves P = Tm P Tm' + Qs by the doubling iteration
 *      P <- P + M P M', M <- M M from P = Qs, M = Tm, until max|M| < 1e-40
 *      (an error after 60 doublings or at the first non-finite entry)
 *   5. the smoother with horizon h on Zm = m ? Z : NaN.
 *
 * Return codes beside -1 / -2: -7 r, p or s beyond the limits; -10 a
 * non-positive sigma^2_i (the message names the column, 0-based); -11
 * T - p <= r p, or a singular Xl'Xl; -12 NaN in Lambda, sigma^2, A, Q, a0 or
 * P0; 5 Q, a P_{t+1|t} or a G not invertible; 6 the VAR is not stationary
 * (the doubling iteration did not converge). */

/* Stationary covariance of the state, step 4 above.  A: r x rp column-major,
 * Q: r x r; P0_out: s x s (symmetric).  Pure host arithmetic; no context. */
int dfm_ss_stationary_cov(const double *A, const double *Q, int r, int p, double *P0_out);

typedef struct dfm_ss_params {
  int32_t r, p;
  const double *lambda;   /* N x r column-major (ld N) */
  const double *sigma2;   /* N */
  const double *A;        /* r x rp column-major */
  const double *Q;        /* r x r */
  const double *a0;       /* s; NULL: zero */
  const double *P0;       /* s x s column-major; NULL: the stationary covariance */
} dfm_ss_params;
typedef struct dfm_ss_spec {
  int32_t horizon;        /* h >= 0 forecast rows */
  int32_t dev;            /* != 0: X is a device pointer on the context's device */
} dfm_ss_spec;

/* X: M panels, panel b column-major T x N at X + b*stride (ldx >= T, stride >=
 * ldx*N), NaN = missing.  Outputs are host memory, row-major, any may be NULL:
 * filtered M x T x r (f_t|t), smoothed M x (T+h) x r (f_t|T), smoothed_cov
 * M x (T+h) x r x r (the factor block of P_t|T), loglik M, n_observed M. */
int dfm_ss_smooth(dfm_ctx *ctx, const double *X, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
                  const dfm_ss_params *params, const dfm_ss_spec *spec, double *filtered, double *smoothed,
                  double *smoothed_cov, double *loglik, int64_t *n_observed);

/* Mixed frequency (Mariano & Murasawa 2003; Banbura & Modugno 2014): series
 * sampled at a lower frequency than the state load on a within-period
 * aggregate of the factors.
 *   low_i in {0,1} per series; weights w_0..w_{n_w-1}, 1 <= n_w <= 8, finite, w_0 != 0
 *   x_ti = lambda_i' f_t  + e_ti   (low_i = 0)
 *   x_ti = lambda_i' ft_t + e_ti   (low_i = 1),  ft_t = sum_{k<n_w} w_k f_{t-k}
 *   f_t as above: VAR(p), A r x rp, Q r x r
 *   state alpha_t = (f_t, ..., f_{t-L+1}), L = max(p, n_w), s = r L; the
 *   companion matrix holds [A 0] in its first r rows and the shift below; a0
 *   has s entries and P0 is s x s; a NULL P0 is the stationary covariance of
 *   this padded companion form (the same doubling iteration).
 * Limits: 1 <= r <= 16, 1 <= p <= 8, 1 <= n_w <= 8, r max(p, n_w) <= 32 (-7
 * beyond); a non-finite weight, w_0 = 0 or a NULL `low` is -2.
 * A quarterly flow observed in the last month of its quarter (NaN in the
 * other two) takes w = (1, 2, 3, 2, 1) for monthly growth rates, a quarterly
 * mean w = (1/3, 1/3, 1/3).
 *
 * The errors are independent across series, so a row is two exact updates of
 * the recursion above, one per class c in the order (high, low), each on the
 * collapsed moments C^c_t, b^c_t of its own series only and skipped when
 * n^c_t = 0.  With Z_h = [I_r 0 ...], Z_l = [w_0 I_r ... w_{n_w-1} I_r 0 ...]:
 *   PZ = P Z_c',  V = Z_c PZ,  z = Z_c a,  G = I_r + C^c_t V
 *   K = PZ G^-1;  d = b^c_t - C^c_t z;  a <- a + K d
 *   P <- P - K C^c_t PZ', then P <- (P + P') / 2
 *   loglik -= 1/2 [ n^c_t log 2 pi + l^c_t + log det G + q^c_t - 2 b^c_t'z
 *                   + z' C^c_t z - d' V G^-1 d ]   (z, V from before the class's update)
 * The prediction step and the backward pass are unchanged at the padded state. */
typedef struct dfm_ss_mf {
  int32_t n_w;
  const double *w;        /* n_w aggregation weights */
  const uint8_t *low;     /* N: != 0 marks a low-frequency series */
} dfm_ss_mf;

/* dfm_ss_smooth of the mixed-frequency model: params->A is r x rp, params->a0
 * (s) and params->P0 (s x s) are those of the padded state.  smoothed_agg:
 * M x (T+h) x r row-major, ft_t|T = Z_l a_t|T (NULL: not wanted).  When no
 * series is marked low the call is dfm_ss_smooth bit for bit: w is ignored,
 * the state is the plain one (s = r p) and smoothed_agg is not written. */
int dfm_ss_smooth_mf(dfm_ctx *ctx, const double *X, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
                     const dfm_ss_params *params, const dfm_ss_mf *mf, const dfm_ss_spec *spec, double *filtered,
                     double *smoothed, double *smoothed_cov, double *loglik, int64_t *n_observed,
                     double *smoothed_agg);

/* Steps 2-4 of the two-step fit.  Zm: T x N column-major (ldx >= T), NaN =
 * missing; F: T x r, L: N x r column-major.  Outputs column-major: sigma_out
 * (N), A_out (r x rp), Q_out (r x r), P0_out (s x s).  Host arithmetic (the
 * panel is read once, the rest is r p sized). */
int dfm_ss_estimate(dfm_ctx *ctx, const double *Zm, int64_t T, int64_t N, int64_t ldx, const double *F,
                    const double *L, int r, int p, double *sigma_out, double *A_out, double *Q_out, double *P0_out);

/* What dfm_ss_fit returns: host memory, any may be NULL.  Panels are T x N
 * column-major (ld T); size the r-dependent ones for em_spec->r, or for 32
 * factors when r is selected (r = info->r on return). */
typedef struct dfm_ss_fit_out {
  double *mu, *sd;                 /* N: the EM's last z-score */
  double *lambda;                  /* N x r column-major: the EM's loadings */
  double *sigma2, *A, *Q, *P0;     /* as dfm_ss_estimate */
  double *filtered, *smoothed, *smoothed_cov, *loglik;   /* as dfm_ss_smooth with M = 1 */
  double *x_smoothed;              /* m ? Z : Lambda f_t|T */
  double *x_completed;             /* m ? X : (Lambda f_t|T) sd + mu; observed entries bit-equal to X */
  double *forecast;                /* h x N column-major (ld h): (Lambda f_{T+k|T}) sd + mu */
  double *em_standardized, *em_completed, *em_factors, *eigvals;   /* dfm_em's Z, X2, F (T x r), eigvals (r) */
} dfm_ss_fit_out;
int dfm_ss_fit(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
               int horizon, dfm_em_info *info, const dfm_ss_fit_out *out);

/* AR(1) idiosyncratic terms (Banbura & Modugno 2014), by quasi-differencing:
 *   x_ti = lambda_i' f_t + e_ti,  e_ti = rho_i e_{t-1,i} + u_ti,
 *   u_ti ~ N(0, sigma^2_i),  |rho_i| < 1
 *   f_t as above: VAR(p).  State alpha_t = (f_t, ..., f_{t-L+1}), L = max(p, 2),
 *   s = r L; the companion matrix holds [A 0] over the shift (the padded form
 *   of the mixed-frequency model); a0 has s entries and P0 is s x s; a NULL P0
 *   is the stationary covariance of the padded form.
 * sigma^2_i is the innovation variance; the stationary variance of e_ti is
 * sigma^2_i / (1 - rho_i^2).
 * Limits: 1 <= r <= 8 (the update has size ru = 2r <= 16), 1 <= p <= 8,
 * r max(p, 2) <= 32 (-7 beyond).  A NULL rho or |rho_i| >= 1 is -2 (the message
 * names the column, 0-based), NaN in rho -12.
 *
 * Run-wise likelihood.  With m_{-1,i} = 0, an observed entry is one of two
 * kinds.  A pair entry, m_ti m_{t-1,i} = 1:
 *   y = x_ti - rho_i x_{t-1,i},  z_i = (lambda_i, -rho_i lambda_i) on alpha[:2r],
 *   v = sigma^2_i
 * A start entry, m_ti = 1 and m_{t-1,i} = 0:
 *   y = x_ti,  z_i = (lambda_i, 0),  v = sigma^2_i / (1 - rho_i^2)
 * Either way the noise of y is independent across series and, within a run of
 * observed entries, across rows, so a row still collapses: with ru = 2r
 *   C_t = sum_i z_i z_i' / v  (ru x ru),  b_t = sum_i z_i y / v  (ru),
 *   q_t = sum_i y^2 / v,  n_t = sum_i m_ti,  l_t = sum_i log v
 * and the recursion is the one above with r replaced by ru in the update only:
 * Pff = P[:ru,:ru], Pf = P[:, :ru], a_f = a[:ru], G = I_ru + C_t Pff.  The
 * prediction step, the backward pass and the outputs are unchanged at the
 * padded state; filtered, smoothed and smoothed_cov stay r-sized.
 * A run that begins after a hole starts from the stationary distribution of
 * e_ti: for a series observed on one consecutive run (late starters and ragged
 * edges included) this is the exact likelihood of the model, and with interior
 * holes it is a composite likelihood that ignores the dependence of e across
 * the hole.
 *
 * Fill (host arithmetic) of a missing (t, i), t < T + h: with ehat_u = x_ui -
 * lambda_i' f_u|T at an observed row u, u the last observed row before t, v the
 * first after it, d1 = t - u, d2 = v - t,
 *   only u (ragged edge, forecast rows):  e = rho^d1 ehat_u
 *   only v (late starter):                e = rho^d2 ehat_v
 *   both (the AR(1) bridge):  e = [rho^d1 (1 - rho^(2 d2)) ehat_u
 *                                  + rho^d2 (1 - rho^(2 d1)) ehat_v] / (1 - rho^(2 (d1 + d2)))
 *   neither: e = 0
 * and the fill is lambda_i' f_t|T + e.
 *
 * Two-step estimate of rho, after step 2 of dfm_ss_fit: eps_ti = Z_ti - f_t'
 * lambda_i over the observed entries, P_i the pair rows of series i,
 *   rho_i = sum_P eps_t eps_{t-1} / sum_P eps_{t-1}^2, clamped to +-0.99
 *   sigma^2_i = sum_P (eps_t - rho_i eps_{t-1})^2 / |P_i|
 * with |P_i| < 3 or a zero denominator: rho_i = 0 and sigma^2_i stays step 2's;
 * a non-positive variance after this is -10. */

/* dfm_ss_smooth with AR(1) idiosyncratic terms: rho has N entries, params->A
 * is r x rp, params->a0 (s) and params->P0 (s x s) are those of the padded
 * state, s = r max(p, 2).  An all-zero rho runs this path too. */
int dfm_ss_smooth_ar(dfm_ctx *ctx, const double *X, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
                     const dfm_ss_params *params, const double *rho, const dfm_ss_spec *spec, double *filtered,
                     double *smoothed, double *smoothed_cov, double *loglik, int64_t *n_observed);

/* dfm_ss_estimate with the two-step estimate of rho: rho_out (N), sigma_out the
 * innovation variances, P0_out (s x s) of the padded form, s = r max(p, 2). */
int dfm_ss_estimate_ar(dfm_ctx *ctx, const double *Zm, int64_t T, int64_t N, int64_t ldx, const double *F,
                       const double *L, int r, int p, double *sigma_out, double *A_out, double *Q_out, double *P0_out,
                       double *rho_out);

/* The fill rule.  X: T x N column-major (ldx >= T), NaN = missing; L: N x r
 * column-major; smoothed: (T + horizon) x r row-major, as dfm_ss_smooth_ar
 * returns it; completed: (T + horizon) x N column-major (ld T + horizon),
 * observed entries copied.  Pure host arithmetic; no context. */
int dfm_ss_ar_fill(const double *X, int64_t T, int64_t N, int64_t ldx, const double *L, int r, const double *rho,
                   const double *smoothed, int64_t horizon, double *completed);

/* dfm_ss_fit with AR(1) idiosyncratic terms: dfm_em, dfm_ss_estimate_ar,
 * dfm_ss_smooth_ar on Zm, then the fill rule on the standardised panel:
 * x_smoothed is the fill's first T rows, x_completed = m ? X : fill sd + mu
 * (observed entries bit-equal to X), forecast the fill's last h rows in the
 * panel's units.  out->P0 is s x s at s = r max(p, 2); rho_out: N (may be NULL). */
int dfm_ss_fit_ar(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
                  int horizon, dfm_em_info *info, const dfm_ss_fit_out *out, double *rho_out);

/* Quasi-maximum likelihood by EM (Doz, Giannone & Reichlin 2012; Banbura &
 * Modugno 2014 for arbitrary missing patterns), dfm_ss_em: M panels of one
 * shape, each with its own parameters and its own stopping time; the whole
 * iteration stays on the device.  The panel is in the units it is given.
 *
 * E-step at theta = (Lambda, sigma^2, A, Q, a0, P0): the collapse, filter and
 * smoother above give loglik(theta), a_t|T, P_t|T and, for t = 2..T,
 *   Cov(f_t, alpha_{t-1} | T) = the first r rows of P_t|T J_{t-1}'.
 * With E_t = f_t|T f_t|T' + Pff_t|T, a_t = a_t|T, f_t = f_t|T:
 *   S11 = sum_{t=2..T} E_t                                         (r x r)
 *   S10 = sum_{t=2..T} [ f_t a_{t-1}' + Cov(f_t, alpha_{t-1}|T) ]  (r x s)
 *   S00 = sum_{t=1..T-1} [ a_t a_t' + P_t|T ]                      (s x s)
 *   per series i: S_i = sum_t m_ti E_t, g_i = sum_t m_ti x_ti f_t,
 *   q_i = sum_t m_ti x_ti^2, n_i = sum_t m_ti.
 * Forecast rows enter no sum; a row with n_t = 0 inside the sample enters the
 * transition sums like any other.
 * M-step (the latent variables are the states; missing entries are not data):
 *   lambda_i = S_i^-1 g_i;  sigma^2_i = (q_i - lambda_i' g_i) / n_i
 *   A = S10 S00^-1;  Q = (S11 - A S10') / (T - 1), then (Q + Q') / 2
 *   update_init: a0 <- a_1|T, P0 <- P_1|T; otherwise a0, P0 stay the start's.
 * Loop from the start theta_0, for j = 0, 1, ...:
 *   1. E-step at theta_j: ll_j
 *   2. j >= 1: c_j = (ll_j - ll_{j-1}) / ((|ll_j| + |ll_{j-1}|) / 2) (0 when
 *      both are zero); converged if tol > 0 and c_j < tol
 *   3. stop if j = max_iter
 *   4. M-step: theta_{j+1}.
 * The call returns theta_j of the last E-step with that E-step's outputs, the
 * path ll_0..ll_j (NaN beyond) and iterations = j.  tol = 0 runs exactly
 * max_iter M-steps; max_iter = 0 is one E-step.  A panel that has stopped is
 * frozen: its kernels exit at once, its buffers are not touched again.  A
 * panel's result does not depend on its neighbours: panel b of a batch is
 * bit-identical to a call on panel b alone with its start.
 *
 * Return codes: -2 bad arguments, T < 2, or a column without an observed
 * entry; -7 the limits; -12 NaN in a start; 5 a start's Q not positive
 * definite, or an S_i, S00, P_{t+1|t} or G not invertible in a pass; 6 a NULL
 * P0 with a non-stationary start; -10 a non-positive sigma^2_i in a start or
 * after an M-step.  A column without an observed entry is found before the
 * first pass, on the host for a host batch and by one small kernel for a
 * device batch.  The messages of a pass name the panel, the column (-10) and
 * the iteration j: "the E-step of iteration j" is the pass at theta_j, "the
 * M-step giving iteration j" the one that produced theta_j. */
typedef struct dfm_ss_em_spec {
  int32_t max_iter;       /* M-steps at the most; < 0: 100 */
  int32_t update_init;    /* != 0: a0, P0 are re-estimated */
  int32_t horizon;        /* h >= 0 forecast rows of the outputs */
  int32_t dev;            /* != 0: X is a device pointer on the context's device */
  double tol;             /* < 0: 1e-4; 0: never stop early */
} dfm_ss_em_spec;
typedef struct dfm_ss_em_info {
  int32_t iterations;     /* j of the last E-step */
  int32_t converged;
  double loglik;          /* ll_j */
  double crit;            /* the last c_j (NaN when j = 0) */
} dfm_ss_em_info;
/* Host memory, any may be NULL; every field has a leading axis M.  The
 * parameters in the layouts of dfm_ss_params; the smoother's outputs as
 * dfm_ss_smooth; loglik_path M x (max_iter + 1) with the default resolved. */
typedef struct dfm_ss_em_out {
  double *lambda, *sigma2, *A, *Q, *a0, *P0;
  double *filtered, *smoothed, *smoothed_cov;
  int64_t *n_observed;
  double *loglik_path;
  double *smoothed_agg;   /* dfm_ss_em_mf: M x (T+h) x r, Z_l a_t|T; dfm_ss_em does not read it */
} dfm_ss_em_out;
/* X as dfm_ss_smooth.  starts: n_start = 1 (shared by all panels) or M
 * dfm_ss_params of one (r, p).  info: M entries, or NULL. */
int dfm_ss_em(dfm_ctx *ctx, const double *X, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
              const dfm_ss_params *starts, int64_t n_start, const dfm_ss_em_spec *spec, const dfm_ss_em_out *out,
              dfm_ss_em_info *info);

/* dfm_ss_em of the mixed-frequency model (dfm_ss_mf above; Banbura & Modugno
 * 2014).  The starts' A is r x rp, their a0 (s) and P0 (s x s) those of the
 * padded state, s = r max(p, n_w); the outputs likewise (A r x rp, a0, P0
 * padded).  The E-step is dfm_ss_smooth_mf's.  The M-step differs in that the
 * aggregation is built into each series' regressor:
 *   S_i = sum_t m_ti Et^c(i)_t,  g_i = sum_t m_ti x_ti f^c(i)_t,
 *   Et^c_t = Z_c (a_t|T a_t|T' + P_t|T) Z_c',  f^c_t = Z_c a_t|T  (c(i) the class of i)
 *   lambda_i, sigma^2_i from them as above;
 *   A = S10[:, :rp] (S00[:rp, :rp])^-1,  Q = (S11 - A S10[:, :rp]') / (T - 1),
 *   symmetrised; the companion matrix's lags beyond p stay zero.
 * The stopping rule, freezing, update_init, return codes and messages are
 * dfm_ss_em's (-7 and -2 as dfm_ss_smooth_mf).  out->smoothed_agg is filled.
 * When no series is marked low the call is dfm_ss_em bit for bit. */
int dfm_ss_em_mf(dfm_ctx *ctx, const double *X, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
                 const dfm_ss_params *starts, int64_t n_start, const dfm_ss_mf *mf, const dfm_ss_em_spec *spec,
                 const dfm_ss_em_out *out, dfm_ss_em_info *info);

/* dfm_ss_fit, then dfm_ss_em (M = 1) on its Zm from its parameters (a0 = 0,
 * P0 the stationary covariance of the two-step VAR).  `out` is filled as by
 * dfm_ss_fit, from the ML parameters and their smoothed factors; mu and sd
 * stay the static EM's.  ml_spec->horizon is the forecast horizon; ml_spec->dev
 * is ignored (em_spec->dev says where X lives).  a0_out (s), loglik_path
 * (max_iter + 1) and ml_info may be NULL. */
int dfm_ss_fit_ml(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
                  const dfm_ss_em_spec *ml_spec, dfm_em_info *info, const dfm_ss_fit_out *out, double *a0_out,
                  double *loglik_path, dfm_ss_em_info *ml_info);

/* dfm_ss_fit (method 0) or dfm_ss_fit_ml (method 1) of the mixed-frequency
 * model.  dfm_em runs on the panel as given (a low series' empty months are
 * ordinary NaN to it) and dfm_ss_estimate as in dfm_ss_fit; then for each low
 * series lambda_i, sigma^2_i are re-estimated by OLS of Z_ti on ft_t = sum_k
 * w_k F_{t-k} over its observed rows t >= n_w - 1 (sigma^2_i = the residual
 * sum of squares over their count; -11 with fewer than r + 1 such rows, the
 * message names the column), P0 is the stationary covariance of the padded
 * companion form, and dfm_ss_smooth_mf / dfm_ss_em_mf take the place of the
 * plain passes.  ml_spec is required: its horizon is the forecast horizon in
 * both methods.  `out` as dfm_ss_fit_ml fills it, with P0 s x s at s = r
 * max(p, n_w), and x_smoothed, x_completed and forecast from Lambda ft_t|T in
 * the low columns; a0_out has s entries; smoothed_agg (T+h) x r row-major;
 * each may be NULL.  When no series is marked low the call is dfm_ss_fit or
 * dfm_ss_fit_ml bit for bit. */
int dfm_ss_fit_mf(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
                  const dfm_ss_em_spec *ml_spec, const dfm_ss_mf *mf, int method, dfm_em_info *info,
                  const dfm_ss_fit_out *out, double *a0_out, double *loglik_path, dfm_ss_em_info *ml_info,
                  double *smoothed_agg);

/* Factor blocks (Banbura, Giannone & Reichlin 2011; Banbura & Modugno 2014,
 * section 2.3): a global factor that every series loads on beside group
 * factors that only their own series load on, each block with its own VAR.
 *   blocks g = 1..n_b of sizes r_g >= 1, sum r_g = r; block g owns the
 *   contiguous factors o_g .. o_g + r_g - 1 (o_1 = 0)
 *   member: N x n_b, != 0: the series loads on the block;
 *   free_ij = member[i, g(j)], g(j) the block that owns factor j
 *   Lambda_ij = 0 wherever free_ij = 0
 *   A_k (k = 1..p) and Q are block-diagonal with the blocks' sizes
 *   P0 and a0 are unrestricted; everything else is the model above, plain
 *   or mixed-frequency.
 * The E-step is unchanged (a zero is a zero to the collapse and the
 * recursion).  M-step, with the sums above (S_i, g_i those of the series'
 * class in the mixed-frequency model):
 *   per series i, J = {j : free_ij}: lambda_i[J] = S_i[J,J]^-1 g_i[J], zero
 *   elsewhere; sigma^2_i = (q_i - lambda_i' g_i) / n_i
 *   per block g, rows G = its factors, columns c = {k r + o_g + j : k < p,
 *   j < r_g}: A[G, c] = S10[G, c] S00[c, c]^-1, zero elsewhere;
 *   Q[G, G] = (S11[G, G] - A[G, c] S10[G, c]') / (T - 1), symmetrised, zero
 *   elsewhere (mixed frequency: k runs over the VAR's own p lags).
 * This is the exact maximiser under the restrictions.  The stopping rule,
 * freezing, update_init, return codes and messages are dfm_ss_em's.
 * -2 also, with a message naming the offender: a NULL struct or field,
 * n_blocks outside 1..16, a size < 1, sum r_g != the starts' r, a series that
 * is a member of no block (the column), a block without a member (the block),
 * a start whose Lambda, A or Q is not zero at a restricted position (the
 * parameter and the entry).  One block of size r that every series is a
 * member of is no restriction: the call is then dfm_ss_em / dfm_ss_em_mf /
 * dfm_ss_fit / dfm_ss_fit_ml / dfm_ss_fit_mf bit for bit. */
typedef struct dfm_ss_blocks {
  int32_t n_blocks;          /* 1..16 */
  const int32_t *block_r;    /* n_blocks sizes, each >= 1, sum = r */
  const uint8_t *member;     /* N x n_blocks column-major (ld N), != 0: the series loads on the block */
} dfm_ss_blocks;

/* dfm_ss_em (mf NULL) or dfm_ss_em_mf with the blocks; every other argument
 * as theirs. */
int dfm_ss_em_blocks(dfm_ctx *ctx, const double *X, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
                     const dfm_ss_params *starts, int64_t n_start, const dfm_ss_mf *mf /* NULL: plain */,
                     const dfm_ss_blocks *blocks, const dfm_ss_em_spec *spec, const dfm_ss_em_out *out,
                     dfm_ss_em_info *info);

/* dfm_ss_fit_mf (mf NULL: dfm_ss_fit for method 0, dfm_ss_fit_ml for method 1)
 * with the blocks:
 *   1. dfm_em on the panel at r = sum r_g (em_spec->r must be that sum: a
 *      selected r is -3): Z, mu, sd and the completed standardised panel
 *   2. R <- Z; for g = 1..n_b in order: (F_g, L_g) = dfm_pca of the member
 *      columns of R at k = r_g (-11 when the block has fewer than r_g
 *      members, the message names the block); F_g into the block's factor
 *      columns, L_g into its members' rows of Lambda (zero elsewhere); F_g L_g'
 *      is subtracted from those columns of R
 *   3. sigma^2_i over the observed entries of Z - F Lambda'; a VAR(p) by OLS
 *      per block on its own F_g (the arithmetic of dfm_ss_estimate): A and Q
 *      block-diagonal; with mf, a low series' lambda_i, sigma^2_i by OLS on
 *      the aggregate of its free factors only (as dfm_ss_fit_mf otherwise;
 *      -11 with fewer observed rows than its free factors + 1)
 *   4. P0 = the stationary covariance
 *   5. the smoother (method 0) or the EM with the blocks (method 1).
 * `out` as dfm_ss_fit_mf fills it; em_factors holds step 2's F. */
int dfm_ss_fit_blocks(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec,
                      int p, const dfm_ss_em_spec *ml_spec, const dfm_ss_mf *mf /* NULL */,
                      const dfm_ss_blocks *blocks, int method, dfm_em_info *info, const dfm_ss_fit_out *out,
                      double *a0_out, double *loglik_path, dfm_ss_em_info *ml_info, double *smoothed_agg);

/* Simulation smoother (Durbin & Koopman 2002), dfm_ss_simulate (dfm_ss_sim.hip):
 * D joint draws of f_1..f_{T+h} given the observed entries of one panel, for
 * the plain model of dfm_ss_smooth, Tt = T + h rows, s = r p.  The smoother's
 * recursion runs once on the panel and leaves C_t, b_t, n_t, P_t|t-1, P_t|t.
 *
 * Per-row gains (they do not depend on the draw; the rows are independent):
 *   n_t > 0: G = I + C_t Pff_t|t-1, K_t = Pf_t|t-1 G^-1 (s x r);  n_t = 0: K_t = 0
 *   t < Tt - 1: J_t = P_t|t Tm' P_{t+1|t}^-1
 *   R_t: the lower-triangular factor of the positive semi-definite C_t, R_t R_t'
 *   = C_t, by the Cholesky loop with one rule for a rank-deficient row (n_t <
 *   r, or a zero loading column): at column j, d = C_jj - sum_{k<j} R_jk^2; if
 *   d <= 1e-12 C_jj column j of R_t is zero, otherwise R_jj = sqrt(d) and the
 *   column follows as usual.  (In exact arithmetic a zero pivot of a PSD matrix
 *   has a zero column below it, so R R' = C still holds; a zero pivot's
 *   rounding residue is about r 2^-53 C_jj, under 2e-15 at r = 16.)
 *   L0: the same factor of P0 (s x s);  Lq: the Cholesky factor of Q (5 when Q
 *   is not positive definite).
 *
 * Draw d, from standard normals z0 (s), u_t (r), zeta_t (r):
 *   alpha+_0 = a0 + L0 z0;  alpha+_t = Tm alpha+_{t-1} + [Lq u_t; 0]  (t >= 1; u_0 is not read)
 *   f+_t = alpha+_t[:r]
 *   b*_t = b_t - C_t f+_t - R_t zeta_t          (rows with n_t > 0; zeta_t is not read otherwise)
 *   c = 0;  per row: if n_t > 0: c <- c + K_t (b*_t - C_t c[:r]);  c_t|t = c;  c <- Tm c
 *   backwards: c_{Tt-1|T} = c_{Tt-1|Tt-1};  c_t|T = c_t|t + J_t (c_{t+1|T} - Tm c_t|t)
 *   draw: f~_t = f+_t + c_t|T[:r].
 * The smoother is affine in the data and in a0: smoothing x - x+ from a zero
 * prior mean and adding alpha+ is a draw from the posterior (the mean
 * correction).  A pseudo-panel x+ enters the filter only through its collapsed
 * b+_t = C_t f+_t + N(0, C_t) = C_t f+_t + R_t zeta_t: none is formed, and a
 * row costs 2 r normals per draw whatever N is.
 *
 * Normals: nz = s + 2 r Tt per draw, draw d's vector [z0 | u_0 zeta_0 | u_1
 * zeta_1 | ...]; z is column-major D x nz, the draw index fastest (ldz >= D),
 * host memory or (z_dev) device memory.  The first s + 2 r T entries of an
 * h-row call are the h = 0 call's.  z is not scanned: a NaN among draw d's
 * normals makes draw d NaN and touches no other draw.  A draw's result depends
 * on neither D, its position in the call nor the pass it falls in.
 *
 * Return codes are dfm_ss_smooth's; -2 also for D < 1, D > 2^24, a NULL z or
 * draws, ldz < D and pass_draws < 0. */
typedef struct dfm_ss_sim_spec {
  int32_t horizon, dev /* X on the device */, z_dev /* z on the device */;
  int64_t pass_draws;   /* 0: the workspace rule; > 0: at most that many draws per pass */
} dfm_ss_sim_spec;
int dfm_ss_simulate(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_ss_params *params,
                    const dfm_ss_sim_spec *spec, int64_t D, const double *z, int64_t ldz,
                    double *draws /* host, D x (T+h) x r row-major */,
                    double *smoothed, double *smoothed_cov, double *loglik /* as dfm_ss_smooth, M = 1; any NULL */);

/* News decomposition of a forecast revision (Banbura & Modugno 2014),
 * dfm_ss_news (dfm_ss_news.hip): which release moved the smoothed path between
 * two vintages of one panel, and by how much.  Two vintages X_old, X_new of one
 * T x N panel share the parameters; Omega_new contains Omega_old, the observed
 * sets.  The releases are the J entries (t_j, i_j) observed in X_new and NaN
 * in X_old.  Entries observed in both may differ (a revision): X_rev has
 * X_new's values on Omega_old and NaN elsewhere.  Three smoothed states over
 * Tt = T + h rows: a_t|old, a_t|rev, a_t|new.  The revision effect is a|rev -
 * a|old, the news effect a|new - a|rev.
 *
 * The news of release j, with c(i) the class of series i and Z_h, Z_l as above
 * (the plain model has the high class only):
 *   I_j = x_new[t_j, i_j] - lambda_{i_j}' Z_{c(i_j)} a_{t_j}|rev
 *   (release_forecast_j is the subtracted term).
 * The weights are the smoother's impulse responses under the NEW mask.  For
 * release j, from c = 0 (s entries), the rows forwards; within a row the
 * classes in the filter's order, and for each class with n^c_t > 0
 *   z = Z_c c
 *   d = beta - C^c_t z,  beta = lambda_{i_j} / sigma^2_{i_j} if t = t_j and c = c(i_j), else 0
 *   c <- c + K^c_t d
 * then c_t|t = c and c <- Tm c.  K^c_t = PZ G^-1 exactly as the filter forms
 * it: the second class of a row uses the P left by the first class's update,
 * a product local to the row that starts from the stored P_t|t-1.  Backwards
 *   c_{Tt-1|T} = c_{Tt-1|Tt-1};  c_t|T = c_t|t + J_t (c_{t+1|T} - Tm c_t|t),
 *   J_t = P_t|t Tm' P_{t+1|t}^-1.
 * The weights of release j at row t are wf_j[t] = c_t|T[:r] and wagg_j[t] =
 * Z_l c_t|T.  The smoother is affine in the data, and observing a value equal
 * to its conditional mean moves nothing, so for every row t, forecast rows
 * included,
 *   a_t|new - a_t|rev = sum_j I_j c^j_t|T.
 * For a target (t, k) the impact of release j is lambda_k' (wf_j[t], or
 * wagg_j[t] when k is a low series) I_j.
 *
 * The covariance recursion is not repeated: the gains C^c_t, K^c_t, J_t are
 * formed once per row and a release is a mean-only recursion, one GPU lane
 * each, that starts at its own row t_j and runs backwards down to t_lo.  A
 * release's weights depend on neither J, its position in the list nor the
 * pass it falls in; they depend on X_new's mask only.
 *
 * X_old, X_new: host, column-major T x N (one ldx).  mf: NULL, or without a
 * marked series, is the plain model.  rel_t, rel_i (J each): the list must be
 * exactly the releases, sorted by (t, i): -2 otherwise, and -2 for an entry
 * observed in X_old and NaN in X_new; the message names the first offending
 * entry.  J = 0 is valid: the smooths are returned and nothing else runs.
 * Other codes are dfm_ss_smooth_mf's; -2 also for J > 2^24, t_lo outside
 * [0, T + h) and pass_releases < 0. */
typedef struct dfm_ss_news_spec {
  int32_t horizon;          /* h >= 0 forecast rows */
  int32_t t_lo;             /* the weights cover the rows t_lo .. T + h - 1 */
  int64_t pass_releases;    /* 0: the workspace rule; > 0: at most that many releases per pass */
} dfm_ss_news_spec;
/* Host memory, any may be NULL.  The smoothed rows as dfm_ss_smooth_mf returns
 * them for X_old, X_rev and X_new, bit for bit ((T+h) x r row-major; the
 * aggregates are not written for the plain model); news and release_forecast
 * J; weights_f and weights_agg J x (T + h - t_lo) x r row-major (weights_agg
 * is not written for the plain model). */
typedef struct dfm_ss_news_out {
  double *smoothed_old, *smoothed_rev, *smoothed_new;
  double *smoothed_agg_old, *smoothed_agg_rev, *smoothed_agg_new;
  double *news, *release_forecast;
  double *weights_f, *weights_agg;
} dfm_ss_news_out;
int dfm_ss_news(dfm_ctx *ctx, const double *X_old, const double *X_new, int64_t T, int64_t N, int64_t ldx,
                const dfm_ss_params *params, const dfm_ss_mf *mf, const dfm_ss_news_spec *spec, int64_t J,
                const int64_t *rel_t, const int64_t *rel_i, const dfm_ss_news_out *out);

/* --------------------------------------------------- targeted predictors
 * targeted_predictors(..., thresholding="hard") (src/targeted_predictors.jl:9-30).
 * JOINT: OLS of y on [w x], White HC0, |t_x| > crit_value (the reference's
 * t_{0.975}(T-q-N) is passed in by the caller: no quantile code on device).
 * PER_CANDIDATE: y on [w x_i] for each i (extension, defect D8).
 * tstat (N) and mask (N, 0/1) are host outputs. */
int dfm_targeted_hard(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw,
                      const double *X, int64_t T, int64_t N, int64_t ldx, int mode,
                      double crit_value, double *tstat, uint8_t *mask);

/* targeted_predictors(..., thresholding="soft") (src/targeted_predictors.jl:31-36):
 * GLMNet.glmnetcv(Z = [w x], y), gaussian lasso (alpha = 1) with standardised
 * columns and an intercept; keep the x columns with a nonzero coefficient at
 * the CV-optimal lambda.  GLMNet is never imported by the reference (D5): the
 * algorithm is glmnet's Fortran elnet1 in its loop order (covariance updates,
 * full cyclic passes with in-pass entry, active-set passes, threshold 1e-7,
 * warm starts over `nlambda` log-spaced lambdas from lambda_max down to
 * lambda_min_ratio * lambda_max (<= 0: 1e-2 if T < q + N else 1e-4), early
 * path exit on the full fit after 5 lambdas when R^2 gains < 1e-5 relative or
 * R^2 > 0.999; no cap on the active set below 4096).  folds: T fold ids 1..K (host-drawn, as the
 * bootstrap draws).  Outputs: path length L, best (0-based argmin of the
 * fold-size-weighted hold-out MSE), lambda (L, original units), meanloss (L),
 * beta (q + N, original scale, at best), intercept a0, mask (N, 0/1).  Any
 * output pointer may be NULL. */
int dfm_targeted_soft(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw,
                      const double *X, int64_t T, int64_t N, int64_t ldx, const int32_t *folds,
                      int nlambda, double lambda_min_ratio, int *nlam_out, int *best_out,
                      double *lambda_out, double *meanloss_out, double *beta_out, double *a0_out,
                      uint8_t *mask);

/* glmnet's elnet1 lasso path (the core of dfm_targeted_soft, for direct use
 * and parity tests): G p x p symmetric (row-major) with unit diagonal over the
 * non-constant columns ju, c = Zs'ys/n, lambdas alms[nlam] in standardised
 * units (decreasing), early = glmnet's early path exit (5 lambdas, R^2 gain
 * < 1e-5 R^2 or R^2 > 0.999), thr = glmnet's threshold (1e-7).  Outputs: the
 * path length *L_out, betas (L x p row-major), rsq (L); NULL skips. */
int dfm_lasso_path(dfm_ctx *ctx, const double *G, const double *c, const uint8_t *ju, int p,
                   const double *alms, int nlam, int early, double thr, double *betas, double *rsq,
                   int *L_out);

/* Launch record of the lasso path kernel (process-wide, every context).  Its
 * leader and helper workgroups meet through bounded spins; each spin that
 * runs out is counted here (and described on stderr and in dfm_last_error)
 * instead of passing silently.  out[i] for i < n (slots below); reset != 0
 * zeroes the record after reading.  Returns DFM_LASSO_NSTATS. */
enum {
  DFM_LASSO_STAT_LAUNCHES = 0,   /* kernel launches, relaunches included */
  DFM_LASSO_STAT_RELAUNCHES,     /* launches after a failed hand-off */
  DFM_LASSO_STAT_TIMEOUTS,       /* timed-out spins, all kinds */
  DFM_LASSO_STAT_TASK_TMO,       /* workgroups whose first timeout was a helper's task poll */
  DFM_LASSO_STAT_DONE_TMO,       /* ... a leader's wait for its helpers */
  DFM_LASSO_STAT_PIPE_TMO,       /* ... a leader's in-workgroup pipeline wait */
  DFM_LASSO_STAT_BUDGET,         /* ... a leader's whole-path time budget */
  DFM_LASSO_STAT_RECOVERED,      /* timed-out polls whose re-read then found the granule */
  DFM_LASSO_STAT_MAX_SKEW_US,    /* max spread of the workgroups' entry times in one launch (us) */
  DFM_LASSO_STAT_LATE_ENTRIES,   /* launches where a workgroup entered after another had exited */
  DFM_LASSO_STAT_MAX_KERNEL_US,  /* longest kernel: first entry to last exit (us) */
  DFM_LASSO_STAT_MAX_HOST_US,    /* longest launch + synchronisation seen by the host (us) */
  DFM_LASSO_STAT_SLOW_LAUNCHES,  /* launches whose host time exceeded 2x the kernel + 50 ms */
  DFM_LASSO_STAT_WAVE_SPLITS,    /* launches where one workgroup's waves left > 1 ms apart */
  DFM_LASSO_NSTATS
};
int dfm_lasso_stats(int64_t *out, int n, int reset);

#ifdef __cplusplus
}
#endif
#endif /* DFM_H */
