// dfm_panel.hip — the host steps of a principal-components pass over ONE
// resident panel that need no fitted model (upload, Gram, full spectrum, top-k
// eigenpairs, reading a row-major block back), shared by the fit, the EM loop
// and the Monte-Carlo batches, and the entry points that take a bare panel:
// dfm_pca, dfm_gram_spectrum, dfm_normalize(_dev).
#include "dfm_host.h"

namespace dfm {

// X column-major T x N (leading dimension ldx) in host memory, or already in
// HBM when dev (then it is transposed in place of the copy, never duplicated)
int upload_panel(dfm_ctx *ctx, const double *X, int T, int N, int64_t ldx, DevPanel &dp, bool dev) {
  hipStream_t st = ctx->stream;
  dp.ld = round_up(N, 16);
  dp.st = st;
  HIPCHK(ctx, stream_malloc((void **)&dp.P, (size_t)T * dp.ld * 8, st));
  const double *src = X;
  int64_t lds = ldx;
  if (!dev) {
    HIPCHK(ctx, stream_malloc((void **)&dp.raw, (size_t)T * N * 8, st));
    HIPCHK(ctx, hipMemcpy2DAsync(dp.raw, (size_t)T * 8, X, (size_t)ldx * 8, (size_t)T * 8, N,
                                 hipMemcpyHostToDevice, st));
    src = dp.raw;
    lds = T;
  }
  hipLaunchKernelGGL(panel_from_colmajor_kernel, dim3((unsigned)((dp.ld + 31) / 32), (T + 31) / 32),
                     dim3(256), 0, st, src, lds, T, N, dp.P, dp.ld);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

// X X' (orient 0) or X'X (orient 1) of the T rows of src
hipError_t panel_gram(dfm_ctx *ctx, int orient, const PanelSrc &src, int T, int N, double *G) {
  const int m = orient == 0 ? T : N;
  Scope sc(ctx, DFM_KC_GRAM);
  return launch_gram(orient, src, m, orient == 0 ? N : T, T, G, m, (int64_t)m * m, 1, ctx->stream);
}

int gram_spectrum(dfm_ctx *ctx, const double *G, int m, std::vector<double> &ev) {
  // (callers check first and give their own text; this is dfm_gram_spectrum's)
  if (m > spectrum_any_max()) return fail(ctx, -30, "full spectrum supported for min(T,N) <= %d", spectrum_any_max());
  hipStream_t st = ctx->stream;
  DevBuf<> evd, wk;
  HIPCHK(ctx, evd.alloc(m));
  if (spectrum_work(m, 1) > 0) HIPCHK(ctx, wk.alloc((size_t)spectrum_work(m, 1)));
  {
    Scope sc(ctx, DFM_KC_EIG_OTHER);
    HIPCHK(ctx, launch_spectrum(G, m, (int64_t)m * m, m, 1, evd.p, wk.p, st));
  }
  ev.resize(m);
  HIPCHK(ctx, hipMemcpyAsync(ev.data(), evd.p, (size_t)m * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return 0;
}

EigArgs ctx_eig_args(dfm_ctx *ctx, int m, int k) {
  EigArgs ea{};
  ea.k = k;
  ea.p = eig_block_p(m, k, ctx->block);
  // a single fit's eigenvectors are polished to the rounding floor (the
  // residual rule at 1e-14; the floor and stagnation tests end it): statistics
  // of the fit with a near-zero value (an LR of ~0.4 between two nearly equal
  // SSRs) move by ~1e-10 relative when its eigenvectors stop at 1e-12 of the
  // gap (a break fit's LR in tests/test_gpu_breaks.py: 4e-10 off the oracle;
  // the tridiagonal path's inverse-iteration vectors: 9e-10)
  ea.tol = std::min(ctx->tol, 1e-14);
  ea.maxit = ctx->maxit; ea.poll = ctx->poll;
  ea.st = ctx->stream; ea.tf = timer_cb; ea.tctx = ctx;
  return ea;
}

int run_eig(dfm_ctx *ctx, const double *G, int m, int k, double *lam, double *Uk, double *trace, int *status_dev,
            char *ws, const double *warm) {
  EigArgs ea = ctx_eig_args(ctx, m, k);
  const int p = ea.p;
  if ((p > 32 || p < k) && m >= 2 && m <= dense_eig_max()) {
    // k beyond the subspace block: tridiagonalisation + inverse iteration (dfm_spec.hip)
    double *wk = nullptr;
    HIPCHK(ctx, hipMalloc(&wk, (size_t)dense_eig_work(m, k) * 8));
    hipError_t e;
    {
      Scope sc(ctx, DFM_KC_EIG_OTHER);
      e = launch_dense_eig(G, m, m, k, lam, Uk, trace, status_dev, wk, ctx->stream);
    }
    hipStreamSynchronize(ctx->stream);
    hipFree(wk);
    if (e != hipSuccess) return fail(ctx, 1000 + (int)e, "dense eigensolver: %s", hipGetErrorString(e));
    return 0;
  }
  if (p > 32 || p < k) return fail(ctx, -20, "eigensolver block %d unsupported for k=%d m=%d", p, k, m);
  char *own = nullptr;   // stream-ordered pool memory: no device-wide sync in the free
  if (!ws) HIPCHK(ctx, stream_malloc((void **)&own, eig_workspace_bytes_padded(m, 1, p <= 16 ? 16 : 32, ctx->maxit),
                                     ctx->stream));
  ea.nb = 1;
  ea.warm = warm; ea.kw = warm ? k : 0;
  ea.ws = ws ? ws : own;
  ea.lam = lam; ea.Uk = Uk; ea.trace_out = trace; ea.status = status_dev;
  const int rc = eig_run(G, m, (int64_t)m * m, m, ea, nullptr, 0);
  if (own) {
    hipFreeAsync(own, ctx->stream);
    hipStreamSynchronize(ctx->stream);
  }
  if (rc != 0) return fail(ctx, rc > 0 ? rc : -21, "eigensolver failed (%d)", rc);
  return 0;
}

int read_rows_colmajor(dfm_ctx *ctx, const double *src, int rows, int cols, double *dst) {
  std::vector<double> tmp((size_t)rows * cols);
  HIPCHK(ctx, hipMemcpyAsync(tmp.data(), src, tmp.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < rows; ++i)
    for (int j = 0; j < cols; ++j) dst[(size_t)j * rows + i] = tmp[(size_t)i * cols + j];
  return 0;
}

}  // namespace dfm

extern "C" {

int dfm_pca(dfm_ctx *ctx, const double *X, int64_t T64, int64_t N64, int64_t ldx, int k,
            double *eigvals, double *F, double *L, double *trace_G) {
  if (!ctx) return -1;
  if (!X || T64 < 1 || N64 < 1 || ldx < T64 || k < 1) return fail(ctx, -2, "dfm_pca: bad arguments");
  const int T = (int)T64, N = (int)N64, m = std::min(T, N);
  if (k > m) return fail(ctx, -2, "dfm_pca: k=%d > min(T,N)=%d", k, m);
  DeviceShare gate(ctx->device);
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  DevPanel dp;
  int rc = upload_panel(ctx, X, T, N, ldx, dp);
  if (rc) return rc;
  const int orient = (N > T) ? 0 : 1;
  DevBuf<> G, lam, Uk, tr, Fd, Ld;
  DevBuf<int> sd;
  HIPCHK(ctx, G.alloc((size_t)m * m));
  HIPCHK(ctx, lam.alloc(k)); HIPCHK(ctx, Uk.alloc((size_t)m * k)); HIPCHK(ctx, tr.alloc(1));
  HIPCHK(ctx, Fd.alloc((size_t)T * k)); HIPCHK(ctx, Ld.alloc((size_t)N * k)); HIPCHK(ctx, sd.alloc(1));
  PanelSrc src{nullptr, dp.P, nullptr, nullptr, dp.ld, 0};
  HIPCHK(ctx, panel_gram(ctx, orient, src, T, N, G.p));
  if ((rc = run_eig(ctx, G.p, m, k, lam.p, Uk.p, tr.p, sd.p))) return rc;
  {
    Scope sc(ctx, DFM_KC_FACTORS);
    if (k <= 32 ? launch_factors(orient, src, T, N, k, 1, Uk.p, Fd.p, Ld.p, nullptr, st)
                : launch_factors_wide(orient, dp.P, dp.ld, T, N, k, Uk.p, Fd.p, Ld.p, nullptr, st, (double)T))
      return fail(ctx, 1001, "factor kernels failed");
  }
  int est = 0;
  if (eigvals) HIPCHK(ctx, hipMemcpyAsync(eigvals, lam.p, (size_t)k * 8, hipMemcpyDeviceToHost, st));
  if (trace_G) HIPCHK(ctx, hipMemcpyAsync(trace_G, tr.p, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(&est, sd.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (F && (rc = read_rows_colmajor(ctx, Fd.p, T, k, F))) return rc;
  if (L && (rc = read_rows_colmajor(ctx, Ld.p, N, k, L))) return rc;
  if (est) return fail(ctx, 2, "eigensolver did not converge");
  return 0;
}

int dfm_gram_spectrum(dfm_ctx *ctx, const double *X, int64_t T64, int64_t N64, int64_t ldx,
                      double *eigvals_m, double *trace_G) {
  if (!ctx) return -1;
  if (!X || !eigvals_m || T64 < 1 || N64 < 1 || ldx < T64) return fail(ctx, -2, "bad arguments");
  const int T = (int)T64, N = (int)N64, m = std::min(T, N);
  if (m > spectrum_any_max()) return fail(ctx, -30, "full spectrum supported for min(T,N) <= %d", spectrum_any_max());
  DeviceShare gate(ctx->device);
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  DevPanel dp;
  int rc = upload_panel(ctx, X, T, N, ldx, dp);
  if (rc) return rc;
  DevBuf<> G;
  HIPCHK(ctx, G.alloc((size_t)m * m));
  PanelSrc src{nullptr, dp.P, nullptr, nullptr, dp.ld, 0};
  HIPCHK(ctx, panel_gram(ctx, (N > T) ? 0 : 1, src, T, N, G.p));
  std::vector<double> ev;
  if ((rc = gram_spectrum(ctx, G.p, m, ev))) return rc;
  std::copy(ev.begin(), ev.end(), eigvals_m);
  if (trace_G) {
    std::vector<double> g((size_t)m * m);
    HIPCHK(ctx, hipMemcpyAsync(g.data(), G.p, g.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    double s = 0;
    for (int i = 0; i < m; ++i) s += g[(size_t)i * m + i];
    *trace_G = s;
  }
  return 0;
}

}  // extern "C"

// normalize (src/utils.jl:33): (A .- mean(A, 1)) ./ std(A, 1) — column z-score
// with the sample std (n - 1 denominator), two passes over the column (mean,
// then the centred sum of squares), then the scaled write.  One wave per
// column of the column-major panel (contiguous in Julia's layout: coalesced);
// Y may alias X.
__global__ __launch_bounds__(256) void normalize_cols_kernel(const double *X, int64_t ldx, int T, int N, double *Y,
                                                             int64_t ldy) {
  const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= N) return;
  const double *x = X + (int64_t)c * ldx;
  double s = 0.0;
  for (int t = lane; t < T; t += 64) s += x[t];
  const double mu = wave_sum(s) / T;
  double v = 0.0;
  for (int t = lane; t < T; t += 64) { const double d = x[t] - mu; v = fma(d, d, v); }
  const double sd = sqrt(wave_sum(v) / (T - 1));
  double *y = Y + (int64_t)c * ldy;
  for (int t = lane; t < T; t += 64) y[t] = (x[t] - mu) / sd;
}

extern "C" int dfm_normalize_dev(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, double *out,
                                 int64_t ldo) {
  if (!ctx) return -1;
  if (!X || !out || T < 2 || N < 1 || ldx < T || ldo < T || T > INT32_MAX || N > INT32_MAX)
    return fail(ctx, -2, "dfm_normalize: bad arguments");
  DeviceShare gate(ctx->device);
  hipSetDevice(ctx->device);
  Scope sc(ctx, DFM_KC_MISC);
  hipLaunchKernelGGL(normalize_cols_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, ctx->stream, X, ldx, (int)T,
                     (int)N, out, ldo);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

extern "C" int dfm_normalize(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, double *out,
                             int64_t ldo) {
  if (!ctx) return -1;
  if (!X || !out || T < 2 || N < 1 || ldx < T || ldo < T) return fail(ctx, -2, "dfm_normalize: bad arguments");
  DeviceShare gate(ctx->device);
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  DevBuf<> d;
  HIPCHK(ctx, d.alloc((size_t)T * N));
  HIPCHK(ctx, hipMemcpy2DAsync(d.p, (size_t)T * 8, X, (size_t)ldx * 8, (size_t)T * 8, N, hipMemcpyHostToDevice, st));
  int rc = dfm_normalize_dev(ctx, d.p, T, N, T, d.p, T);
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpy2DAsync(out, (size_t)ldo * 8, d.p, (size_t)T * 8, (size_t)T * 8, N, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return 0;
}
