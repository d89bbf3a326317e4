// dfm_windows.hip — expanding / rolling window refits and their forecast step
// (dfm_windows, dfm_windows_dev, dfm_windows_forecast, dfm_windows_ex).
#include "dfm_host.h"

// ----------------------------------------------------------- expanding windows
// pseudo_out_of_sample_forecasts, refit part (src/utils.jl:54-72): for
// date_index = T-P+1..T (1-based) the model is refit on rows 1..date_index-1,
// i.e. window w = 0..P-1 uses the first n_w = T-P+w rows.  Every window is a
// masked replicate of the full panel (idx = identity, eta_t = 1{t < n_w}):
//  N > T : the window Gram is the leading n_w x n_w block of H = X X' (the
//          prefix-Gram identity) -> ONE Gram for all windows,
//          then the factored batched eigensolver (H . Z GEMMs);
//  T >= N: per-window Grams X_w' X_w from the masked fused-gather Gram kernel.
// Each window runs the IC sweep k = 1..kmax (the refit is the IC-sweep
// constructor, :53-66), picks r_w, and fits OLS+HC2 on [w F_r] over its rows.
__global__ void window_scale_kernel(const double *__restrict__ Uk, int T, int k, int Tfirst, int dn,
                                    double *__restrict__ F) {
  const int rep = blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)T * k) return;
  const int t = (int)(e / k), n = Tfirst + dn * rep;
  F[(int64_t)rep * T * k + e] = t < n ? sqrt((double)n) * Uk[(int64_t)rep * T * k + e] : 0.0;
}

// ---- forecast step of pseudo_out_of_sample_forecasts (src/utils.jl:54-72)
// with get_factors repaired (defect D4: the local rotation = L (L'L)^-1 of
// src/DynamicFactorModel.jl:126, L = block 1's full loadings).  For the
// window's first r columns rotation is L_j n / lambda_j (N > T: L'L =
// Lambda / n) or L_j / N (T >= N: L'L = N I), so with the new row
// x~ = (x_n - mean(X_w)) / std(X_w) (scalar moments of all window entries,
// Julia 0.3 mean/std of a matrix):
//   N > T : F_new_j = sum_{s<n} (x~ . x_s) F_j[s] / lambda_j,
//           x~ . x_s = (H[n][s] - mean * rowsum_s) / std   (H = X X', prefix Gram)
//   T >= N: F_new_j = x~ . V_j / sqrt(N)
// and the forecast is [w_n F_new] beta (src/DynamicFactorModel.jl:152-155).
__global__ void panel_row_sums_kernel(const double *__restrict__ P, int64_t ld, int N, double *__restrict__ rs,
                                      double *__restrict__ ss) {
  __shared__ double r1[256], r2[256];
  const int t = blockIdx.x, tid = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int c = tid; c < N; c += 256) { const double v = P[(int64_t)t * ld + c]; a += v; b = fma(v, v, b); }
  r1[tid] = a; r2[tid] = b;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { r1[tid] += r1[tid + o]; r2[tid] += r2[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) { rs[t] = r1[0]; ss[t] = r2[0]; }
}

__global__ void window_forecast_kernel(int orient, const double *__restrict__ Xp, int64_t ld, int T, int N, int n0,
                                       int len, int q, int kmax, const double *__restrict__ H, int64_t ldH,
                                       const double *__restrict__ F, const double *__restrict__ Uk,
                                       const double *__restrict__ lam, const double *__restrict__ rs,
                                       const double *__restrict__ ss, const int *__restrict__ kr,
                                       const double *__restrict__ coef, const double *__restrict__ y,
                                       const double *__restrict__ w, double *__restrict__ pred,
                                       double *__restrict__ truev) {
  __shared__ double red[256];
  __shared__ double smom[2];
  // the window's rows a0 .. n - 1 (expanding: a0 = 0; rolling: the last len
  // rows before n, relocated to rows 0 .. len - 1 of F)
  const int wi = blockIdx.x, tid = threadIdx.x, n = n0 + wi, a0 = len > 0 ? n - len : 0, r = kr[wi], d = q + kmax;
  if (tid == 0) {   // scalar moments of the window's (n - a0) x N entries (fixed order)
    double a = 0.0, b = 0.0;
    for (int s = a0; s < n; ++s) { a += rs[s]; b += ss[s]; }
    const double cnt = (double)(n - a0) * N, mu = a / cnt;
    smom[0] = mu;
    smom[1] = sqrt((b - cnt * mu * mu) / (cnt - 1.0));
  }
  __syncthreads();
  const double mu = smom[0], sd = smom[1];
  double yhat = 0.0;
  for (int j = 0; j < r; ++j) {
    double part = 0.0;
    if (orient == 0) {
      const double *Hn = H + (int64_t)n * ldH;
      const double *Fw = F + (int64_t)wi * T * kmax;
      for (int s = a0 + tid; s < n; s += 256)
        part = fma((Hn[s] - mu * rs[s]) / sd, Fw[(int64_t)(s - a0) * kmax + j], part);
    } else {
      const double *xn = Xp + (int64_t)n * ld;
      const double *V = Uk + (int64_t)wi * N * kmax;
      for (int c = tid; c < N; c += 256) part = fma((xn[c] - mu) / sd, V[(int64_t)c * kmax + j], part);
    }
    red[tid] = part;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    const double fnew = orient == 0 ? red[0] / lam[(int64_t)wi * kmax + j] : red[0] / sqrt((double)N);
    yhat = fma(fnew, coef[(int64_t)wi * d + q + j], yhat);
    __syncthreads();
  }
  if (tid == 0) {
    for (int i = 0; i < q; ++i) yhat = fma(w[(int64_t)i * T + n], coef[(int64_t)wi * d + i], yhat);
    pred[wi] = yhat;
    truev[wi] = y[n];
  }
}

// window wi as a masked "replicate" of the panel: rows t < n_w are panel rows
// a_w + t (expanding: a_w = 0, n_w = n0 + wi; rolling: n_w = len, a_w = n0 +
// wi - len), rows past n_w carry eta = 0
__global__ void window_draws_kernel(int T, int n0, int len, int32_t *__restrict__ idx, double *__restrict__ eta) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x, wi = blockIdx.y;
  if (t >= T) return;
  const int nw = len > 0 ? len : n0 + wi, aw = len > 0 ? n0 + wi - len : 0;
  idx[(int64_t)wi * T + t] = t < nw ? aw + t : t;
  eta[(int64_t)wi * T + t] = t < nw ? 1.0 : 0.0;
}
// The refit of each window (pseudo_out_of_sample_forecasts' model_args,
// src/utils.jl:64-65): len = 0 expanding windows (rows 0 .. T-P+w-1), len > 0
// rolling windows of len rows ending at T-P+w-1; r > 0 the workhorse
// constructor at fixed r (:28, clamped to ceil(m_w/2), :116-119), r = 0 the
// IC-sweep constructor (:53) by crit over k <= kmax_w, r < 0 the 3-arg default
// r = ceil(m_w/2) (D2); breaks: model_args' break_indices, the same rows for
// every (expanding) window.
struct WinSpec {
  int len = 0, r = 0, crit = -1, kmax = 0;
  const int64_t *breaks = nullptr;
  int nbreaks = 0;
};
static int windows_impl(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw, const double *X,
                        int64_t T64, int64_t N64, int64_t ldx, int P, const WinSpec &ws, int64_t *r_out,
                        double *V_out, double *crit_out, double *eig_out, double *coef_out, double *tstat_out,
                        double *pred_out, double *true_out, bool dev);
static int windows_breaks_impl(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw, const double *X,
                               int T, int N, int64_t ldx, int P, const WinSpec &ws, int K, int64_t *r_out,
                               double *V_out, double *crit_out, double *eig_out, double *coef_out,
                               double *tstat_out, double *pred_out, double *true_out);

extern "C" int dfm_windows(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw,
                           const double *X, int64_t T64, int64_t N64, int64_t ldx, int P, int crit,
                           int kmax, int64_t *r_out, double *V_out, double *crit_out, double *eig_out,
                           double *coef_out, double *tstat_out) {
  WinSpec ws;
  ws.crit = crit; ws.kmax = kmax;
  return windows_impl(ctx, y, w, q, ldw, X, T64, N64, ldx, P, ws, r_out, V_out, crit_out, eig_out,
                      coef_out, tstat_out, nullptr, nullptr, false);
}

extern "C" int dfm_windows_dev(dfm_ctx *ctx, const double *y_dev, const double *w_dev, int q, int64_t ldw,
                               const double *X_dev, int64_t T64, int64_t N64, int64_t ldx, int P, int crit,
                               int kmax, int64_t *r_out, double *V_out, double *crit_out, double *eig_out,
                               double *coef_out, double *tstat_out) {
  WinSpec ws;
  ws.crit = crit; ws.kmax = kmax;
  return windows_impl(ctx, y_dev, w_dev, q, ldw, X_dev, T64, N64, ldx, P, ws, r_out, V_out, crit_out,
                      eig_out, coef_out, tstat_out, nullptr, nullptr, true);
}

extern "C" int dfm_windows_forecast(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw,
                                    const double *X, int64_t T64, int64_t N64, int64_t ldx, int P, int crit,
                                    int kmax, int64_t *r_out, double *pred_out, double *true_out) {
  if (!pred_out || !true_out) return fail(ctx, -2, "dfm_windows_forecast: output pointers required");
  WinSpec ws;
  ws.crit = crit; ws.kmax = kmax;
  return windows_impl(ctx, y, w, q, ldw, X, T64, N64, ldx, P, ws, r_out, nullptr, nullptr, nullptr,
                      nullptr, nullptr, pred_out, true_out, false);
}

extern "C" int dfm_windows_ex(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw, const double *X,
                              int64_t T64, int64_t N64, int64_t ldx, int P, const dfm_window_spec *spec, int dev,
                              int64_t *r_out, double *V_out, double *crit_out, double *eig_out, double *coef_out,
                              double *tstat_out, double *pred_out, double *true_out) {
  if (!ctx) return -1;
  if (!spec) return fail(ctx, -2, "dfm_windows_ex: spec required");
  if (spec->kind != DFM_WIN_EXPANDING && spec->kind != DFM_WIN_ROLLING)
    return fail(ctx, -2, "dfm_windows_ex: unknown window kind %d", spec->kind);
  if ((pred_out == nullptr) != (true_out == nullptr))
    return fail(ctx, -2, "dfm_windows_ex: pred_out and true_out go together");
  WinSpec ws;
  ws.len = spec->kind == DFM_WIN_ROLLING ? spec->length : 0;
  if (spec->kind == DFM_WIN_ROLLING && spec->length < 2) return fail(ctx, -2, "dfm_windows_ex: rolling length < 2");
  ws.r = spec->r; ws.crit = spec->crit; ws.kmax = spec->kmax;
  ws.breaks = spec->breaks; ws.nbreaks = spec->nbreaks;
  return windows_impl(ctx, y, w, q, ldw, X, T64, N64, ldx, P, ws, r_out, V_out, crit_out, eig_out, coef_out,
                      tstat_out, pred_out, true_out, dev != 0);
}

// Masked explicit window Grams for N > T windows past the factored solver's
// T range: G_w[i][j] = eta_i eta_j H[idx_i][idx_j] (H = X X', the prefix Gram)
__global__ void window_gram_kernel(const double *__restrict__ H, int64_t ldH, const int32_t *__restrict__ idx,
                                   const double *__restrict__ eta, int T, double *__restrict__ G) {
  const int i = blockIdx.y, wi = blockIdx.z;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= T) return;
  const int32_t *ix = idx + (int64_t)wi * T;
  const double *et = eta + (int64_t)wi * T;
  const double ei = et[i], ej = et[j];
  G[((int64_t)wi * T + i) * T + j] = (ei != 0.0 && ej != 0.0) ? ei * ej * H[(int64_t)ix[i] * ldH + ix[j]] : 0.0;
}

static int windows_impl(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw, const double *X,
                        int64_t T64, int64_t N64, int64_t ldx, int P, const WinSpec &ws, int64_t *r_out,
                        double *V_out, double *crit_out, double *eig_out, double *coef_out, double *tstat_out,
                        double *pred_out, double *true_out, bool dev) {
  if (!ctx) return -1;
  DeviceShare gate(ctx->device);
  const int T = (int)T64, N = (int)N64;
  if (!y || !X || T < 4 || N < 1 || ldx < T || P < 1 || T - P < 2 || q < 0 || (q > 0 && (!w || ldw < T)) ||
      !r_out)
    return fail(ctx, -2, "dfm_windows: bad arguments");
  const int crit = ws.crit, len = ws.len;
  if (crit < -1 || crit > 6 || (ws.r == 0 && crit < 0))
    return fail(ctx, -31, "dfm_windows: unknown criterion %d (the IC sweep needs one)", crit);
  const bool pcp = crit >= 0 && crit <= 2;
  const int n0 = T - P;
  if (len > n0) return fail(ctx, -2, "dfm_windows: rolling length %d exceeds the %d rows before the first window", len, n0);
  if (ws.nbreaks < 0 || (ws.nbreaks > 0 && !ws.breaks)) return fail(ctx, -2, "dfm_windows: bad break list");
  if (ws.nbreaks > 0 && len > 0)
    return fail(ctx, -2, "dfm_windows: break_indices apply to expanding windows (the same rows in every refit, "
                         "src/utils.jl:64)");
  // window wi: rows aw(wi) .. aw(wi) + nw(wi) - 1 (relocated to rows 0 .. nw - 1)
  auto nw = [&](int wi) { return len > 0 ? len : n0 + wi; };
  auto aw = [&](int wi) { return len > 0 ? n0 + wi - len : 0; };
  const int orient = len > 0 ? (N > len ? 0 : 1) : (N > T ? 0 : 1);
  if (orient == 1 && len == 0 && N > n0)
    return fail(ctx, -2, "dfm_windows: windows straddle the T >= N / N > T branches");
  // window w's factor count: the sweep k = 1..kmax_w, kmax_w = ceil(m_w / 2)
  // (the IC-sweep constructor's default, src/DynamicFactorModel.jl:54) capped
  // by the caller's kmax (D11); fixed r clamped to ceil(m_w/2) (:116-119);
  // the 3-arg default ceil(m_w/2) (D2); m_w = min(n_w, N)
  auto kd_w = [&](int wi) { return (std::min(nw(wi), N) + 1) / 2; };
  auto kmax_w = [&](int wi) {
    const int kd = kd_w(wi);
    if (ws.r > 0) return std::min(ws.r, kd);
    if (ws.r < 0) return kd;
    return ws.kmax > 0 ? std::min(ws.kmax, kd) : kd;
  };
  int kmax = kmax_w(P - 1);   // the widest window's: row stride of eig_out / coef_out
  if (ws.nbreaks > 0)
    return windows_breaks_impl(ctx, y, w, q, ldw, X, T, N, ldx, P, ws, kmax, r_out, V_out, crit_out, eig_out,
                               coef_out, tstat_out, pred_out, true_out);
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const int m = orient == 0 ? T : N;
  // kmax beyond the subspace block (or a design wider than 32): each window's
  // sweep reads its full spectrum, the r_w eigenvectors come from the dense
  // batched eigensolver (diagonal blocks of H zero-padded to T x T for N > T)
  const int p = eig_block_p(m, kmax, ctx->block);
  const bool wide = p > 32 || p < kmax || q + kmax > 32;
  if ((pcp || wide) && m > std::min(spectrum_any_max(), dense_eig_max()))
    return fail(ctx, -31, "dfm_windows: PCp / kmax > 24 need each window's full spectrum: supported for "
                          "min(T,N) <= %d", std::min(spectrum_any_max(), dense_eig_max()));
  const int Pb = (p <= 16 || wide) ? 16 : 32;
  // N > T past the factored solver's T range: per-window masked Grams, explicit-Gram solver
  const bool explicit_gram = orient == 0 && !wide && T > fact_t_max();
  DevPanel dp;
  int rc = upload_panel(ctx, X, T, N, ldx, dp, dev);
  if (rc) return rc;
  std::vector<int> hTn(P), hkr(P), hR0(P);
  // scratch: bump allocation from the context's arena (sized by the largest
  // earlier call; stream-ordered reuse), overflow from the stream-ordered pool
  if (ctx->warena_need > ctx->warena_cap) {
    hipStreamSynchronize(st);
    hipFree(ctx->warena);
    ctx->warena = nullptr;
    ctx->warena_cap = 0;
    if (hipMalloc((void **)&ctx->warena, ctx->warena_need) == hipSuccess) ctx->warena_cap = ctx->warena_need;
  }
  std::vector<void *> frees;
  size_t aoff = 0, aneed = 0;
  auto dal = [&](size_t bytes) -> void * {
    const size_t b = (std::max<size_t>(bytes, 8) + 255) & ~size_t(255);
    aneed += b;
    if (aoff + b <= ctx->warena_cap) { void *ptr = ctx->warena + aoff; aoff += b; return ptr; }
    void *ptr = nullptr;
    if (stream_malloc(&ptr, b, st) != hipSuccess) return nullptr;
    frees.push_back(ptr);
    return ptr;
  };
  struct Freer {
    std::vector<void *> &v; hipStream_t s; dfm_ctx *c; size_t &need;
    ~Freer() { for (void *x : v) hipFreeAsync(x, s); c->warena_need = std::max(c->warena_need, need); }
  } freer{frees, st, ctx, aneed};
  // window w as a "replicate" of the panel: relocated rows, row mask t < n_w
  int32_t *didx = (int32_t *)dal((size_t)P * T * 4);
  double *deta = (double *)dal((size_t)P * T * 8);
  double *dy = (double *)dal((size_t)T * 8), *dw = (double *)dal((size_t)T * std::max(q, 1) * 8);
  double *tr = (double *)dal((size_t)P * 8);
  int *stt = (int *)dal((size_t)P * 4), *ost = (int *)dal((size_t)P * 4);
  int *dTn = (int *)dal((size_t)P * 4), *dkr = (int *)dal((size_t)P * 4), *dR0 = (int *)dal((size_t)P * 4);
  if (!didx || !deta || !dy || !dw || !tr || !stt || !ost || !dTn || !dkr || !dR0)
    return fail(ctx, 1002, "dfm_windows: out of device memory");
  hipLaunchKernelGGL(window_draws_kernel, dim3((unsigned)((T + 255) / 256), P), dim3(256), 0, st, T, n0, len, didx,
                     deta);
  const hipMemcpyKind yk = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HIPCHK(ctx, hipMemcpyAsync(dy, y, (size_t)T * 8, yk, st));
  if (q > 0) HIPCHK(ctx, hipMemcpy2DAsync(dw, (size_t)T * 8, w, (size_t)ldw * 8, (size_t)T * 8, q, yk, st));
  PanelSrc msrc{nullptr, dp.P, didx, deta, dp.ld, T};   // window w = its rows of X, relocated
  // ---- the windows' Grams: N > T one Gram H = X X' (every window's Gram is a
  // diagonal block of it); T >= N per-window G
  double *H = nullptr, *G = nullptr;
  int64_t ldH = 0;
  if (orient == 0) {
    ldH = round_up(T, 16);
    H = (double *)dal((size_t)T * ldH * 8);
    if (!H) return fail(ctx, 1002, "dfm_windows: out of device memory");
    HIPCHK(ctx, hipMemsetAsync(H, 0, (size_t)T * ldH * 8, st));
    PanelSrc es{nullptr, dp.P, nullptr, nullptr, dp.ld, 0};
    Scope sc(ctx, DFM_KC_GRAM);
    HIPCHK(ctx, launch_gram(0, es, T, N, T, H, ldH, 0, 1, st));   // ONE Gram for every window
  } else {
    G = (double *)dal((size_t)P * N * N * 8);
    if (!G) return fail(ctx, 1002, "dfm_windows: out of device memory");
    Scope sc(ctx, DFM_KC_GRAM);
    HIPCHK(ctx, launch_gram(1, msrc, N, T, T, G, N, (int64_t)N * N, P, st));
  }
  // N > T windows as diagonal blocks of H: expanding = leading (n0 + w) blocks,
  // rolling = the len x len block at row/column n0 + w - len
  const double *Hb = H ? (len > 0 ? H + (int64_t)(n0 - len) * (ldH + 1) : H) : nullptr;
  const int64_t sHb = len > 0 ? ldH + 1 : 0;
  const int mv0 = len > 0 ? len : n0, dmv = len > 0 ? 0 : 1;
  // ---- full spectra (PCp's sigma^2, and the whole sweep when wide)
  double *pev = nullptr;   // P x pst
  const int pst = orient == 0 ? (len > 0 ? len : T - 1) : N;
  if (pcp || wide) {
    pev = (double *)dal((size_t)P * pst * 8);
    double *pwk = spectrum_work(pst, P) > 0 ? (double *)dal((size_t)spectrum_work(pst, P) * 8) : nullptr;
    if (!pev || (spectrum_work(pst, P) > 0 && !pwk)) return fail(ctx, 1002, "dfm_windows: out of device memory");
    Scope sc(ctx, DFM_KC_EIG_OTHER);
    if (orient == 0) HIPCHK(ctx, launch_spectrum_var(Hb, ldH, sHb, pst, mv0, dmv, P, pev, pwk, st));
    else HIPCHK(ctx, launch_spectrum(G, N, (int64_t)N * N, N, P, pev, pwk, st));
  }
  std::vector<double> hev;
  if (pev) {
    hev.resize((size_t)P * pst);
    HIPCHK(ctx, hipMemcpyAsync(hev.data(), pev, hev.size() * 8, hipMemcpyDeviceToHost, st));
  }
  // ---- narrow: top-kmax pairs of every window by the batched subspace solver
  int kv = kmax;   // eigenvectors kept per window (stride of F, Uk, lam, coef)
  double *lam = nullptr, *Uk = nullptr, *F = nullptr;
  std::vector<double> hl((size_t)P * kmax), ht(P);
  if (!wide) {
    lam = (double *)dal((size_t)P * kmax * 8); Uk = (double *)dal((size_t)P * m * kmax * 8);
    F = (double *)dal((size_t)P * T * kmax * 8);
    if (!lam || !Uk || !F) return fail(ctx, 1002, "dfm_windows: out of device memory");
    EigArgs ea;   // cold starts; each branch adds its batch, workspace and outputs
    ea.k = kmax; ea.p = p;
    ea.warm = nullptr; ea.kw = 0;
    ea.tol = ctx->tol; ea.maxit = ctx->maxit; ea.poll = ctx->poll;
    ea.st = st; ea.tf = timer_cb; ea.tctx = ctx;
    if (orient == 0 && !explicit_gram) {
      char *ews = (char *)dal(eig_workspace_bytes_padded(m, P, Pb, ctx->maxit));
      double *zero = (double *)dal((size_t)T * 8), *hd = (double *)dal((size_t)T * 8);
      char *fws = (char *)dal(fact_workspace_bytes(T, P, Pb));
      int *off = (int *)dal((size_t)P * (T + 1) * 4), *lst = (int *)dal((size_t)P * T * 4);
      if (!ews || !zero || !hd || !fws || !off || !lst) return fail(ctx, 1002, "dfm_windows: out of device memory");
      HIPCHK(ctx, hipMemsetAsync(zero, 0, (size_t)T * 8, st));
      rc = fact_precompute(dp.P, dp.ld, T, N, 0, nullptr, nullptr, H, ldH, zero, zero, zero, hd, st);
      if (rc) return fail(ctx, rc, "precompute");
      HIPCHK(ctx, hipMemsetAsync(zero, 0, (size_t)T * 8, st));
      FactBase fb{T, 0, ldH, zero, zero, zero, H, zero, hd};
      ea.nb = P; ea.ws = ews;
      ea.lam = lam; ea.Uk = Uk; ea.trace_out = tr; ea.status = stt;
      FactArgs fa;
      fa.idx = didx; fa.eta = deta; fa.fws = fws;
      fa.off = off; fa.lst = lst;
      fa.pb = ctx_poll(ctx);
      rc = eig_run_factored(fb, ea, fa);
      if (rc) return fail(ctx, rc > 0 ? rc : -21, "eigensolver failed (%d)", rc);
    } else if (orient == 0) {
      // T > the factored solver's range: the windows' masked T x T Grams in
      // chunks (<= 2 GB), each chunk by the explicit-Gram subspace solver
      const int64_t per = (int64_t)T * T * 8;
      const int Pc = (int)std::max<int64_t>(1, std::min<int64_t>(P, (int64_t)(2LL << 30) / per));
      double *Gc = (double *)dal((size_t)Pc * per);
      char *ews = (char *)dal(eig_workspace_bytes_padded(m, Pc, Pb, ctx->maxit));
      if (!Gc || !ews) return fail(ctx, 1002, "dfm_windows: out of device memory");
      for (int c0 = 0; c0 < P; c0 += Pc) {
        const int pc = std::min(Pc, P - c0);
        {
          Scope sc(ctx, DFM_KC_GRAM);
          hipLaunchKernelGGL(window_gram_kernel, dim3((unsigned)((T + 255) / 256), T, pc), dim3(256), 0, st, H, ldH,
                             didx + (size_t)c0 * T, deta + (size_t)c0 * T, T, Gc);
          HIPCHK(ctx, hipGetLastError());
        }
        ea.nb = pc; ea.ws = ews;
        ea.lam = lam + (size_t)c0 * kmax; ea.Uk = Uk + (size_t)c0 * T * kmax;
        ea.trace_out = tr + c0; ea.status = stt + c0;
        rc = eig_run(Gc, T, (int64_t)T * T, T, ea, nullptr, 0);
        if (rc) return fail(ctx, rc > 0 ? rc : -21, "eigensolver failed (%d)", rc);
      }
    } else {
      char *ews = (char *)dal(eig_workspace_bytes_padded(m, P, Pb, ctx->maxit));
      double *Ld = (double *)dal((size_t)P * N * kmax * 8);
      if (!ews || !Ld) return fail(ctx, 1002, "dfm_windows: out of device memory");
      ea.nb = P; ea.ws = ews;
      ea.lam = lam; ea.Uk = Uk; ea.trace_out = tr; ea.status = stt;
      rc = eig_run(G, N, (int64_t)N * N, N, ea, nullptr, 0);
      if (rc) return fail(ctx, rc > 0 ? rc : -21, "eigensolver failed (%d)", rc);
      Scope sc(ctx, DFM_KC_FACTORS);
      launch_factors(1, msrc, T, N, kmax, P, Uk, F, Ld, nullptr, st);
    }
    if (orient == 0) {
      Scope sc(ctx, DFM_KC_FACTORS);
      hipLaunchKernelGGL(window_scale_kernel, dim3((unsigned)(((int64_t)T * kmax + 255) / 256), P), dim3(256), 0,
                         st, Uk, T, kmax, mv0, dmv, F);
    }
    std::vector<int> hs(P);
    HIPCHK(ctx, hipMemcpyAsync(hl.data(), lam, hl.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(ht.data(), tr, (size_t)P * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(hs.data(), stt, (size_t)P * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int wi = 0; wi < P; ++wi)
      if (hs[wi]) return fail(ctx, 2, "eigensolver did not converge for window %d", wi);
  } else {
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int wi = 0; wi < P; ++wi) {   // eigenvalues and trace from the window's spectrum
      ht[wi] = tail_sum(&hev[(size_t)wi * pst], orient == 0 ? nw(wi) : N, 0);
      for (int j = 0; j < kmax; ++j) hl[(size_t)wi * kmax + j] = hev[(size_t)wi * pst + j];
    }
  }
  // ---- per window on the host (arithmetic only): the IC sweep and r_w, or
  // the fixed / default r_w and its criterion value
  std::vector<double> ic(7 * (size_t)kmax);
  for (int wi = 0; wi < P; ++wi) {
    const int n = nw(wi);
    double s2 = NAN;
    // src/criteria.jl:18: V(ceil(m_w/2)) of the window's unrestricted fit = spectral tail
    if (pcp) s2 = sigma2_tail(&hev[(size_t)wi * pst], std::min(n, N), (double)N * n);
    const int kw = kmax_w(wi);
    int rsel = kw;
    double cv = NAN;
    if (ws.r == 0) {
      dfm_ic_sweep(&hl[(size_t)wi * kmax], kw, kw, ht[wi], n, N, s2, ic.data());
      rsel = first_argmin(&ic[(size_t)crit * kw], kw);
      cv = ic[(size_t)crit * kw + rsel - 1];
    } else if (crit >= 0) {   // the workhorse constructor's criterion at r_w (:50)
      dfm_ic_sweep(&hl[(size_t)wi * kmax], kw, kw, ht[wi], n, N, s2, ic.data());
      cv = ic[(size_t)crit * kw + kw - 1];
    }
    hTn[wi] = n;
    hkr[wi] = rsel;
    hR0[wi] = aw(wi);
    r_out[wi] = rsel;
    if (crit_out) crit_out[wi] = cv;
    if (V_out) {
      double sacc = ht[wi];
      for (int j = 0; j < rsel; ++j) sacc -= hl[(size_t)wi * kmax + j];
      V_out[wi] = sacc / ((double)N * n);
    }
  }
  if (eig_out) std::copy(hl.begin(), hl.end(), eig_out);
  HIPCHK(ctx, hipMemcpyAsync(dTn, hTn.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(dkr, hkr.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(dR0, hR0.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
  // ---- wide: the r_w eigenvectors (kv = max_w r_w) and factors of every window
  if (wide) {
    kv = *std::max_element(hkr.begin(), hkr.end());
    lam = (double *)dal((size_t)P * kv * 8); Uk = (double *)dal((size_t)P * m * kv * 8);
    F = (double *)dal((size_t)P * T * kv * 8);
    double *dwk = (double *)dal((size_t)P * dense_eig_work(m, kv) * 8);
    if (!lam || !Uk || !F || !dwk) return fail(ctx, 1002, "dfm_windows: out of device memory");
    hipError_t e;
    {
      Scope sc(ctx, DFM_KC_EIG_OTHER);
      e = orient == 0 ? launch_dense_eig_batched(Hb, ldH, sHb, T, mv0, dmv, P, kv, lam, Uk, tr, stt, dwk, st)
                      : launch_dense_eig_batched(G, N, (int64_t)N * N, N, N, 0, P, kv, lam, Uk, tr, stt, dwk, st);
    }
    if (e != hipSuccess) return fail(ctx, 1000 + (int)e, "dense eigensolver: %s", hipGetErrorString(e));
    Scope sc(ctx, DFM_KC_FACTORS);
    if (orient == 0) {
      hipLaunchKernelGGL(window_scale_kernel, dim3((unsigned)(((int64_t)T * kv + 255) / 256), P), dim3(256), 0, st,
                         Uk, T, kv, mv0, dmv, F);
    } else {
      double *Ld = (double *)dal((size_t)P * N * kv * 8);
      if (!Ld) return fail(ctx, 1002, "dfm_windows: out of device memory");
      if (kv <= 32) {
        launch_factors(1, msrc, T, N, kv, P, Uk, F, Ld, nullptr, st);
      } else {
        double *Xw = (double *)dal((size_t)P * T * dp.ld * 8);
        if (!Xw) return fail(ctx, 1002, "dfm_windows: out of device memory");
        HIPCHK(ctx, launch_materialize(msrc, T, N, dp.ld, P, Xw, st));
        if (launch_factors_wide(1, Xw, dp.ld, T, N, kv, Uk, F, Ld, nullptr, st, (double)T, P, (int64_t)T * dp.ld,
                                (int64_t)T * kv))
          return fail(ctx, 1001, "factor kernels failed");
      }
    }
  }
  // ---- OLS + HC2 of every window on [w F_{r_w}] over its rows
  const int dv = q + kv;
  double *coef = (double *)dal((size_t)P * dv * 8), *tst = (double *)dal((size_t)P * dv * 8);
  if (!coef || !tst) return fail(ctx, 1002, "dfm_windows: out of device memory");
  if (dv <= 32) {
    Scope sc(ctx, DFM_KC_OLS);
    launch_ols(P, st, dy, dw, q, F, T, kv, dTn, dkr, coef, tst, nullptr, nullptr, ost, len > 0 ? dR0 : nullptr);
  } else {   // per window: its own width q + r_w
    const int dmax = q + kv;
    double *owk = (double *)dal((size_t)ols_wide_work(T, dmax) * 8);
    if (!owk) return fail(ctx, 1002, "dfm_windows: out of device memory");
    Scope sc(ctx, DFM_KC_OLS);
    for (int wi = 0; wi < P; ++wi)
      HIPCHK(ctx, launch_ols_wide_batched(1, dy + hR0[wi], dw + hR0[wi], q, F + (size_t)wi * T * kv, T, kv, hkr[wi],
                                          dTn + wi, coef + (size_t)wi * dv, tst + (size_t)wi * dv, nullptr, nullptr,
                                          ost + wi, owk, st));
  }
  {
    std::vector<int> ho(P);
    HIPCHK(ctx, hipMemcpyAsync(ho.data(), ost, (size_t)P * 4, hipMemcpyDeviceToHost, st));
    std::vector<int> hs2(P, 0);
    if (wide) HIPCHK(ctx, hipMemcpyAsync(hs2.data(), stt, (size_t)P * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int wi = 0; wi < P; ++wi) {
      if (hs2[wi]) return fail(ctx, 2, "dense eigensolver: window %d lost orthogonality", wi);
      if (ho[wi]) return fail(ctx, 3, "singular design matrix in window %d", wi);
    }
  }
  // outputs keep the q + kmax row stride of the header (NaN past q + r_w)
  auto restride = [&](const double *dsrc, double *out) -> int {
    std::vector<double> h((size_t)P * dv);
    HIPCHK(ctx, hipMemcpyAsync(h.data(), dsrc, h.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const int dk = q + kmax;
    for (int wi = 0; wi < P; ++wi)
      for (int c = 0; c < dk; ++c)
        out[(size_t)wi * dk + c] = (c < dv && c < q + hkr[wi]) ? h[(size_t)wi * dv + c] : NAN;
    return 0;
  };
  if (coef_out && (rc = restride(coef, coef_out))) return rc;
  if (tstat_out && (rc = restride(tst, tstat_out))) return rc;
  if (pred_out) {   // forecast step: predict row n = n0 + w from window w's fit
    double *rs = (double *)dal((size_t)T * 8), *ss = (double *)dal((size_t)T * 8);
    double *dp_ = (double *)dal((size_t)P * 8), *dt_ = (double *)dal((size_t)P * 8);
    if (!rs || !ss || !dp_ || !dt_) return fail(ctx, 1002, "dfm_windows: out of device memory");
    Scope sc(ctx, DFM_KC_MISC);
    hipLaunchKernelGGL(panel_row_sums_kernel, dim3(T), dim3(256), 0, st, dp.P, dp.ld, N, rs, ss);
    hipLaunchKernelGGL(window_forecast_kernel, dim3(P), dim3(256), 0, st, orient, dp.P, dp.ld, T, N, n0, len, q, kv,
                       H, ldH, F, Uk, lam, rs, ss, dkr, coef, dy, dw, dp_, dt_);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(pred_out, dp_, (size_t)P * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(true_out, dt_, (size_t)P * 8, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(ctx, hipStreamSynchronize(st));
  return 0;
}

// Expanding windows of a model with structural breaks (model_args'
// break_indices, src/utils.jl:64 -> src/DynamicFactorModel.jl:73, :98): each
// window is the break-aware fit of dfm_model_fit_breaks on its leading rows
// (per-block PCA with the window's full-sample T, N, D7), read back, and —
// for the forecast step — dfm_predict on the next row.  X, y, w host or
// device memory (the fit copies with hipMemcpyDefault).
static int windows_breaks_impl(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw, const double *X,
                               int T, int N, int64_t ldx, int P, const WinSpec &ws, int K, int64_t *r_out,
                               double *V_out, double *crit_out, double *eig_out, double *coef_out,
                               double *tstat_out, double *pred_out, double *true_out) {
  const int n0 = T - P;
  for (int j = 0; j < ws.nbreaks; ++j)
    if (ws.breaks[j] >= n0)
      return fail(ctx, -9, "dfm_windows: break row %lld is not inside the first window (%d rows)",
                  (long long)ws.breaks[j], n0);
  for (int wi = 0; wi < P; ++wi) {
    const int n = n0 + wi;
    const int kd = (std::min(n, N) + 1) / 2;
    const int rarg = ws.r > 0 ? ws.r : (ws.r < 0 ? kd : 0);
    dfm_model *M = nullptr;
    int rc = dfm_model_fit_breaks(ctx, y, w, q, ldw, X, n, N, ldx, rarg, ws.crit, ws.kmax, ws.breaks, ws.nbreaks,
                                  &M);
    if (rc) return rc;
    struct Kill { dfm_model *m; ~Kill() { dfm_model_destroy(m); } } kill{M};
    int64_t r = 0, kmx = 0, ne = 0;
    double V = 0, cv = 0, tr = 0;
    dfm_model_scalars(M, &r, &V, &cv, &tr);
    dfm_model_dims(M, &r, &kmx, &ne);
    const int d = q + (int)r;
    std::vector<double> ev(ne), co(d), ts(d);
    if ((rc = dfm_model_read(M, ev.data(), co.data(), ts.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                             nullptr)))
      return rc;
    r_out[wi] = r;
    if (V_out) V_out[wi] = V;
    if (crit_out) crit_out[wi] = ws.crit >= 0 ? cv : NAN;
    if (eig_out)
      for (int j = 0; j < K; ++j) eig_out[(size_t)wi * K + j] = j < ne ? ev[j] : NAN;
    const int dk = q + K;
    for (int c = 0; c < dk; ++c) {
      if (coef_out) coef_out[(size_t)wi * dk + c] = c < d ? co[c] : NAN;
      if (tstat_out) tstat_out[(size_t)wi * dk + c] = c < d ? ts[c] : NAN;
    }
    if (pred_out) {   // predict row n from this window's fit (D4-repaired get_factors)
      if ((rc = dfm_predict(M, 1, q > 0 ? w + n : nullptr, ldw, X + n, ldx, pred_out + wi))) return rc;
      HIPCHK(ctx, hipMemcpy(true_out + wi, y + n, 8, hipMemcpyDefault));
    }
  }
  return 0;
}
