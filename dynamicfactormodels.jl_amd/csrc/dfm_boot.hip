// dfm_boot.hip — the bootstrap: dfm_bootstrap(_dev), its lanes (parts of a
// small job on their own contexts / streams / host threads) and
// dfm_bootstrap_multi (shards over several models, typically one per GPU).
#include "dfm_host.h"

#ifdef DFM_DEBUG_MEM
// Debug build: a device buffer inside 64 KB guard bands of 0xA5 bytes, its
// body poisoned (0xFF).  check() reports guard bytes that changed (offsets
// relative to the body: negative = the front band) and, given the host copy
// the body was loaded from, body rows that no longer match it (row = `rowb`
// bytes: a replicate's draws).
struct GuardBuf {
  static constexpr size_t kG = 65536;
  char *raw = nullptr;
  void *p = nullptr;
  size_t n = 0;
  hipError_t alloc(size_t bytes) {
    n = std::max<size_t>(bytes, 8);
    hipError_t e = hipMalloc((void **)&raw, n + 2 * kG);
    if (e != hipSuccess) return e;
    (void)hipMemset(raw, 0xA5, kG);
    (void)hipMemset(raw + kG, 0xFF, n);
    (void)hipMemset(raw + kG + n, 0xA5, kG);
    (void)hipDeviceSynchronize();
    p = raw + kG;
    return hipSuccess;
  }
  int check(const char *name, const void *host, int64_t rowb) {
    if (!raw) return 0;
    std::vector<unsigned char> h(n + 2 * kG);
    (void)hipDeviceSynchronize();
    (void)hipMemcpy(h.data(), raw, h.size(), hipMemcpyDeviceToHost);
    int bad = 0;
    int64_t first = 0, last = 0, cnt = 0;
    for (size_t i = 0; i < h.size(); ++i) {
      if (i >= kG && i < kG + n) continue;
      if (h[i] != 0xA5) {
        const int64_t o = (int64_t)i - (int64_t)kG;
        if (!cnt) first = o;
        last = o;
        ++cnt;
      }
    }
    if (cnt) {
      fprintf(stderr, "[dfm debug] %s: %lld guard bytes changed, body offsets %lld .. %lld (body %zu bytes)\n", name,
              (long long)cnt, (long long)first, (long long)last, n);
      ++bad;
    }
    if (host && rowb > 0) {
      const unsigned char *b = h.data() + kG, *q = (const unsigned char *)host;
      int64_t nrow = (int64_t)n / rowb, rbad = 0, r0 = -1, r1 = -1;
      for (int64_t r = 0; r < nrow; ++r)
        if (memcmp(b + r * rowb, q + r * rowb, (size_t)rowb) != 0) {
          if (r0 < 0) r0 = r;
          r1 = r;
          ++rbad;
        }
      if (rbad) {
        fprintf(stderr, "[dfm debug] %s: %lld of %lld rows changed on the device during the call (rows %lld .. %lld)\n",
                name, (long long)rbad, (long long)nrow, (long long)r0, (long long)r1);
        ++bad;
      }
    }
    hipFree(raw);
    raw = nullptr;
    return bad;
  }
  ~GuardBuf() { if (raw) hipFree(raw); }
};
#endif

#if defined(DFM_DEBUG_MEM) || defined(DFM_LANE_SKEW_AB)
// DFM_LANE_SKEW_US (debug build): hold one bootstrap lane back this long on the
// device (> 0: the second lane, < 0: the caller's), so a cross-lane ordering
// hazard shows up deterministically instead of at the mercy of scheduling
__global__ void dbg_spin_kernel(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
#ifdef DFM_DEBUG_MEM
static int dbg_lane_skew_us() {
  const char *e = getenv("DFM_LANE_SKEW_US");
  return e ? atoi(e) : 0;
}
#else
// (A/B builds only: the debug build's lane skew as a timing experiment, no poisoning)
static int dbg_lane_skew_us() {
  static const int v = [] { const char *e = getenv("DFM_LANE_SKEW_US"); return e ? atoi(e) : 0; }();
  return v;
}
#endif
#endif

static void note_iters(dfm_ctx *ctx) {
  ctx->eig_batches++;
  ctx->eig_iters += g_last_iters;
  ctx->eig_iters_max = std::max<int64_t>(ctx->eig_iters_max, g_last_iters);
  ctx->rep_iters += g_last_rep_iters;
  ctx->gemm_products += g_last_gemm_products;
  ctx->gemm_products_f32 += g_last_gemm_products_f32;
  ctx->gemm_products_split_last += g_last_gemm_products_split_last;
  ctx->gemm_products_split3 += g_last_gemm_products_split3;
}

// Per-batch device workspace layout for the bootstrap.
struct BootWs {
  double *G, *lam, *Uk, *trace, *F, *L, *colssr, *coef, *tstat, *blam, *btr, *gwk;
  int *status, *ost, *off, *lst;
  char *eig, *chow, *fact, *fload;
  size_t eig_bytes, chow_bytes, fact_bytes, fload_bytes;
};
static size_t boot_ws_bytes(const dfm_model *M, int nb, int P, int maxit, bool chow, bool fact, BootWs *o,
                            char *base) {
  const int m = M->m, r = M->r, T = M->T, N = M->N, d = M->q + M->r;
  size_t off = 0;
  auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += (bytes + 255) & ~size_t(255); return p; };
  BootWs w{};
  w.G = (double *)take(fact ? 8 : (size_t)nb * m * m * 8);
  w.lam = (double *)take((size_t)nb * r * 8);
  w.Uk = (double *)take((size_t)nb * m * r * 8);
  w.trace = (double *)take((size_t)nb * 8);
  w.F = (double *)take((size_t)nb * T * r * 8);
  w.L = (double *)take((size_t)M->nblk * nb * N * r * 8);   // block j at w.L + j nb N r
  w.colssr = (double *)take((size_t)nb * N * 8);
  w.coef = (double *)take((size_t)nb * d * 8);
  w.tstat = (double *)take((size_t)nb * d * 8);
  w.blam = (double *)take(M->nblk > 1 ? (size_t)nb * r * 8 : 8);   // one break block's lambdas
  w.btr = (double *)take(M->nblk > 1 ? (size_t)nb * 8 : 8);
  w.status = (int *)take((size_t)nb * 4);
  w.ost = (int *)take((size_t)nb * 4);
  w.eig_bytes = eig_workspace_bytes_padded(m, nb, P, maxit);
  w.eig = take(w.eig_bytes);
  w.chow_bytes = chow ? chow_workspace_bytes(T, N, r, nb) : 0;
  w.chow = take(w.chow_bytes);
  w.fact_bytes = fact ? fact_workspace_bytes(T, nb, P) : 0;
  w.fact = take(w.fact_bytes);
  w.fload_bytes = fact ? fact_loadings_bytes(T, N, r, nb) : 0;
  w.fload = take(w.fload_bytes);
  w.off = (int *)take(fact ? (size_t)nb * (T + 1) * 4 : 4);
  w.lst = (int *)take(fact ? (size_t)nb * T * 4 : 4);
  w.gwk = (double *)take(use_gram_wk(M) ? gram_wk_work(T, N, r, nb) * 8 : 8);
  if (o) *o = w;
  return off;
}

// (extern "C": the unmangled names these two have in every kernel trace)
extern "C" __global__ void or_flag_kernel(const int *s, int nb, int *flag, int bit) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb && s[i]) atomicOr(flag, bit);
}

extern "C" __global__ void or_status_kernel(const int *s1, const int *s2, int nb, int *flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nb) {
    if (s1[i]) atomicOr(flag, 1);
    if (s2[i]) atomicOr(flag, 2);
  }
}

static int bootstrap_one(dfm_model *M, int kind, int64_t B, const int32_t *idx, const double *eta,
                         const dfm_stat *stats, int ns, double *out);

// Small jobs (a rank's shard of a multi-GPU bootstrap: C3 at 8 GPUs is 1 250
// replicates per device; C2's 999) leave the chip part-idle: the
// per-replicate passes (y2, Rayleigh-Ritz, ap2, Chebyshev, Chow: one
// workgroup or one wave per replicate) run ~1 round of the resident slots or
// less, and every launch gap and convergence poll is exposed.  Such jobs run
// as lanes — contiguous parts of the replicate range on their own streams,
// each driven by its own host thread — so one lane's latency-bound passes
// overlap another's GEMMs (measured at C3 with two Python-driven contexts:
// 1 250 replicates 4.12 -> 3.76 ms, 2 500: 6.96 -> 6.55 ms; 9 999 gains < 2 %
// and stays one lane, keeping its kernels' timings solo).  Every kernel is
// batch-invariant (a replicate's result never depends on its batch), so the
// rows are bit-identical to one lane (tests/test_gpu_multi.py).
constexpr int64_t kLaneMin = 512, kLaneMax = 6000;
static int lane_count(const dfm_model *M, int64_t B, const dfm_stat *stats, int ns) {
  // DFM_NO_LANES=1 (diagnostic): one lane, so a kernel trace shows solo durations;
  // DFM_LANES=n (A/B): n lanes (1..4) wherever lanes apply
  static const bool no_lanes = [] { const char *e = getenv("DFM_NO_LANES"); return e && atoi(e) != 0; }();
  static const int forced = [] { const char *e = getenv("DFM_LANES"); return e ? atoi(e) : 0; }();
  if (no_lanes) return 1;
  if (M->is_lane || M->batch != 0 || B < kLaneMin || B > kLaneMax || ns < 0 || (ns > 0 && !stats)) return 1;
  const int p = eig_block_p(M->m, M->r, M->ctx->block);
  if (p > 32 || p < M->r) return 1;
  for (int i = 0; i < ns; ++i)
    if (stats[i].kind < 0 || stats[i].kind > DFM_STAT_SUPWALD_ALL) return 1;
  if (M->r > 16) return 1;   // the subspace solver's paths (not the dense / GEMM-built wide ones)
  if (forced > 0) return std::min(forced, dfm_model::kMaxLanes);
  return 2;
}

static int bootstrap_lanes(dfm_model *M, int nl, int kind, int64_t B, const int32_t *idx, const double *eta,
                           const dfm_stat *stats, int ns, double *out) {
  dfm_ctx *ctx = M->ctx;
  hipSetDevice(ctx->device);
  for (int j = 0; j < nl - 1; ++j) {
    if (M->lane[j]) continue;
    dfm_ctx *lc = nullptr;
    int rc = dfm_ctx_create(ctx->device, &lc);
    if (rc) return fail(ctx, 1002, "bootstrap lane: no context (%d)", rc);
    dfm_model *L = nullptr;
    rc = dfm_model_clone(M, lc, &L);
    if (rc) {
      const std::string e = lc->err;
      dfm_ctx_destroy(lc);
      return fail(ctx, rc, "bootstrap lane: %s", e.c_str());
    }
    L->is_lane = true;
    L->count_ctx = ctx;
    ctx->kids.push_back(lc);
    M->lane[j] = L;
    M->lane_worker[j] = new LaneWorker();
  }
  // the lanes' work starts after the caller's work on the main stream (its
  // inputs).  Measured and rejected: starting the second lane half a step
  // late (an event after the first lane's first eigen-iteration product), so
  // the lanes' GEMMs and latency-bound passes alternate instead of running in
  // lock-step: C3 1 250 replicates 3.81 -> 3.93 ms, C2 283 k -> 265 k
  if (!ctx->gate) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->gate, hipEventDisableTiming));
  HIPCHK(ctx, hipEventRecord(ctx->gate, ctx->stream));
  for (int j = 0; j < nl - 1; ++j) {
    dfm_ctx *lc = M->lane[j]->ctx;
    lc->tol = ctx->tol; lc->tol_values = ctx->tol_values; lc->maxit = ctx->maxit;
    lc->block = ctx->block; lc->poll = ctx->poll; lc->timing = ctx->timing;
    M->lane[j]->mode = M->mode;
    HIPCHK(ctx, hipStreamWaitEvent(lc->stream, ctx->gate, 0));
  }
#if defined(DFM_DEBUG_MEM) || defined(DFM_LANE_SKEW_AB)
  if (const int sk = dbg_lane_skew_us()) {   // wall clock: 100 ticks per microsecond
    hipLaunchKernelGGL(dbg_spin_kernel, dim3(1), dim3(64), 0, sk > 0 ? M->lane[0]->ctx->stream : ctx->stream,
                       (long long)std::abs(sk) * 100);
#ifdef DFM_DEBUG_MEM
    fprintf(stderr, "[dfm debug] lane skew %d us\n", sk);
#endif
  }
#endif
  // lane j takes replicates [b_j, b_{j+1}), b_j = ceil(j B / nl) (lane 0 = this thread)
  const int64_t width = dfm_stats_width(M, stats, ns), T = M->T;
  auto b_at = [&](int j) { return (j * B + nl - 1) / nl; };
  int rcl[dfm_model::kMaxLanes] = {};
  for (int j = 1; j < nl; ++j) {
    dfm_model *L = M->lane[j - 1];
    const int64_t b0 = b_at(j), b1 = b_at(j + 1);
    int *rc = &rcl[j];
    M->lane_worker[j - 1]->run([=]() {
      hipSetDevice(L->ctx->device);
      *rc = bootstrap_one(L, kind, b1 - b0, idx + b0 * T, eta ? eta + b0 * T : nullptr, stats, ns,
                          out ? out + b0 * width : nullptr);
    });
  }
  rcl[0] = bootstrap_one(M, kind, b_at(1), idx, eta, stats, ns, out);
  for (int j = 1; j < nl; ++j) M->lane_worker[j - 1]->wait();
  // the lanes' host-side counters join the caller's context (their kernel
  // timings when the caller's are read: merge_kids; their device-side
  // GEMM-product counts went to ctx->cnt_dev directly)
  for (int j = 0; j < nl - 1; ++j) {
    dfm_ctx *lc = M->lane[j]->ctx;
    if (lc->pend.size() > 4096) merge_kid(ctx, lc);   // (bounded: a long timed run)
    ctx->eig_batches += lc->eig_batches;
    ctx->eig_iters += lc->eig_iters;
    ctx->eig_iters_max = std::max(ctx->eig_iters_max, lc->eig_iters_max);
    ctx->rep_iters += lc->rep_iters;
    ctx->gemm_products += lc->gemm_products;
    ctx->gemm_products_f32 += lc->gemm_products_f32;
    ctx->gemm_products_split_last += lc->gemm_products_split_last;
    ctx->gemm_products_split3 += lc->gemm_products_split3;
    lc->eig_batches = lc->eig_iters = lc->eig_iters_max = lc->rep_iters = lc->gemm_products = 0;
    lc->gemm_products_f32 = lc->gemm_products_split_last = lc->gemm_products_split3 = 0;
  }
  if (rcl[0]) return rcl[0];
  for (int j = 1; j < nl; ++j)
    if (rcl[j]) return fail(ctx, rcl[j], "bootstrap lane %d: %s", j, M->lane[j - 1]->ctx->err.c_str());
  return 0;
}

extern "C" {

int dfm_bootstrap_dev(dfm_model *M, int kind, int64_t B, const int32_t *idx, const double *eta,
                      const dfm_stat *stats, int ns, double *out) {
  if (!M) return -1;
  DeviceShare gate(M->ctx->device);
  const int nl = idx && (kind != DFM_BOOT_WILD || eta) ? lane_count(M, B, stats, ns) : 1;
  if (nl > 1) return bootstrap_lanes(M, nl, kind, B, idx, eta, stats, ns, out);
  return bootstrap_one(M, kind, B, idx, eta, stats, ns, out);
}

static int bootstrap_one(dfm_model *M, int kind, int64_t B, const int32_t *idx, const double *eta,
                         const dfm_stat *stats, int ns, double *out) {
  if (!M) return -1;
  dfm_ctx *ctx = M->ctx;
  if (B < 0 || !idx || (kind == DFM_BOOT_WILD && !eta) || (ns > 0 && (!stats || !out)) || ns < 0)
    return fail(ctx, -2, "dfm_bootstrap: bad arguments");
  if (kind != DFM_BOOT_WILD && kind != DFM_BOOT_RESIDUAL) return fail(ctx, -2, "bad bootstrap kind");
  if (B == 0) return 0;
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const int m = M->m, r = M->r, T = M->T, N = M->N, q = M->q;
  // stat descriptors
  std::vector<StatDesc> sd(ns);
  int64_t width = 0;
  bool chow = false, pcp = false, sup = false;
  int chow_bp = -1, sup_lo = -1, sup_hi = -1;
  for (int i = 0; i < ns; ++i) {
    const dfm_stat s = stats[i];
    if (s.kind < 0 || s.kind > DFM_STAT_SUPWALD_ALL) return fail(ctx, -6, "unknown stat kind %d", s.kind);
    if (s.kind == DFM_STAT_LOADINGS && (s.arg0 < 0 || s.arg0 >= M->nblk))
      return fail(ctx, -6, "loadings of break block %d outside 0..%d", s.arg0, M->nblk - 1);
    if (s.kind == DFM_STAT_CRIT) {
      const int c = s.arg0 >= 0 ? s.arg0 : M->crit;
      if (c < 0 || c > 6) return fail(ctx, -6, "criterion stat without a criterion");
      if (c <= 2) pcp = true;
    }
    if (s.kind == DFM_STAT_EIGVAL && (s.arg0 < 0 || s.arg0 >= r))
      return fail(ctx, -6, "eigenvalue index %d outside 0..%d", s.arg0, r - 1);
    if ((s.kind == DFM_STAT_COEF || s.kind == DFM_STAT_TSTAT) && (s.arg0 < 0 || s.arg0 >= q + r))
      return fail(ctx, -6, "coefficient index %d outside 0..%d", s.arg0, q + r - 1);
    if (chow_stat(s.kind)) {
      if (s.arg0 < r || s.arg0 > T - r) return fail(ctx, -7, "break period %d out of range", s.arg0);
      if (chow && s.arg0 != chow_bp) return fail(ctx, -7, "one break period per call");
      if (M->nblk > 64) return fail(ctx, -7, "Chow statistics support at most 64 break blocks");
      chow = true; chow_bp = s.arg0;
      if (s.kind <= DFM_STAT_WALD && (s.arg1 < 0 || s.arg1 >= N)) return fail(ctx, -7, "variable index");
    }
    if (sup_stat(s.kind)) {
      if (s.arg0 > s.arg1 || s.arg0 < r || s.arg1 > T - r)
        return fail(ctx, -7, "break period range %d..%d outside %d..%d", s.arg0, s.arg1, r, T - r);
      if (sup && (s.arg0 != sup_lo || s.arg1 != sup_hi)) return fail(ctx, -7, "one break period range per call");
      if (M->nblk > 1) return fail(ctx, -7, "sup-Chow statistics need a model fitted without breaks");
      if (r > 16) return fail(ctx, -7, "sup-Chow statistics support r <= 16 (r = %d)", r);
      sup = true; sup_lo = s.arg0; sup_hi = s.arg1;
    }
    sd[i] = {s.kind, s.arg0, s.arg1, (int)width};
    width += stat_width(M, s.kind);
  }
  // Statistics that read only the eigenvalues and the trace let the
  // eigensolver stop on the (quadratic) eigenvalue bound instead of the
  // eigenvector residual: same 1e-12-relative accuracy for what is returned.
  bool values_only = ns > 0;
  for (int i = 0; i < ns; ++i)
    values_only = values_only && (stats[i].kind == DFM_STAT_V || stats[i].kind == DFM_STAT_CRIT ||
                                  stats[i].kind == DFM_STAT_EIGVAL || stats[i].kind == DFM_STAT_TRACE ||
                                  stats[i].kind == DFM_STAT_ITERS);
  const double etol = (values_only && ctx->tol_values > 0) ? -ctx->tol_values : ctx->tol;
  // Statistics invariant to rotations within span(F_r) — the Chow tests
  // (src/chowtest.jl reads F only through projections on it), V, criteria,
  // eigenvalues, and the w-columns' coefficients / t-statistics (the factor
  // block of the design spans the same space) — need the wanted SUBSPACE, not
  // each eigenvector: the strict rule then measures every wanted residual
  // against the gap to the first unwanted Ritz value (EigWork::subspace).
  // Factor-column coefficients / t-statistics keep the per-vector gap.
  bool subspace_only = ns > 0;
  for (int i = 0; i < ns; ++i) {
    const int kd = stats[i].kind;
    subspace_only = subspace_only && (kd == DFM_STAT_V || kd == DFM_STAT_CRIT || kd == DFM_STAT_EIGVAL ||
                                      kd == DFM_STAT_TRACE || kd == DFM_STAT_ITERS || chow_stat(kd) ||
                                      sup_stat(kd) || ((kd == DFM_STAT_COEF || kd == DFM_STAT_TSTAT) && stats[i].arg0 < q));
  }
  const int esub = (subspace_only && !values_only) ? 1 : 0;
  // Fields the statistics read (demand-driven, as the stopping rule above):
  // V, the criteria, eigenvalues and the trace need only the eigensolve;
  // the replicate factors F* and loadings L* (the factored path's loadings
  // GEMM) are formed for coefficients / t-statistics, the Chow tests and the
  // host-closure fields, the OLS + HC2 pass for coefficients / t-statistics.
  bool need_fl = false, need_ols = false;
  for (int i = 0; i < ns; ++i) {
    const int kd = stats[i].kind;
    need_ols = need_ols || kd == DFM_STAT_COEF || kd == DFM_STAT_TSTAT;
    need_fl = need_fl || kd == DFM_STAT_COEF || kd == DFM_STAT_TSTAT || chow_stat(kd) || sup_stat(kd) ||
              kd == DFM_STAT_FACTORS || kd == DFM_STAT_LOADINGS;
  }
  const int p = eig_block_p(m, r, ctx->block);
  // r beyond the subspace eigensolver's block: dense batched eigenpairs,
  // materialised replicate panels for the factor GEMMs, GEMM-built OLS
  const bool wide = p > 32 || p < r;
  const int P = (p <= 16 || wide) ? 16 : 32;
  if (wide && (M->m > dense_eig_max()))
    return fail(ctx, -20, "bootstrap at r=%d > 24 needs min(T,N) <= %d", r, dense_eig_max());
  const bool chow_wide = chow && r > 16;   // GEMM-built Chow tests on materialised replicates
  // PCp reads each replicate's full spectrum, so its Gram is formed: direct path
  const bool fact = (M->orient == 0) && (M->mode != 1) && r <= 16 && T <= fact_t_max() && M->nblk == 1 && !pcp &&
                    !wide;
  // direct path, N > T, no breaks: the replicate Grams by the factored
  // identity (gram_fact_kernel, 2 T^2 r flop each) instead of the SYRK
  const bool gid = !fact && (M->orient == 0) && M->nblk == 1 && r >= 1 && r <= 16 && T <= 4096;
  // the factored solver's own block (k + 4 columns, fact_block_p) and the
  // register template it selects: its workspace layout (eig_iters_ptr) follows
  // pf, not the direct solvers' p
  const int pf = fact ? fact_block_p(m, r, ctx->block) : p;
  const int Pf = pf <= 16 ? 16 : 32;
  // T >= N, no breaks, small N: the batch's Grams by one weighted GEMM (gram_wk)
  const bool gwk = use_gram_wk(M);
  if (pcp && m > spectrum_any_max())
    return fail(ctx, -31, "PCp criteria inside the bootstrap need each replicate's full spectrum: "
                          "supported for min(T,N) <= %d", spectrum_any_max());
  int64_t nb = M->batch;
  if (nb <= 0) {
    if (fact) {
      // No per-replicate Gram: a replicate's workspace is O((T + N) P) (C3:
      // ~0.8 MB), so one batch holds the whole job up to a 16 GB budget —
      // the latency-bound per-replicate kernels then fill the chip.
      const double per = (double)boot_ws_bytes(M, 1024, P, ctx->maxit, chow, true, nullptr, nullptr) / 1024.0;
      nb = (int64_t)std::max(1.0, std::min(16384.0, std::floor(16e9 / per)));
    } else {
      double gbytes = (double)m * m * 8 * (pcp ? 3 : 1);
      if (gwk) gbytes += 8.0 * (double)gram_wk_work(T, N, r, 1);
      if (wide)
        gbytes += 8.0 * ((double)dense_eig_work(m, r) + (double)T * M->ld + (double)ols_wide_work(T, q + r));
      if (chow_wide) gbytes += 8.0 * ((double)chow_wide_work(T, N, r) + (double)T * M->ld + 3.0 * N);
      nb = (int64_t)std::max(1.0, std::min(4096.0, std::floor((wide ? 4e9 : 1.5e9) / gbytes)));
    }
    // equal batches (no small tail batch running the iterations half-empty)
    const int64_t nbat = (B + nb - 1) / nb;
    nb = (B + nbat - 1) / nbat;
  }
  nb = std::min<int64_t>(nb, B);
  if ((fact || gid) && !M->fact_ready) {
    // H = E E' by the MFMA Gram kernel (K1), then EL, S, cF, diag(H)
    M->ldH = round_up(T, 16);
    HIPCHK(ctx, dalloc(&M->H, (size_t)T * M->ldH));
    HIPCHK(ctx, dalloc(&M->EL, (size_t)T * r));
    HIPCHK(ctx, dalloc(&M->S, (size_t)r * r));
    HIPCHK(ctx, dalloc(&M->cF, T));
    HIPCHK(ctx, dalloc(&M->hd, T));
    HIPCHK(ctx, hipMemsetAsync(M->H, 0, (size_t)T * M->ldH * 8, st));
    PanelSrc es{nullptr, M->Ep, nullptr, nullptr, M->ld, 0};
    {
      Scope sc(ctx, DFM_KC_GRAM);
      HIPCHK(ctx, launch_gram(0, es, T, N, T, M->H, M->ldH, 0, 1, st));
    }
    int rc0 = fact_precompute(M->Ep, M->ld, T, N, r, M->L, M->F, M->H, M->ldH, M->EL, M->S, M->cF, M->hd, st);
    if (rc0) return fail(ctx, rc0, "factored precompute failed");
    // F'F once per model (it was one launch per solve on every lane's stream)
    HIPCHK(ctx, dalloc(&M->FtF, 256));
    HIPCHK(ctx, launch_fact_ftf(FactBase{T, r, M->ldH, M->F, M->EL, M->S, M->H, M->cF, M->hd}, M->FtF, st));
    // H32 = float(H / hmax) for the fp32 middle products (a clone rebuilds it here, on its own stream, as it
    // rebuilds H: fact_ready is not copied)
    HIPCHK(ctx, hipMalloc((void **)&M->H32, (size_t)T * M->ldH * sizeof(float)));
    HIPCHK(ctx, launch_fact_h32(M->H, M->ldH, T, M->hd, M->H32, st));
    // ... and its bf16 split for the same products as six bf16 terms (H32 stays for DFM_FACT_SPLIT=0)
    HIPCHK(ctx, hipMalloc(&M->Hs, hsplit_bytes(T)));
    HIPCHK(ctx, launch_fact_hsplit(M->H, M->ldH, T, M->hd, M->Hs, st));
    std::vector<double> hdh(T);
    HIPCHK(ctx, hipMemcpyAsync(hdh.data(), M->hd, (size_t)T * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    M->hmax = fact_hmax(hdh.data(), T);
    M->fact_ready = true;
  }
  if (gwk && !M->Kwk) {
    HIPCHK(ctx, dalloc(&M->Kwk, (size_t)gram_wk_tp(T) * gram_wk_ldk(N)));
    HIPCHK(ctx, dalloc(&M->A0wk, (size_t)N * N));
    HIPCHK(ctx, gram_wk_precompute(M->Ep, M->ld, T, N, r, M->F, M->L, M->Kwk, M->A0wk, st));
  }
  if (gid && !M->FSF) {
    HIPCHK(ctx, dalloc(&M->FSF, (size_t)T * M->ldH));
    HIPCHK(ctx, launch_fact_fsf(T, r, M->F, M->S, M->FSF, M->ldH, st));
  }
  const size_t need = boot_ws_bytes(M, (int)nb, P, ctx->maxit, chow && !chow_wide, fact, nullptr, nullptr);
  if (need > M->ws_bytes) {
    hipFree(M->ws);
    M->ws = nullptr; M->ws_bytes = 0;
#ifdef DFM_DEBUG_MEM
    // debug build: a 64 KB guard band of 0xA5 after the workspace, checked at the end of the call
    HIPCHK(ctx, hipMalloc(&M->ws, need + GuardBuf::kG));
    DFM_POISON_SYNC(M->ws, need);
    (void)hipMemset(M->ws + need, 0xA5, GuardBuf::kG);
    (void)hipStreamSynchronize(nullptr);
#else
    HIPCHK(ctx, hipMalloc(&M->ws, need));
#endif
    M->ws_bytes = need;
  }
  if (ns > M->sd_cap) {
    hipFree(M->sd_dev);
    HIPCHK(ctx, dalloc(&M->sd_dev, ns));
    M->sd_cap = ns;
    M->sd_host.clear();
  }
  // the descriptors go up only when they change: a pageable upload per call
  // was a host round trip in front of every small job's first kernel
  if (ns && (M->sd_host.size() != (size_t)ns || memcmp(M->sd_host.data(), sd.data(), ns * sizeof(StatDesc)) != 0)) {
    M->sd_host.clear();
    HIPCHK(ctx, hipMemcpyAsync(M->sd_dev, sd.data(), ns * sizeof(StatDesc), hipMemcpyHostToDevice, st));
    M->sd_host = sd;
  }
  BootWs w;
  boot_ws_bytes(M, (int)nb, P, ctx->maxit, chow && !chow_wide, fact, &w, M->ws);
  {   // the status flag, and the OLS status rows no OLS pass writes: one launch
    ZeroSpans zs{};
    zs.p[0] = M->flag_dev; zs.n[0] = 1;
    if (!need_ols) { zs.p[1] = w.ost; zs.n[1] = nb; }
    HIPCHK(ctx, launch_zero_spans(zs, st));
  }
  // PCp: the unrestricted full-sample Gram of every replicate (no breaks,
  // src/criteria.jl:18), its spectrum, sigma^2 per replicate
  DevBuf pG, pEv, pWk, pSig, wDe, wX, wOls, wCh, wSc;
  // the sweep's own workspace, bounded by the replicates per sweep launch (not M->ws, which scales with the batch)
  const size_t sw_bytes = sup ? chow_sweep_workspace_bytes(T, N, r, sup_hi - sup_lo + 1, (int)nb) : 0;
  if (sw_bytes > M->sw_bytes) {
    hipFree(M->sw_ws);
    M->sw_ws = nullptr; M->sw_bytes = 0;
    HIPCHK(ctx, hipMalloc(&M->sw_ws, sw_bytes));
    DFM_POISON_SYNC(M->sw_ws, sw_bytes);
    M->sw_bytes = sw_bytes;
  }
  if (wide) {
    HIPCHK(ctx, dalloc(&wDe.p, (size_t)nb * dense_eig_work(m, r)));
    if (q + r > 32) HIPCHK(ctx, dalloc(&wOls.p, (size_t)nb * ols_wide_work(T, q + r)));
  }
  if (r > 32 || chow_wide) HIPCHK(ctx, dalloc(&wX.p, (size_t)nb * T * M->ld));
  if (chow_wide) {
    HIPCHK(ctx, dalloc(&wCh.p, (size_t)nb * chow_wide_work(T, N, r)));
    HIPCHK(ctx, dalloc(&wSc.p, (size_t)3 * nb * N));
  }
  // what every subspace solve of this job shares; each call adds its batch, block, start and outputs
  EigArgs ea0;
  ea0.k = r; ea0.kw = r;
  ea0.tol = etol; ea0.maxit = ctx->maxit; ea0.poll = ctx->poll;
  ea0.ws = w.eig; ea0.status = w.status;
  ea0.st = st; ea0.tf = timer_cb; ea0.tctx = ctx;
  ea0.subspace = esub;
  // top-r eigenpairs of n Grams (stride mm*mm): subspace iteration or dense
  auto eig_any = [&](const double *G, int mm, int n, const double *warm, double *lam, double *Uk, double *tr,
                     int64_t b0) -> int {
    if (!wide) {
      EigArgs ea = ea0;
      ea.nb = n; ea.p = eig_block_p(mm, r, ctx->block);
      ea.warm = warm;
      ea.lam = lam; ea.Uk = Uk; ea.trace_out = tr;
      int rc = eig_run(G, mm, (int64_t)mm * mm, mm, ea, nullptr, b0);
      if (rc) return fail(ctx, rc > 0 ? rc : -21, "eigensolver failed (%d)", rc);
      note_iters(ctx);
      return 0;
    }
    Scope sc(ctx, DFM_KC_EIG_OTHER);
    hipError_t e = launch_dense_eig_batched(G, mm, (int64_t)mm * mm, mm, mm, 0, n, r, lam, Uk, tr, w.status, wDe.p,
                                            st);
    return e == hipSuccess ? 0 : fail(ctx, 1000 + (int)e, "dense eigensolver: %s", hipGetErrorString(e));
  };
  // factors of n replicate panels (rows T_rows of src) into F (+ row offset)
  auto factors_any = [&](const PanelSrc &ps, int Trows, int n, double *Fo, const double *Uk, double *Lo) -> int {
    Scope sc(ctx, DFM_KC_FACTORS);
    if (r <= 32) {
      launch_factors(M->orient, ps, Trows, N, r, n, Uk, Fo, Lo, nullptr, st, (double)T, (int64_t)T * r);
      return 0;
    }
    HIPCHK(ctx, launch_materialize(ps, Trows, N, M->ld, n, wX.p, st));
    if (launch_factors_wide(M->orient, wX.p, M->ld, Trows, N, r, Uk, Fo, Lo, nullptr, st, (double)T, n,
                            (int64_t)Trows * M->ld, (int64_t)T * r))
      return fail(ctx, 1001, "factor kernels failed");
    return 0;
  };
  if (pcp) {
    HIPCHK(ctx, dalloc(&pG.p, (size_t)nb * m * m));
    HIPCHK(ctx, dalloc(&pEv.p, (size_t)nb * m));
    HIPCHK(ctx, dalloc(&pSig.p, (size_t)nb));
    if (spectrum_work(m, (int)nb) > 0) HIPCHK(ctx, dalloc(&pWk.p, (size_t)spectrum_work(m, (int)nb)));
  }
  FactBase fb{T, r, M->ldH, M->F, M->EL, M->S, M->H, M->cF, M->hd, M->FtF, M->H32, M->hmax, M->Hs};
  for (int64_t b0 = 0; b0 < B; b0 += nb) {
    const int n = (int)std::min<int64_t>(nb, B - b0);
    PanelSrc src{M->Cp, M->Ep, idx + b0 * T, kind == DFM_BOOT_WILD ? eta + b0 * T : nullptr, M->ld, T};
    if (fact) {
      const double *et = kind == DFM_BOOT_WILD ? eta + b0 * T : nullptr;
      // the base fit's wanted-eigenvalue spread lambda_1 / lambda_r bounds the
      // warm first filter's degree (eig_run_fact2_t)
      const double spread = (M->lam.size() >= (size_t)r && r > 0 && M->lam[r - 1] > 0.0) ? M->lam[0] / M->lam[r - 1]
                                                                                        : 0.0;
      // ... and its lambda_r, in G*'s scale (both are eigenvalues of X X'), sets the interval end of a warm
      // solve that starts with the filter: a number of the model alone, the same for every batch, lane and shard
      // (fact implies nblk == 1, so M->lam[r - 1] is lambda_r of the one full-sample Gram, not a sum over break blocks)
      const double lamk = spread >= 1.0 ? M->lam[r - 1] : 0.0;
      EigArgs ea = ea0;
      ea.nb = n; ea.p = pf;
      ea.warm = M->Ub;
      ea.lam = w.lam; ea.Uk = need_fl ? w.Uk : nullptr; ea.trace_out = w.trace;
      FactArgs fa;
      fa.idx = idx + b0 * T; fa.eta = et; fa.fws = w.fact;
      fa.off = w.off; fa.lst = w.lst;
      fa.cnt = (M->count_ctx ? M->count_ctx : ctx)->cnt_dev;
      fa.spread = spread; fa.lamk = lamk;
      // M->F = sqrt(T) M->Ub element by element (factors_rows_kernel: fact implies the N > T branch, one break
      // block and r <= 32), so the solver's P'D F is that multiple of its P'D Q0's first r columns
      fa.fscale = sqrt((double)T);
      fa.pb = ctx_poll(ctx);
      int rc = eig_run_factored(fb, ea, fa);
      if (rc) return fail(ctx, rc > 0 ? rc : -21, "eigensolver failed (%d)", rc);
      note_iters(ctx);
      if (need_fl) {
        Scope sc(ctx, DFM_KC_FACTORS);
        rc = fact_loadings(fb, M->Ep, M->ld, N, M->L, w.Uk, et, w.off, w.lst, n, w.F, w.L, w.fload, st);
        if (rc) return fail(ctx, rc, "factored loadings failed");
      }
    } else if (M->nblk > 1) {
      // refit per break block (src/bootstrap.jl:36, :48 pass dfm.break_indices):
      // block j of X*_b is rows a..a+t_j-1 of C + diag(eta_b) E[idx_b, :]
      for (int j = 0; j < M->nblk; ++j) {
        const int a = M->ba[j], tj = M->bt[j], mj = M->bm[j];
        PanelSrc sj{M->Cp + (size_t)a * M->ld, M->Ep, idx + b0 * T + a,
                    kind == DFM_BOOT_WILD ? eta + b0 * T + a : nullptr, M->ld, T};
        {
          Scope sc(ctx, DFM_KC_GRAM);
          HIPCHK(ctx, launch_gram(M->orient, sj, mj, M->orient == 0 ? N : tj, tj, w.G, mj, (int64_t)mj * mj, n, st));
        }
        int rc = eig_any(w.G, mj, n, M->Ubs[j], w.blam, w.Uk, w.btr, b0);
        if (rc) return rc;
        hipLaunchKernelGGL(or_flag_kernel, dim3((n + 255) / 256), dim3(256), 0, st, w.status, n, M->flag_dev, 1);
        if (need_fl && (rc = factors_any(sj, tj, n, w.F + (size_t)a * r, w.Uk, w.L + (size_t)j * nb * N * r)))
          return rc;
        hipLaunchKernelGGL(block_accum_kernel, dim3((n + 255) / 256), dim3(256), 0, st, w.blam, w.btr, n, r,
                           w.lam, w.trace, j == 0 ? 1 : 0);
      }
    } else {
      {
        Scope sc(ctx, DFM_KC_GRAM);
        if (gid)
          HIPCHK(ctx, launch_gram_fact(fb, M->FSF, idx + b0 * T, kind == DFM_BOOT_WILD ? eta + b0 * T : nullptr, n,
                                       w.G, m, (int64_t)m * m, st));
        else if (gwk)
          HIPCHK(ctx, launch_gram_wk(M->Ep, M->ld, T, N, r, M->F, M->L, M->Kwk, M->A0wk, idx + b0 * T,
                                     kind == DFM_BOOT_WILD ? eta + b0 * T : nullptr, T, n, w.gwk, w.G, st));
        else
          HIPCHK(ctx, launch_gram(M->orient, src, m, M->orient == 0 ? N : T, T, w.G, m, (int64_t)m * m, n, st));
      }
      int rc = eig_any(w.G, m, n, M->Ub, w.lam, w.Uk, w.trace, b0);
      if (rc) return rc;
      bool done_f = !need_fl;
      if (gwk && need_fl) {   // T >= N: F* = (F (L' L*) + D P (E L*)) / N, no pass over the resampled panel
        Scope sc(ctx, DFM_KC_FACTORS);
        done_f = launch_factors_cols_fact(M->Ep, M->ld, T, N, r, M->F, M->L, r, idx + b0 * T,
                                          kind == DFM_BOOT_WILD ? eta + b0 * T : nullptr, T, n, w.Uk, w.F, w.L,
                                          (int64_t)T * r, gram_wk_scratch(w.gwk, T, N, r, n), st);
      }
      if (!done_f && (rc = factors_any(src, T, n, w.F, w.Uk, w.L))) return rc;
    }
    if (!need_ols) {
      // (no design to be singular: w.ost zeroed at the top of the call)
    } else if (q + r <= 32) {
      Scope sc(ctx, DFM_KC_OLS);
      launch_ols(n, st, M->y, M->w, q, w.F, T, r, nullptr, nullptr, w.coef,
                         w.tstat, nullptr, nullptr, w.ost);
    } else {
      Scope sc(ctx, DFM_KC_OLS);
      HIPCHK(ctx, launch_ols_wide_batched(n, M->y, M->w, q, w.F, T, r, r, nullptr, w.coef, w.tstat, nullptr, nullptr,
                                          w.ost, wOls.p, st));
    }
    if (pcp) {
      const double *Gp = w.G;
      if (M->nblk > 1) {   // the blocks' Grams are not the full-sample one
        Scope sc(ctx, DFM_KC_GRAM);
        HIPCHK(ctx, launch_gram(M->orient, src, m, M->orient == 0 ? N : T, T, pG.p, m, (int64_t)m * m, n, st));
        Gp = pG.p;
      }
      Scope sc(ctx, DFM_KC_EIG_OTHER);
      HIPCHK(ctx, launch_spectrum(Gp, m, (int64_t)m * m, m, n, pEv.p, pWk.p, st));
      hipLaunchKernelGGL(tail_sigma2_kernel, dim3((n + 255) / 256), dim3(256), 0, st, pEv.p, m, n,
                         (double)N * (double)T, pSig.p);
    }
    {
      Scope sc(ctx, DFM_KC_STATS);
      if (ns)
      {
        // the eigensolver's per-replicate step counts (DFM_STAT_ITERS): the
        // workspace of this batch's (last block's) subspace solve
        // (the factored solver carves its workspace for ITS block pf, which
        // can select a narrower template than the direct solvers' P)
        const int *iters = wide ? nullptr
                                : eig_iters_ptr(w.eig, M->nblk > 1 ? M->bm.back() : m, n, fact ? Pf : P, ctx->maxit);
        hipLaunchKernelGGL(stats_kernel, dim3((n + 127) / 128), dim3(128), 0, st, n, T, N, r, q,
                           M->crit, M->sigma2, pcp ? pSig.p : nullptr, w.lam, w.trace, w.coef, w.tstat, iters,
                           M->sd_dev, ns, out + b0 * width, width, w.status, w.ost, M->flag_dev);
      } else {
        hipLaunchKernelGGL(or_status_kernel, dim3((n + 255) / 256), dim3(256), 0, st, w.status, w.ost,
                           n, M->flag_dev);
      }
      // the replicates' factors / a block's loadings, row by row (host closures)
      for (int i = 0; i < ns; ++i) {
        if (sd[i].kind != DFM_STAT_FACTORS && sd[i].kind != DFM_STAT_LOADINGS) continue;
        const bool fk = sd[i].kind == DFM_STAT_FACTORS;
        const int64_t cnt = fk ? (int64_t)T * r : (int64_t)N * r;
        const double *srcp = fk ? w.F : w.L + (size_t)sd[i].arg0 * nb * N * r;
        HIPCHK(ctx, hipMemcpy2DAsync(out + b0 * width + sd[i].off, (size_t)width * 8, srcp, (size_t)cnt * 8,
                                     (size_t)cnt * 8, n, hipMemcpyDeviceToDevice, st));
      }
    }
    if (chow) {
      Scope sc(ctx, DFM_KC_CHOW);
      // per-variable statistics for every requested Chow stat share one pass
      double *LR = nullptr, *LM = nullptr, *WD = nullptr;
      int64_t ostride = width;
      for (int i = 0; i < ns; ++i) {
        double *base = out + b0 * width + sd[i].off;
        switch (sd[i].kind) {
          case DFM_STAT_LR_ALL: LR = base; break;
          case DFM_STAT_LM_ALL: LM = base; break;
          case DFM_STAT_WALD_ALL: WD = base; break;
          default: break;
        }
      }
      // single-variable Chow stats are served by a full pass too (cheap); they
      // are copied out of a scratch row afterwards.
      const double *scr;
      if (!chow_wide) {
        HIPCHK(ctx, launch_chow(M->orient, src, T, N, r, chow_bp, n, w.F, w.L, LR, LM, WD, ostride,
                                w.chow, w.chow_bytes, st, M->nblk, M->ba.data(), (int64_t)nb * N * r));
        // scratch rows live at the end of the chow workspace: [3][nb][N]
        scr = (const double *)(w.chow + w.chow_bytes) - (size_t)3 * n * N;   // launch_chow's [3][n][N]
      } else {
        // the whole replicate panel (r > 32 without breaks: factors_any already did)
        if (r <= 32 || M->nblk > 1) HIPCHK(ctx, launch_materialize(src, T, N, M->ld, n, wX.p, st));
        HIPCHK(ctx, launch_chow_wide(n, wX.p, M->ld, (int64_t)T * M->ld, nullptr, T, N, r, chow_bp, w.F,
                                     (int64_t)T * r, w.L, (int64_t)N * r, LR, LM, WD, ostride, wSc.p, wCh.p, st,
                                     M->nblk, M->ba.data(), (int64_t)nb * N * r));
        scr = wSc.p;
      }
      for (int i = 0; i < ns; ++i) {
        if (sd[i].kind < DFM_STAT_LR || sd[i].kind > DFM_STAT_WALD) continue;
        const int which = sd[i].kind - DFM_STAT_LR;
        HIPCHK(ctx, hipMemcpy2DAsync(out + b0 * width + sd[i].off, (size_t)width * 8,
                                     scr + ((size_t)which * n) * N + sd[i].arg1, (size_t)N * 8, 8, n,
                                     hipMemcpyDeviceToDevice, st));
      }
    }
    if (sup) {   // sup over bp of every wanted statistic, written into the caller's rows (timed per kernel)
      ChowSweepOut so;
      so.os = width;
      for (int i = 0; i < ns; ++i)
        if (sup_stat(sd[i].kind)) so.sup[sd[i].kind - DFM_STAT_SUPLR_ALL] = out + b0 * width + sd[i].off;
      HIPCHK(ctx, launch_chow_sweep(src, T, N, r, sup_lo, sup_hi, n, w.F, w.L, so, M->sw_ws, sw_bytes, st,
                                    timer_cb, ctx));
    }
  }
  // the status flag through the context's pinned slot (a pageable read-back
  // is a staging copy kernel and ~25 us of host time at the end of every job)
  int flag = 0;
  int *fl = ctx->pollbuf.host ? ctx->pollbuf.host + ctx->pollbuf.cap - 1 : &flag;
  HIPCHK(ctx, hipMemcpyAsync(fl, M->flag_dev, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  flag = *fl;
#ifdef DFM_DEBUG_MEM
  {
    std::vector<unsigned char> g(GuardBuf::kG);
    (void)hipMemcpy(g.data(), M->ws + M->ws_bytes, g.size(), hipMemcpyDeviceToHost);
    int64_t cnt = 0, first = -1;
    for (size_t i = 0; i < g.size(); ++i)
      if (g[i] != 0xA5) { if (first < 0) first = (int64_t)i; ++cnt; }
    if (cnt) {
      fprintf(stderr, "[dfm debug] bootstrap workspace (%s, %zu bytes, batch %lld): %lld guard bytes written past "
              "its end, first at +%lld\n", M->is_lane ? "lane" : "main", M->ws_bytes, (long long)nb, (long long)cnt,
              (long long)first);
      return fail(ctx, 9001, "debug build: bootstrap workspace overrun");
    }
  }
#endif
  if (flag & 1) return fail(ctx, 2, "eigensolver did not converge for some replicate");
  if (flag & 2) return fail(ctx, 3, "singular design matrix in some replicate");
  return 0;
}

int dfm_bootstrap(dfm_model *M, int kind, int64_t B, const int32_t *idx, const double *eta,
                  const dfm_stat *stats, int ns, double *out) {
  if (!M) return -1;
  dfm_ctx *ctx = M->ctx;
  if (B < 0 || !idx || (kind == DFM_BOOT_WILD && !eta)) return fail(ctx, -2, "dfm_bootstrap: bad arguments");
  if (B == 0) return 0;
  for (int64_t i = 0; i < B * M->T; ++i)
    if (idx[i] < 0 || idx[i] >= M->T) return fail(ctx, -8, "resample index out of range at %lld", (long long)i);
  // the whole call under the device gate — the uploads and the result copy
  // too, not only dfm_bootstrap_dev's kernels (nested: that share is this one)
  DeviceShare gate(ctx->device);
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const int64_t width = dfm_stats_width(M, stats, ns);
  int32_t *di = nullptr;
  double *de = nullptr, *dout = nullptr;
#ifdef DFM_DEBUG_MEM
  // debug build: the draws and the output rows inside guard bands, checked
  // (with the draws themselves) after the call
  GuardBuf gi, ge, go;
  HIPCHK(ctx, gi.alloc((size_t)B * M->T * 4));
  if (eta) HIPCHK(ctx, ge.alloc((size_t)B * M->T * 8));
  HIPCHK(ctx, go.alloc((size_t)B * std::max<int64_t>(width, 1) * 8));
  di = (int32_t *)gi.p; de = (double *)ge.p; dout = (double *)go.p;
#else
  HIPCHK(ctx, dalloc(&di, (size_t)B * M->T));
  if (eta) HIPCHK(ctx, dalloc(&de, (size_t)B * M->T));
  HIPCHK(ctx, dalloc(&dout, (size_t)B * std::max<int64_t>(width, 1)));
#endif
  HIPCHK(ctx, hipMemcpyAsync(di, idx, (size_t)B * M->T * 4, hipMemcpyHostToDevice, st));
  if (eta) HIPCHK(ctx, hipMemcpyAsync(de, eta, (size_t)B * M->T * 8, hipMemcpyHostToDevice, st));
  int rc = dfm_bootstrap_dev(M, kind, B, di, kind == DFM_BOOT_WILD ? de : nullptr, stats, ns, dout);
  if (rc == 0 && width > 0)
    rc = hipMemcpyAsync(out, dout, (size_t)B * width * 8, hipMemcpyDeviceToHost, st) == hipSuccess ? 0 : 1001;
  hipStreamSynchronize(st);
#ifdef DFM_DEBUG_MEM
  {
    const int bad = gi.check("idx", idx, M->T * 4) + (eta ? ge.check("eta", eta, M->T * 8) : 0) +
                    go.check("out", nullptr, width * 8);
    if (bad && rc == 0) rc = fail(ctx, 9001, "debug build: %d guard / input violations (stderr)", bad);
  }
#else
  hipFree(di); hipFree(de); hipFree(dout);
#endif
  return rc;
}

}  // extern "C"

// wild_bootstrap / residual_bootstrap (src/bootstrap.jl:21-51) with the
// replicate loop (:43) sharded over n models (one per context, typically one
// per GPU, each a dfm_model_clone of the same fit): replicate b runs on model
// floor(b n / B), i.e. contiguous shards, each driven by its own host thread
// on its own stream; rows land in order in the caller's out (B x width).
// No collective: the shards are independent and the host buffer is the
// gather.  Contexts must be distinct (one host thread per context).
extern "C" int dfm_bootstrap_multi(dfm_model *const *models, int n, int kind, int64_t B, const int32_t *idx,
                                   const double *eta, const dfm_stat *stats, int ns, double *out) {
  if (!models || n < 1 || !models[0]) return -1;
  dfm_ctx *c0 = models[0]->ctx;
  for (int g = 0; g < n; ++g) {
    if (!models[g]) return fail(c0, -2, "dfm_bootstrap_multi: model %d is NULL", g);
    const dfm_model *a = models[g], *b = models[0];
    if (a->T != b->T || a->N != b->N || a->r != b->r || a->q != b->q || a->nblk != b->nblk || a->crit != b->crit)
      return fail(c0, -2, "dfm_bootstrap_multi: model %d is not a copy of model 0", g);
    for (int h = 0; h < g; ++h)
      if (models[h]->ctx == a->ctx) return fail(c0, -2, "dfm_bootstrap_multi: models %d and %d share a context", h, g);
  }
  if (B < 0 || !idx || (kind == DFM_BOOT_WILD && !eta)) return fail(c0, -2, "dfm_bootstrap_multi: bad arguments");
  if (B == 0) return 0;
  const int64_t width = dfm_stats_width(models[0], stats, ns);
  if (width < 0) return fail(c0, -2, "dfm_bootstrap_multi: bad stat list");
  const int64_t T = models[0]->T;
  std::vector<int> rcs(n, 0);
  std::vector<std::thread> th;
  for (int g = 0; g < n; ++g) {
    const int64_t b0 = ((int64_t)g * B + n - 1) / n, b1 = ((int64_t)(g + 1) * B + n - 1) / n;
    if (b1 <= b0) continue;
    th.emplace_back([=, &rcs]() {
      rcs[g] = dfm_bootstrap(models[g], kind, b1 - b0, idx + b0 * T, eta ? eta + b0 * T : nullptr, stats, ns,
                             out ? out + b0 * width : nullptr);
    });
  }
  for (auto &t : th) t.join();
  for (int g = 0; g < n; ++g)
    if (rcs[g]) {
      const std::string msg = models[g]->ctx->err;
      return fail(c0, rcs[g], "shard %d: %s", g, msg.c_str());
    }
  return 0;
}
