// dfm_mc.hip — Monte-Carlo batches (dfm_mc): M independent panels of one
// shape fitted and tested in one pass, the loop of the reference's driver
// script (src/Bai_Ng.jl:12-39: factor_model_DGP -> normalize -> the IC-sweep
// constructor -> number_of_factors, per (T, N, r) tuple and repetition) and of
// the size / power tables of Breitung–Eickmeier (2011).
//
// Per chunk of n panels:
//   mc_panel_kernel   column-major panels -> ONE tall row-major (n T) x ld panel
//                     (ld = round_up(N, 16), zero padding), z-scored on the way
//   Grams             panel b = rows b T .. b T + T - 1 of the tall panel: a
//                     PanelSrc with relocated rows idx_b[t] = b T + t (the
//                     rolling windows' device, dfm_windows.hip), launch_gram
//   spectrum + select launch_spectrum, then mc_select_kernel: V(k) by the trace
//                     identity, PCp's sigma^2 as the spectral tail, the seven
//                     criteria for k = 1..kmax, the first arg-min of each
//   fit stage         (statistics asked for) the panels grouped by their r — one
//                     group at a fixed r, one per distinct r^ otherwise; a group
//                     is another relocation list — through the batched stages
//                     of the bootstrap: top-r eigenpairs, launch_factors,
//                     stats_kernel, launch_chow, launch_chow_sweep.  No OLS.
// Every kernel is batch-invariant, so a panel's results do not depend on the
// chunk it falls in nor on the group it is fitted with.
#include "dfm_host.h"

namespace {

constexpr int MC_TR = 64;   // rows per staged tile: one per lane of a column's wave
constexpr int MC_SW = 16;   // strip width: 16 doubles = one 128-B line per row
constexpr int64_t MC_CHUNK_BYTES = (int64_t)2 << 30;   // workspace bound of a chunk (the windows code's precedent)
constexpr int MC_CHUNK_MAX = 32768;                    // panels per chunk (grid.y of the batched launches)
constexpr int MC_RFIT_MAX = 32, MC_RSUP_MAX = 16;      // the fit stage's r limits (launch_factors; dfm_chow_sweep)
#ifndef DFM_MC_SPEC_SLICE   // (A/B builds: make EXTRA=-DDFM_MC_SPEC_SLICE=n)
#define DFM_MC_SPEC_SLICE 256
#endif
constexpr int MC_SPEC_SLICE = DFM_MC_SPEC_SLICE;       // launch_spectrum's LDS form serves batches up to this

// Strip (blockIdx.x) of 16 columns of panel blockIdx.y: wave w owns columns
// 4 w .. 4 w + 3 of the strip.  Column statistics exactly as
// normalize_cols_kernel (dfm_panel.hip) — one wave per column, lane-strided
// sums, wave_sum, the variance accumulated with fma, (x - mu) / sd — so the
// values are bit-identical to dfm_normalize_dev of the panel alone.  Reads run
// along a column (64 consecutive doubles per wave); the tile goes out row by
// row, 8 lanes x 16 B per row: whole 128-B lines, no 8-B stores at stride ld.
__global__ __launch_bounds__(256) void mc_panel_kernel(const double *__restrict__ X, int64_t ldx, int64_t stride,
                                                       int T, int N, int normalize, double *__restrict__ P,
                                                       int64_t ld) {
  __shared__ double tile[MC_TR][MC_SW + 1];
  const int b = blockIdx.y, c0 = blockIdx.x * MC_SW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double *Xb = X + (int64_t)b * stride;
  double mu[4], sd[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + 4 * wave + j;
    mu[j] = 0.0; sd[j] = 1.0;
    if (normalize && c < N) {
      const double *x = Xb + (int64_t)c * ldx;
      double s = 0.0;
      for (int t = lane; t < T; t += 64) s += x[t];
      mu[j] = wave_sum(s) / T;
      double v = 0.0;
      for (int t = lane; t < T; t += 64) { const double d = x[t] - mu[j]; v = fma(d, d, v); }
      sd[j] = sqrt(wave_sum(v) / (T - 1));
    }
  }
  for (int t0 = 0; t0 < T; t0 += MC_TR) {
    __syncthreads();   // the previous tile has left
    const int t = t0 + lane;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = c0 + 4 * wave + j;
      double v = 0.0;
      if (c < N && t < T) {
        const double x = Xb[(int64_t)c * ldx + t];
        v = normalize ? (x - mu[j]) / sd[j] : x;
      }
      tile[lane][4 * wave + j] = v;
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // 64 rows x 8 column pairs
      const int ch = tid + 256 * h, row = ch >> 3, cp = ch & 7;
      if (t0 + row < T) {
        double2 v;
        v.x = tile[row][2 * cp];
        v.y = tile[row][2 * cp + 1];
        *reinterpret_cast<double2 *>(P + ((int64_t)b * T + t0 + row) * ld + c0 + 2 * cp) = v;
      }
    }
  }
}

// Relocated rows of a group of panels inside the chunk's tall panel:
// idx[j][t] = b_j T + t, b_j = list[j] (list == nullptr: b_j = j, the whole
// chunk), and the group's rows of the per-panel sigma^2 vector.
__global__ void mc_group_kernel(const int *__restrict__ list, int T, int32_t *__restrict__ idx,
                                const double *__restrict__ sig2, double *__restrict__ sig2g) {
  const int j = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  const int b = list ? list[j] : j;
  if (t < T) idx[(int64_t)j * T + t] = (int32_t)((int64_t)b * T + t);
  if (t == 0 && sig2 && sig2g) sig2g[j] = sig2[b];
}

// One thread per panel, on the panel's spectrum (descending, row stride m) and
// trace: PCp's sigma^2 as the spectral tail (tail_sigma2_kernel's order), the
// panel's 7 x kmax table and the first arg-min of each row by criteria_sweep.
__global__ void mc_select_kernel(const double *__restrict__ ev, const double *__restrict__ trace, int m, int n, int T,
                                 int N, int kmax, int crit, double *__restrict__ sig2, int *__restrict__ rsel,
                                 int64_t *__restrict__ r_hat, double *__restrict__ ic, double *__restrict__ eig) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  const double *e = ev + (int64_t)b * m;
  const double sigma2 = sigma2_tail(e, m, (double)N * (double)T);
  sig2[b] = sigma2;
  for (int k = 0; k < kmax; ++k) eig[(int64_t)b * kmax + k] = e[k];
  int arg[7];
  criteria_sweep(e, kmax, trace[b], sigma2, T, N, ic + (int64_t)b * 7 * kmax, arg);
#pragma unroll
  for (int q = 0; q < 7; ++q) r_hat[(int64_t)b * 7 + q] = arg[q];
  rsel[b] = crit >= 0 ? arg[crit] : 0;
}

// The groups' staged rows (group order) into the chunk's rows (panel order)
__global__ void mc_scatter_rows_kernel(const double *__restrict__ rows, const int *__restrict__ list, int n,
                                       int64_t width, double *__restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * width) return;
  const int64_t j = e / width, c = e - j * width;
  out[(int64_t)list[j] * width + c] = rows[e];
}

inline bool mc_stat_ok(int k) {
  return k == DFM_STAT_V || k == DFM_STAT_CRIT || k == DFM_STAT_EIGVAL || k == DFM_STAT_TRACE || chow_stat(k) ||
         sup_stat(k);
}

// bump allocation out of one stream-ordered block
struct McArena {
  char *base = nullptr;
  size_t off = 0;
  hipStream_t st = nullptr;
  template <class Tp>
  Tp *take(size_t count) {
    Tp *p = base ? (Tp *)(base + off) : nullptr;
    off += (std::max<size_t>(count, 1) * sizeof(Tp) + 255) & ~size_t(255);
    return p;
  }
  // (the synchronise: an early return may leave copies from / to the call's host vectors in flight)
  ~McArena() {
    if (!base) return;
    hipStreamSynchronize(st);
    hipFreeAsync(base, st);
  }
};

}  // namespace

extern "C" int64_t dfm_mc_stats_width(int64_t N, const dfm_stat *stats, int nstats) {
  if (N < 1 || nstats < 0 || (nstats > 0 && !stats)) return -1;
  int64_t w = 0;
  for (int i = 0; i < nstats; ++i) {
    if (!mc_stat_ok(stats[i].kind)) return -6;
    w += all_var_stat(stats[i].kind) ? N : 1;
  }
  return w;
}

extern "C" int dfm_mc(dfm_ctx *ctx, const double *X, int64_t M, int64_t T64, int64_t N64, int64_t ldx, int64_t stride,
                      const dfm_mc_spec *spec, const dfm_stat *stats, int ns, int64_t *r_hat, double *ic, double *eig,
                      double *out) {
  if (!ctx) return -1;
  DeviceShare gate(ctx->device);
  if (!spec) return fail(ctx, -2, "dfm_mc: spec required");
  if (M < 0 || ns < 0 || (ns > 0 && !stats)) return fail(ctx, -2, "dfm_mc: bad arguments");
  // ---- every argument check, before any device work
  for (int i = 0; i < ns; ++i) {
    const int k = stats[i].kind;
    if (k < 0 || k > DFM_STAT_SUPWALD_ALL) return fail(ctx, -6, "unknown stat kind %d", k);
    if (!mc_stat_ok(k))
      return fail(ctx, -6, "dfm_mc: stat kind %d needs y / w or has rows whose length depends on the panel's r "
                           "(COEF, TSTAT, ITERS, FACTORS, LOADINGS are not Monte-Carlo statistics)", k);
  }
  if (M == 0) return 0;
  if (!X || T64 < 2 || N64 < 1 || ldx < T64 || stride < ldx * N64) return fail(ctx, -2, "dfm_mc: bad panel layout");
  if (T64 > (1 << 24) || N64 > (1 << 24)) return fail(ctx, -2, "dfm_mc: panel too large");
  const int T = (int)T64, N = (int)N64, m = std::min(T, N), mfn = ceil_half(m);
  const int orient = N > T ? 0 : 1;   // src/DynamicFactorModel.jl:86 (N > T: X X') vs :77 (X'X)
  const int64_t ld = round_up(N, 16);
  if ((int64_t)T * ld * 8 >= MC_CHUNK_BYTES) return fail(ctx, -2, "dfm_mc: panel too large");
  if (m > spectrum_any_max())
    return fail(ctx, -31, "dfm_mc: supported for min(T,N) <= %d (got %d)", spectrum_any_max(), m);
  const int crit = spec->crit;
  if (spec->r < 0) return fail(ctx, -2, "dfm_mc: r < 0");
  if (crit < -1 || crit > 6 || (spec->r == 0 && crit < 0))
    return fail(ctx, -3, "dfm_mc: unknown criterion %d (the per-panel selection needs one)", crit);
  if (spec->batch < 0) return fail(ctx, -2, "dfm_mc: batch < 0");
  const int kmax = std::min(spec->kmax > 0 ? spec->kmax : mfn, mfn);   // src/DynamicFactorModel.jl:54 (D11)
  const int rfix = spec->r > 0 ? std::min(spec->r, mfn) : 0;           // :116-119
  const int rmax = rfix > 0 ? rfix : kmax;                             // the largest r any panel can be fitted at
  std::vector<StatDesc> sd(ns);
  int64_t width = 0;
  bool chow = false, sup = false, pcp = false, need_fl = false;
  int chow_bp = -1, sup_lo = -1, sup_hi = -1;
  for (int i = 0; i < ns; ++i) {
    const dfm_stat s = stats[i];
    if (s.kind == DFM_STAT_CRIT) {
      const int c = s.arg0 >= 0 ? s.arg0 : crit;
      if (c < 0 || c > 6) return fail(ctx, -6, "criterion stat without a criterion");
      if (c <= 2) pcp = true;
    }
    if (s.kind == DFM_STAT_EIGVAL && (s.arg0 < 0 || s.arg0 >= rmax))
      return fail(ctx, -6, "eigenvalue index %d outside 0..%d", s.arg0, rmax - 1);
    if (chow_stat(s.kind)) {
      if (s.arg0 < rmax || s.arg0 > T - rmax)
        return fail(ctx, -7, "break period %d outside %d..%d", s.arg0, rmax, T - rmax);
      if (chow && s.arg0 != chow_bp) return fail(ctx, -7, "one break period per call");
      if (s.kind <= DFM_STAT_WALD && (s.arg1 < 0 || s.arg1 >= N)) return fail(ctx, -7, "variable index");
      chow = true; chow_bp = s.arg0;
    }
    if (sup_stat(s.kind)) {
      if (s.arg0 > s.arg1 || s.arg0 < rmax || s.arg1 > T - rmax)
        return fail(ctx, -7, "break period range %d..%d outside %d..%d", s.arg0, s.arg1, rmax, T - rmax);
      if (sup && (s.arg0 != sup_lo || s.arg1 != sup_hi)) return fail(ctx, -7, "one break period range per call");
      sup = true; sup_lo = s.arg0; sup_hi = s.arg1;
    }
    need_fl = need_fl || chow_stat(s.kind) || sup_stat(s.kind);
    sd[i] = {s.kind, s.arg0, s.arg1, (int)width};
    width += all_var_stat(s.kind) ? N : 1;
  }
  const int rlim = sup ? MC_RSUP_MAX : MC_RFIT_MAX;
  if (ns > 0 && out && rfix > rlim)
    return fail(ctx, -7, "dfm_mc: the fit stage serves r <= %d%s (r = %d)", rlim, sup ? " with a sup statistic" : "",
                rfix);
  const bool fit = ns > 0 && out;   // (out == NULL skips the fit stage, as every NULL output skips its work)
  // the sweep runs when something reads it (a PCp criterion stat: its per-panel sigma^2)
  const bool sweep = r_hat || ic || eig || rfix == 0 || pcp;
  if (!fit && !sweep) return 0;
  const int rf = std::min(rmax, rlim);   // widest fit (a larger r^ fails the call after the sweep)
  auto wide_at = [&](int r) { const int p = eig_block_p(m, r, ctx->block); return p > 32 || p < r; };
  bool any_wide = false, any_sub = false;
  for (int r = rfix > 0 ? rfix : 1; fit && r <= rf; ++r) (wide_at(r) ? any_wide : any_sub) = true;
  const int rch = std::min(rf, 16), rcw = rf;   // widest r of launch_chow / of launch_chow_wide
  const bool chow_wide = chow && rf > 16;
  // ---- chunk: stacked panel, Grams and workspaces bounded; n T < 2^31 (idx) and the
  // tall panel below 4 GB (launch_chow's 32-bit row offsets) whatever the caller's batch
  const int64_t spec_per = spectrum_work(m, 1);
  double per = 8.0 * ((double)T * ld + (double)m * m);
  if (!spec->dev) per += 8.0 * (double)stride;
  if (sweep) per += 8.0 * ((double)m + (double)spec_per + 8.0 * kmax + 16);
  if (fit) {
    per += 8.0 * ((double)rf * (1 + m + T + N) + 2.0 * width + 8) + 8.0 * T;
    if (any_sub) per += (double)eig_workspace_bytes_padded(m, 1024, rf + 8 <= 16 ? 16 : 32, ctx->maxit) / 1024.0;
    if (any_wide) per += 8.0 * (double)dense_eig_work(m, rf);
    if (chow) per += (double)chow_workspace_bytes(T, N, rch, 1024) / 1024.0;
    if (chow_wide) per += 8.0 * ((double)chow_wide_work(T, N, rcw) + (double)T * ld + 3.0 * N);
  }
  const int64_t hard = std::min<int64_t>(std::min<int64_t>(MC_CHUNK_MAX, (((int64_t)1 << 31) - 1) / T),
                                         (((int64_t)1 << 32) - 1) / ((int64_t)T * ld * 8));
  int64_t nc = spec->batch > 0 ? spec->batch : std::max<int64_t>(1, (int64_t)((double)MC_CHUNK_BYTES / per));
  nc = std::max<int64_t>(1, std::min(std::min(nc, hard), M));
  if (spec->batch <= 0) {   // equal chunks (no small tail chunk)
    const int64_t nch = (M + nc - 1) / nc;
    nc = (M + nch - 1) / nch;
  }
  // (the sup sweep chunks its replicates inside its own bounded workspace)
  const size_t sw_bytes = sup ? chow_sweep_workspace_bytes(T, N, rch, sup_hi - sup_lo + 1, (int)nc) : 0;
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  // ---- one stream-ordered block, carved twice (sizes, then pointers)
  struct Ws {
    double *raw, *P, *G, *tr, *ev, *swk, *sig2, *sig2g, *dic, *deig, *lam, *Uk, *F, *L, *rows, *dout, *dwk, *zeroC;
    double *wX, *wCh, *wSc;
    int64_t *drh;
    int32_t *idx, *gidx;
    int *rsel, *status, *zst, *list, *flag;
    StatDesc *sdd;
    char *eigws, *chws, *swws;
    size_t eig_bytes, ch_bytes;
  } w{};
  const int64_t span = (nc - 1) * stride + ldx * (int64_t)(N - 1) + T;   // a chunk's panels, gaps included
  const int nsl = (m > 32 && m <= 128) ? (int)std::min<int64_t>(nc, MC_SPEC_SLICE) : (int)nc;
  const int Pmax = eig_block_p(m, rf, ctx->block) <= 16 ? 16 : 32;
  auto carve = [&](McArena &a) {
    w.raw = a.take<double>(spec->dev ? 1 : (size_t)span);
    w.P = a.take<double>((size_t)nc * T * ld);
    w.idx = a.take<int32_t>((size_t)nc * T);
    w.G = a.take<double>((size_t)nc * m * m);
    w.tr = a.take<double>((size_t)nc + 1);
    w.flag = a.take<int>(1);
    w.zst = a.take<int>((size_t)nc);
    if (sweep) {
      w.ev = a.take<double>((size_t)nc * m);
      w.swk = a.take<double>((size_t)spectrum_work(m, nsl));
      w.sig2 = a.take<double>((size_t)nc);
      w.rsel = a.take<int>((size_t)nc);
      w.drh = a.take<int64_t>((size_t)nc * 7);
      w.dic = a.take<double>((size_t)nc * 7 * kmax);
      w.deig = a.take<double>((size_t)nc * kmax);
    }
    if (fit) {
      w.gidx = a.take<int32_t>((size_t)nc * T);
      w.list = a.take<int>((size_t)nc);
      w.sig2g = a.take<double>((size_t)nc);
      w.lam = a.take<double>((size_t)(nc + 1) * rf);   // (+ 1: a lone problem's second copy, below)
      w.Uk = a.take<double>((size_t)(nc + 1) * m * rf);
      w.F = a.take<double>((size_t)nc * T * rf);
      w.L = a.take<double>((size_t)nc * N * rf);
      w.status = a.take<int>((size_t)nc + 1);
      w.sdd = a.take<StatDesc>((size_t)ns);
      w.rows = a.take<double>((size_t)nc * width);
      w.dout = a.take<double>((size_t)nc * width);
      w.eig_bytes = any_sub ? eig_workspace_bytes_padded(m, (int)nc + 1, Pmax, ctx->maxit) : 0;
      if (any_sub && Pmax == 32)
        w.eig_bytes = std::max(w.eig_bytes, eig_workspace_bytes_padded(m, (int)nc + 1, 16, ctx->maxit));
      w.eigws = a.take<char>(w.eig_bytes);
      w.dwk = a.take<double>(any_wide ? (size_t)nc * dense_eig_work(m, rf) : 1);
      w.ch_bytes = chow ? chow_workspace_bytes(T, N, rch, (int)nc) : 0;
      w.chws = a.take<char>(w.ch_bytes);
      w.zeroC = a.take<double>(chow ? (size_t)T * ld : 1);
      w.swws = a.take<char>(sw_bytes);
      w.wX = a.take<double>(chow_wide ? (size_t)nc * T * ld : 1);
      w.wCh = a.take<double>(chow_wide ? (size_t)nc * chow_wide_work(T, N, rcw) : 1);
      w.wSc = a.take<double>(chow_wide ? (size_t)3 * nc * N : 1);
    }
  };
  McArena sizing;
  carve(sizing);
  McArena ar;
  ar.st = st;
  if (stream_malloc((void **)&ar.base, sizing.off, st) != hipSuccess)
    return fail(ctx, 1002, "dfm_mc: out of device memory (%zu bytes for chunks of %lld panels)", sizing.off,
                (long long)nc);
  carve(ar);
  {   // what every chunk shares: the whole-chunk relocation list, zeroed status words, descriptors, Chow's zero C
    Scope sc(ctx, DFM_KC_MISC);
    hipLaunchKernelGGL(mc_group_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)nc), dim3(256), 0, st,
                       (const int *)nullptr, T, w.idx, (const double *)nullptr, (double *)nullptr);
    ZeroSpans zs{};
    zs.p[0] = w.flag; zs.n[0] = 1;
    zs.p[1] = w.zst; zs.n[1] = nc;
    HIPCHK(ctx, launch_zero_spans(zs, st));
  }
  if (fit) HIPCHK(ctx, hipMemcpyAsync(w.sdd, sd.data(), ns * sizeof(StatDesc), hipMemcpyHostToDevice, st));
  if (fit && chow) HIPCHK(ctx, hipMemsetAsync(w.zeroC, 0, (size_t)T * ld * 8, st));
  const int K = orient == 0 ? N : T;
  std::vector<int> hsel, hlist;
  for (int64_t c0 = 0; c0 < M; c0 += nc) {
    const int n = (int)std::min<int64_t>(nc, M - c0);
    // ---- a. layout (+ z-score): the chunk's panels as one tall row-major panel
    const double *src = X + c0 * stride;
    if (!spec->dev) {
      const int64_t sp = (int64_t)(n - 1) * stride + ldx * (int64_t)(N - 1) + T;
      HIPCHK(ctx, hipMemcpyAsync(w.raw, src, (size_t)sp * 8, hipMemcpyHostToDevice, st));
      src = w.raw;
    }
    {
      Scope sc(ctx, DFM_KC_MISC);
      hipLaunchKernelGGL(mc_panel_kernel, dim3((unsigned)(ld / MC_SW), (unsigned)n), dim3(256), 0, st, src, ldx, stride,
                         T, N, spec->normalize != 0 ? 1 : 0, w.P, ld);
      HIPCHK(ctx, hipGetLastError());
    }
    // ---- b. Grams: panel b = relocated rows b T .. b T + T - 1 (no C, no eta: instantiated)
    const PanelSrc psrc{nullptr, w.P, w.idx, nullptr, ld, T};
    {
      Scope sc(ctx, DFM_KC_GRAM);
      HIPCHK(ctx, launch_gram(orient, psrc, m, K, T, w.G, m, (int64_t)m * m, n, st));
    }
    // ---- c. spectra, the criterion sweep and its arg-mins
    if (sweep) {
      {
        Scope sc(ctx, DFM_KC_EIG_OTHER);
        hipLaunchKernelGGL(eig_trace_kernel, dim3(n), dim3(64), 0, st, w.G, (int64_t)m, (int64_t)m * m, m, w.tr);
        // (slices: one form of the tridiagonalisation whatever the chunk size, so a panel's
        // eigenvalues do not depend on it)
        for (int s0 = 0; s0 < n; s0 += nsl)
          HIPCHK(ctx, launch_spectrum(w.G + (size_t)s0 * m * m, m, (int64_t)m * m, m, std::min(nsl, n - s0),
                                      w.ev + (size_t)s0 * m, w.swk, st));
      }
      {
        Scope sc(ctx, DFM_KC_STATS);
        hipLaunchKernelGGL(mc_select_kernel, dim3((n + 127) / 128), dim3(128), 0, st, w.ev, w.tr, m, n, T, N, kmax,
                           crit, w.sig2, w.rsel, w.drh, w.dic, w.deig);
        HIPCHK(ctx, hipGetLastError());
      }
      if (r_hat) HIPCHK(ctx, hipMemcpyAsync(r_hat + c0 * 7, w.drh, (size_t)n * 7 * 8, hipMemcpyDeviceToHost, st));
      if (ic)
        HIPCHK(ctx, hipMemcpyAsync(ic + c0 * 7 * kmax, w.dic, (size_t)n * 7 * kmax * 8, hipMemcpyDeviceToHost, st));
      if (eig) HIPCHK(ctx, hipMemcpyAsync(eig + c0 * kmax, w.deig, (size_t)n * kmax * 8, hipMemcpyDeviceToHost, st));
    }
    if (!fit) continue;
    // ---- d. fit stage: the panels grouped by their r (group g = list[g0[g] .. g0[g+1]))
    std::vector<int> gr, g0;
    if (rfix > 0) {
      gr.push_back(rfix); g0.push_back(0); g0.push_back(n);
    } else {
      hsel.resize(n);
      HIPCHK(ctx, hipMemcpyAsync(hsel.data(), w.rsel, (size_t)n * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      hlist.clear();
      g0.push_back(0);
      for (int r = 1; r <= kmax; ++r) {
        for (int b = 0; b < n; ++b) {
          if (hsel[b] != r) continue;
          if (r > rlim)
            return fail(ctx, -7, "dfm_mc: panel %lld selected r = %d: the fit stage serves r <= %d%s",
                        (long long)(c0 + b), r, rlim, sup ? " with a sup statistic" : "");
          hlist.push_back(b);
        }
        if ((int)hlist.size() > g0.back()) { gr.push_back(r); g0.push_back((int)hlist.size()); }
      }
      if ((int)hlist.size() != n) return fail(ctx, 4, "dfm_mc: a panel's criteria are not finite (no arg-min)");
      HIPCHK(ctx, hipMemcpyAsync(w.list, hlist.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    }
    const bool ident = rfix > 0;
    double *rows = ident ? w.dout : w.rows;
    for (size_t g = 0; g < gr.size(); ++g) {
      const int r = gr[g], j0 = g0[g], ng = g0[g + 1] - g0[g];
      const int32_t *gi = ident ? w.idx : w.gidx + (size_t)j0 * T;
      double *Gg = w.G + (size_t)j0 * m * m, *lam = w.lam + (size_t)j0 * rf, *Uk = w.Uk + (size_t)j0 * m * rf;
      double *F = w.F + (size_t)j0 * T * rf, *L = w.L + (size_t)j0 * N * rf, *tr = w.tr + j0;
      double *grow = rows + (size_t)j0 * width;
      int *status = w.status + j0;
      const double *sg = pcp ? w.sig2 : nullptr;
      if (!ident) {   // the group's relocation list and Grams (the chunk's Grams are spent: the sweep read them)
        {
          Scope sc(ctx, DFM_KC_MISC);
          hipLaunchKernelGGL(mc_group_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)ng), dim3(256), 0, st,
                             (const int *)(w.list + j0), T, w.gidx + (size_t)j0 * T, (const double *)w.sig2,
                             w.sig2g + j0);
        }
        if (pcp) sg = w.sig2g + j0;
        Scope sc(ctx, DFM_KC_GRAM);
        const PanelSrc gs{nullptr, w.P, gi, nullptr, ld, T};
        HIPCHK(ctx, launch_gram(orient, gs, m, K, T, Gg, m, (int64_t)m * m, ng, st));
      }
      const PanelSrc gsrc{nullptr, w.P, gi, nullptr, ld, T};
      // top-r eigenpairs (hashed start, sign-canonicalised), polished as a single fit's are
      if (!wide_at(r)) {
        // eig_run gives a LONE problem the single fit's filter schedule (degree 4 where a batch runs
        // degree 2): a group of one is solved as two copies of its Gram (stride 0), so a panel's
        // eigenvectors do not depend on how many panels share its r in its chunk
        const int nbe = ng == 1 ? 2 : ng;
        EigArgs ea = ctx_eig_args(ctx, m, r);
        ea.nb = nbe;
        ea.ws = w.eigws;
        ea.lam = lam; ea.Uk = Uk; ea.trace_out = tr; ea.status = status;
        const int rc = eig_run(Gg, m, ng == 1 ? 0 : (int64_t)m * m, m, ea, nullptr, 0);
        if (rc) return fail(ctx, rc > 0 ? rc : -21, "eigensolver failed (%d)", rc);
        ctx->eig_batches++;
        ctx->eig_iters += g_last_iters;
        ctx->eig_iters_max = std::max<int64_t>(ctx->eig_iters_max, g_last_iters);
        ctx->rep_iters += g_last_rep_iters;
      } else {
        Scope sc(ctx, DFM_KC_EIG_OTHER);
        const hipError_t e = launch_dense_eig_batched(Gg, m, (int64_t)m * m, m, m, 0, ng, r, lam, Uk, tr, status,
                                                      w.dwk, st);
        if (e != hipSuccess) return fail(ctx, 1000 + (int)e, "dense eigensolver: %s", hipGetErrorString(e));
      }
      if (need_fl) {
        Scope sc(ctx, DFM_KC_FACTORS);
        if (launch_factors(orient, gsrc, T, N, r, ng, Uk, F, L, nullptr, st))
          return fail(ctx, -4, "r=%d too large", r);
      }
      {
        Scope sc(ctx, DFM_KC_STATS);
        hipLaunchKernelGGL(stats_kernel, dim3((ng + 127) / 128), dim3(128), 0, st, ng, T, N, r, 0, crit, (double)NAN,
                           sg, lam, tr, (const double *)nullptr, (const double *)nullptr, (const int *)nullptr,
                           w.sdd, ns, grow, width, status, w.zst, w.flag);
      }
      if (chow) {
        Scope sc(ctx, DFM_KC_CHOW);
        double *LR = nullptr, *LM = nullptr, *WD = nullptr;
        for (int i = 0; i < ns; ++i) {
          if (sd[i].kind == DFM_STAT_LR_ALL) LR = grow + sd[i].off;
          if (sd[i].kind == DFM_STAT_LM_ALL) LM = grow + sd[i].off;
          if (sd[i].kind == DFM_STAT_WALD_ALL) WD = grow + sd[i].off;
        }
        const double *scr;
        if (r <= 16) {
          // launch_chow has no {no C, idx} form: a zero common component selects its {C, idx} one (x + 0 = x)
          const PanelSrc cs{w.zeroC, w.P, gi, nullptr, ld, T};
          const size_t cb = chow_workspace_bytes(T, N, r, ng);
          HIPCHK(ctx, launch_chow(orient, cs, T, N, r, chow_bp, ng, F, L, LR, LM, WD, width, w.chws, cb, st));
          scr = (const double *)(w.chws + cb) - (size_t)3 * ng * N;
        } else {   // the GEMM-built tests on the group's materialised panels
          HIPCHK(ctx, launch_materialize(gsrc, T, N, ld, ng, w.wX, st));
          HIPCHK(ctx, launch_chow_wide(ng, w.wX, ld, (int64_t)T * ld, nullptr, T, N, r, chow_bp, F, (int64_t)T * r, L,
                                       (int64_t)N * r, LR, LM, WD, width, w.wSc, w.wCh, st));
          scr = w.wSc;
        }
        for (int i = 0; i < ns; ++i) {   // single-variable statistics out of the pass's scratch rows
          if (sd[i].kind < DFM_STAT_LR || sd[i].kind > DFM_STAT_WALD) continue;
          const int which = sd[i].kind - DFM_STAT_LR;
          HIPCHK(ctx, hipMemcpy2DAsync(grow + sd[i].off, (size_t)width * 8, scr + ((size_t)which * ng) * N + sd[i].arg1,
                                       (size_t)N * 8, 8, ng, hipMemcpyDeviceToDevice, st));
        }
      }
      if (sup) {
        ChowSweepOut so;
        so.os = width;
        for (int i = 0; i < ns; ++i)
          if (sup_stat(sd[i].kind)) so.sup[sd[i].kind - DFM_STAT_SUPLR_ALL] = grow + sd[i].off;
        HIPCHK(ctx, launch_chow_sweep(gsrc, T, N, r, sup_lo, sup_hi, ng, F, L, so, w.swws, sw_bytes, st, timer_cb,
                                      ctx));
      }
    }
    if (!ident) {   // the groups' rows into panel order
      Scope sc(ctx, DFM_KC_STATS);
      hipLaunchKernelGGL(mc_scatter_rows_kernel, dim3((unsigned)(((int64_t)n * width + 255) / 256)), dim3(256), 0, st,
                         w.rows, w.list, n, width, w.dout);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out + c0 * width, w.dout, (size_t)n * width * 8, hipMemcpyDeviceToHost, st));
  }
  int flag = 0;
  HIPCHK(ctx, hipMemcpyAsync(&flag, w.flag, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (flag & 1) return fail(ctx, 2, "eigensolver did not converge for some panel");
  return 0;
}
