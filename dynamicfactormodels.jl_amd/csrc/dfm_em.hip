// dfm_em.hip — principal components of a panel with missing observations:
// the EM iteration of Stock & Watson (2002) in the form McCracken & Ng (2016)
// use for FRED-MD (factors_em, DEMEAN = 2).  X is T x N with NaN marking a
// missing entry, obs = !isnan(X):
//
//   X2 = X with missing := mean of the column's observed entries
//   (mu, sd), Z = z-score of X2; r fixed or the first arg-min of crit on Z
//   (F, L) = principal_components(Z)[:, 1:r];  C = F L'
//   repeat:  X2 = obs ? X : C * sd + mu   (the mu, sd that produced C)
//            (mu, sd), Z from the new X2; r re-selected when it is not fixed
//            (F, L) again, Cnew = F L'
//            err = ||Cnew - C||_F^2 / ||C||_F^2;  C = Cnew
//   until err <= tol or max_iter iterations.
//
// The loop stays on the device.  Per iteration:
//   em_fill_kernel     fill + column mean / std + z-score in one launch over the
//                      row-major T x ld panel; the raw panel's NaNs are the mask
//   launch_gram        the MFMA Gram of Z (X'X for T >= N, XX' for N > T)
//   eig_run            top-k pairs, warm-started from the previous iteration's
//                      vectors (k = r, or kmax when r is re-selected: then the
//                      warm block keeps its width whatever r^ does)
//   launch_factors     F and L of the first r vectors
//   em_common_kernel   Cnew = F L' over the old C, with per-row partial sums of
//                      (Cnew - C)^2 and C^2; ordered_sum_kernel finishes them
// and only the two sums, the solver's status, the bad-column flag and (when r
// is re-selected) the k eigenvalues and the trace cross to the host, through
// the context's pinned poll slots.
#include "dfm_host.h"

namespace {

constexpr int EM_TR = 64;   // rows per staged tile: one per lane of a column's wave
constexpr int EM_SW = 16;   // strip width: 16 doubles = one 128-B line per row

// Strip blockIdx.x of 16 columns, all T rows: the workgroup owns its columns,
// so a column's sums run in one fixed order whatever the grid.  Every pass
// walks the strip in tiles of 64 rows, 8 lanes x 16 B per row (whole 128-B
// lines of the row-major panels); thread tid touches the same elements
// (row tid >> 3 and + 32, column pair tid & 7) in every pass, so it reads back
// only X2 values it wrote itself.  The statistics are normalize_cols_kernel's
// (dfm_panel.hip): wave w owns columns 4 w .. 4 w + 3 of the strip, lane l sums
// rows l, l + 64, ... in order, wave_sum, the variance accumulated with fma
// around the mean, z = (x - mu) / sd — bit-identical to dfm_normalize_dev for
// a panel without a missing entry.
//   C == nullptr (the initial fill): missing := the mean of the column's
//     observed entries; their count goes to nobs.
//   otherwise missing := C * sd_io + mu_io, the moments that produced C.
//   standardize == 0: mu = 0, sd = 1, Z = X2.
// mu_io / sd_io are read (this strip's 16) before they are rewritten.  A
// column whose std is zero or not finite lowers *badcol to its index.
__global__ __launch_bounds__(256) void em_fill_kernel(const double *__restrict__ Xr, const double *__restrict__ C,
                                                      int T, int N, int64_t ld, int standardize,
                                                      double *__restrict__ X2, double *__restrict__ Z, double *mu_io,
                                                      double *sd_io, int *__restrict__ nobs, int *__restrict__ badcol) {
  __shared__ double tile[EM_TR][EM_SW + 1];
  __shared__ double s_a[EM_SW], s_b[EM_SW];   // fill: (mu0, -) or (mu_old, sd_old); then the new (mu, sd)
  const int c0 = blockIdx.x * EM_SW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cp = tid & 7, r0 = tid >> 3;   // this thread's column pair and first row of a tile
  const bool init = C == nullptr;
  if (init) {   // observed mean and count of every column of the strip
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int cnt[4] = {0, 0, 0, 0};
    for (int t0 = 0; t0 < T; t0 += EM_TR) {
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int row = r0 + 32 * h;
        double2 v = make_double2(0.0, 0.0);
        if (t0 + row < T) v = *reinterpret_cast<const double2 *>(Xr + (int64_t)(t0 + row) * ld + c0 + 2 * cp);
        tile[row][2 * cp] = v.x;
        tile[row][2 * cp + 1] = v.y;
      }
      __syncthreads();
      if (t0 + lane < T) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double x = tile[lane][4 * wave + j];
          if (!isnan(x)) { s[j] += x; ++cnt[j]; }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double sum = wave_sum(s[j]);
      int n = cnt[j];
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o);
      if (lane == 0) {
        s_a[4 * wave + j] = sum / n;
        s_b[4 * wave + j] = 0.0;
        if (c0 + 4 * wave + j < N) nobs[c0 + 4 * wave + j] = n;
      }
    }
  } else if (tid < EM_SW) {
    const bool in = c0 + tid < N;
    s_a[tid] = in ? mu_io[c0 + tid] : 0.0;
    s_b[tid] = in ? sd_io[c0 + tid] : 0.0;
  }
  __syncthreads();
  const double fa0 = s_a[2 * cp], fa1 = s_a[2 * cp + 1], fb0 = s_b[2 * cp], fb1 = s_b[2 * cp + 1];
  const bool in0 = c0 + 2 * cp < N, in1 = c0 + 2 * cp + 1 < N;
  // ---- pass 1: X2, and the column sums
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int t0 = 0; t0 < T; t0 += EM_TR) {
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = r0 + 32 * h;
      double2 v = make_double2(0.0, 0.0);
      if (t0 + row < T) {
        const int64_t o = (int64_t)(t0 + row) * ld + c0 + 2 * cp;
        v = *reinterpret_cast<const double2 *>(Xr + o);
        double2 f = make_double2(fa0, fa1);
        if (!init) {
          const double2 c = *reinterpret_cast<const double2 *>(C + o);
          f.x = fma(c.x, fb0, fa0);
          f.y = fma(c.y, fb1, fa1);
        }
        v.x = in0 ? (isnan(v.x) ? f.x : v.x) : 0.0;
        v.y = in1 ? (isnan(v.y) ? f.y : v.y) : 0.0;
        *reinterpret_cast<double2 *>(X2 + o) = v;
        if (!standardize) *reinterpret_cast<double2 *>(Z + o) = v;
      }
      tile[row][2 * cp] = v.x;
      tile[row][2 * cp + 1] = v.y;
    }
    __syncthreads();
    if (standardize && t0 + lane < T) {
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += tile[lane][4 * wave + j];
    }
  }
  if (!standardize) {
    if (tid < EM_SW && c0 + tid < N) { mu_io[c0 + tid] = 0.0; sd_io[c0 + tid] = 1.0; }
    return;
  }
  double mu[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) mu[j] = wave_sum(s[j]) / T;
  // ---- pass 2: the centred sums of squares
  double q[4] = {0.0, 0.0, 0.0, 0.0};
  for (int t0 = 0; t0 < T; t0 += EM_TR) {
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = r0 + 32 * h;
      double2 v = make_double2(0.0, 0.0);
      if (t0 + row < T) v = *reinterpret_cast<const double2 *>(X2 + (int64_t)(t0 + row) * ld + c0 + 2 * cp);
      tile[row][2 * cp] = v.x;
      tile[row][2 * cp + 1] = v.y;
    }
    __syncthreads();
    if (t0 + lane < T) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { const double d = tile[lane][4 * wave + j] - mu[j]; q[j] = fma(d, d, q[j]); }
    }
  }
  __syncthreads();   // every thread holds its fill values: s_a / s_b now take the new moments
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double sd = sqrt(wave_sum(q[j]) / (T - 1));
    const int c = c0 + 4 * wave + j;
    if (lane == 0) {
      s_a[4 * wave + j] = mu[j];
      s_b[4 * wave + j] = sd;
      if (c < N) {
        mu_io[c] = mu[j];
        sd_io[c] = sd;
        if (!(sd > 0.0) || isinf(sd)) atomicMin(badcol, c);
      }
    }
  }
  __syncthreads();
  // ---- pass 3: Z
  const double m0 = s_a[2 * cp], m1 = s_a[2 * cp + 1], d0 = s_b[2 * cp], d1 = s_b[2 * cp + 1];
  for (int t0 = 0; t0 < T; t0 += EM_TR) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = r0 + 32 * h;
      if (t0 + row < T) {
        const int64_t o = (int64_t)(t0 + row) * ld + c0 + 2 * cp;
        double2 v = *reinterpret_cast<const double2 *>(X2 + o);
        v.x = in0 ? (v.x - m0) / d0 : 0.0;
        v.y = in1 ? (v.y - m1) / d1 : 0.0;
        *reinterpret_cast<double2 *>(Z + o) = v;
      }
    }
  }
}

// Row blockIdx.x of the common component: Cnew[t][n] = sum_j F[t][j] L[n][j]
// (the fma chain of common_residual_kernel) written over the old C, with the
// row's sums of (Cnew - C)^2 and C^2 (old) reduced in a fixed order into
// part[t] and part[T + t].  r <= 32; padding columns stay zero.
__global__ __launch_bounds__(256) void em_common_kernel(const double *__restrict__ F, const double *__restrict__ L,
                                                        int T, int N, int r, int64_t ld, double *__restrict__ C,
                                                        double *__restrict__ part) {
  __shared__ double sF[32];
  __shared__ double red[2][256];
  const int t = blockIdx.x, tid = threadIdx.x;
  if (tid < r) sF[tid] = F[(int64_t)t * r + tid];
  __syncthreads();
  double dd = 0.0, cc = 0.0;
  for (int64_t n = tid; n < ld; n += 256) {
    double c = 0.0;
    if (n < N)
      for (int j = 0; j < r; ++j) c = fma(sF[j], L[n * r + j], c);
    const double old = C[(int64_t)t * ld + n], d = c - old;
    dd = fma(d, d, dd);
    cc = fma(old, old, cc);
    C[(int64_t)t * ld + n] = c;
  }
  red[0][tid] = dd;
  red[1][tid] = cc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
    __syncthreads();
  }
  if (tid == 0) { part[t] = red[0][0]; part[T + t] = red[1][0]; }
}

// What a run leaves on the device for its caller (freed with the object).
struct EmRun {
  hipStream_t st = nullptr;
  DevPanel raw;                 // the caller's panel, row-major, NaN = missing
  double *arena = nullptr;      // every double buffer below
  int *ints = nullptr;          // nobs (N), badcol, eigensolver status
  char *ews = nullptr;          // eigensolver workspace
  double *X2p = nullptr, *Zp = nullptr, *Cp = nullptr, *mu = nullptr, *sd = nullptr, *G = nullptr, *lam = nullptr,
         *tr = nullptr, *Uk[2] = {nullptr, nullptr}, *Ur = nullptr, *F = nullptr, *L = nullptr, *part = nullptr,
         *sums = nullptr, *Zc = nullptr, *X2c = nullptr;
  int r = 0, k = 0, cur = 0;
  std::vector<double> hlam;     // the last solve's k eigenvalues
  dfm_em_info info{};
  ~EmRun() {
    if (arena) hipFreeAsync(arena, st);
    if (ints) hipFreeAsync(ints, st);
    if (ews) hipFreeAsync(ews, st);
  }
};

// The loop.  On success run.Zc / run.X2c hold the completed panels column-major
// (T x N, leading dimension T), run.mu / run.sd / run.F / run.L / run.hlam the
// rest, run.r the final number of factors.
int em_core(dfm_ctx *ctx, const double *X, int64_t T64, int64_t N64, int64_t ldx, const dfm_em_spec *spec,
            EmRun &run) {
  if (!X || !spec || T64 < 2 || N64 < 1 || ldx < T64) return fail(ctx, -2, "dfm_em: bad arguments");
  if (T64 > (1 << 24) || N64 > (1 << 24)) return fail(ctx, -2, "panel too large");
  const int T = (int)T64, N = (int)N64, m = std::min(T, N), mfn = ceil_half(m);
  const bool select = spec->r <= 0;
  const int crit = spec->crit;
  if (select) {
    if (crit < 0 || crit > 6) return fail(ctx, -3, "dfm_em: selecting r needs a criterion (got %d)", crit);
    if (crit <= 2)
      return fail(ctx, -3, "dfm_em: a PCp criterion needs the full spectrum in every iteration; "
                           "select r with ICp1-3 or BIC");
  }
  auto block_ok = [&](int k) { const int p = eig_block_p(m, k, ctx->block); return p >= k && p <= 32; };
  int k;   // eigenpairs per solve
  if (select) {
    k = spec->kmax > 0 ? std::min(spec->kmax, mfn) : mfn;
    if (spec->kmax <= 0)
      while (k > 1 && !block_ok(k)) --k;
    if (!block_ok(k)) return fail(ctx, -7, "dfm_em: kmax = %d exceeds the subspace block of the eigensolver", k);
  } else {
    k = std::min(spec->r, mfn);
    if (!block_ok(k) || k > 32) return fail(ctx, -7, "dfm_em: r = %d exceeds the subspace block of the eigensolver", k);
  }
  const int max_iter = spec->max_iter > 0 ? spec->max_iter : 50;
  const double tol = spec->tol < 0 ? 1e-6 : spec->tol;
  const int standardize = spec->standardize != 0;
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  run.st = st;
  int rc = upload_panel(ctx, X, T, N, ldx, run.raw, spec->dev != 0);
  if (rc) return rc;
  const int64_t ld = run.raw.ld;
  const int orient = (N > T) ? 0 : 1;
  // ---- one arena, carved in 128-B units
  const size_t panel = (size_t)T * ld;
  size_t off = 0;
  auto carve = [&](size_t n) { const size_t o = off; off += (size_t)round_up((int64_t)n, 16); return o; };
  const size_t oX2 = carve(panel), oZ = carve(panel), oC = carve(panel), omu = carve(N), osd = carve(N),
               oG = carve((size_t)m * m), olam = carve(k), otr = carve(1), oU0 = carve((size_t)m * k),
               oU1 = carve((size_t)m * k), oUr = carve((size_t)m * k), oF = carve((size_t)T * k),
               oL = carve((size_t)N * k), opart = carve((size_t)2 * T), osums = carve(2),
               oZc = carve((size_t)T * N), oX2c = carve((size_t)T * N);
  HIPCHK(ctx, stream_malloc((void **)&run.arena, off * 8, st));
  HIPCHK(ctx, stream_malloc((void **)&run.ints, ((size_t)N + 2) * 4, st));
  double *A = run.arena;
  run.X2p = A + oX2; run.Zp = A + oZ; run.Cp = A + oC; run.mu = A + omu; run.sd = A + osd; run.G = A + oG;
  run.lam = A + olam; run.tr = A + otr; run.Uk[0] = A + oU0; run.Uk[1] = A + oU1; run.Ur = A + oUr; run.F = A + oF;
  run.L = A + oL; run.part = A + opart; run.sums = A + osums; run.Zc = A + oZc; run.X2c = A + oX2c;
  int *nobs = run.ints, *badcol = run.ints + N, *status = run.ints + N + 1;
  const int p = eig_block_p(m, k, ctx->block), P = p <= 16 ? 16 : 32;
  HIPCHK(ctx, stream_malloc((void **)&run.ews, eig_workspace_bytes_padded(m, 1, P, ctx->maxit), st));
  HIPCHK(ctx, hipMemsetAsync(run.Cp, 0, panel * 8, st));
  HIPCHK(ctx, hipMemsetAsync(badcol, 0x7f, 4, st));
  HIPCHK(ctx, hipMemsetAsync(status, 0, 4, st));
  // ---- the pinned slots of one iteration's read-back: doubles {d, c, trace, lam[k]}, then ints {bad, status}
  const int nd = 3 + k;
  std::vector<double> pageable;
  double *slot;
  if (ctx_poll(ctx) && (size_t)ctx->pollbuf.cap * sizeof(int) >= (size_t)(nd + 1) * 8) slot = (double *)ctx->pollbuf.host;
  else { pageable.resize(nd + 1); slot = pageable.data(); }
  int *islot = (int *)(slot + nd);
  const dim3 fgrid((unsigned)(ld / EM_SW));
  auto fill = [&](const double *C) {
    Scope sc(ctx, DFM_KC_MISC);
    hipLaunchKernelGGL(em_fill_kernel, fgrid, dim3(256), 0, st, run.raw.P, C, T, N, ld, standardize, run.X2p, run.Zp,
                       run.mu, run.sd, nobs, badcol);
  };
  const PanelSrc src{nullptr, run.Zp, nullptr, nullptr, ld, 0};
  run.hlam.assign(k, 0.0);
  int r = select ? 0 : k;
  double err = INFINITY;
  auto bad_sd = [&]() -> int {
    return islot[0] < N ? fail(ctx, -8, "dfm_em: column %d (0-based) has zero standard deviation", islot[0]) : 0;
  };
  // PCA of the resident Z and the common component over run.Cp; reads back the
  // iteration's scalars.  warm: start from the previous solve's vectors.
  auto step = [&](bool warm) -> int {
    HIPCHK(ctx, panel_gram(ctx, orient, src, T, N, run.G));
    // (the run's own workspace: no allocation, free or synchronise per solve)
    if ((rc = run_eig(ctx, run.G, m, k, run.lam, run.Uk[run.cur ^ 1], run.tr, status, run.ews,
                      warm ? run.Uk[run.cur] : nullptr)))
      return rc;
    run.cur ^= 1;
    const double *U = run.Uk[run.cur];
    if (select) {   // r^ = first arg-min of crit over 1..k on this Z: the k eigenvalues and the trace
      HIPCHK(ctx, hipMemcpyAsync(slot + 2, run.tr, 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(slot + 3, run.lam, (size_t)k * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(islot, badcol, 8, hipMemcpyDeviceToHost, st));   // badcol, status
      HIPCHK(ctx, hipStreamSynchronize(st));
      if ((rc = bad_sd())) return rc;   // before the solver's status: a NaN column keeps it from converging
      if (islot[1]) return fail(ctx, 2, "eigensolver did not converge");
      std::vector<double> ic((size_t)7 * k);
      dfm_ic_sweep(slot + 3, k, k, slot[2], T, N, NAN, ic.data());
      r = first_argmin(&ic[(size_t)crit * k], k);
    }
    if (r < k) {   // the first r of the k vectors, contiguous
      HIPCHK(ctx, hipMemcpy2DAsync(run.Ur, (size_t)r * 8, U, (size_t)k * 8, (size_t)r * 8, m, hipMemcpyDeviceToDevice,
                                   st));
      U = run.Ur;
    }
    {
      Scope sc(ctx, DFM_KC_FACTORS);
      if (launch_factors(orient, src, T, N, r, 1, U, run.F, run.L, nullptr, st)) return fail(ctx, -7, "r=%d too large", r);
    }
    {
      Scope sc(ctx, DFM_KC_MISC);
      hipLaunchKernelGGL(em_common_kernel, dim3(T), dim3(256), 0, st, run.F, run.L, T, N, r, ld, run.Cp, run.part);
      hipLaunchKernelGGL(ordered_sum_kernel, dim3(1), dim3(256), 0, st, run.part, T, run.sums);
      hipLaunchKernelGGL(ordered_sum_kernel, dim3(1), dim3(256), 0, st, run.part + T, T, run.sums + 1);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(slot, run.sums, 16, hipMemcpyDeviceToHost, st));
    if (!select) HIPCHK(ctx, hipMemcpyAsync(slot + 3, run.lam, (size_t)k * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(islot, badcol, 8, hipMemcpyDeviceToHost, st));   // badcol, status
    HIPCHK(ctx, hipStreamSynchronize(st));
    if ((rc = bad_sd())) return rc;
    if (islot[1]) return fail(ctx, 2, "eigensolver did not converge");
    std::copy(slot + 3, slot + 3 + k, run.hlam.begin());
    return 0;
  };
  // ---- the initial fill: the columns' observed means
  fill(nullptr);
  HIPCHK(ctx, hipGetLastError());
  std::vector<int> hn(N);
  HIPCHK(ctx, hipMemcpyAsync(hn.data(), nobs, (size_t)N * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  int64_t seen = 0;
  for (int j = 0; j < N; ++j) {
    if (hn[j] < 2)
      return fail(ctx, -8, "dfm_em: column %d (0-based) has %d observed entries; at least 2 are needed", j, hn[j]);
    seen += hn[j];
  }
  const int64_t n_missing = (int64_t)T * N - seen;
  rc = step(false);
  if (rc) return rc;
  // ---- the iteration.  A panel without a missing entry never changes: its
  // solves start cold, so the repeated fit reproduces C bit for bit (err == 0).
  int it = 0;
  while (err > tol && it < max_iter) {
    ++it;
    fill(run.Cp);
    rc = step(n_missing > 0);
    if (rc) return rc;
    err = slot[0] / slot[1];
  }
  {
    Scope sc(ctx, DFM_KC_MISC);
    const dim3 g((N + 31) / 32, (T + 31) / 32);
    hipLaunchKernelGGL(colmajor_from_rows_kernel, g, dim3(256), 0, st, run.Zp, ld, T, N, run.Zc);
    hipLaunchKernelGGL(colmajor_from_rows_kernel, g, dim3(256), 0, st, run.X2p, ld, T, N, run.X2c);
  }
  HIPCHK(ctx, hipGetLastError());
  run.r = r;
  run.k = k;
  run.info.iterations = it;
  run.info.converged = err <= tol ? 1 : 0;
  run.info.r = r;
  run.info.pad = 0;
  run.info.err = err;
  run.info.n_missing = n_missing;
  return 0;
}

}  // namespace

extern "C" {

int dfm_em(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *spec, double *Z,
           double *X2, double *mu, double *sd, double *F, double *L, double *eigvals, dfm_em_info *info) {
  if (!ctx) return -1;
  DeviceShare gate(ctx->device);
  EmRun run;
  int rc = em_core(ctx, X, T, N, ldx, spec, run);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  const size_t tn = (size_t)T * N * 8;
  if (Z) HIPCHK(ctx, hipMemcpyAsync(Z, run.Zc, tn, hipMemcpyDeviceToHost, st));
  if (X2) HIPCHK(ctx, hipMemcpyAsync(X2, run.X2c, tn, hipMemcpyDeviceToHost, st));
  if (mu) HIPCHK(ctx, hipMemcpyAsync(mu, run.mu, (size_t)N * 8, hipMemcpyDeviceToHost, st));
  if (sd) HIPCHK(ctx, hipMemcpyAsync(sd, run.sd, (size_t)N * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (F && (rc = read_rows_colmajor(ctx, run.F, (int)T, run.r, F))) return rc;
  if (L && (rc = read_rows_colmajor(ctx, run.L, (int)N, run.r, L))) return rc;
  if (eigvals) std::copy(run.hlam.begin(), run.hlam.begin() + run.r, eigvals);
  if (info) *info = run.info;
  return 0;
}

int dfm_model_fit_em(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw, const double *X, int64_t T,
                     int64_t N, int64_t ldx, const dfm_em_spec *spec, dfm_model **out, dfm_em_info *info) {
  if (!ctx || !out) return -1;
  *out = nullptr;
  if (!y || T < 2 || q < 0 || (q > 0 && (!w || ldw < T))) return fail(ctx, -2, "dfm_model_fit_em: bad arguments");
  for (int64_t t = 0; t < T; ++t)
    if (std::isnan(y[t])) return fail(ctx, -2, "dfm_model_fit_em: y[%lld] is NaN", (long long)t);
  for (int j = 0; j < q; ++j)
    for (int64_t t = 0; t < T; ++t)
      if (std::isnan(w[(size_t)j * ldw + t]))
        return fail(ctx, -2, "dfm_model_fit_em: w[%lld, %d] is NaN", (long long)t, j);
  DeviceShare gate(ctx->device);
  EmRun run;
  int rc = em_core(ctx, X, T, N, ldx, spec, run);
  if (rc) return rc;
  // the workhorse fit of the resident completed panel at the final r, cold: the
  // model of dfm_model_fit(y, w, Z, r) bit for bit
  dfm_model *M = nullptr;
  rc = dfm_model_fit(ctx, y, w, q, ldw, run.Zc, T, N, T, run.r, spec->crit >= 0 && spec->crit <= 6 ? spec->crit : -1,
                     spec->kmax, &M);
  if (rc) return rc;
  hipStream_t st = ctx->stream;
  M->em_mu.resize(N);
  M->em_sd.resize(N);
  hipError_t e = dalloc(&M->emX2, (size_t)T * N);
  if (e == hipSuccess) e = hipMemcpyAsync(M->emX2, run.X2c, (size_t)T * N * 8, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(M->em_mu.data(), run.mu, (size_t)N * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(M->em_sd.data(), run.sd, (size_t)N * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    dfm_model_destroy(M);
    return fail(ctx, 1000 + (int)e, "dfm_model_fit_em: %s", hipGetErrorString(e));
  }
  if (info) *info = run.info;
  *out = M;
  return 0;
}

int dfm_model_em_read(const dfm_model *m, double *X2, double *mu, double *sd) {
  if (!m || !m->emX2) return -1;
  dfm_ctx *ctx = m->ctx;
  if (mu) std::copy(m->em_mu.begin(), m->em_mu.end(), mu);
  if (sd) std::copy(m->em_sd.begin(), m->em_sd.end(), sd);
  if (X2) {
    hipSetDevice(ctx->device);
    HIPCHK(ctx, hipMemcpyAsync(X2, m->emX2, (size_t)m->T * m->N * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return 0;
}

}  // extern "C"
