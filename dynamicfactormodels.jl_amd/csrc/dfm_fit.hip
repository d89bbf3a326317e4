// dfm_fit.hip — the fit and everything read from or computed on a fitted
// model: dfm_model_fit(_breaks), the model readers / setters, destroy and
// clone, the model-level criterion / Chow / hard-threshold entry points and
// predict / get_factors.  (The steps over a bare panel are in dfm_panel.hip.)
#include "dfm_host.h"

// the half-built model of a fit: destroyed on every return that does not release it
struct ModelGuard {
  dfm_model *m;
  explicit ModelGuard(dfm_model *m_) : m(m_) {}
  ModelGuard(const ModelGuard &) = delete;
  ModelGuard &operator=(const ModelGuard &) = delete;
  ~ModelGuard() { if (m) dfm_model_destroy(m); }
  dfm_model *release() { dfm_model *r = m; m = nullptr; return r; }
};

extern "C" {

int dfm_model_destroy(dfm_model *m) {
  if (!m) return -1;
  for (int j = 0; j < dfm_model::kMaxLanes - 1; ++j) {
    delete m->lane_worker[j];
    m->lane_worker[j] = nullptr;
    if (m->lane[j]) {   // the lane model, then its context (the model held the last reference but one)
      dfm_ctx *lc = m->lane[j]->ctx;
      hipSetDevice(lc->device);
      hipStreamSynchronize(lc->stream);
      merge_kid(m->ctx, lc);   // its unread kernel timings
      auto &kd = m->ctx->kids;
      kd.erase(std::remove(kd.begin(), kd.end(), lc), kd.end());
      dfm_model_destroy(m->lane[j]);
      dfm_ctx_destroy(lc);
      m->lane[j] = nullptr;
    }
  }
  hipSetDevice(m->ctx->device);
  hipStreamSynchronize(m->ctx->stream);
  for (double *p : {m->Xp, m->Cp, m->Ep, m->y, m->w, m->F, m->Lall, m->Ub, m->colssr, m->H, m->EL, m->S,
                    m->cF, m->hd, m->FtF, m->FSF, m->Kwk, m->A0wk})
    hipFree(p);
  hipFree(m->H32);
  hipFree(m->Hs);
  hipFree(m->emX2);
  for (size_t j = 1; j < m->Ubs.size(); ++j) hipFree(m->Ubs[j]);
  hipFree(m->ws);
  hipFree(m->sw_ws);
  hipFree(m->sd_dev);
  hipFree(m->flag_dev);
  dfm_ctx *ctx = m->ctx;
  delete m;
  ctx_release(ctx);
  return 0;
}

int dfm_model_fit(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw,
                  const double *X, int64_t T64, int64_t N64, int64_t ldx, int r, int crit, int kmax,
                  dfm_model **out) {
  return dfm_model_fit_breaks(ctx, y, w, q, ldw, X, T64, N64, ldx, r, crit, kmax, nullptr, 0, out);
}

int dfm_model_fit_breaks(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw,
                         const double *X, int64_t T64, int64_t N64, int64_t ldx, int r, int crit,
                         int kmax, const int64_t *breaks, int nbreaks, dfm_model **out) {
  if (!ctx || !out) return -1;
  DeviceShare gate(ctx->device);
  *out = nullptr;
  if (!y || !X || T64 < 2 || N64 < 1 || ldx < T64 || q < 0 || (q > 0 && (!w || ldw < T64)))
    return fail(ctx, -2, "dfm_model_fit: bad arguments");
  if (T64 > (1 << 24) || N64 > (1 << 24)) return fail(ctx, -2, "panel too large");
  if (crit < -1 || crit > 6) return fail(ctx, -3, "unknown criterion %d", crit);
  if (r <= 0 && crit < 0) return fail(ctx, -3, "IC sweep needs a criterion");
  if (nbreaks < 0 || (nbreaks > 0 && !breaks)) return fail(ctx, -2, "dfm_model_fit: bad break list");
  for (int j = 0; j < nbreaks; ++j)   // src/DynamicFactorModel.jl:73: vcat(1, breaks, T+1)
    if (breaks[j] <= (j ? breaks[j - 1] : 0) || breaks[j] >= T64)
      return fail(ctx, -9, "break indices must increase strictly inside 1..T-1 (0-based rows)");
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const int T = (int)T64, N = (int)N64, m = std::min(T, N);
  const int mfn = ceil_half(m);  // max_factor_number, src/DynamicFactorModel.jl:101
  dfm_model *M = new dfm_model();
  ModelGuard guard(M);   // declared before the temporaries: they are freed first
  ++ctx->refs;
  M->ctx = ctx; M->T = T; M->N = N; M->q = q; M->crit = crit; M->m = m;
  // src/DynamicFactorModel.jl:77 (T >= N) vs :86 (N > T), with the FULL-sample
  // T and N for every break block (:72, defect D7)
  M->orient = (N > T) ? 0 : 1;
  M->ld = round_up(N, 16);
  const int nblk = nbreaks + 1;
  M->nblk = nblk;
  for (int j = 0; j < nblk; ++j) {
    const int a = j ? (int)breaks[j - 1] : 0, e = j < nbreaks ? (int)breaks[j] : T;
    M->ba.push_back(a);
    M->bt.push_back(e - a);
    M->bm.push_back(M->orient == 0 ? e - a : N);   // size of the block's Gram
  }
  const bool nob = nblk == 1;
  // per block: the Gram (block 0 borrows Gfull when there are no breaks) and the eigenpairs of the last solve
  std::vector<const double *> Gb(nblk, nullptr);
  std::vector<DevBuf<>> Gown(nblk), lamd(nblk), Ukd(nblk);
  DevBuf<> Xraw, Gfull, tr_d;
  DevBuf<int> st_d;
  const size_t panel = (size_t)T * M->ld;
  HIPCHK(ctx, dalloc(&M->Xp, panel));
  HIPCHK(ctx, dalloc(&M->Cp, panel));
  HIPCHK(ctx, dalloc(&M->Ep, panel));
  HIPCHK(ctx, dalloc(&M->y, T));
  HIPCHK(ctx, dalloc(&M->w, (size_t)T * std::max(q, 1)));
  HIPCHK(ctx, Xraw.alloc((size_t)T * N));
  // host or device inputs (hipMemcpyDefault: the windows driver refits from a resident panel)
  HIPCHK(ctx, hipMemcpy2DAsync(Xraw.p, (size_t)T * 8, X, (size_t)ldx * 8, (size_t)T * 8, N, hipMemcpyDefault, st));
  HIPCHK(ctx, hipMemcpyAsync(M->y, y, (size_t)T * 8, hipMemcpyDefault, st));
  if (q > 0)
    HIPCHK(ctx, hipMemcpy2DAsync(M->w, (size_t)T * 8, w, (size_t)ldw * 8, (size_t)T * 8, q, hipMemcpyDefault, st));
  {
    Scope sc(ctx, DFM_KC_MISC);
    hipLaunchKernelGGL(panel_from_colmajor_kernel, dim3((unsigned)((M->ld + 31) / 32), (T + 31) / 32),
                       dim3(256), 0, st, Xraw.p, (int64_t)T, T, N, M->Xp, M->ld);
  }
  HIPCHK(ctx, hipGetLastError());
  // block j's panel: rows ba[j] .. ba[j] + bt[j] - 1 of X
  auto block_src = [&](int j) { return PanelSrc{nullptr, M->Xp + (size_t)M->ba[j] * M->ld, nullptr, nullptr, M->ld, 0}; };
  const bool pcp = crit >= 0 && crit <= 2;
  if (kmax <= 0) kmax = mfn;  // src/DynamicFactorModel.jl:54 (D11)
  kmax = std::min(kmax, mfn);
  M->kmax = kmax;
  const double NT = (double)N * (double)T;
  // --- PCp's sigma^2 = V(ceil(m/2)) of the UNRESTRICTED fit DynamicFactorModel(y, w, x):
  // full sample, no breaks (src/criteria.jl:18, :23, :28)
  std::vector<double> spec_full;
  // the sweep reports all 7 criteria: PCp rows need sigma^2 (NaN when the full
  // spectrum is out of reach and the chosen criterion is not a PCp one)
  const bool full_spec = pcp || (nob && r <= 0 && (kmax > 24 || m <= spectrum_max()));
  if (full_spec && m > spectrum_any_max())
    return fail(ctx, -30, "PCp criteria / kmax > 24 need the full spectrum; supported for "
                          "min(T,N) <= %d (got %d)", spectrum_any_max(), m);
  int rc = 0;
  if (nob || full_spec) {
    HIPCHK(ctx, Gfull.alloc((size_t)m * m));
    HIPCHK(ctx, panel_gram(ctx, M->orient, PanelSrc{nullptr, M->Xp, nullptr, nullptr, M->ld, 0}, T, N, Gfull.p));
  }
  if (full_spec) {
    if ((rc = gram_spectrum(ctx, Gfull.p, m, spec_full))) return rc;
    M->sigma2 = sigma2_total_minus_top(spec_full.data(), m, NT);
  }
  // --- per block: Gram, the eigenvalues the sweep needs, trace
  std::vector<int> kk(nblk, 0);
  std::vector<std::vector<double>> bev(nblk), blam(nblk);
  std::vector<double> btr(nblk, 0.0);
  HIPCHK(ctx, tr_d.alloc(1));
  HIPCHK(ctx, st_d.alloc(1));
  auto top_eig = [&](int j, int k) -> int {
    HIPCHK(ctx, lamd[j].alloc(k)); HIPCHK(ctx, Ukd[j].alloc((size_t)M->bm[j] * k));
    kk[j] = k;
    int rc2 = run_eig(ctx, Gb[j], M->bm[j], k, lamd[j].p, Ukd[j].p, tr_d.p, st_d.p);
    if (rc2) return rc2;
    int est = 0;
    blam[j].resize(k);
    HIPCHK(ctx, hipMemcpyAsync(blam[j].data(), lamd[j].p, (size_t)k * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(&btr[j], tr_d.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(&est, st_d.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (est) return fail(ctx, 2, "eigensolver did not converge");
    return 0;
  };
  const int r_req = (r <= 0) ? kmax : std::min(r, mfn);
  for (int j = 0; j < nblk; ++j) {
    // the reference slices F_j[:, 1:k] (:33, :131): a block needs >= k eigenpairs
    if (M->bm[j] < r_req)
      return fail(ctx, -9, "break block %d has %d rows: fewer than the %d factors requested", j, M->bt[j], r_req);
    if (nob) Gb[j] = Gfull.p;
    else {
      if (Gown[j].alloc((size_t)M->bm[j] * M->bm[j]) != hipSuccess) return fail(ctx, 1002, "out of memory");
      if (panel_gram(ctx, M->orient, block_src(j), M->bt[j], N, Gown[j].p) != hipSuccess)
        return fail(ctx, 1001, "block Gram failed");
      Gb[j] = Gown[j].p;
    }
    if (r <= 0) {   // the sweep's eigenvalues of this block
      if (nob && full_spec) bev[j] = spec_full;
      else if (!nob && M->bm[j] <= spectrum_any_max() && (kmax > 24 || pcp)) {
        if ((rc = gram_spectrum(ctx, Gb[j], M->bm[j], bev[j]))) return rc;
      } else if (kmax > 24) {
        return fail(ctx, -30, "kmax > 24 needs the full spectrum of every block; supported for Gram "
                              "size <= %d (block %d: %d)", spectrum_any_max(), j, M->bm[j]);
      }
      if (bev[j].empty()) {   // top-k pairs: the sweep's eigenvalues and the trace
        if ((rc = top_eig(j, kmax))) return rc;
        bev[j] = blam[j];
      } else {                // a spectrum gave the eigenvalues: only the trace (the Gram's diagonal)
        hipLaunchKernelGGL(eig_trace_kernel, dim3(1), dim3(64), 0, st, Gb[j], (int64_t)M->bm[j],
                           (int64_t)M->bm[j] * M->bm[j], M->bm[j], tr_d.p);
        HIPCHK(ctx, hipMemcpyAsync(&btr[j], tr_d.p, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
      }
    } else {
      if ((rc = top_eig(j, r_req))) return rc;
      bev[j] = blam[j];
    }
  }
  double trace = 0.0;
  for (int j = 0; j < nblk; ++j) trace += btr[j];
  // eigenvalue i summed over blocks: V(k) = (trace - sum_{i<=k} ev[i]) / (N T)
  const int n_ev = (int)bev[0].size();
  std::vector<double> ev(n_ev, 0.0);
  for (int j = 0; j < nblk; ++j)
    for (int i = 0; i < n_ev && i < (int)bev[j].size(); ++i) ev[i] += bev[j][i];
  if (r <= 0) {
    M->swept = true;
    M->ic.assign(7 * kmax, 0.0);
    dfm_ic_sweep(ev.data(), (int)ev.size(), kmax, trace, T, N, full_spec ? M->sigma2 : NAN, M->ic.data());
    r = first_argmin(&M->ic[(size_t)crit * kmax], kmax);
  }
  r = std::min(r, mfn);   // src/DynamicFactorModel.jl:116-119
  M->r = r;
  for (int j = 0; j < nblk; ++j)
    if (r > kk[j] && (rc = top_eig(j, r))) return rc;   // the sweep used spectra: now the r eigenvectors
  // eigenvalues reported: kmax of the sweep (when it ran) or r; per block summed
  {
    const size_t ne = (size_t)(M->swept ? std::max(kmax, r) : r);
    M->lam.assign(ne, NAN);
    for (size_t j = 0; j < ne && j < ev.size(); ++j) M->lam[j] = ev[j];
    for (int i = 0; i < r; ++i) {
      double s = 0.0;
      for (int j = 0; j < nblk; ++j) s += blam[j][i];
      M->lam[i] = s;
    }
    M->blam.resize(nblk);
    for (int j = 0; j < nblk; ++j) M->blam[j].assign(blam[j].begin(), blam[j].begin() + r);
  }
  M->k_eig = kk[0];
  // --- factors, loadings per block for r (first r canonical eigenvectors)
  HIPCHK(ctx, dalloc(&M->F, (size_t)T * r));
  HIPCHK(ctx, dalloc(&M->colssr, N));
  M->Ubs.assign(nblk, nullptr);
  M->Ls.assign(nblk, nullptr);
  HIPCHK(ctx, dalloc(&M->Lall, (size_t)nblk * N * r));
  for (int j = 0; j < nblk; ++j) {
    const int mj = M->bm[j];
    HIPCHK(ctx, dalloc(&M->Ubs[j], (size_t)mj * r));
    M->Ls[j] = M->Lall + (size_t)j * N * r;
    if (j == 0) { M->Ub = M->Ubs[0]; M->L = M->Ls[0]; }
    HIPCHK(ctx, hipMemcpy2DAsync(M->Ubs[j], (size_t)r * 8, Ukd[j].p, (size_t)kk[j] * 8, (size_t)r * 8, mj,
                                 hipMemcpyDeviceToDevice, st));
  }
  for (int j = 0; j < nblk; ++j) {
    Scope sc(ctx, DFM_KC_FACTORS);
    if (r <= 32) {
      if (launch_factors(M->orient, block_src(j), M->bt[j], N, r, 1, M->Ubs[j], M->F + (size_t)M->ba[j] * r,
                         M->Ls[j], nob ? M->colssr : nullptr, st, (double)T, 0))
        return fail(ctx, -4, "r=%d too large", r);
    } else if (launch_factors_wide(M->orient, M->Xp + (size_t)M->ba[j] * M->ld, M->ld, M->bt[j], N, r, M->Ubs[j],
                                   M->F + (size_t)M->ba[j] * r, M->Ls[j], nob ? M->colssr : nullptr, st,
                                   (double)T)) {
      return fail(ctx, 1001, "factor kernels failed");
    }
    if (nob && M->orient == 1) {
      DevBuf<> lr;
      HIPCHK(ctx, lr.alloc(r));
      HIPCHK(ctx, hipMemcpyAsync(lr.p, lamd[0].p, (size_t)r * 8, hipMemcpyDeviceToDevice, st));
      hipLaunchKernelGGL(colssr_cols_kernel, dim3((N + 255) / 256, 1), dim3(256), 0, st, Gfull.p, m,
                         (int64_t)m * m, N, r, lr.p, M->Ub, M->colssr);
      HIPCHK(ctx, hipStreamSynchronize(st));
    }
  }
  for (int j = 0; j < nblk; ++j) {   // :33 per subperiod
    Scope sc(ctx, DFM_KC_MISC);
    const size_t o = (size_t)M->ba[j] * M->ld;
    hipLaunchKernelGGL(common_residual_kernel, dim3((unsigned)((M->ld + 255) / 256), M->bt[j]), dim3(256), 0,
                       st, M->Xp + o, M->ld, M->bt[j], N, r, M->F + (size_t)M->ba[j] * r, M->Ls[j], M->Cp + o,
                       M->Ep + o);
  }
  HIPCHK(ctx, hipGetLastError());
  if (!nob)
    hipLaunchKernelGGL(col_ssq_kernel, dim3((N + 255) / 256), dim3(256), 0, st, M->Ep, M->ld, T, N, M->colssr);
  // --- V(r) by brute force over the explicit residual panel (src/criteria.jl:5)
  double essq = 0.0;
  DevBuf<> rows, tot;
  HIPCHK(ctx, rows.alloc(T)); HIPCHK(ctx, tot.alloc(1));
  hipLaunchKernelGGL(panel_row_ssq_kernel, dim3(T), dim3(256), 0, st, M->Ep, M->ld, T, rows.p);
  hipLaunchKernelGGL(ordered_sum_kernel, dim3(1), dim3(256), 0, st, rows.p, T, tot.p);
  HIPCHK(ctx, hipMemcpyAsync(&essq, tot.p, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  // --- OLS + HC2 on [w vcat(F_j)] (:40-48, :130-133)
  const int d = q + r;
  if (d > T) return fail(ctx, -5, "q + r = %d regressors exceed the %d observations", d, T);
  DevBuf<> coef, tst, cov, res, wk;
  DevBuf<int> ost;
  HIPCHK(ctx, coef.alloc(d)); HIPCHK(ctx, tst.alloc(d)); HIPCHK(ctx, cov.alloc((size_t)d * d));
  HIPCHK(ctx, res.alloc(T)); HIPCHK(ctx, ost.alloc(1));
  if (d <= 32) {
    Scope sc(ctx, DFM_KC_OLS);
    launch_ols(1, st, M->y, M->w, q, M->F, T, r, nullptr, nullptr, coef.p, tst.p, cov.p, res.p, ost.p);
  } else {   // wide design: GEMM-built OLS (dfm_wide.hip)
    HIPCHK(ctx, wk.alloc((size_t)ols_wide_work(T, d)));
    Scope sc(ctx, DFM_KC_OLS);
    HIPCHK(ctx, launch_ols_wide(M->y, M->w, q, M->F, T, r, coef.p, tst.p, cov.p, res.p, ost.p, wk.p, st));
  }
  HIPCHK(ctx, hipGetLastError());
  M->coef.resize(d); M->tstat.resize(d); M->cov.resize((size_t)d * d); M->resid.resize(T);
  int ols_bad = 0;
  HIPCHK(ctx, hipMemcpyAsync(M->coef.data(), coef.p, (size_t)d * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(M->tstat.data(), tst.p, (size_t)d * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(M->cov.data(), cov.p, (size_t)d * d * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(M->resid.data(), res.p, (size_t)T * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(&ols_bad, ost.p, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (ols_bad) return fail(ctx, 3, "singular design matrix D'D");
  M->trace = trace;
  M->V = essq / NT;
  if (crit >= 0) M->critval = criterion(crit, M->V, r, M->sigma2, T, N);
  HIPCHK(ctx, dalloc(&M->flag_dev, 4));
  *out = guard.release();
  return 0;
}

int dfm_model_blocks(const dfm_model *m) { return m ? m->nblk : -1; }

int dfm_model_block(const dfm_model *m, int j, int64_t *row0, int64_t *rows, double *eigvals, double *L) {
  if (!m) return -1;
  if (j < 0 || j >= m->nblk) return fail(m->ctx, -2, "block %d out of range", j);
  if (row0) *row0 = m->ba[j];
  if (rows) *rows = m->bt[j];
  if (eigvals) std::copy(m->blam[j].begin(), m->blam[j].end(), eigvals);
  if (L) {
    hipSetDevice(m->ctx->device);
    return read_rows_colmajor(m->ctx, m->Ls[j], m->N, m->r, L);
  }
  return 0;
}

int dfm_model_dims(const dfm_model *m, int64_t *r, int64_t *kmax, int64_t *n_eig) {
  if (!m) return -1;
  if (r) *r = m->r;
  if (kmax) *kmax = m->swept ? m->kmax : 0;
  if (n_eig) *n_eig = (int64_t)m->lam.size();
  return 0;
}

int dfm_model_scalars(const dfm_model *m, int64_t *r, double *V, double *cv, double *tr) {
  if (!m) return -1;
  if (r) *r = m->r;
  if (V) *V = m->V;
  if (cv) *cv = m->critval;
  if (tr) *tr = m->trace;
  return 0;
}

int dfm_model_read(const dfm_model *m, double *eigvals, double *coef, double *tstat, double *coef_cov,
                   double *ols_resid, double *F, double *L, double *E, double *ic_values) {
  if (!m) return -1;
  dfm_ctx *ctx = m->ctx;
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  if (eigvals) std::copy(m->lam.begin(), m->lam.end(), eigvals);
  if (coef) std::copy(m->coef.begin(), m->coef.end(), coef);
  if (tstat) std::copy(m->tstat.begin(), m->tstat.end(), tstat);
  if (coef_cov) std::copy(m->cov.begin(), m->cov.end(), coef_cov);
  if (ols_resid) std::copy(m->resid.begin(), m->resid.end(), ols_resid);
  if (ic_values && !m->ic.empty()) std::copy(m->ic.begin(), m->ic.end(), ic_values);
  if (F && read_rows_colmajor(ctx, m->F, m->T, m->r, F)) return fail(ctx, 1001, "copy F");
  if (L && read_rows_colmajor(ctx, m->L, m->N, m->r, L)) return fail(ctx, 1001, "copy L");
  if (E) {
    DevBuf<> d_out;
    HIPCHK(ctx, d_out.alloc((size_t)m->T * m->N));
    hipLaunchKernelGGL(colmajor_from_rows_kernel, dim3((m->N + 31) / 32, (m->T + 31) / 32), dim3(256), 0,
                       st, m->Ep, m->ld, m->T, m->N, d_out.p);
    HIPCHK(ctx, hipMemcpyAsync(E, d_out.p, (size_t)m->T * m->N * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  return 0;
}

int dfm_model_set_mode(dfm_model *m, int mode) {
  if (!m || mode < 0 || mode > 2) return -1;
  m->mode = mode;
  return 0;
}

int dfm_model_fact_block(const dfm_model *m, int *p, int *pz) {
  if (!m) return -1;
  const int b = (m->orient == 0 && m->mode != 1 && m->r >= 1 && m->r <= 16 && m->T <= fact_t_max() && m->nblk == 1)
                    ? fact_block_p(m->m, m->r, m->ctx->block) : 0;
  if (p) *p = b;
  if (pz) *pz = (b + 1) & ~1;
  return b > 0 ? 0 : 1;
}

int dfm_model_set_batch(dfm_model *m, int64_t batch) {
  if (!m || batch < 0) return -1;
  m->batch = batch;
  return 0;
}

int64_t dfm_stats_width(const dfm_model *m, const dfm_stat *stats, int nstats) {
  if (!m || (!stats && nstats)) return -1;
  int64_t w = 0;
  for (int i = 0; i < nstats; ++i) w += stat_width(m, stats[i].kind);
  return w;
}

// criterion_<name>(dfm) of a fitted model (src/criteria.jl:17-53) at its r:
// V(r) is the model's; PCp's sigma^2 is V(ceil(m/2)) of the unrestricted
// 3-arg fit DynamicFactorModel(y, w, x) (:18, :23, :28; no breaks, D2): the
// spectral tail of the resident panel's full Gram spectrum, computed once.
int dfm_model_criterion(dfm_model *M, int crit, double *value) {
  if (!M || !value) return -1;
  dfm_ctx *ctx = M->ctx;
  if (crit < 0 || crit > 6) return fail(ctx, -31, "unknown criterion %d", crit);
  DeviceShare gate(ctx->device);
  if (crit <= 2 && std::isnan(M->sigma2)) {
    const int m = M->m;
    if (m > spectrum_any_max())
      return fail(ctx, -30, "PCp criteria need the full spectrum: supported for min(T,N) <= %d", spectrum_any_max());
    hipSetDevice(ctx->device);
    DevBuf<> G;
    HIPCHK(ctx, G.alloc((size_t)m * m));
    HIPCHK(ctx, panel_gram(ctx, M->orient, PanelSrc{nullptr, M->Xp, nullptr, nullptr, M->ld, 0}, M->T, M->N, G.p));
    std::vector<double> ev;
    const int rc = gram_spectrum(ctx, G.p, m, ev);
    if (rc) return rc;
    M->sigma2 = sigma2_total_minus_top(ev.data(), m, (double)M->N * M->T);   // as the fit's sigma^2
  }
  *value = criterion(crit, M->V, M->r, M->sigma2, M->T, M->N);
  return 0;
}

// One variable's LR / LM / Wald (src/chowtest.jl:19-42): the all-variables
// kernel runs once per break period and the model keeps its N x 3 results,
// so a caller's loop over the variables costs one pass over the panel.
int dfm_chow(dfm_model *M, int64_t bp, int64_t i, double *LR, double *LM, double *Wald) {
  if (!M) return -1;
  if (i < 0 || i >= M->N) return fail(M->ctx, -2, "variable index %lld out of range", (long long)i);
  if (M->chow_bp != bp) {
    std::vector<double> c((size_t)3 * M->N);
    int rc = dfm_chow_all(M, bp, c.data(), c.data() + M->N, c.data() + 2 * M->N);
    if (rc) return rc;
    M->chow_cache.swap(c);
    M->chow_bp = bp;
  }
  if (LR) *LR = M->chow_cache[(size_t)i];
  if (LM) *LM = M->chow_cache[(size_t)M->N + i];
  if (Wald) *Wald = M->chow_cache[(size_t)2 * M->N + i];
  return 0;
}

int dfm_chow_all(dfm_model *M, int64_t bp, double *LR, double *LM, double *Wald) {
  if (!M) return -1;
  dfm_ctx *ctx = M->ctx;
  if (bp < M->r || bp > M->T - M->r) return fail(ctx, -7, "break period %lld out of range", (long long)bp);
  if (M->nblk > 64) return fail(ctx, -7, "Chow statistics support at most 64 break blocks");
  DeviceShare gate(ctx->device);
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  if (M->r > 16) {   // any r: the GEMM-built tests (dfm_wide.hip)
    DevBuf wk, sc3;
    HIPCHK(ctx, dalloc(&wk.p, (size_t)chow_wide_work(M->T, M->N, M->r)));
    HIPCHK(ctx, dalloc(&sc3.p, (size_t)3 * M->N));
    {
      Scope sc(ctx, DFM_KC_CHOW);
      HIPCHK(ctx, launch_chow_wide(1, M->Xp, M->ld, 0, M->Ep, M->T, M->N, M->r, (int)bp, M->F, 0, M->L, 0, nullptr,
                                   nullptr, nullptr, M->N, sc3.p, wk.p, st));
    }
    double *outs[3] = {LR, LM, Wald};
    for (int i = 0; i < 3; ++i)
      if (outs[i]) HIPCHK(ctx, hipMemcpyAsync(outs[i], sc3.p + (size_t)i * M->N, (size_t)M->N * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
  }
  const size_t bytes = chow_workspace_bytes(M->T, M->N, M->r, 1);
  char *ws = nullptr;
  HIPCHK(ctx, hipMalloc(&ws, bytes));
  PanelSrc src{nullptr, M->Xp, nullptr, nullptr, M->ld, 0};
  {
    Scope sc(ctx, DFM_KC_CHOW);
    HIPCHK(ctx, launch_chow(M->orient, src, M->T, M->N, M->r, (int)bp, 1, M->F, M->L, nullptr, nullptr,
                            nullptr, M->N, ws, bytes, st, M->nblk, M->ba.data(), (int64_t)M->N * M->r));
  }
  const double *scr = (const double *)(ws + bytes) - (size_t)3 * M->N;
  double *outs[3] = {LR, LM, Wald};
  for (int i = 0; i < 3; ++i)
    if (outs[i]) HIPCHK(ctx, hipMemcpyAsync(outs[i], scr + (size_t)i * M->N, (size_t)M->N * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  hipFree(ws);
  return 0;
}

// Every break period bp_lo..bp_hi in one device pass (dfm_chow_sweep.hip).
int dfm_chow_sweep(dfm_model *M, int64_t bp_lo, int64_t bp_hi, int stats, double *LR, double *LM, double *Wald,
                   double *sup, int64_t *argsup) {
  if (!M) return -1;
  dfm_ctx *ctx = M->ctx;
  if (bp_lo > bp_hi || bp_lo < M->r || bp_hi > M->T - M->r)
    return fail(ctx, -7, "break period range %lld..%lld outside %d..%d", (long long)bp_lo, (long long)bp_hi, M->r,
                M->T - M->r);
  if (M->nblk > 1) return fail(ctx, -7, "dfm_chow_sweep needs a model fitted without breaks");
  if (M->r > 16) return fail(ctx, -7, "dfm_chow_sweep supports r <= 16 (r = %d)", M->r);
  if (stats < 0 || stats > 7) return fail(ctx, -2, "dfm_chow_sweep: stats mask %d", stats);
  if (stats == 0) stats = 7;
  DeviceShare gate(ctx->device);
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const int N = M->N, nbp = (int)(bp_hi - bp_lo + 1);
  double *curves[3] = {LR, LM, Wald};
  const bool red = sup || argsup;
  DevBuf dcur, dsup;
  int64_t *darg = nullptr;
  ChowSweepOut so;
  so.os = N;
  int ncur = 0;
  for (int s = 0; s < 3; ++s) ncur += curves[s] ? 1 : 0;
  if (ncur) HIPCHK(ctx, dalloc(&dcur.p, (size_t)ncur * nbp * N));
  if (sup) HIPCHK(ctx, dalloc(&dsup.p, (size_t)3 * N));
  if (argsup) HIPCHK(ctx, dalloc(&darg, (size_t)3 * N));
  for (int s = 0, c = 0; s < 3; ++s) {
    if (curves[s]) so.curve[s] = dcur.p + (size_t)(c++) * nbp * N;
    if (red && (stats >> s & 1)) {
      if (sup) so.sup[s] = dsup.p + (size_t)s * N;
      if (argsup) so.argsup[s] = darg + (size_t)s * N;
    }
  }
  const size_t bytes = chow_sweep_workspace_bytes(M->T, N, M->r, nbp, 1);
  DevBuf ws;
  hipError_t e = dalloc(&ws.p, bytes / 8);
  PanelSrc src{nullptr, M->Xp, nullptr, nullptr, M->ld, 0};
  if (e == hipSuccess)
    e = launch_chow_sweep(src, M->T, N, M->r, (int)bp_lo, (int)bp_hi, 1, M->F, M->L, so, (char *)ws.p, bytes, st,
                          timer_cb, ctx);
  for (int s = 0; s < 3 && e == hipSuccess; ++s) {
    if (curves[s])
      e = hipMemcpyAsync(curves[s], so.curve[s], (size_t)nbp * N * 8, hipMemcpyDeviceToHost, st);
    const bool done = so.sup[s] || so.argsup[s];
    if (e == hipSuccess && sup) {
      if (done) e = hipMemcpyAsync(sup + (size_t)s * N, so.sup[s], (size_t)N * 8, hipMemcpyDeviceToHost, st);
      else std::fill(sup + (size_t)s * N, sup + (size_t)(s + 1) * N, (double)NAN);
    }
    if (e == hipSuccess && argsup) {
      if (done) e = hipMemcpyAsync(argsup + (size_t)s * N, so.argsup[s], (size_t)N * 8, hipMemcpyDeviceToHost, st);
      else std::fill(argsup + (size_t)s * N, argsup + (size_t)(s + 1) * N, (int64_t)-1);
    }
  }
  const hipError_t es = hipStreamSynchronize(st);
  hipFree(darg);
  HIPCHK(ctx, e);
  HIPCHK(ctx, es);
  return 0;
}

int dfm_targeted_hard(dfm_ctx *ctx, const double *y, const double *w, int q, int64_t ldw,
                      const double *X, int64_t T64, int64_t N64, int64_t ldx, int mode,
                      double crit_value, double *tstat, uint8_t *mask) {
  if (!ctx) return -1;
  if (!y || !X || !tstat || !mask || T64 < 2 || N64 < 1 || ldx < T64 || q < 0 || (q > 0 && (!w || ldw < T64)))
    return fail(ctx, -2, "dfm_targeted_hard: bad arguments");
  if (mode != DFM_TP_JOINT && mode != DFM_TP_PER_CANDIDATE) return fail(ctx, -2, "bad mode");
  const int T = (int)T64, N = (int)N64;
  if (mode == DFM_TP_JOINT && q + N >= T)
    return fail(ctx, 3, "joint hard thresholding is singular for q + N >= T (defect D8); use PER_CANDIDATE");

  if (mode == DFM_TP_PER_CANDIDATE && (q < 1 || q > 16)) return fail(ctx, -32, "PER_CANDIDATE needs 1 <= q <= 16");
  DeviceShare gate(ctx->device);
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  DevPanel dp;
  int rc = upload_panel(ctx, X, T, N, ldx, dp);
  if (rc) return rc;
  double *dy = nullptr, *dw = nullptr, *dt = nullptr;
  uint8_t *dm = nullptr;
  int *bad = nullptr;
  char *ws = nullptr;
  const size_t wsb = targeted_workspace_bytes(mode, T, N, q);
  HIPCHK(ctx, dalloc(&dy, T)); HIPCHK(ctx, dalloc(&dw, (size_t)T * std::max(q, 1)));
  HIPCHK(ctx, dalloc(&dt, N)); HIPCHK(ctx, hipMalloc(&dm, N)); HIPCHK(ctx, dalloc(&bad, 1));
  HIPCHK(ctx, hipMalloc(&ws, wsb));
  HIPCHK(ctx, hipMemcpyAsync(dy, y, (size_t)T * 8, hipMemcpyHostToDevice, st));
  if (q > 0) HIPCHK(ctx, hipMemcpy2DAsync(dw, (size_t)T * 8, w, (size_t)ldw * 8, (size_t)T * 8, q, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemsetAsync(bad, 0, 4, st));
  if (mode == DFM_TP_JOINT && q + N > 64) {   // any width: GEMM-built OLS with HC0 (dfm_wide.hip)
    DevBuf wk;
    HIPCHK(ctx, dalloc(&wk.p, (size_t)targeted_joint_wide_work(T, q, N, dp.ld)));
    Scope sc(ctx, DFM_KC_MISC);
    HIPCHK(ctx, launch_targeted_joint_wide(dy, dw, q, dp.P, dp.ld, T, N, crit_value, dt, dm, bad, wk.p, st));
  } else {
    Scope sc(ctx, DFM_KC_MISC);
    HIPCHK(ctx, launch_targeted(mode, dy, dw, q, dp.P, dp.ld, T, N, crit_value, dt, dm, ws, wsb, st, bad));
  }
  int hb = 0;
  HIPCHK(ctx, hipMemcpyAsync(tstat, dt, (size_t)N * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(mask, dm, (size_t)N, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(&hb, bad, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  hipFree(dy); hipFree(dw); hipFree(dt); hipFree(dm); hipFree(bad); hipFree(ws);
  if (hb) return fail(ctx, 3, "singular design matrix");
  return 0;
}

}  // extern "C"

// ---- get_factors / predict on new rows (src/DynamicFactorModel.jl:125-128,
// :152-155; D4 repaired, dfm_predict.hip).  x_new (nn x N) and w_new (nn x q)
// column-major, host or device memory (hipMemcpyDefault); outputs host.
static int predict_impl(dfm_model *M, int64_t nn, const double *w_new, int64_t ldw, const double *x_new,
                        int64_t ldx, double *F_out, double *yhat) {
  if (!M) return -1;
  dfm_ctx *ctx = M->ctx;
  const int q = M->q, r = M->r, N = M->N, T = M->T;
  if (nn < 1 || !x_new || ldx < nn || (yhat && q > 0 && (!w_new || ldw < nn)) || (!F_out && !yhat))
    return fail(ctx, -2, "dfm_predict: bad arguments");
  DeviceShare gate(ctx->device);
  hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  double *xd = nullptr, *wd = nullptr, *bd = nullptr, *wk = nullptr, *Fd = nullptr, *yd = nullptr;
  struct Fr { std::vector<double *> v; ~Fr() { for (double *p : v) hipFree(p); } } fr;
  auto al = [&](double **p, size_t n) { hipError_t e = dalloc(p, n); if (e == hipSuccess) fr.v.push_back(*p); return e; };
  HIPCHK(ctx, al(&xd, (size_t)nn * N));
  HIPCHK(ctx, al(&wd, (size_t)nn * std::max(q, 1)));
  HIPCHK(ctx, al(&bd, (size_t)q + r));
  HIPCHK(ctx, al(&wk, (size_t)T + 2));
  HIPCHK(ctx, al(&Fd, (size_t)nn * std::max(r, 1)));
  HIPCHK(ctx, al(&yd, (size_t)nn));
  HIPCHK(ctx, hipMemcpy2DAsync(xd, (size_t)nn * 8, x_new, (size_t)ldx * 8, (size_t)nn * 8, N, hipMemcpyDefault, st));
  if (yhat && q > 0)
    HIPCHK(ctx, hipMemcpy2DAsync(wd, (size_t)nn * 8, w_new, (size_t)ldw * 8, (size_t)nn * 8, q, hipMemcpyDefault, st));
  HIPCHK(ctx, hipMemcpyAsync(bd, M->coef.data(), (size_t)(q + r) * 8, hipMemcpyHostToDevice, st));
  {
    Scope sc(ctx, DFM_KC_MISC);
    HIPCHK(ctx, launch_predict(M->Xp, M->ld, T, N, M->L, r, xd, nn, nn, wd, nn, q, yhat ? bd : nullptr, wk, Fd, yd,
                               st));
  }
  if (F_out) HIPCHK(ctx, hipMemcpyAsync(F_out, Fd, (size_t)nn * r * 8, hipMemcpyDeviceToHost, st));
  if (yhat) HIPCHK(ctx, hipMemcpyAsync(yhat, yd, (size_t)nn * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return 0;
}

extern "C" int dfm_get_factors(dfm_model *m, int64_t n_new, const double *x_new, int64_t ldx, double *F_out) {
  if (!F_out) return m ? fail(m->ctx, -2, "dfm_get_factors: output required") : -1;
  return predict_impl(m, n_new, nullptr, 0, x_new, ldx, F_out, nullptr);
}

extern "C" int dfm_predict(dfm_model *m, int64_t n_new, const double *w_new, int64_t ldw, const double *x_new,
                           int64_t ldx, double *out) {
  if (!out) return m ? fail(m->ctx, -2, "dfm_predict: output required") : -1;
  return predict_impl(m, n_new, w_new, ldw, x_new, ldx, nullptr, out);
}

// ------------------------------------------------------------ multi-device
// A fitted model copied onto another context (another GPU, or a second
// context of the same GPU): every device buffer and host field, so the copy's
// bootstrap replicates are bit-identical to the original's.
extern "C" int dfm_model_clone(const dfm_model *S, dfm_ctx *ctx, dfm_model **out) {
  if (!S || !ctx || !out) return -1;
  *out = nullptr;
  dfm_ctx *sc = S->ctx;
  DeviceShare gate_src(sc->device), gate_dst(ctx->device);
  hipSetDevice(sc->device);
  HIPCHK(ctx, hipStreamSynchronize(sc->stream));
  dfm_model *M = new dfm_model();
  ++ctx->refs;
  M->ctx = ctx;
  M->T = S->T; M->N = S->N; M->q = S->q; M->r = S->r; M->crit = S->crit; M->kmax = S->kmax; M->m = S->m;
  M->orient = S->orient; M->k_eig = S->k_eig; M->swept = S->swept; M->ld = S->ld;
  M->lam = S->lam; M->coef = S->coef; M->tstat = S->tstat; M->cov = S->cov; M->resid = S->resid; M->ic = S->ic;
  M->trace = S->trace; M->V = S->V; M->critval = S->critval; M->sigma2 = S->sigma2;
  M->batch = S->batch; M->mode = S->mode;
  M->nblk = S->nblk; M->ba = S->ba; M->bt = S->bt; M->bm = S->bm; M->blam = S->blam;
  // device-to-device (peer) copies: no staging through host memory.  They are
  // issued on the NEW context's stream and completed before the clone is
  // returned: hipMemcpyPeer would run them on the legacy null stream, which
  // returns before a device-to-device copy lands and which the context's
  // non-blocking stream does not wait for — round 4's intermittent wrong
  // two-lane rows were the second lane's first kernels (H = E E', EL = E L,
  // F S F', the warm start) reading a partly copied fit
  // (tests/test_gpu_multi.py::test_clone_is_complete_before_its_first_bootstrap)
  auto dup = [&](const double *src, size_t n, double **dst) -> int {
    hipSetDevice(ctx->device);
    if (dalloc(dst, n) != hipSuccess) return 1;
    if (!src || n == 0) return 0;
    return hipMemcpyPeerAsync(*dst, ctx->device, src, sc->device, n * 8, ctx->stream) == hipSuccess ? 0 : 1;
  };
  const size_t T = S->T, N = S->N, r = S->r, panel = T * S->ld;
  int bad = 0;
  bad |= dup(S->Xp, panel, &M->Xp);
  bad |= dup(S->Cp, panel, &M->Cp);
  bad |= dup(S->Ep, panel, &M->Ep);
  bad |= dup(S->y, T, &M->y);
  bad |= dup(S->w, T * std::max(S->q, 1), &M->w);
  bad |= dup(S->F, T * r, &M->F);
  bad |= dup(S->colssr, N, &M->colssr);
  bad |= dup(S->Lall, (size_t)S->nblk * N * r, &M->Lall);
  M->Ubs.assign(S->nblk, nullptr);
  M->Ls.assign(S->nblk, nullptr);
  for (int j = 0; j < S->nblk && !bad; ++j) {
    bad |= dup(S->Ubs[j], (size_t)S->bm[j] * r, &M->Ubs[j]);
    M->Ls[j] = M->Lall + (size_t)j * N * r;
  }
  M->Ub = M->Ubs.empty() ? nullptr : M->Ubs[0];
  M->L = M->Lall;
  if (S->emX2 && !bad) {   // a dfm_model_fit_em model stays one
    bad |= dup(S->emX2, T * N, &M->emX2);
    M->em_mu = S->em_mu; M->em_sd = S->em_sd;
  }
  hipSetDevice(ctx->device);
  if (!bad) bad = dalloc(&M->flag_dev, 4) != hipSuccess;
  if (!bad) bad = hipStreamSynchronize(ctx->stream) != hipSuccess;   // every copy landed
  if (bad) {
    dfm_model_destroy(M);
    return fail(ctx, 1002, "dfm_model_clone: device copy failed");
  }
  *out = M;
  return 0;
}
