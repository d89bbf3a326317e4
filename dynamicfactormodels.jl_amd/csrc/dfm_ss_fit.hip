// dfm_ss_fit.hip — the fits of the state-space factor model, host code only:
// the two-step estimator of Doz, Giannone & Reichlin (2011) (dfm_ss_fit: dfm_em,
// ss_estimate of dfm_ss_host.h, then ss_smooth_core of dfm_ss.hip), its iteration
// to the quasi-maximum likelihood (dfm_ss_fit_ml: ss_em_core of dfm_ss_em.hip in
// the smoother's place), both with mixed frequencies (dfm_ss_fit_mf) and all of
// them with factor blocks (dfm_ss_fit_blocks: the block-wise start), and the
// two-step estimator with AR(1) idiosyncratic terms (dfm_ss_fit_ar).  The
// steps and the return codes are stated in include/dfm.h.
#include "dfm_host.h"
#include "dfm_ss_host.h"

namespace {

// dfm_ss_fit, and with `ml` dfm_ss_fit_ml: the EM from the two-step parameters
// takes the place of step 5's smoother.
// mf (with a marked series): dfm_ss_fit_mf — the low series' start values by
// ss_mf_start, the padded state, and Lambda ft_t|T for the low columns.
// blocks with bl (checked, a restriction): dfm_ss_fit_blocks — the block-wise
// start in the place of the EM's F and L, and the EM with the blocks.
int ss_fit_impl(dfm_ctx *ctx, const char *who, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
                int horizon, dfm_em_info *info, const dfm_ss_fit_out *out, const dfm_ss_em_spec *ml, double *a0_out,
                double *loglik_path, dfm_ss_em_info *ml_info, const dfm_ss_mf *mf = nullptr, double *agg_out = nullptr,
                const dfm_ss_blocks *blocks = nullptr, const SsBlocks *bl = nullptr) {
  if (!X || !em_spec || !out || T < 2 || N < 1 || ldx < T || horizon < 0) return fail(ctx, -2, "%s: bad arguments", who);
  int ml_iter = 0;
  double ml_tol = 0.0;
  if (ml && ss_em_defaults(ml->max_iter, ml->tol, ml->horizon, &ml_iter, &ml_tol)) return fail(ctx, -2, "%s: bad arguments", who);
  if (p < 1 || p > SS_PMAX) return ss_param_error(ctx, who, p < 1 ? -2 : SS_E_LIMIT, -1);
  const int Lg = mf ? ss_mf_lags(p, mf->n_w) : p;   // lags of the state
  if (em_spec->r > SS_RMAX || (em_spec->r > 0 && em_spec->r * Lg > SS_SMAX)) return ss_param_error(ctx, who, SS_E_LIMIT, -1);
  DeviceShare gate(ctx->device);
  const size_t tn = (size_t)T * N;
  const int cap = 32;
  std::vector<double> Z(tn), mu((size_t)N), sd((size_t)N), F((size_t)T * cap), L((size_t)N * cap), ev(cap), Xh;
  dfm_em_info inf{};
  int rc = dfm_em(ctx, X, T, N, ldx, em_spec, Z.data(), out->em_completed, mu.data(), sd.data(), F.data(), L.data(),
                  ev.data(), &inf);
  if (rc) return rc;
  const int r = inf.r, s = r * p, sp = r * Lg, h = horizon;   // s: the VAR's columns; sp: the state
  if ((rc = ss_check_dims(r, Lg))) return ss_param_error(ctx, who, rc, -1);
  const double *Xs = X;   // the raw panel on the host: its NaN pattern is the mask
  int64_t lds = ldx;
  if (em_spec->dev) {
    Xh.resize(tn);
    hipSetDevice(ctx->device);
    HIPCHK(ctx, hipMemcpy2DAsync(Xh.data(), (size_t)T * 8, X, (size_t)ldx * 8, (size_t)T * 8, (size_t)N,
                                 hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    Xs = Xh.data();
    lds = T;
  }
  std::vector<double> Zm(tn);
  for (int64_t i = 0; i < N; ++i)
    for (int64_t t = 0; t < T; ++t)
      Zm[(size_t)i * T + t] = std::isnan(Xs[(size_t)i * lds + t]) ? NAN : Z[(size_t)i * T + t];
  std::vector<double> sig((size_t)N), A((size_t)r * s), Q((size_t)r * r), P0((size_t)s * s);
  int64_t where = -1;
  if (bl) {   // the block-wise start: every block's principal components of what the blocks before it left
    std::vector<double> R(Z), Rg(tn), Fg((size_t)T * r), Lg((size_t)N * r), evg((size_t)r);
    std::fill(L.begin(), L.begin() + (size_t)N * r, 0.0);
    int off[SS_BMAX + 1];
    for (int g = 0; g <= bl->o.nb; ++g) off[g] = bl->o.off[g];
    for (int g = 0; g < bl->o.nb; ++g) {
      const uint8_t *mem = blocks->member + (size_t)g * N;
      const int rg = off[g + 1] - off[g];
      const int64_t ng = ss_blocks_gather(R.data(), T, N, mem, Rg.data());
      if (ng < rg)
        return fail(ctx, SS_E_VAR, "%s: block %d (0-based) has %lld members, fewer than its %d factors", who, g,
                    (long long)ng, rg);
      if ((rc = dfm_pca(ctx, Rg.data(), T, ng, T, rg, evg.data(), Fg.data(), Lg.data(), nullptr))) return rc;
      ss_blocks_deflate(R.data(), T, N, mem, off[g], rg, Fg.data(), Lg.data(), ng, F.data(), L.data());
    }
    rc = ss_blocks_estimate(Zm.data(), T, N, T, F.data(), L.data(), r, p, bl->o.nb, off, sig.data(), A.data(), Q.data(),
                            P0.data(), &where);
    if (rc == SS_E_VAR)
      return fail(ctx, rc, "%s: block %lld (0-based): the VAR needs T - p > r_g p rows and a non-singular Xl'Xl", who,
                  (long long)where);
  } else {
    rc = ss_estimate(Zm.data(), T, N, T, F.data(), L.data(), r, p, sig.data(), A.data(), Q.data(), P0.data(), &where);
  }
  if (rc) return ss_param_error(ctx, who, rc, where);
  const int64_t Tt = T + h;
  std::vector<double> sm((size_t)Tt * r), agg, Apad;
  if (mf) {
    rc = ss_mf_start(Zm.data(), T, N, T, F.data(), r, mf->w, mf->n_w, mf->low, L.data(), sig.data(), &where,
                     bl ? bl->free : nullptr);
    if (rc == SS_E_VAR)
      return fail(ctx, rc, "%s: low-frequency column %lld (0-based) has fewer than %s + 1 observed rows t >= n_w - 1", who,
                  (long long)where, bl ? "its free factors" : "r");
    if (rc) return ss_param_error(ctx, who, rc, where);
    agg.resize((size_t)Tt * r);
    Apad.resize((size_t)r * sp);
    ss_mf_pad_A(A.data(), r, p, Lg, Apad.data());
    P0.resize((size_t)sp * sp);
    if ((rc = ss_stationary_cov(Apad.data(), Q.data(), r, Lg, P0.data()))) return ss_param_error(ctx, who, rc, -1);
  }
  const double *As = mf ? Apad.data() : A.data();   // the state's A
  if (!ml) {
    const SsParams pr{r, Lg, L.data(), sig.data(), As, Q.data(), nullptr, P0.data()};
    rc = ss_smooth_core(ctx, Zm.data(), 1, T, N, T, (int64_t)tn, false, pr, h, out->filtered, sm.data(),
                        out->smoothed_cov, out->loglik, nullptr, mf, mf ? agg.data() : nullptr);
    if (rc) return rc;
  } else {
    const dfm_ss_params start{r, Lg, L.data(), sig.data(), As, Q.data(), nullptr, P0.data()};
    std::vector<double> L2((size_t)N * r), sig2((size_t)N), A2((size_t)r * s), Q2((size_t)r * r), a02((size_t)sp),
        P02((size_t)sp * sp);
    const dfm_ss_em_out eo{L2.data(), sig2.data(), A2.data(), Q2.data(), a02.data(), P02.data(), out->filtered,
                           sm.data(), out->smoothed_cov, nullptr, loglik_path, mf ? agg.data() : nullptr};
    dfm_ss_em_info mi{};
    rc = ss_em_core(ctx, who, Zm.data(), 1, T, N, T, (int64_t)tn, false, &start, 1, ml_iter, ml_tol, ml->update_init != 0, h,
                    eo, &mi, mf, p, bl);
    if (rc) return rc;
    L = L2, sig = sig2, A = A2, Q = Q2, P0 = P02;
    if (out->loglik) *out->loglik = mi.loglik;
    if (a0_out) std::copy(a02.begin(), a02.end(), a0_out);
    if (ml_info) *ml_info = mi;
  }
  auto put = [](double *dst, const std::vector<double> &v, size_t n) {
    if (dst) std::copy(v.begin(), v.begin() + n, dst);
  };
  put(out->em_standardized, Z, tn);
  put(out->mu, mu, (size_t)N);
  put(out->sd, sd, (size_t)N);
  put(out->em_factors, F, (size_t)T * r);
  put(out->lambda, L, (size_t)N * r);
  put(out->eigvals, ev, (size_t)r);
  put(out->sigma2, sig, (size_t)N);
  put(out->A, A, (size_t)r * s);
  put(out->Q, Q, (size_t)r * r);
  put(out->P0, P0, (size_t)sp * sp);
  put(out->smoothed, sm, (size_t)Tt * r);
  if (mf && agg_out) std::copy(agg.begin(), agg.end(), agg_out);
  // the common component of the smoothed factors, Lambda f_t|T (the fma chain of the EM's); a low-frequency
  // column's is Lambda ft_t|T
  auto common = [&](int64_t t, int64_t i) {
    const double *f = mf && mf->low[i] ? agg.data() : sm.data();
    double c = 0.0;
    for (int j = 0; j < r; ++j) c = fma(f[(size_t)t * r + j], L[(size_t)j * N + i], c);
    return c;
  };
  if (out->x_smoothed || out->x_completed)
    for (int64_t i = 0; i < N; ++i)
      for (int64_t t = 0; t < T; ++t) {
        const double x = Xs[(size_t)i * lds + t];
        const bool obs = !std::isnan(x);
        const double c = obs ? 0.0 : common(t, i);
        if (out->x_smoothed) out->x_smoothed[(size_t)i * T + t] = obs ? Z[(size_t)i * T + t] : c;
        if (out->x_completed) out->x_completed[(size_t)i * T + t] = obs ? x : fma(c, sd[i], mu[i]);
      }
  if (out->forecast)
    for (int64_t i = 0; i < N; ++i)
      for (int64_t k = 0; k < h; ++k) out->forecast[(size_t)i * h + k] = fma(common(T + k, i), sd[i], mu[i]);
  if (info) *info = inf;
  return 0;
}

// dfm_ss_fit_ar: the two-step fit with AR(1) idiosyncratic terms — dfm_em,
// ss_estimate_ar, the smoother at the padded state, then the fill rule
// (ss_ar_fill) on the standardised panel for all three panels.
int ss_fit_ar_impl(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
                   int horizon, dfm_em_info *info, const dfm_ss_fit_out *out, double *rho_out) {
  const char *who = "dfm_ss_fit_ar";
  if (!X || !em_spec || !out || T < 2 || N < 1 || ldx < T || horizon < 0 || horizon > (1 << 20))
    return fail(ctx, -2, "%s: bad arguments", who);
  if (p < 1 || p > SS_PMAX) return ss_ar_error(ctx, who, p < 1 ? -2 : SS_E_LIMIT, -1);
  const int Lg = ss_ar_lags(p);
  if (em_spec->r > SS_AR_RMAX || (em_spec->r > 0 && em_spec->r * Lg > SS_SMAX)) return ss_ar_error(ctx, who, SS_E_LIMIT, -1);
  DeviceShare gate(ctx->device);
  const size_t tn = (size_t)T * N;
  const int cap = 32;
  std::vector<double> Z(tn), mu((size_t)N), sd((size_t)N), F((size_t)T * cap), L((size_t)N * cap), ev(cap), Xh;
  dfm_em_info inf{};
  int rc = dfm_em(ctx, X, T, N, ldx, em_spec, Z.data(), out->em_completed, mu.data(), sd.data(), F.data(), L.data(),
                  ev.data(), &inf);
  if (rc) return rc;
  const int r = inf.r, s = r * p, sp = r * Lg, h = horizon;   // s: the VAR's columns; sp: the state
  if (r > SS_AR_RMAX || ss_check_dims(r, Lg)) return ss_ar_error(ctx, who, SS_E_LIMIT, -1);
  const double *Xs = X;   // the raw panel on the host: its NaN pattern is the mask
  int64_t lds = ldx;
  if (em_spec->dev) {
    Xh.resize(tn);
    hipSetDevice(ctx->device);
    HIPCHK(ctx, hipMemcpy2DAsync(Xh.data(), (size_t)T * 8, X, (size_t)ldx * 8, (size_t)T * 8, (size_t)N,
                                 hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    Xs = Xh.data();
    lds = T;
  }
  std::vector<double> Zm(tn);
  for (int64_t i = 0; i < N; ++i)
    for (int64_t t = 0; t < T; ++t)
      Zm[(size_t)i * T + t] = std::isnan(Xs[(size_t)i * lds + t]) ? NAN : Z[(size_t)i * T + t];
  std::vector<double> sig((size_t)N), rho((size_t)N), A((size_t)r * s), Apad((size_t)r * sp), Q((size_t)r * r),
      P0((size_t)sp * sp);
  int64_t where = -1;
  rc = ss_estimate_ar(Zm.data(), T, N, T, F.data(), L.data(), r, p, sig.data(), A.data(), Q.data(), P0.data(), rho.data(),
                      &where);
  if (rc) return ss_ar_error(ctx, who, rc, where);
  ss_mf_pad_A(A.data(), r, p, Lg, Apad.data());
  const int64_t Tt = T + h;
  std::vector<double> sm((size_t)Tt * r), fill((size_t)Tt * N);
  const SsParams pr{r, Lg, L.data(), sig.data(), Apad.data(), Q.data(), nullptr, P0.data()};
  rc = ss_smooth_core(ctx, Zm.data(), 1, T, N, T, (int64_t)tn, false, pr, h, out->filtered, sm.data(), out->smoothed_cov,
                      out->loglik, nullptr, nullptr, nullptr, nullptr, who, rho.data());
  if (rc) return rc;
  ss_ar_fill(Zm.data(), T, N, T, L.data(), r, rho.data(), sm.data(), h, fill.data());
  auto put = [](double *dst, const std::vector<double> &v, size_t n) {
    if (dst) std::copy(v.begin(), v.begin() + n, dst);
  };
  put(out->em_standardized, Z, tn);
  put(out->mu, mu, (size_t)N);
  put(out->sd, sd, (size_t)N);
  put(out->em_factors, F, (size_t)T * r);
  put(out->lambda, L, (size_t)N * r);
  put(out->eigvals, ev, (size_t)r);
  put(out->sigma2, sig, (size_t)N);
  put(out->A, A, (size_t)r * s);
  put(out->Q, Q, (size_t)r * r);
  put(out->P0, P0, (size_t)sp * sp);
  put(out->smoothed, sm, (size_t)Tt * r);
  put(rho_out, rho, (size_t)N);
  for (int64_t i = 0; i < N; ++i) {
    for (int64_t t = 0; t < T; ++t) {
      const double x = Xs[(size_t)i * lds + t], z = fill[(size_t)i * Tt + t];
      if (out->x_smoothed) out->x_smoothed[(size_t)i * T + t] = z;
      if (out->x_completed) out->x_completed[(size_t)i * T + t] = std::isnan(x) ? fma(z, sd[i], mu[i]) : x;
    }
    for (int64_t k = 0; k < h && out->forecast; ++k)
      out->forecast[(size_t)i * h + k] = fma(fill[(size_t)i * Tt + T + k], sd[i], mu[i]);
  }
  if (info) *info = inf;
  return 0;
}

}  // namespace

extern "C" {

int dfm_ss_fit_ar(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
                  int horizon, dfm_em_info *info, const dfm_ss_fit_out *out, double *rho_out) {
  if (!ctx) return -1;
  return ss_fit_ar_impl(ctx, X, T, N, ldx, em_spec, p, horizon, info, out, rho_out);
}

int dfm_ss_fit(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
               int horizon, dfm_em_info *info, const dfm_ss_fit_out *out) {
  if (!ctx) return -1;
  return ss_fit_impl(ctx, "dfm_ss_fit", X, T, N, ldx, em_spec, p, horizon, info, out, nullptr, nullptr, nullptr, nullptr);
}

int dfm_ss_fit_ml(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
                  const dfm_ss_em_spec *ml_spec, dfm_em_info *info, const dfm_ss_fit_out *out, double *a0_out,
                  double *loglik_path, dfm_ss_em_info *ml_info) {
  if (!ctx) return -1;
  if (!ml_spec) return fail(ctx, -2, "dfm_ss_fit_ml: bad arguments");
  return ss_fit_impl(ctx, "dfm_ss_fit_ml", X, T, N, ldx, em_spec, p, ml_spec->horizon, info, out, ml_spec, a0_out, loglik_path, ml_info);
}

int dfm_ss_fit_mf(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec, int p,
                  const dfm_ss_em_spec *ml_spec, const dfm_ss_mf *mf, int method, dfm_em_info *info,
                  const dfm_ss_fit_out *out, double *a0_out, double *loglik_path, dfm_ss_em_info *ml_info,
                  double *smoothed_agg) {
  const char *who = "dfm_ss_fit_mf";
  if (!ctx) return -1;
  if (!ml_spec || (method != 0 && method != 1)) return fail(ctx, -2, "%s: bad arguments", who);
  // r may be selected by the fit: the limits are checked again once it is known
  int L = 0;
  if (int rc = ss_mf_args(ctx, who, mf, N, true, em_spec && em_spec->r > 0 ? em_spec->r : 1, p, "p, n_w", &L)) return rc;
  if (!L)
    return method ? dfm_ss_fit_ml(ctx, X, T, N, ldx, em_spec, p, ml_spec, info, out, a0_out, loglik_path, ml_info)
                  : dfm_ss_fit(ctx, X, T, N, ldx, em_spec, p, ml_spec->horizon, info, out);
  return ss_fit_impl(ctx, who, X, T, N, ldx, em_spec, p, ml_spec->horizon, info, out, method ? ml_spec : nullptr, a0_out,
                     loglik_path, ml_info, mf, smoothed_agg);
}

int dfm_ss_fit_blocks(dfm_ctx *ctx, const double *X, int64_t T, int64_t N, int64_t ldx, const dfm_em_spec *em_spec,
                      int p, const dfm_ss_em_spec *ml_spec, const dfm_ss_mf *mf, const dfm_ss_blocks *blocks, int method,
                      dfm_em_info *info, const dfm_ss_fit_out *out, double *a0_out, double *loglik_path,
                      dfm_ss_em_info *ml_info, double *smoothed_agg) {
  const char *who = "dfm_ss_fit_blocks";
  if (!ctx) return -1;
  if (!ml_spec || !em_spec || N < 1 || (method != 0 && method != 1)) return fail(ctx, -2, "%s: bad arguments", who);
  if (em_spec->r <= 0) return fail(ctx, -3, "%s: the number of factors must be fixed at the sum of the blocks' sizes", who);
  bool trivial = false;
  SsBlocks bl{};
  std::vector<uint16_t> free;
  if (int rc = ss_blocks_args(ctx, who, blocks, N, em_spec->r, &trivial, &bl, free)) return rc;
  if (trivial) {
    if (mf) return dfm_ss_fit_mf(ctx, X, T, N, ldx, em_spec, p, ml_spec, mf, method, info, out, a0_out, loglik_path, ml_info,
                                 smoothed_agg);
    return method ? dfm_ss_fit_ml(ctx, X, T, N, ldx, em_spec, p, ml_spec, info, out, a0_out, loglik_path, ml_info)
                  : dfm_ss_fit(ctx, X, T, N, ldx, em_spec, p, ml_spec->horizon, info, out);
  }
  int L = 0;
  if (mf)
    if (int rc = ss_mf_args(ctx, who, mf, N, true, em_spec->r, p, "p, n_w", &L)) return rc;
  return ss_fit_impl(ctx, who, X, T, N, ldx, em_spec, p, ml_spec->horizon, info, out, method ? ml_spec : nullptr, a0_out,
                     loglik_path, ml_info, L ? mf : nullptr, L ? smoothed_agg : nullptr, blocks, &bl);
}

}  // extern "C"
