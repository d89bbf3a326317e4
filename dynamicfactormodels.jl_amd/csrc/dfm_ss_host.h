// dfm_ss_host.h — the host arithmetic of the state-space pass (dfm_ss.hip):
// the limits, the companion form of a VAR(p), the stationary covariance by the
// doubling iteration, the argument checks of the smoother's parameters and
// steps 2-3 of the two-step fit (dfm_ss_fit.hip: idiosyncratic variances,
// VAR(p) by OLS), and of the quasi-ML EM (dfm_ss_em.hip) the spec's defaults,
// the stopping rule and the checks; of the mixed-frequency model the limits,
// [A 0], Z_l and the fit's start values of the low series; of the factor
// blocks the checks, the free mask and the fit's block-wise start; of the AR(1)
// idiosyncratic terms the limits, the checks of rho, its two-step estimate and
// the fill rule; the panels per
// pass of both drivers; of the simulation smoother (dfm_ss_sim.hip) the
// factor of a positive semi-definite matrix, the count of normals, the
// argument checks and the draws per pass; of the news decomposition
// (dfm_ss_news.hip) the argument checks, the check of the release list, the
// revised panel and the releases per pass.
// No HIP includes: a plain C++ compiler builds it alone (tests/c_harness).
//
// Layout: every matrix the caller passes is column-major (include/dfm.h);
// the companion matrix, the state covariances and the r x r innovation
// covariance used inside the library are row-major.
#pragma once
#include <math.h>
#include <stdint.h>
#include <vector>

namespace dfm {

constexpr int SS_RMAX = 16, SS_PMAX = 8, SS_SMAX = 32;

// Return codes of the state-space entry points (beside the library's -2 / -7)
constexpr int SS_E_LIMIT = -7;        // r, p or s = r p beyond the limits
constexpr int SS_E_SIGMA = -10;       // a non-positive idiosyncratic variance
constexpr int SS_E_VAR = -11;         // T - p <= r p, or a singular Xl'Xl
constexpr int SS_E_NAN = -12;         // NaN in Lambda, sigma^2, A, Q, a0 or P0
constexpr int SS_E_SINGULAR = 5;      // Q, a P_{t+1|t} or a G not invertible
constexpr int SS_E_EXPLOSIVE = 6;     // the VAR is not stationary

inline int ss_check_dims(int r, int p) {
  if (r < 1 || p < 1) return -2;
  if (r > SS_RMAX || p > SS_PMAX || r * p > SS_SMAX) return SS_E_LIMIT;
  return 0;
}

// Companion matrix Tm (s x s row-major) of A = [A_1 ... A_p] (r x rp
// column-major): A in the first r rows, the identity shift below.
inline void ss_companion(const double *A, int r, int p, double *Tm) {
  const int s = r * p;
  for (int e = 0; e < s * s; ++e) Tm[e] = 0.0;
  for (int i = 0; i < r; ++i)
    for (int k = 0; k < s; ++k) Tm[i * s + k] = A[(size_t)k * r + i];
  for (int i = r; i < s; ++i) Tm[i * s + (i - r)] = 1.0;
}

// One doubling step: P <- P + M P M', M <- M M (s x s row-major; W: 2 s^2 scratch).
inline void ss_doubling_step(double *P, double *M, int s, double *W) {
  double *MP = W, *MM = W + (size_t)s * s;
  for (int i = 0; i < s; ++i)
    for (int j = 0; j < s; ++j) {
      double a = 0.0, b = 0.0;
      for (int k = 0; k < s; ++k) {
        a += M[i * s + k] * P[k * s + j];
        b += M[i * s + k] * M[k * s + j];
      }
      MP[i * s + j] = a;
      MM[i * s + j] = b;
    }
  for (int i = 0; i < s; ++i)
    for (int j = 0; j < s; ++j) {
      double a = 0.0;
      for (int k = 0; k < s; ++k) a += MP[i * s + k] * M[j * s + k];
      P[i * s + j] += a;
    }
  for (int e = 0; e < s * s; ++e) M[e] = MM[e];
}

// Solution of P = Tm P Tm' + Qs (Qs: Q in the top-left r x r block) by the
// doubling iteration from P = Qs, M = Tm; stops when max|M| < 1e-40.
// A, Q column-major; P0 s x s (symmetric).  SS_E_EXPLOSIVE after 60 doublings
// or at the first non-finite entry.
inline int ss_stationary_cov(const double *A, const double *Q, int r, int p, double *P0) {
  const int rc = ss_check_dims(r, p);
  if (rc) return rc;
  if (!A || !Q || !P0) return -2;
  const int s = r * p;
  for (int e = 0; e < r * s; ++e)
    if (isnan(A[e])) return SS_E_NAN;
  for (int e = 0; e < r * r; ++e)
    if (isnan(Q[e])) return SS_E_NAN;
  std::vector<double> M((size_t)s * s), P((size_t)s * s, 0.0), W((size_t)2 * s * s);
  ss_companion(A, r, p, M.data());
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < r; ++j) P[i * s + j] = Q[(size_t)j * r + i];
  for (int it = 0; it < 60; ++it) {
    ss_doubling_step(P.data(), M.data(), s, W.data());
    double big = 0.0;
    for (int e = 0; e < s * s; ++e) {
      if (!isfinite(M[e]) || !isfinite(P[e])) return SS_E_EXPLOSIVE;
      big = fmax(big, fabs(M[e]));
    }
    if (big < 1e-40) {
      for (int i = 0; i < s; ++i)
        for (int j = 0; j < s; ++j) P0[i * s + j] = 0.5 * (P[i * s + j] + P[j * s + i]);
      return 0;
    }
  }
  return SS_E_EXPLOSIVE;
}

// Cholesky of the n x n row-major SPD matrix G in place (lower triangle);
// false on a non-positive pivot.
inline bool ss_cholesky(double *G, int n) {
  for (int j = 0; j < n; ++j) {
    double d = G[j * n + j];
    for (int k = 0; k < j; ++k) d -= G[j * n + k] * G[j * n + k];
    if (!(d > 0.0) || !isfinite(d)) return false;
    d = sqrt(d);
    G[j * n + j] = d;
    for (int i = j + 1; i < n; ++i) {
      double v = G[i * n + j];
      for (int k = 0; k < j; ++k) v -= G[i * n + k] * G[j * n + k];
      G[i * n + j] = v / d;
    }
  }
  return true;
}

// The smoother's parameters: dims, NaN, non-positive variances.  *where: the
// offending column of sigma^2 (SS_E_SIGMA).  a0, P0 may be null.
inline int ss_check_params(int64_t N, int r, int p, const double *L, const double *sigma2, const double *A,
                           const double *Q, const double *a0, const double *P0, int64_t *where) {
  const int rc = ss_check_dims(r, p);
  if (rc) return rc;
  if (!L || !sigma2 || !A || !Q || N < 1) return -2;
  const int s = r * p;
  auto any_nan = [](const double *v, size_t n) {
    for (size_t e = 0; e < n; ++e)
      if (isnan(v[e])) return true;
    return false;
  };
  if (any_nan(L, (size_t)N * r) || any_nan(sigma2, (size_t)N) || any_nan(A, (size_t)r * s) ||
      any_nan(Q, (size_t)r * r) || (a0 && any_nan(a0, (size_t)s)) || (P0 && any_nan(P0, (size_t)s * s)))
    return SS_E_NAN;
  for (int64_t i = 0; i < N; ++i)
    if (!(sigma2[i] > 0.0) || isinf(sigma2[i])) {
      if (where) *where = i;
      return SS_E_SIGMA;
    }
  return 0;
}

// Step 2 of the two-step fit: sigma2_i = sum_t m_ti (Z_ti - f_t' lambda_i)^2 / n_i.
// Zm: T x N column-major (ldz >= T), NaN = missing; F: T x r column-major
// (ld T); L: N x r column-major (ld N).  *where names the column of a failed
// variance (SS_E_SIGMA).
inline int ss_idio_var(const double *Zm, int64_t T, int64_t N, int64_t ldz, const double *F, const double *L, int r,
                       double *sigma2, int64_t *where) {
  for (int64_t i = 0; i < N; ++i) {
    double ss = 0.0;
    int64_t n = 0;
    for (int64_t t = 0; t < T; ++t) {
      const double z = Zm[(size_t)i * ldz + t];
      if (isnan(z)) continue;
      double c = 0.0;
      for (int j = 0; j < r; ++j) c = fma(F[(size_t)j * T + t], L[(size_t)j * N + i], c);
      ss += (z - c) * (z - c);
      ++n;
    }
    const double v = n > 0 ? ss / (double)n : 0.0;
    sigma2[i] = v;
    if (!(v > 0.0) || isinf(v)) {
      if (where) *where = i;
      return SS_E_SIGMA;
    }
  }
  return 0;
}

// Step 3: VAR(p) by OLS without intercept on F (T x r column-major, ld T):
//   Y = F[p:], Xl = [F[p-1:T-1], ..., F[0:T-p]],
//   A' = (Xl'Xl)^-1 Xl'Y, U = Y - Xl A', Q = U'U / (T - p)
// A (r x rp) and Q (r x r) column-major.  SS_E_VAR for T - p <= r p or a
// singular Xl'Xl, SS_E_SINGULAR for a Q that is not positive definite.
inline int ss_var_ols(const double *F, int64_t T, int r, int p, double *A, double *Q) {
  const int s = r * p;
  const int64_t n = T - p;
  if (n <= s) return SS_E_VAR;
  // Xl[t][k r + j] = F[p - 1 - k + t][j]
  auto xl = [&](int64_t t, int c) { return F[(size_t)(c % r) * T + (p - 1 - c / r + t)]; };
  std::vector<double> G((size_t)s * s), B((size_t)s * r), U((size_t)n * r);
  for (int a = 0; a < s; ++a)
    for (int b = 0; b <= a; ++b) {
      double v = 0.0;
      for (int64_t t = 0; t < n; ++t) v += xl(t, a) * xl(t, b);
      G[a * s + b] = G[b * s + a] = v;
    }
  for (int a = 0; a < s; ++a)
    for (int j = 0; j < r; ++j) {
      double v = 0.0;
      for (int64_t t = 0; t < n; ++t) v += xl(t, a) * F[(size_t)j * T + p + t];
      B[a * r + j] = v;
    }
  if (!ss_cholesky(G.data(), s)) return SS_E_VAR;
  for (int j = 0; j < r; ++j) {   // G x = B[:, j] by the two triangular solves
    for (int a = 0; a < s; ++a) {
      double v = B[a * r + j];
      for (int k = 0; k < a; ++k) v -= G[a * s + k] * B[k * r + j];
      B[a * r + j] = v / G[a * s + a];
    }
    for (int a = s - 1; a >= 0; --a) {
      double v = B[a * r + j];
      for (int k = a + 1; k < s; ++k) v -= G[k * s + a] * B[k * r + j];
      B[a * r + j] = v / G[a * s + a];
    }
  }
  // B = A' (rp x r): A[i][c] = B[c][i], column-major r x rp
  for (int c = 0; c < s; ++c)
    for (int i = 0; i < r; ++i) A[(size_t)c * r + i] = B[c * r + i];
  for (int64_t t = 0; t < n; ++t)
    for (int j = 0; j < r; ++j) {
      double v = F[(size_t)j * T + p + t];
      for (int c = 0; c < s; ++c) v -= xl(t, c) * B[c * r + j];
      U[(size_t)t * r + j] = v;
    }
  std::vector<double> Qc((size_t)r * r);
  for (int i = 0; i < r; ++i)
    for (int j = 0; j <= i; ++j) {
      double v = 0.0;
      for (int64_t t = 0; t < n; ++t) v += U[(size_t)t * r + i] * U[(size_t)t * r + j];
      v /= (double)n;
      Q[(size_t)j * r + i] = Q[(size_t)i * r + j] = v;
      Qc[i * r + j] = Qc[j * r + i] = v;
    }
  return ss_cholesky(Qc.data(), r) ? 0 : SS_E_SINGULAR;
}

// The arguments of steps 2-4: dims, pointers, NaN in F or L.
inline int ss_estimate_args(const double *Zm, int64_t T, int64_t N, int64_t ldz, const double *F, const double *L, int r,
                            int p, const double *sigma2, const double *A, const double *Q, const double *P0) {
  const int rc = ss_check_dims(r, p);
  if (rc) return rc;
  if (!Zm || !F || !L || !sigma2 || !A || !Q || !P0 || T < 2 || N < 1 || ldz < T) return -2;
  for (size_t e = 0; e < (size_t)T * r; ++e)
    if (isnan(F[e])) return SS_E_NAN;
  for (size_t e = 0; e < (size_t)N * r; ++e)
    if (isnan(L[e])) return SS_E_NAN;
  return 0;
}

// Steps 2-4 of the two-step fit: ss_idio_var, ss_var_ols, then
//   P0 = ss_stationary_cov(A, Q)
// Outputs column-major: sigma2 (N), A (r x rp), Q (r x r), P0 (s x s); *where
// names the column of a failed variance.
inline int ss_estimate(const double *Zm, int64_t T, int64_t N, int64_t ldz, const double *F, const double *L, int r,
                       int p, double *sigma2, double *A, double *Q, double *P0, int64_t *where) {
  int rc = ss_estimate_args(Zm, T, N, ldz, F, L, r, p, sigma2, A, Q, P0);
  if (rc) return rc;
  if ((rc = ss_idio_var(Zm, T, N, ldz, F, L, r, sigma2, where))) return rc;
  if ((rc = ss_var_ols(F, T, r, p, A, Q))) return rc;
  return ss_stationary_cov(A, Q, r, p, P0);
}

// ------------------------------------------- mixed frequency (dfm_ss_smooth_mf)
// A low-frequency series loads on sum_k w_k f_{t-k}, k < n_w: the state keeps
// L = max(p, n_w) lags of the factors, s = r L.
constexpr int SS_WMAX = 8;

inline int ss_mf_lags(int p, int n_w) { return p > n_w ? p : n_w; }

// The limits at the padded state, then the weights (finite, w_0 != 0) and the mask.
inline int ss_mf_check(int r, int p, int n_w, const double *w, const uint8_t *low) {
  if (n_w < 1 || p < 1) return -2;
  if (n_w > SS_WMAX) return SS_E_LIMIT;
  const int rc = ss_check_dims(r, ss_mf_lags(p, n_w));
  if (rc) return rc;
  if (!w || !low) return -2;
  for (int k = 0; k < n_w; ++k)
    if (!isfinite(w[k])) return -2;
  return w[0] != 0.0 ? 0 : -2;
}

inline bool ss_mf_any_low(const uint8_t *low, int64_t N) {
  for (int64_t i = 0; i < N; ++i)
    if (low[i]) return true;
  return false;
}

// [A 0]: A (r x rp column-major) followed by r (L - p) zero columns.  Its
// companion matrix (ss_companion at p = L) is the padded one: [A 0] in the
// first r rows, the identity shift below.
inline void ss_mf_pad_A(const double *A, int r, int p, int L, double *Apad) {
  for (int e = 0; e < r * r * L; ++e) Apad[e] = e < r * r * p ? A[e] : 0.0;
}

// Z_l = [w_0 I_r ... w_{n_w-1} I_r 0 ...], r x s row-major.
inline void ss_mf_zl(const double *w, int n_w, int r, int s, double *Zl) {
  for (int e = 0; e < r * s; ++e) Zl[e] = 0.0;
  for (int k = 0; k < n_w; ++k)
    for (int i = 0; i < r; ++i) Zl[i * s + k * r + i] = w[k];
}

// Start values of the low-frequency series for the fit: lambda_i, sigma^2_i by
// OLS of Zm_ti on ft_t = sum_k w_k F[t-k] over the observed rows t >= n_w - 1,
// sigma^2_i = the residual sum of squares over their count.  Zm: T x N
// column-major (ldz), F: T x r, L: N x r column-major; L and sigma2 are
// rewritten for the marked series only.  SS_E_VAR with fewer than r + 1 such
// rows or a singular ft'ft, SS_E_SIGMA for a non-positive variance; *where
// names the column.
// free (factor blocks; null: every factor): bit j of free[i] says that series
// i loads on factor j.  The regression is then on the aggregate of its free
// factors only: row and column j of ft'ft become e_j and ft'z_j zero for the
// others, which leaves lambda_ij = 0 there and the free sub-system's solution
// (r + 1 becomes the count of its free factors + 1).
inline int ss_mf_start(const double *Zm, int64_t T, int64_t N, int64_t ldz, const double *F, int r, const double *w,
                       int n_w, const uint8_t *low, double *L, double *sigma2, int64_t *where,
                       const uint16_t *free = nullptr) {
  if (!Zm || !F || !w || !low || !L || !sigma2 || r < 1 || r > SS_RMAX || n_w < 1 || n_w > SS_WMAX || T < 1 || ldz < T)
    return -2;
  std::vector<double> ft((size_t)T * r, 0.0), G((size_t)r * r), g((size_t)r);
  for (int64_t t = n_w - 1; t < T; ++t)
    for (int j = 0; j < r; ++j) {
      double v = 0.0;
      for (int k = 0; k < n_w; ++k) v = fma(w[k], F[(size_t)j * T + t - k], v);
      ft[(size_t)t * r + j] = v;
    }
  for (int64_t i = 0; i < N; ++i) {
    if (!low[i]) continue;
    if (where) *where = i;
    const double *z = Zm + (size_t)i * ldz;
    std::fill(G.begin(), G.end(), 0.0);
    std::fill(g.begin(), g.end(), 0.0);
    int64_t n = 0;
    for (int64_t t = n_w - 1; t < T; ++t) {
      if (isnan(z[t])) continue;
      ++n;
      for (int a = 0; a < r; ++a) {
        g[a] += ft[(size_t)t * r + a] * z[t];
        for (int b = 0; b <= a; ++b) G[a * r + b] += ft[(size_t)t * r + a] * ft[(size_t)t * r + b];
      }
    }
    int nfree = r;
    if (free)
      for (int a = 0; a < r; ++a) {
        if ((free[i] >> a) & 1) continue;
        --nfree;
        g[a] = 0.0;
        for (int b = 0; b < r; ++b) G[a * r + b] = G[b * r + a] = a == b ? 1.0 : 0.0;
      }
    if (n < nfree + 1 || !ss_cholesky(G.data(), r)) return SS_E_VAR;
    for (int a = 0; a < r; ++a) {
      double v = g[a];
      for (int k = 0; k < a; ++k) v -= G[a * r + k] * g[k];
      g[a] = v / G[a * r + a];
    }
    for (int a = r - 1; a >= 0; --a) {
      double v = g[a];
      for (int k = a + 1; k < r; ++k) v -= G[k * r + a] * g[k];
      g[a] = v / G[a * r + a];
    }
    double rss = 0.0;
    for (int64_t t = n_w - 1; t < T; ++t) {
      if (isnan(z[t])) continue;
      double c = 0.0;
      for (int a = 0; a < r; ++a) c = fma(ft[(size_t)t * r + a], g[a], c);
      rss += (z[t] - c) * (z[t] - c);
    }
    const double v = rss / (double)n;
    if (!(v > 0.0) || isinf(v)) return SS_E_SIGMA;
    for (int a = 0; a < r; ++a) L[(size_t)a * N + i] = (!free || ((free[i] >> a) & 1)) ? g[a] : 0.0;
    sigma2[i] = v;
  }
  return 0;
}

// ------------------------------- AR(1) idiosyncratic terms (dfm_ss_smooth_ar)
// e_ti = rho_i e_{t-1,i} + u_ti: an observed entry whose predecessor is
// observed enters quasi-differenced and loads on (f_t, f_{t-1}), so the update
// has size 2r and the state keeps L = max(p, 2) lags, s = r L (include/dfm.h).
constexpr int SS_AR_RMAX = 8;            // 2r <= 16: what the filter's update block holds
constexpr double SS_AR_RHO_MAX = 0.99;   // the clamp of the two-step estimate

inline int ss_ar_lags(int p) { return p > 2 ? p : 2; }

// The limits at the padded state, then rho: null or |rho_i| >= 1 is -2 (*where:
// the column, -1 for a null rho), NaN is SS_E_NAN.
inline int ss_ar_check(int r, int p, int64_t N, const double *rho, int64_t *where) {
  if (where) *where = -1;
  if (r < 1 || p < 1 || N < 1) return -2;
  if (r > SS_AR_RMAX) return SS_E_LIMIT;
  const int rc = ss_check_dims(r, ss_ar_lags(p));
  if (rc) return rc;
  if (!rho) return -2;
  for (int64_t i = 0; i < N; ++i)
    if (isnan(rho[i])) return SS_E_NAN;
  for (int64_t i = 0; i < N; ++i)
    if (!(fabs(rho[i]) < 1.0)) {
      if (where) *where = i;
      return -2;
    }
  return 0;
}

// The two-step estimate of rho after step 2: eps_ti = Zm_ti - f_t' lambda_i at
// the observed entries, P_i the rows t whose entry and predecessor are both
// observed,
//   rho_i = sum_P eps_t eps_{t-1} / sum_P eps_{t-1}^2, clamped to +-SS_AR_RHO_MAX,
//   sigma2_i = sum_P (eps_t - rho_i eps_{t-1})^2 / |P_i|   (the innovation variance).
// |P_i| < 3 or a zero denominator: rho_i = 0 and sigma2_i stays as it came
// (step 2's).  Layouts as ss_idio_var; *where names the column of a
// non-positive variance (SS_E_SIGMA).
inline int ss_ar_estimate(const double *Zm, int64_t T, int64_t N, int64_t ldz, const double *F, const double *L, int r,
                          double *sigma2, double *rho, int64_t *where) {
  std::vector<double> eps((size_t)T);
  for (int64_t i = 0; i < N; ++i) {
    for (int64_t t = 0; t < T; ++t) {
      const double z = Zm[(size_t)i * ldz + t];
      double c = 0.0;
      for (int j = 0; j < r; ++j) c = fma(F[(size_t)j * T + t], L[(size_t)j * N + i], c);
      eps[(size_t)t] = z - c;   // NaN where z is
    }
    double num = 0.0, den = 0.0;
    int64_t n = 0;
    for (int64_t t = 1; t < T; ++t) {
      if (isnan(eps[(size_t)t]) || isnan(eps[(size_t)t - 1])) continue;
      num += eps[(size_t)t] * eps[(size_t)t - 1];
      den += eps[(size_t)t - 1] * eps[(size_t)t - 1];
      ++n;
    }
    rho[i] = 0.0;
    if (n >= 3 && den > 0.0) {
      double rh = num / den;
      if (rh > SS_AR_RHO_MAX) rh = SS_AR_RHO_MAX;
      if (rh < -SS_AR_RHO_MAX) rh = -SS_AR_RHO_MAX;
      double ss = 0.0;
      for (int64_t t = 1; t < T; ++t) {
        if (isnan(eps[(size_t)t]) || isnan(eps[(size_t)t - 1])) continue;
        const double u = eps[(size_t)t] - rh * eps[(size_t)t - 1];
        ss += u * u;
      }
      rho[i] = rh;
      sigma2[i] = ss / (double)n;
    }
    if (!(sigma2[i] > 0.0) || isinf(sigma2[i])) {
      if (where) *where = i;
      return SS_E_SIGMA;
    }
  }
  return 0;
}

// Steps 2-4 of the two-step fit with AR(1) terms: ss_idio_var, ss_ar_estimate,
// ss_var_ols, then the stationary covariance of the padded form [A 0] at L =
// max(p, 2) lags.  As ss_estimate, but P0 is s x s at s = r L and rho (N) is
// written too.
inline int ss_estimate_ar(const double *Zm, int64_t T, int64_t N, int64_t ldz, const double *F, const double *L, int r,
                          int p, double *sigma2, double *A, double *Q, double *P0, double *rho, int64_t *where) {
  if (r < 1 || p < 1) return -2;
  if (r > SS_AR_RMAX) return SS_E_LIMIT;
  const int Lg = ss_ar_lags(p);
  int rc = ss_check_dims(r, Lg);
  if (rc) return rc;
  if ((rc = ss_estimate_args(Zm, T, N, ldz, F, L, r, p, sigma2, A, Q, P0))) return rc;
  if (!rho) return -2;
  if ((rc = ss_idio_var(Zm, T, N, ldz, F, L, r, sigma2, where))) return rc;
  if ((rc = ss_ar_estimate(Zm, T, N, ldz, F, L, r, sigma2, rho, where))) return rc;
  if ((rc = ss_var_ols(F, T, r, p, A, Q))) return rc;
  std::vector<double> Apad((size_t)r * r * Lg);
  ss_mf_pad_A(A, r, p, Lg, Apad.data());
  return ss_stationary_cov(Apad.data(), Q, r, Lg, P0);
}

// The fill of the AR(1) model.  X: T x N column-major (ldx), NaN = missing; L:
// N x r column-major; S: the smoothed factors, (T + h) x r row-major as the
// smoother returns them; out: (T + h) x N column-major (ld T + h).  An
// observed entry is copied.  A missing (t, i), t < T + h, becomes lambda_i'
// f_t|T + e, where with ehat_u = x_ui - lambda_i' f_u|T, u the last observed
// row before t, v the first after it, d1 = t - u, d2 = v - t:
//   only u:  e = rho^d1 ehat_u          only v:  e = rho^d2 ehat_v
//   both:    e = [rho^d1 (1 - rho^(2 d2)) ehat_u + rho^d2 (1 - rho^(2 d1)) ehat_v] / (1 - rho^(2 (d1 + d2)))
//   neither: e = 0
inline void ss_ar_fill(const double *X, int64_t T, int64_t N, int64_t ldx, const double *L, int r, const double *rho,
                       const double *S, int64_t h, double *out) {
  const int64_t Tt = T + h;
  std::vector<double> c((size_t)Tt);
  for (int64_t i = 0; i < N; ++i) {
    const double *x = X + (size_t)i * ldx, rh = rho[i];
    double *o = out + (size_t)i * Tt;
    for (int64_t t = 0; t < Tt; ++t) {
      double v = 0.0;
      for (int j = 0; j < r; ++j) v = fma(S[(size_t)t * r + j], L[(size_t)j * N + i], v);
      c[(size_t)t] = v;
    }
    int64_t u = -1, v = 0;   // the last observed row before t, the first after it (T: none; found once per gap)
    for (int64_t t = 0; t < Tt; ++t) {
      if (t < T && !isnan(x[t])) {
        o[t] = x[t];
        u = t;
        continue;
      }
      if (v <= t) {
        v = t + 1;
        while (v < T && isnan(x[v])) ++v;
      }
      const bool hu = u >= 0, hv = v < T;
      const double eu = hu ? x[u] - c[(size_t)u] : 0.0, ev = hv ? x[v] - c[(size_t)v] : 0.0;
      const double d1 = (double)(t - u), d2 = (double)(v - t);
      double e = 0.0;
      if (hu && hv)
        e = (pow(rh, d1) * (1.0 - pow(rh, 2.0 * d2)) * eu + pow(rh, d2) * (1.0 - pow(rh, 2.0 * d1)) * ev) /
            (1.0 - pow(rh, 2.0 * (d1 + d2)));
      else if (hu)
        e = pow(rh, d1) * eu;
      else if (hv)
        e = pow(rh, d2) * ev;
      o[t] = c[(size_t)t] + e;
    }
  }
}

// ------------------------------------------------ the quasi-ML EM (dfm_ss_em)
constexpr int SS_EM_MAX_ITER = 100, SS_EM_ITER_CAP = 1 << 20;
constexpr double SS_EM_TOL = 1e-4;

// The spec's defaults: max_iter < 0 -> 100, tol < 0 -> 1e-4.  -2 for a NaN
// tol, a negative horizon or an iteration count beyond the cap.
inline int ss_em_defaults(int max_iter_in, double tol_in, int horizon, int *max_iter, double *tol) {
  if (isnan(tol_in) || horizon < 0 || horizon > (1 << 20) || max_iter_in > SS_EM_ITER_CAP) return -2;
  *max_iter = max_iter_in < 0 ? SS_EM_MAX_ITER : max_iter_in;
  *tol = tol_in < 0.0 ? SS_EM_TOL : tol_in;
  return 0;
}

// c_j = (ll_j - ll_{j-1}) / ((|ll_j| + |ll_{j-1}|) / 2); 0 when both are zero.
inline double ss_em_criterion(double ll, double ll_prev) {
  const double den = 0.5 * (fabs(ll) + fabs(ll_prev));
  return den > 0.0 ? (ll - ll_prev) / den : 0.0;
}

// Banbura-Modugno's rule: converged when tol > 0 and c_j < tol (tol = 0 never stops).
inline bool ss_em_converged(double c, double tol) { return tol > 0.0 && c < tol; }

// The batch's layout and the starts' count; T < 2 is refused (the transition
// sums need two rows).
inline int ss_em_check_args(bool have_x, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
                            bool have_starts, int64_t n_start) {
  if (M < 0 || !have_starts || (n_start != 1 && n_start != M)) return -2;
  if (M == 0) return 0;
  if (!have_x || T < 2 || N < 1 || ldx < T || stride < ldx * N) return -2;
  if (T > (1 << 24) || N > (1 << 24)) return -2;
  return 0;
}

// One start: ss_check_params, then Q positive definite (SS_E_SINGULAR).
inline int ss_em_check_start(int64_t N, int r, int p, const double *L, const double *sigma2, const double *A,
                             const double *Q, const double *a0, const double *P0, int64_t *where) {
  const int rc = ss_check_params(N, r, p, L, sigma2, A, Q, a0, P0, where);
  if (rc) return rc;
  std::vector<double> Qc((size_t)r * r);
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < r; ++j) Qc[i * r + j] = 0.5 * (Q[(size_t)j * r + i] + Q[(size_t)i * r + j]);
  return ss_cholesky(Qc.data(), r) ? 0 : SS_E_SINGULAR;
}

// First column without an observed entry of a host batch (layout of dfm_mc):
// true, with its panel and column, when there is one.
inline bool ss_em_empty_column(const double *X, int64_t M, int64_t T, int64_t N, int64_t ldx, int64_t stride,
                               int64_t *panel, int64_t *col) {
  for (int64_t b = 0; b < M; ++b)
    for (int64_t i = 0; i < N; ++i) {
      const double *x = X + b * stride + i * ldx;
      int64_t t = 0;
      while (t < T && isnan(x[t])) ++t;
      if (t == T) {
        *panel = b;
        *col = i;
        return true;
      }
    }
  return false;
}

// ------------------------------------------ factor blocks (dfm_ss_em_blocks)
// Block g of n_blocks owns the contiguous factors off[g] .. off[g + 1] - 1;
// member (N x n_blocks column-major, ld N) says which series load on it.
// Lambda_ij = 0 where series i is no member of factor j's block; every A_k
// and Q are block-diagonal.
constexpr int SS_BMAX = 16;

// Why a block specification is refused (ss_blocks_check), in the order it is looked for.
enum SsBlocksBad {
  SS_BLK_OK = 0,
  SS_BLK_NULL,     // a null struct field
  SS_BLK_COUNT,    // n_blocks outside 1..16
  SS_BLK_SIZE,     // a block of size < 1 (*where: the block)
  SS_BLK_SUM,      // the sizes do not sum to r (*where: their sum)
  SS_BLK_SERIES,   // a series that is a member of no block (*where: the column)
  SS_BLK_EMPTY     // a block without a member (*where: the block)
};

inline SsBlocksBad ss_blocks_check(int n_blocks, const int32_t *block_r, const uint8_t *member, int64_t N, int r,
                                   int64_t *where) {
  if (!block_r || !member) return SS_BLK_NULL;
  if (n_blocks < 1 || n_blocks > SS_BMAX) return SS_BLK_COUNT;
  int64_t sum = 0;
  for (int g = 0; g < n_blocks; ++g) {
    *where = g;
    if (block_r[g] < 1) return SS_BLK_SIZE;
    sum += block_r[g];
  }
  *where = sum;
  if (sum != r) return SS_BLK_SUM;
  for (int64_t i = 0; i < N; ++i) {
    bool any = false;
    for (int g = 0; g < n_blocks; ++g) any = any || member[(size_t)g * N + i];
    *where = i;
    if (!any) return SS_BLK_SERIES;
  }
  for (int g = 0; g < n_blocks; ++g) {
    bool any = false;
    for (int64_t i = 0; i < N; ++i) any = any || member[(size_t)g * N + i];
    *where = g;
    if (!any) return SS_BLK_EMPTY;
  }
  return SS_BLK_OK;
}

// One block that every series is a member of: no restriction.
inline bool ss_blocks_trivial(int n_blocks, const uint8_t *member, int64_t N) {
  if (n_blocks != 1) return false;
  for (int64_t i = 0; i < N; ++i)
    if (!member[i]) return false;
  return true;
}

// off[0 .. n_blocks]: the first factor of every block, then r.
inline void ss_blocks_offsets(int n_blocks, const int32_t *block_r, int *off) {
  off[0] = 0;
  for (int g = 0; g < n_blocks; ++g) off[g + 1] = off[g] + block_r[g];
}

// free[i]: bit j set when series i loads on factor j (r <= 16 factors).
inline void ss_blocks_free_mask(int n_blocks, const int *off, const uint8_t *member, int64_t N, uint16_t *free) {
  for (int64_t i = 0; i < N; ++i) {
    unsigned m = 0;
    for (int g = 0; g < n_blocks; ++g)
      if (member[(size_t)g * N + i])
        for (int j = off[g]; j < off[g + 1]; ++j) m |= 1u << j;
    free[i] = (uint16_t)m;
  }
}

// A start must hold zeros where the restriction does.  0, or the first
// offender: 1 Lambda[*row, *col], 2 A[*row, *col] (r x rp), 3 Q[*row, *col].
// L (ld N), A, Q column-major.
inline int ss_blocks_check_start(int64_t N, int r, int p, const double *L, const double *A, const double *Q,
                                 int n_blocks, const int *off, const uint16_t *free, int64_t *row, int64_t *col) {
  int of[SS_RMAX];   // the block of a factor
  for (int g = 0; g < n_blocks; ++g)
    for (int j = off[g]; j < off[g + 1]; ++j) of[j] = g;
  auto at = [&](int which, int64_t i, int64_t j) {
    *row = i, *col = j;
    return which;
  };
  for (int j = 0; j < r; ++j)
    for (int64_t i = 0; i < N; ++i)
      if (!((free[i] >> j) & 1) && L[(size_t)j * N + i] != 0.0) return at(1, i, j);
  for (int c = 0; c < r * p; ++c)
    for (int i = 0; i < r; ++i)
      if (of[i] != of[c % r] && A[(size_t)c * r + i] != 0.0) return at(2, i, c);
  for (int c = 0; c < r; ++c)
    for (int i = 0; i < r; ++i)
      if (of[i] != of[c] && Q[(size_t)c * r + i] != 0.0) return at(3, i, c);
  return 0;
}

// The block-wise start of the fit, its host steps.  R (T x N column-major, ld
// T) starts as the completed standardised panel; for every block in order the
// caller takes the principal components of the block's member columns
// (ss_blocks_gather), and ss_blocks_deflate stores them and subtracts their
// common component from those columns.
// The member columns of R side by side into Rg (T x the count, ld T); returns the count.
inline int64_t ss_blocks_gather(const double *R, int64_t T, int64_t N, const uint8_t *member_g, double *Rg) {
  int64_t n = 0;
  for (int64_t i = 0; i < N; ++i) {
    if (!member_g[i]) continue;
    for (int64_t t = 0; t < T; ++t) Rg[(size_t)n * T + t] = R[(size_t)i * T + t];
    ++n;
  }
  return n;
}

// Fg (T x rg, ld T) into columns o .. o + rg - 1 of F (ld T), Lg (ng x rg, ld
// ng) into the members' rows of those columns of L (N x r, ld N; the other
// rows are not touched), and R[:, members] -= Fg Lg'.
inline void ss_blocks_deflate(double *R, int64_t T, int64_t N, const uint8_t *member_g, int o, int rg, const double *Fg,
                              const double *Lg, int64_t ng, double *F, double *L) {
  for (int j = 0; j < rg; ++j)
    for (int64_t t = 0; t < T; ++t) F[(size_t)(o + j) * T + t] = Fg[(size_t)j * T + t];
  int64_t n = 0;
  for (int64_t i = 0; i < N; ++i) {
    if (!member_g[i]) continue;
    for (int j = 0; j < rg; ++j) L[(size_t)(o + j) * N + i] = Lg[(size_t)j * ng + n];
    for (int64_t t = 0; t < T; ++t) {
      double c = 0.0;
      for (int j = 0; j < rg; ++j) c = fma(Fg[(size_t)j * T + t], Lg[(size_t)j * ng + n], c);
      R[(size_t)i * T + t] -= c;
    }
    ++n;
  }
}

// Steps 2-4 of the fit with blocks: ss_idio_var on the whole of F and L, then
// ss_var_ols per block on its own columns of F into the block of A_k and Q
// (zero elsewhere), then the stationary covariance.  Arguments and outputs as
// ss_estimate; *where names the column of a failed variance, or the block of
// a failed VAR.
inline int ss_blocks_estimate(const double *Zm, int64_t T, int64_t N, int64_t ldz, const double *F, const double *L, int r,
                              int p, int n_blocks, const int *off, double *sigma2, double *A, double *Q, double *P0,
                              int64_t *where) {
  int rc = ss_estimate_args(Zm, T, N, ldz, F, L, r, p, sigma2, A, Q, P0);
  if (rc) return rc;
  if ((rc = ss_idio_var(Zm, T, N, ldz, F, L, r, sigma2, where))) return rc;
  for (int e = 0; e < r * r * p; ++e) A[e] = 0.0;
  for (int e = 0; e < r * r; ++e) Q[e] = 0.0;
  std::vector<double> Ag, Qg;
  for (int g = 0; g < n_blocks; ++g) {
    const int o = off[g], rg = off[g + 1] - o;
    Ag.assign((size_t)rg * rg * p, 0.0);
    Qg.assign((size_t)rg * rg, 0.0);
    if (where) *where = g;
    if ((rc = ss_var_ols(F + (size_t)o * T, T, rg, p, Ag.data(), Qg.data()))) return rc;
    for (int k = 0; k < p; ++k)
      for (int j = 0; j < rg; ++j)
        for (int i = 0; i < rg; ++i) A[(size_t)(k * r + o + j) * r + o + i] = Ag[(size_t)(k * rg + j) * rg + i];
    for (int j = 0; j < rg; ++j)
      for (int i = 0; i < rg; ++i) Q[(size_t)(o + j) * r + o + i] = Qg[(size_t)j * rg + i];
  }
  return ss_stationary_cov(A, Q, r, p, P0);
}

// ------------------------------------------------- panels per pass (both drivers)
// The half-GB rule of the smoother and the EM: as many panels per pass as keep
// what they hold on the device (bytes_per_panel > 0 each) within 2^29 bytes, at
// the most M and a launch grid's 65535, at the least one.
inline int64_t ss_panels_per_pass(int64_t M, size_t bytes_per_panel) {
  int64_t n = (int64_t)(((size_t)1 << 29) / bytes_per_panel);
  if (n > 65535) n = 65535;
  if (n > M) n = M;
  return n < 1 ? 1 : n;
}

// ------------------------------------- the simulation smoother (dfm_ss_simulate)
constexpr int64_t SS_SIM_DMAX = (int64_t)1 << 24;   // draws per call

// Lower-triangular factor R of the positive semi-definite n x n row-major Cm
// (its lower triangle is read), R R' = Cm; R: n x n row-major, the upper
// triangle zero.  The Cholesky loop with one rule for a rank-deficient matrix:
// at column j, d = C_jj - sum_{k<j} R_jk^2; d <= 1e-12 C_jj (or a NaN d) leaves
// column j zero, otherwise R_jj = sqrt(d) and the column follows as usual.
inline void ss_psd_cholesky(const double *Cm, int n, double *R) {
  for (int e = 0; e < n * n; ++e) R[e] = 0.0;
  for (int j = 0; j < n; ++j) {
    const double cjj = Cm[j * n + j];
    double d = cjj;
    for (int k = 0; k < j; ++k) d -= R[j * n + k] * R[j * n + k];
    if (!(d > 1e-12 * cjj)) continue;
    d = sqrt(d);
    R[j * n + j] = d;
    for (int i = j + 1; i < n; ++i) {
      double v = Cm[i * n + j];
      for (int k = 0; k < j; ++k) v -= R[i * n + k] * R[j * n + k];
      R[i * n + j] = v / d;
    }
  }
}

// Standard normals per draw: z0 (s), then u_t (r) and zeta_t (r) for each of the Tt rows.
inline int64_t ss_sim_nz(int64_t Tt, int r, int s) { return (int64_t)s + 2 * (int64_t)r * Tt; }

// The draws' arguments: 1 <= D <= 2^24, z and the output present, ldz >= D,
// 0 <= horizon <= 2^20, pass_draws >= 0.
inline int ss_sim_check_args(int64_t D, bool have_z, bool have_draws, int64_t ldz, int64_t horizon, int64_t pass_draws) {
  if (D < 1 || D > SS_SIM_DMAX || !have_z || !have_draws || ldz < D) return -2;
  if (horizon < 0 || horizon > (1 << 20) || pass_draws < 0) return -2;
  return 0;
}

// Draws per pass.  pass_draws > 0: that many (at the most D).  Otherwise the
// smoother's half-GB rule over the doubles a draw keeps on the device: c_t|t
// (Tt x s), its output rows as the lanes store them and as they leave for the
// host (2 Tt r), and its normals when they come from the host (z_host);
// rounded down to whole waves of 64 draws once there is more than one.
inline int64_t ss_sim_draws_per_pass(int64_t Tt, int r, int s, int64_t D, int64_t pass_draws, bool z_host = true) {
  if (pass_draws > 0) return pass_draws < D ? pass_draws : D;
  const int64_t per = 8 * (Tt * s + 2 * Tt * r + (z_host ? ss_sim_nz(Tt, r, s) : 0));
  int64_t n = ((int64_t)1 << 29) / per;
  if (n > 64) n &= ~(int64_t)63;
  if (n < 1) n = 1;
  return n < D ? n : D;
}

// ------------------------------------------------ the news decomposition (dfm_ss_news)
constexpr int64_t SS_NEWS_JMAX = (int64_t)1 << 24;   // releases per call

// The call's own arguments: 0 <= J <= 2^24 with both lists present when J > 0,
// 0 <= horizon <= 2^20, 0 <= t_lo < T + horizon, pass_releases >= 0.
inline int ss_news_check_args(int64_t J, bool have_lists, int64_t T, int64_t horizon, int64_t t_lo,
                              int64_t pass_releases) {
  if (J < 0 || J > SS_NEWS_JMAX || (J > 0 && !have_lists)) return -2;
  if (T < 1 || horizon < 0 || horizon > (1 << 20) || pass_releases < 0) return -2;
  return (t_lo < 0 || t_lo >= T + horizon) ? -2 : 0;
}

// Why a release list is refused (ss_news_check_releases), in the order it is looked for.
enum SsNewsBad {
  SS_NEWS_OK = 0,
  SS_NEWS_RANGE,       // an entry outside the panel
  SS_NEWS_UNSORTED,    // an entry before its predecessor in (t, i)
  SS_NEWS_DUPLICATE,   // an entry equal to its predecessor
  SS_NEWS_DROPPED,     // observed in X_old, NaN in X_new: the old set is no subset of the new one
  SS_NEWS_NOT_NEW,     // a listed entry that is NaN in X_new or observed in X_old
  SS_NEWS_MISSING      // a release (observed in X_new, NaN in X_old) that the list leaves out
};

// The list must be exactly the entries observed in X_new and NaN in X_old,
// sorted by (t, i).  First the list alone (range, order), then the panels row
// by row; *bt, *bi: the first offending entry.  Panels column-major T x N (ldx).
inline SsNewsBad ss_news_check_releases(const double *X_old, const double *X_new, int64_t T, int64_t N, int64_t ldx,
                                        int64_t J, const int64_t *rel_t, const int64_t *rel_i, int64_t *bt,
                                        int64_t *bi) {
  auto bad = [&](SsNewsBad why, int64_t t, int64_t i) {
    *bt = t, *bi = i;
    return why;
  };
  for (int64_t j = 0; j < J; ++j) {
    const int64_t t = rel_t[j], i = rel_i[j];
    if (t < 0 || t >= T || i < 0 || i >= N) return bad(SS_NEWS_RANGE, t, i);
    if (j == 0) continue;
    if (t == rel_t[j - 1] && i == rel_i[j - 1]) return bad(SS_NEWS_DUPLICATE, t, i);
    if (t < rel_t[j - 1] || (t == rel_t[j - 1] && i < rel_i[j - 1])) return bad(SS_NEWS_UNSORTED, t, i);
  }
  int64_t j = 0;
  for (int64_t t = 0; t < T; ++t)
    for (int64_t i = 0; i < N; ++i) {
      const bool o = !isnan(X_old[i * ldx + t]), n = !isnan(X_new[i * ldx + t]);
      const bool listed = j < J && rel_t[j] == t && rel_i[j] == i;
      if (o && !n) return bad(SS_NEWS_DROPPED, t, i);
      if (listed && !(n && !o)) return bad(SS_NEWS_NOT_NEW, t, i);
      if (!listed && n && !o) return bad(SS_NEWS_MISSING, t, i);
      if (listed) ++j;
    }
  return SS_NEWS_OK;
}

// X_rev: X_new's values on the old observed set, NaN elsewhere (T x N, ld T).
inline void ss_news_revised(const double *X_old, const double *X_new, int64_t T, int64_t N, int64_t ldx, double *X_rev) {
  for (int64_t i = 0; i < N; ++i)
    for (int64_t t = 0; t < T; ++t) X_rev[i * T + t] = isnan(X_old[i * ldx + t]) ? NAN : X_new[i * ldx + t];
}

// Releases per pass.  pass_releases > 0: that many (at the most J).  Otherwise
// the half-GB rule over the doubles a release keeps on the device: c_t|t (Tt x
// s), its weights as the lanes store them and as they leave for the host (2
// (Tt - t_lo) r, twice with the aggregate's), beta (r) and its row and class;
// rounded down to whole waves of 64 once there is more than one.
inline int64_t ss_news_releases_per_pass(int64_t Tt, int64_t t_lo, int r, int s, bool agg, int64_t J,
                                         int64_t pass_releases) {
  if (pass_releases > 0) return pass_releases < J ? pass_releases : J;
  const int64_t per = 8 * (Tt * s + (agg ? 4 : 2) * (Tt - t_lo) * r + r + 1);
  int64_t n = ((int64_t)1 << 29) / per;
  if (n > 64) n &= ~(int64_t)63;
  if (n < 1) n = 1;
  return n < J ? n : J;
}

}  // namespace dfm
