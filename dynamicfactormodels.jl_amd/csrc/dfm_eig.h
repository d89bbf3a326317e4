// dfm_eig.h — what the explicit-Gram solver (dfm_eig.hip) and the factored
// bootstrap solver (dfm_fact.hip) share: the workspace record, three
// host-launched kernels that dfm_eig.hip defines and instantiates for
// P = 16, 32, a few constants and host helpers.  Private to those two files
// (dfm_internal.h declares what the rest of the library sees).
#pragma once
#include "dfm_internal.h"

namespace dfm {

constexpr int EROWS = 64;  // rows per workgroup in gq/apply

struct EigWork {
  double *Q, *Y, *U;       // nb x m x P
  double *S;               // nb x m x P: the direct path's second Horner vector (filters of degree > 2)
  double *part;            // nb x nrb x 3 x P x P
  double *rpart;           // nb x nrb x P
  double *upart;           // nb x nrb x P: the Ritz vectors' squared norms by row block (judged_residual)
  double *small;           // nb x SMALL_STRIDE (A, Bm, theta, dead)
  int *done, *iters, *active;
  double *trace;           // nb
  long long *dbg;          // phase stamps of replicate 0 (SMALL_STAMP) when a diagnostic build points it at a buffer; null
  // strict rule's gap: 0 = distance to the neighbouring Ritz values (every
  // wanted eigenVECTOR converged); 1 = distance to the first unwanted Ritz
  // value theta_k (the wanted SUBSPACE converged: for statistics invariant to
  // rotations within span(F_r) — Chow tests, V, criteria, eigenvalues)
  int subspace;
  int no_vectors;          // eigenvalue-only caller (Uk == nullptr): the Ritz vectors are never written
};
template <int P> constexpr int small_stride() { return 2 * P * P + 4 * P; }

// Jacobi sweeps per Rayleigh-Ritz step.  The projected matrix need not be
// diagonalised exactly at every outer iteration: the next iteration starts
// from the (nearly) rotated basis, so the inner sweeps accumulate across outer
// iterations, and the residual test of check_converged includes any leftover
// off-diagonal coupling.
constexpr int kJacobiSweeps = 2;
constexpr int kChebDMax = 8;   // highest filter degree (shifted_cheb's coefficient arrays hold kChebDMax + 1)

// The stopping rule of both solvers (check_converged in dfm_eig.hip,
// decide_converged in dfm_fact.hip: each sums its residual partials and
// records next[j] = res in its own order, then asks here).
// Wanted Ritz pair j < k with squared residual rs, th0 = |theta_1|, itc = the
// Rayleigh-Ritz steps taken, prev = the previous step's residuals.
//   tol >= 0, the strict rule: res_j <= tol gap_j (eigenvector error ~
//   res / gap), gap_j the distance to the neighbouring Ritz values or, in the
//   subspace form (EigWork::subspace; k == p has no unwanted value: the
//   neighbours), to the first unwanted one theta_k; or the rounding floor
//   res_j <= 2e-14 th0; or res_j <= 1e-11 th0 and stagnating (no 2x decrease).
//   tol < 0, eigenvalue-only statistics (V, criteria, eigenvalues, trace): a
//   Ritz value's error is quadratic in its residual, |theta_j - lambda_j| <=
//   bnd_j = res_j^2 / (gap_j / 2) (Kato-Temple, neighbour gap halved for
//   safety) <= -tol |theta_j|, or the floor; the caller sums bnd_j and
//   theta_j over its columns for energy_converged.
struct ColumnVerdict {
  bool ok, floor;   // this column passes; it sits at the rounding floor
  double res, bnd;  // sqrt(rs); the eigenvalue bound (tol < 0, else 0)
};
DFM_DEV ColumnVerdict column_verdict(double rs, int j, const double *th, double th0, const double *prev, int k,
                                     int p, double tol, int itc, int subspace) {
  ColumnVerdict v;
  v.res = sqrt(rs);
  double gap = INFINITY;
  if (subspace && tol >= 0.0 && k < p) {
    gap = fabs(th[j] - th[k]);
  } else {
    if (j > 0) gap = fmin(gap, fabs(th[j] - th[j - 1]));
    if (j + 1 < p) gap = fmin(gap, fabs(th[j] - th[j + 1]));
  }
  v.floor = v.res <= 2e-14 * th0;
  if (tol < 0.0) {
    v.bnd = rs / (0.5 * gap);
    v.ok = v.bnd <= -tol * fabs(th[j]) || v.floor;
  } else {
    const bool stagn = itc > 2 && v.res <= 1e-11 * th0 && v.res > 0.5 * prev[j];
    v.bnd = 0.0;
    v.ok = v.res <= tol * gap || v.floor || stagn;
  }
  return v;
}
// tol < 0: the summed bound (bsum, tsum: the wave's totals of bnd_j and
// theta_j) moves the residual energy trace - sum_j theta_j, the numerator of
// V(k) (src/criteria.jl:5), by at most -tol relative — the energy floored at
// 1e-6 trace: below that the reference's own rounding of ||E||^2 already
// exceeds -tol relative (exact-rank panels) — or every column is at the floor.
// Called by one whole wave; floor_ok is this lane's columns' conjunction.
DFM_DEV bool energy_converged(double bsum, double tsum, double trace, double tol, bool floor_ok) {
  const double vnum = fmax(fabs(trace - tsum), 1e-6 * fabs(trace));
  return bsum <= -tol * vnum || !__any(!floor_ok);
}

EigWork carve(char *base, int m, int nb, int P, int maxit);
// Sum of the unconverged-replicate counts seen by the products of iterations
// 0..last (shift = 1: the product of iteration it runs before that
// iteration's convergence check, so it sees active[it-1]; active[-1] = nb).
int64_t count_rep_iters(const int *active_dev, int last, int shift, int nb, hipStream_t st);
// Shifted Chebyshev coefficients T*_d(y) = T_d(2y - 1) = sum_i a_i y^i, a[0..kChebDMax]
void shifted_cheb(int d, double *a);

// ps: row stride (the factored solver's compact rows hold ps = pz <= P columns)
template <int P>
__global__ void eig_init_kernel(double *__restrict__ Q, int m, int p, const double *__restrict__ warm,
                                int kw, int *__restrict__ done, uint64_t seed, int64_t rep0, int ps = P);
template <int P>
__global__ __launch_bounds__(64) void eig_small_kernel(EigWork w, int p, int nrb, int jsweeps);
template <int P>
__global__ __launch_bounds__(256) void eig_final_kernel(EigWork w, int m, int k, double *__restrict__ lam,
                                                        double *__restrict__ Uk, int *__restrict__ status,
                                                        double *__restrict__ trace_out, long long *cnt = nullptr,
                                                        int last_gemm = -1, int last_cheb = -1, int cp0 = 0,
                                                        int cp1 = 0, int skip0 = 0);
#define DFM_EIG_SHARED_KERNELS(X, P)                                                                          \
  X __global__ void eig_init_kernel<P>(double *__restrict__, int, int, const double *__restrict__, int,       \
                                       int *__restrict__, uint64_t, int64_t, int);                            \
  X __global__ void eig_small_kernel<P>(EigWork, int, int, int);                                              \
  X __global__ void eig_final_kernel<P>(EigWork, int, int, double *__restrict__, double *__restrict__,        \
                                        int *__restrict__, double *__restrict__, long long *, int, int, int,  \
                                        int, int);
DFM_EIG_SHARED_KERNELS(extern template, 16)
DFM_EIG_SHARED_KERNELS(extern template, 32)

// Brackets a group of launches for the per-class kernel timing
// (dfm_ctx_read_timing): begin on construction, end on scope exit — an early
// error return closes its bracket.  A null timer_fn makes it a no-op.
struct TimerScope {
  TimerScope(const EigArgs &a, int cls) : tf(a.tf), tctx(a.tctx), cls(cls) { if (tf) tf(tctx, cls, 1); }
  ~TimerScope() { if (tf) tf(tctx, cls, 0); }
  TimerScope(const TimerScope &) = delete;
  TimerScope &operator=(const TimerScope &) = delete;
  timer_fn tf;
  void *tctx;
  int cls;
};

}  // namespace dfm
