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
