// dfm_eig_debug.hip — debug entries of the two top-k eigensolvers
// (tests/test_gpu_eig.py): dfm_debug_eig (eig_run of dfm_eig.hip: the three
// fused instantiations, the unfused kernel chain, P = 16 or 32) and
// dfm_debug_dense_eig (launch_dense_eig_batched of dfm_spec.hip).  Each
// allocates the solver's workspace, runs it on the context's stream and
// synchronises; neither is declared in include/dfm.h.  Returns 0, -1 for bad
// arguments, 1 when a replicate's status is 1 (not converged; the dense
// path: a rank-deficient orthonormalisation block), 1000 + hipError for a
// launcher or runtime error.  Outputs are the caller's device buffers and
// are never cleared here: a test fills them with NaN and sees what a kernel
// did not write.
#include "dfm_host.h"
#include <vector>

namespace dfm {

// 0, or 1 when any of the nb device status words is non-zero; synchronises first
static int dbg_eig_finish(int rc, hipError_t e, const int *status, int nb, hipStream_t st) {
  const hipError_t s = hipStreamSynchronize(st);   // always: the workspace is freed after the return
  if (rc >= 1000 || rc < 0) return rc;
  if (e == hipSuccess) e = s;
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return 1000 + (int)e;
  std::vector<int> h((size_t)nb, 0);
  e = hipMemcpy(h.data(), status, (size_t)nb * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return 1000 + (int)e;
  for (int v : h)
    if (v != 0) return 1;
  return rc;
}

}  // namespace dfm

// eig_run on nb matrices G + rep * strideG (m x m at ldg).  block goes
// through eig_block_p as in ctx_eig_args; tol, maxit, subspace, warm (m x kw,
// may be null with kw = 0) and fused (EigArgs::fused) are passed through;
// poll is the context's.  p < k, p > 32 and p > m are left to eig_run's own
// check (-1, before it touches the workspace).  lam: nb x k, Uk: nb x m x k or null
// (eigenvalue-only), trace, status, iters: nb each (device; iters may be null).
extern "C" int dfm_debug_eig(dfm_ctx *ctx, const double *G, int64_t ldg, int64_t strideG, int m, int nb, int k,
                             int block, double tol, int maxit, int subspace, const double *warm, int kw, int fused,
                             double *lam, double *Uk, double *trace, int *status, int *iters) {
  using namespace dfm;
  if (!ctx || !G || !lam || !trace || !status || m < 1 || nb < 1 || k < 1 || ldg < m || maxit < 1 || kw < 0 ||
      (kw > 0 && !warm) || (nb > 1 && strideG != 0 && strideG < (int64_t)m * ldg) || fused < -1 || fused > 1)
    return -1;
  hipStream_t st = ctx_stream(ctx);
  EigArgs a{};
  a.nb = nb; a.k = k; a.p = eig_block_p(m, k, block);
  a.warm = kw > 0 ? warm : nullptr; a.kw = kw;
  a.tol = tol; a.maxit = maxit; a.poll = ctx->poll;
  a.lam = lam; a.Uk = Uk; a.trace_out = trace; a.status = status;
  a.st = st; a.tf = nullptr; a.tctx = nullptr;
  a.subspace = subspace; a.fused = fused;
  const int P = a.p <= 16 ? 16 : 32;
  char *ws = nullptr;
  if (hipMalloc((void **)&ws, eig_workspace_bytes_padded(m, nb, P, maxit)) != hipSuccess) return 1002;
  a.ws = ws;
  std::vector<int> ih((size_t)nb, 0);
  int rc = eig_run(G, ldg, strideG, m, a, iters ? ih.data() : nullptr, 0);
  rc = dbg_eig_finish(rc, hipSuccess, status, nb, st);
  if (iters && rc >= 0 && rc < 1000 && hipMemcpy(iters, ih.data(), (size_t)nb * 4, hipMemcpyHostToDevice) != hipSuccess)
    rc = 1000 + (int)hipGetLastError();
  hipFree(ws);
  return rc;
}

// launch_dense_eig_batched with mv0 = m, dmv = 0 (plain m x m matrices),
// whose own argument check is under test (1001).
extern "C" int dfm_debug_dense_eig(dfm_ctx *ctx, const double *G, int64_t ldg, int64_t strideG, int m, int nb, int k,
                                   double *lam, double *Uk, double *trace, int *status) {
  using namespace dfm;
  if (!ctx || !G || !lam || !Uk || !trace || !status || nb < 1 || m < 1 || k < 1 || ldg < m) return -1;
  hipStream_t st = ctx_stream(ctx);
  double *work = nullptr;
  if (hipMalloc((void **)&work, (size_t)nb * (size_t)dense_eig_work(m, k) * 8) != hipSuccess) return 1002;
  const hipError_t e = launch_dense_eig_batched(G, ldg, strideG, m, m, 0, nb, k, lam, Uk, trace, status, work, st);
  const int rc = e != hipSuccess ? dbg_eig_finish(1000 + (int)e, e, status, nb, st)
                                 : dbg_eig_finish(0, e, status, nb, st);
  hipFree(work);
  return rc;
}
