// dfm_gemm_debug.hip — debug entries of the fp64 MFMA GEMM and Gram kernels
// (tests/test_gpu_gemm64.py): dfm_debug_gemm (gemmh_kernel),
// dfm_debug_gemm_zrm (gemmh_zrm_kernel), dfm_debug_gemm_loadings
// (gemm_loadings_kernel) and dfm_debug_gram (gram_kernel, gram_dma_kernel,
// gram_splitk_sum_kernel through launch_gram / launch_gram_plain_scaled).
// Each runs the library's own launcher on the context's stream and
// synchronises; none is declared in include/dfm.h.  Returns 0, -1 for bad
// arguments, 1000 + hipError for a launcher or runtime error.  Outputs are
// the caller's device buffers and are never cleared here: a test fills them
// with NaN and sees what a kernel did not write.
#include "dfm_internal.h"

namespace dfm {

// Z (T x nb pz, row-major, column block = replicate) -> the replicate-major 16-row chunks of launch_gemm_zrm
// (zrm_ix; chunk rows past T zero): dfm_fact_debug.hip's dbg_pack_z32_kernel in fp64
__global__ void dbg_pack_z64_kernel(const double *__restrict__ Z, int T, int nb, int pz, double *__restrict__ Zc) {
  const int64_t zrs = zrm_stride(T, pz), n = (int64_t)nb * zrs;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int rep = (int)(i / zrs);
  const int64_t o = i - (int64_t)rep * zrs;
  const int ch = (int)(o / (16 * pz)), w = (int)(o - (int64_t)ch * 16 * pz), c = w >> 4, s = 16 * ch + (w & 15);
  Zc[zrm_ix(rep, s, c, pz, zrs)] = s < T ? Z[(int64_t)s * nb * pz + (int64_t)rep * pz + c] : 0.0;
}
// A (K x N) -> Eaug (Kp x ld, zero rows past K and zero columns past N), as fact_loadings' [E; L'; 0]
__global__ void dbg_pack_eaug_kernel(const double *__restrict__ A, int K, int N, int Kp, int64_t ld,
                                     double *__restrict__ Eaug) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)Kp * ld) return;
  const int64_t k = i / ld, n = i - k * ld;
  Eaug[i] = (k < K && n < N) ? A[k * N + n] : 0.0;
}
// B (nrep blocks of K x r) -> ZF (nrep blocks of Kp x rp, zero rows past K, zero column r when rp > r), as boot_zf_kernel's
__global__ void dbg_pack_zf_kernel(const double *__restrict__ B, int K, int r, int nrep, int Kp, int rp,
                                   double *__restrict__ ZF) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)nrep * Kp * rp) return;
  const int64_t rep = i / ((int64_t)Kp * rp), o = i - rep * Kp * rp, k = o / rp, j = o - k * rp;
  ZF[i] = (k < K && j < r) ? B[(rep * K + k) * r + j] : 0.0;
}

static int dbg_finish(hipError_t e, hipStream_t st) {
  const hipError_t s = hipStreamSynchronize(st);   // always: the caller's buffers are free to go after the return
  if (e == hipSuccess) e = s;
  if (e == hipSuccess) e = hipGetLastError();
  return e == hipSuccess ? 0 : 1000 + (int)e;
}

}  // namespace dfm

// C (M x Nc, ldc) = A B on gemmh_kernel, the operands in launch_gemm's own
// layout and passed through: A M x lda with zero k-padding, B round_up(K, 16)
// x ldb with zero rows past K.  launch_gemm's argument check is the one
// under test (1001 = 1000 + hipErrorInvalidValue).
extern "C" int dfm_debug_gemm(dfm_ctx *ctx, const double *A, int64_t lda, const double *B, int64_t ldb, double *C,
                              int64_t ldc, int M, int Nc, int K) {
  using namespace dfm;
  if (!ctx || !A || !B || !C) return -1;
  hipStream_t st = ctx_stream(ctx);
  return dbg_finish(launch_gemm(A, lda, B, ldb, C, ldc, M, Nc, K, st), st);
}

// C (T x nb pz at ldc, column-interleaved) = H Z on gemmh_zrm_kernel with
// M = K = T, as the factored solver launches it.  H: T x ldH, ldH >=
// round_up(T, 16), zero k-padding; Z: plain row-major T x nb pz, packed here
// into the replicate-major chunks.  col_done (nb ints), clist (nb ints) and
// ccount (one int) are device arrays passed through unchanged; each may be
// null, clist and ccount only together.
extern "C" int dfm_debug_gemm_zrm(dfm_ctx *ctx, const double *H, int64_t ldH, int T, const double *Z, int nb, int pz,
                                  double *C, int64_t ldc, const int *col_done, const int *clist, const int *ccount) {
  using namespace dfm;
  if (!ctx || !H || !Z || !C || T < 1 || nb < 1 || pz < 1 || ldH < (T + 15) / 16 * 16 || ldc < (int64_t)nb * pz ||
      (int64_t)nb * pz > INT32_MAX || !clist != !ccount)
    return -1;
  hipStream_t st = ctx_stream(ctx);
  const int64_t zrs = (int64_t)((T + 15) & ~15) * pz;
  double *Zc = nullptr;
  if (hipMalloc((void **)&Zc, (size_t)nb * zrs * 8) != hipSuccess) return 1002;
  hipLaunchKernelGGL(dbg_pack_z64_kernel, dim3((unsigned)(((int64_t)nb * zrs + 255) / 256)), dim3(256), 0, st, Z, T, nb,
                     pz, Zc);
  const int rc = dbg_finish(launch_gemm_zrm(H, ldH, Zc, pz, zrs, C, ldc, T, nb * pz, T, st, col_done, clist, ccount), st);
  hipFree(Zc);
  return rc;
}

// Lout (nrep x N x r) = ( A' B_rep ) invT on gemm_loadings_kernel.  A: plain
// K x N (the transposed left operand, rows = k); B: nrep plain K x r blocks.
// Builds Eaug (Kp x ld, ld = round_up(N, 16), Kp = round_up(K, 16)) and ZF
// (nrep blocks of Kp x rp, rp = r rounded up to even) as fact_loadings and
// boot_zf_kernel lay them out.
extern "C" int dfm_debug_gemm_loadings(dfm_ctx *ctx, const double *A, const double *B, int N, int nrep, int K, int r,
                                       double invT, double *Lout) {
  using namespace dfm;
  if (!ctx || !A || !B || !Lout || N < 1 || nrep < 1 || K < 1 || r < 1 || (int64_t)nrep * (r + 1) > INT32_MAX) return -1;
  hipStream_t st = ctx_stream(ctx);
  const int rp = (r + 1) / 2 * 2, Kp = (K + 15) / 16 * 16;
  const int64_t ld = ((int64_t)N + 15) / 16 * 16, ne = (int64_t)Kp * ld, nz = (int64_t)nrep * Kp * rp;
  double *buf = nullptr;
  if (hipMalloc((void **)&buf, (size_t)(ne + nz) * 8) != hipSuccess) return 1002;
  double *Eaug = buf, *ZF = buf + ne;
  hipLaunchKernelGGL(dbg_pack_eaug_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, A, K, N, Kp, ld, Eaug);
  hipLaunchKernelGGL(dbg_pack_zf_kernel, dim3((unsigned)((nz + 255) / 256)), dim3(256), 0, st, B, K, r, nrep, Kp, rp, ZF);
  const int rc = dbg_finish(launch_gemm_loadings(Eaug, ld, ZF, Kp, rp, N, nrep, K, r, invT, Lout, st), st);
  hipFree(buf);
  return rc;
}

// The Gram dispatch.  mode 0: launch_gram on the panel source (C, E, idx,
// eta, ld, rs) — C, idx and eta may be null — for nrep replicates into G
// (m x m at ldg, strideG apart).  mode 1: launch_gram_plain_scaled(E, ld, m,
// K, G, ldg, alpha), whose own argument check is under test.  The panels
// arrive padded as the library holds them (ld % 16 == 0, zero columns past
// N); orient 0 = ROWS (E has m rows, K columns), 1 = COLS (K rows, m columns).
extern "C" int dfm_debug_gram(dfm_ctx *ctx, int mode, int orient, const double *C, const double *E, int64_t ld,
                              const int32_t *idx, const double *eta, int64_t rs, int nrep, int m, int K, int T,
                              double *G, int64_t ldg, int64_t strideG, double alpha) {
  using namespace dfm;
  if (!ctx || !E || !G || m < 1 || K < 1 || nrep < 1 || ldg < m || (mode != 0 && mode != 1)) return -1;
  if (mode == 0) {
    if ((orient != 0 && orient != 1) || ld % 16 != 0 || ld < (orient == 0 ? K : m) || (nrep > 1 && strideG < m * ldg) ||
        ((idx || eta) && rs < (orient == 0 ? m : K)))
      return -1;
  } else if (ld < K) {
    return -1;
  }
  hipStream_t st = ctx_stream(ctx);
  hipError_t e;
  if (mode == 0) {
    PanelSrc src{C, E, idx, eta, ld, rs};
    e = launch_gram(orient, src, m, K, T, G, ldg, strideG, nrep, st);
  } else {
    e = launch_gram_plain_scaled(E, ld, m, K, G, ldg, alpha, st);
  }
  return dbg_finish(e, st);
}
