// dfm_fact_debug.hip — dfm_debug_hz_f32 (tests/test_gpu_f32_filter.py),
// dfm_debug_hz_split (tests/test_gpu_bf16_split.py) and dfm_debug_hz_split_rows
// (tests/test_gpu_split_last.py): the fp32 and the bf16-split H.Z GEMM of the
// factored solver's warm filter, on operands packed as the solver packs them
// (zrm_ix, Zs: dfm_internal.h).
#include "dfm_internal.h"
#include <vector>

namespace dfm {

__global__ void dbg_diag_kernel(const double *__restrict__ H, int64_t ldH, int T, double *__restrict__ hd) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < T) hd[t] = H[(int64_t)t * ldH + t];
}
// Z (T x nb pz, row-major, column block = replicate) -> Z32 chunks (zrm_ix, float, chunk rows past T zero)
__global__ void dbg_pack_z32_kernel(const double *__restrict__ Z, int T, int nb, int pz, float *__restrict__ Z32) {
  const int64_t zrs = zrm_stride(T, pz), n = (int64_t)nb * zrs;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int rep = (int)(i / zrs);
  const int64_t o = i - (int64_t)rep * zrs;
  const int ch = (int)(o / (16 * pz)), w = (int)(o - (int64_t)ch * 16 * pz), c = w >> 4, s = 16 * ch + (w & 15);
  Z32[zrm_ix(rep, s, c, pz, zrs)] = s < T ? (float)Z[(int64_t)s * nb * pz + (int64_t)rep * pz + c] : 0.0f;
}
// Z -> Zs (dfm_internal.h), one wave per chunk with the solver's own store: the chunk's doubles are gathered into
// the wave's LDS stage first, column-major, rows past T zero
__global__ __launch_bounds__(256) void dbg_pack_zs_kernel(const double *__restrict__ Z, int T, int nb, int pz,
                                                          char *__restrict__ Zs) {
  __shared__ double stage[4][16 * 32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nch = (T + 15) >> 4;
  const int64_t zrs = zrm_stride(T, pz), id = (int64_t)blockIdx.x * 4 + wave;
  if (id >= (int64_t)nb * nch) return;
  const int rep = (int)(id / nch), ch = (int)(id - (int64_t)rep * nch);
  for (int e = lane; e < 16 * pz; e += 64) {
    const int c = e >> 4, s = 16 * ch + (e & 15);
    stage[wave][e] = s < T ? Z[(int64_t)s * nb * pz + (int64_t)rep * pz + c] : 0.0;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  zsplit_store_chunk<false>(stage[wave], pz, lane, Zs + __builtin_amdgcn_readfirstlane(rep) * zrs * 8 +
                                                          (int64_t)__builtin_amdgcn_readfirstlane(ch) * 96 * pz);
}
__global__ void dbg_unpack_hz32_kernel(const float *__restrict__ C32, int T, int nb, int pz, double *__restrict__ out) {
  const int64_t n = (int64_t)T * nb * pz, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = (int)(i / ((int64_t)nb * pz));
  const int x = (int)(i - (int64_t)s * nb * pz), rep = x / pz, c = x - rep * pz;
  out[i] = (double)C32[zrm_ix(rep, s, c, pz, zrm_stride(T, pz))];
}
}  // namespace dfm

// Debug entry, not part of include/dfm.h.  H: device, T x ldH fp64, ldH >=
// round_up(T, 16) with zero padding columns; Z: device, T x nb pz fp64
// (replicate rep's columns rep pz .. rep pz + pz - 1).  Builds H32 =
// float(H / hmax) (fact_h32_kernel) and Z32, runs gemmh_zrm_f32_kernel and
// writes out = double(H32 Z32) as T x nb pz — NOT rescaled by hmax, which is
// returned in *hmax_out (may be null).
extern "C" int dfm_debug_hz_f32(dfm_ctx *ctx, const double *H, int64_t ldH, int T, const double *Z, int nb, int pz,
                                double *out, double *hmax_out) {
  using namespace dfm;
  if (!ctx || !H || !Z || !out || T < 1 || nb < 1 || pz < 1 || ldH < (T + 15) / 16 * 16 || (ldH & 3)) return -1;
  hipStream_t st = ctx_stream(ctx);
  const int64_t zrs = (int64_t)((T + 15) & ~15) * pz;
  char *buf = nullptr;
  const size_t b_hd = ((size_t)T * 8 + 255) & ~size_t(255), b_h32 = ((size_t)T * ldH * 4 + 255) & ~size_t(255),
               b_z = ((size_t)nb * zrs * 4 + 255) & ~size_t(255);
  if (hipMalloc((void **)&buf, b_hd + b_h32 + 2 * b_z) != hipSuccess) return 1002;
  double *hd = (double *)buf;
  float *H32 = (float *)(buf + b_hd), *Z32 = (float *)(buf + b_hd + b_h32), *C32 = (float *)(buf + b_hd + b_h32 + b_z);
  hipLaunchKernelGGL(dbg_diag_kernel, dim3((T + 255) / 256), dim3(256), 0, st, H, ldH, T, hd);
  hipError_t e = launch_fact_h32(H, ldH, T, hd, H32, st);
  hipLaunchKernelGGL(dbg_pack_z32_kernel, dim3((unsigned)(((int64_t)nb * zrs + 255) / 256)), dim3(256), 0, st, Z, T, nb,
                     pz, Z32);
  if (e == hipSuccess) e = launch_gemm_zrm_f32(H32, ldH, Z32, pz, zrs, C32, T, nb * pz, T, st);
  hipLaunchKernelGGL(dbg_unpack_hz32_kernel, dim3((unsigned)(((int64_t)T * nb * pz + 255) / 256)), dim3(256), 0, st, C32,
                     T, nb, pz, out);
  std::vector<double> hdh(T);
  if (e == hipSuccess) e = hipMemcpyAsync(hdh.data(), hd, (size_t)T * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipGetLastError();
  hipFree(buf);
  if (e != hipSuccess) return 1000 + (int)e;
  if (hmax_out) *hmax_out = fact_hmax(hdh.data(), T);
  return 0;
}

// The same for the bf16-split product: Hs (fact_hsplit_kernel) and Zs (the
// solver's zsplit_store_chunk), gemmh_zrm_split_kernel, out = double(C32);
// pz <= 32.
extern "C" int dfm_debug_hz_split(dfm_ctx *ctx, const double *H, int64_t ldH, int T, const double *Z, int nb, int pz,
                                  double *out, double *hmax_out) {
  using namespace dfm;
  if (!ctx || !H || !Z || !out || T < 1 || nb < 1 || pz < 1 || pz > 32 || ldH < (T + 15) / 16 * 16) return -1;
  hipStream_t st = ctx_stream(ctx);
  const int64_t zrs = (int64_t)((T + 15) & ~15) * pz;
  const int nch = (T + 15) >> 4;
  char *buf = nullptr;
  const size_t b_hd = ((size_t)T * 8 + 255) & ~size_t(255), b_hs = (hsplit_bytes(T) + 255) & ~size_t(255),
               b_z = ((size_t)nb * zrs * 8 + 255) & ~size_t(255), b_c = ((size_t)nb * zrs * 4 + 255) & ~size_t(255);
  if (hipMalloc((void **)&buf, b_hd + b_hs + b_z + b_c) != hipSuccess) return 1002;
  double *hd = (double *)buf;
  char *Hs = buf + b_hd, *Zs = buf + b_hd + b_hs;
  float *C32 = (float *)(buf + b_hd + b_hs + b_z);
  hipLaunchKernelGGL(dbg_diag_kernel, dim3((T + 255) / 256), dim3(256), 0, st, H, ldH, T, hd);
  hipError_t e = launch_fact_hsplit(H, ldH, T, hd, Hs, st);
  hipLaunchKernelGGL(dbg_pack_zs_kernel, dim3((unsigned)(((int64_t)nb * nch + 3) / 4)), dim3(256), 0, st, Z, T, nb, pz, Zs);
  if (e == hipSuccess) e = launch_gemm_zrm_split(Hs, Zs, pz, zrs, C32, T, nb * pz, T, st);
  hipLaunchKernelGGL(dbg_unpack_hz32_kernel, dim3((unsigned)(((int64_t)T * nb * pz + 255) / 256)), dim3(256), 0, st, C32,
                     T, nb, pz, out);
  std::vector<double> hdh(T);
  if (e == hipSuccess) e = hipMemcpyAsync(hdh.data(), hd, (size_t)T * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipGetLastError();
  hipFree(buf);
  if (e != hipSuccess) return 1000 + (int)e;
  if (hmax_out) *hmax_out = fact_hmax(hdh.data(), T);
  return 0;
}

// The split product through the kernel's fp64 epilogue (round 19,
// tests/test_gpu_split_last.py): the same Hs and Zs, and
// launch_gemm_zrm_split_rows writes hmax C32 straight into the caller's out
// (device, T rows of nb pz columns, row stride ldo >= nb pz).  Nothing of out
// but those T x nb pz elements is written.
extern "C" int dfm_debug_hz_split_rows(dfm_ctx *ctx, const double *H, int64_t ldH, int T, const double *Z, int nb, int pz,
                                       double *out, int64_t ldo, double *hmax_out) {
  using namespace dfm;
  if (!ctx || !H || !Z || !out || T < 1 || nb < 1 || pz < 1 || pz > 32 || ldH < (T + 15) / 16 * 16 ||
      ldo < (int64_t)nb * pz)
    return -1;
  hipStream_t st = ctx_stream(ctx);
  const int64_t zrs = (int64_t)((T + 15) & ~15) * pz;
  const int nch = (T + 15) >> 4;
  char *buf = nullptr;
  const size_t b_hd = ((size_t)T * 8 + 255) & ~size_t(255), b_hs = (hsplit_bytes(T) + 255) & ~size_t(255),
               b_z = ((size_t)nb * zrs * 8 + 255) & ~size_t(255);
  if (hipMalloc((void **)&buf, b_hd + b_hs + b_z) != hipSuccess) return 1002;
  double *hd = (double *)buf;
  char *Hs = buf + b_hd, *Zs = buf + b_hd + b_hs;
  hipLaunchKernelGGL(dbg_diag_kernel, dim3((T + 255) / 256), dim3(256), 0, st, H, ldH, T, hd);
  hipError_t e = launch_fact_hsplit(H, ldH, T, hd, Hs, st);
  hipLaunchKernelGGL(dbg_pack_zs_kernel, dim3((unsigned)(((int64_t)nb * nch + 3) / 4)), dim3(256), 0, st, Z, T, nb, pz, Zs);
  std::vector<double> hdh(T);   // hmax first: it is the launch's scale, as FactBase::hmax is the solver's
  if (e == hipSuccess) e = hipMemcpyAsync(hdh.data(), hd, (size_t)T * 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  const double hmax = e == hipSuccess ? fact_hmax(hdh.data(), T) : 1.0;
  if (e == hipSuccess) e = launch_gemm_zrm_split_rows(Hs, Zs, pz, zrs, out, ldo, hmax, T, nb * pz, T, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipGetLastError();
  hipFree(buf);
  if (e != hipSuccess) return 1000 + (int)e;
  if (hmax_out) *hmax_out = hmax;
  return 0;
}
