// dfm_fact_debug.hip — dfm_debug_hz_f32 (tests/test_gpu_f32_filter.py), dfm_debug_hz_split
// (tests/test_gpu_bf16_split.py), dfm_debug_hz_split_rows (tests/test_gpu_split_last.py) and dfm_debug_hz_split3
// (tests/test_gpu_split3.py): the fp32 and the bf16-split H.Z GEMM of the factored solver's warm filter, on operands packed as the solver packs them (zrm_ix, Zs:
// dfm_internal.h).
#include "dfm_internal.h"
#include <algorithm>
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
                                                          char *__restrict__ Zs, int planes) {
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
                                                          (int64_t)__builtin_amdgcn_readfirstlane(ch) * 96 * pz, planes);
}
// Every 16-B piece of plane l in Hs (npc = its piece count, mrows = hsplit_rows(T)) and in the nb replicates' Zs
// chunks (nch chunks of 6 pz pieces in a block of zrs / 2 pieces) to bf16 NaNs: what a three-term product must not read
__global__ void dbg_poison_l_kernel(uint4 *__restrict__ Hs, int64_t npc, int mrows, uint4 *__restrict__ Zs, int nb,
                                    int nch, int pz, int64_t zrs) {
  const uint4 nan = {0x7FC07FC0u, 0x7FC07FC0u, 0x7FC07FC0u, 0x7FC07FC0u};
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, nz = (int64_t)nb * nch * 6 * pz;
  if (i < npc && (i / (2 * mrows)) % 3 == 2) Hs[i] = nan;
  if (i < nz) {
    const int64_t rep = i / ((int64_t)nch * 6 * pz), j = i - rep * nch * 6 * pz;
    if (j % (6 * pz) >= 4 * pz) Zs[rep * (zrs / 2) + j] = nan;
  }
}
__global__ void dbg_unpack_hz32_kernel(const float *__restrict__ C32, int T, int nb, int pz, double *__restrict__ out) {
  const int64_t n = (int64_t)T * nb * pz, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = (int)(i / ((int64_t)nb * pz));
  const int x = (int)(i - (int64_t)s * nb * pz), rep = x / pz, c = x - rep * pz;
  out[i] = (double)C32[zrm_ix(rep, s, c, pz, zrm_stride(T, pz))];
}
// The three entries: one allocation [hd | packed H | packed Z | C32], the diagonal, H and Z packed as the solver packs
// them — Hs (fact_hsplit_kernel) and Zs (the solver's zsplit_store_chunk), or for F32 H32 = float(H / hmax)
// (fact_h32_kernel) and Z32 — then the product.  F32 and Split write out = double(C32) as T x nb pz, NOT rescaled by
// hmax; SplitRows reads hmax back first (it is the launch's scale, as FactBase::hmax is the solver's) and lets
// launch_gemm_zrm_split_rows write hmax C32 straight into out (row stride ldo).
// Split3: the three-term product on a Z packed with two planes into a zeroed block (as the solver's passes leave it
// in front of such a product); poison_l fills plane l of both operands with NaNs before the launch.
enum class DbgHz { F32, Split, SplitRows, Split3 };
static int dbg_hz(DbgHz kind, dfm_ctx *ctx, const double *H, int64_t ldH, int T, const double *Z, int nb, int pz,
                  double *out, int64_t ldo, double *hmax_out, bool poison_l = false) {
  const bool split = kind != DbgHz::F32, rows = kind == DbgHz::SplitRows;
  if (!ctx || !H || !Z || !out || T < 1 || nb < 1 || pz < 1 || ldH < (T + 15) / 16 * 16 ||
      (split ? pz > 32 : (ldH & 3) != 0) || (rows && ldo < (int64_t)nb * pz))
    return -1;
  hipStream_t st = ctx_stream(ctx);
  const int64_t zrs = (int64_t)((T + 15) & ~15) * pz;
  auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t b_hd = up((size_t)T * 8), b_h = up(split ? hsplit_bytes(T) : (size_t)T * ldH * 4),
               b_z = up((size_t)nb * zrs * (split ? 8 : 4)), b_c = rows ? 0 : up((size_t)nb * zrs * 4);
  char *buf = nullptr;
  if (hipMalloc((void **)&buf, b_hd + b_h + b_z + b_c) != hipSuccess) return 1002;
  double *hd = (double *)buf;
  char *Hp = buf + b_hd, *Zp = Hp + b_h;
  float *C32 = (float *)(Zp + b_z);
  hipLaunchKernelGGL(dbg_diag_kernel, dim3((T + 255) / 256), dim3(256), 0, st, H, ldH, T, hd);
  hipError_t e = split ? launch_fact_hsplit(H, ldH, T, hd, Hp, st) : launch_fact_h32(H, ldH, T, hd, (float *)Hp, st);
  const bool three = kind == DbgHz::Split3;
  if (split) {
    const int nch = (T + 15) >> 4;
    if (three) hipMemsetAsync(Zp, 0, b_z, st);
    hipLaunchKernelGGL(dbg_pack_zs_kernel, dim3((unsigned)(((int64_t)nb * nch + 3) / 4)), dim3(256), 0, st, Z, T, nb, pz,
                       Zp, three ? 2 : 3);
    if (poison_l) {
      const int64_t npc = (int64_t)(hsplit_bytes(T) / 16), n = std::max(npc, (int64_t)nb * nch * 6 * pz);
      hipLaunchKernelGGL(dbg_poison_l_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (uint4 *)Hp, npc,
                         hsplit_rows(T), (uint4 *)Zp, nb, nch, pz, zrs);
    }
  } else
    hipLaunchKernelGGL(dbg_pack_z32_kernel, dim3((unsigned)(((int64_t)nb * zrs + 255) / 256)), dim3(256), 0, st, Z, T, nb,
                       pz, (float *)Zp);
  std::vector<double> hdh(T);
  auto read_hmax = [&]() {   // behind everything queued so far
    if (e == hipSuccess) e = hipMemcpyAsync(hdh.data(), hd, (size_t)T * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? fact_hmax(hdh.data(), T) : 1.0;
  };
  double hmax = 1.0;
  if (rows) {
    hmax = read_hmax();
    if (e == hipSuccess) e = launch_gemm_zrm_split_rows(Hp, Zp, pz, zrs, out, ldo, hmax, T, nb * pz, T, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  } else {
    if (e == hipSuccess)
      e = split ? launch_gemm_zrm_split(Hp, Zp, pz, zrs, C32, T, nb * pz, T, three ? 3 : 6, st)
                : launch_gemm_zrm_f32((const float *)Hp, ldH, (const float *)Zp, pz, zrs, C32, T, nb * pz, T, st);
    hipLaunchKernelGGL(dbg_unpack_hz32_kernel, dim3((unsigned)(((int64_t)T * nb * pz + 255) / 256)), dim3(256), 0, st, C32,
                       T, nb, pz, out);
    hmax = read_hmax();
  }
  if (e == hipSuccess) e = hipGetLastError();
  hipFree(buf);
  if (e != hipSuccess) return 1000 + (int)e;
  if (hmax_out) *hmax_out = hmax;
  return 0;
}
}  // namespace dfm

// Debug entries, not part of include/dfm.h.  H: device, T x ldH fp64, ldH >= round_up(T, 16) with zero padding
// columns (a multiple of 4 for the fp32 kernel); Z: device, T x nb pz fp64 (replicate rep's columns rep pz .. rep pz +
// pz - 1; pz <= 32 for the split kernel); out: device, T x nb pz; hmax is returned in *hmax_out (may be null).
// gemmh_zrm_f32_kernel:
extern "C" int dfm_debug_hz_f32(dfm_ctx *ctx, const double *H, int64_t ldH, int T, const double *Z, int nb, int pz,
                                double *out, double *hmax_out) {
  return dfm::dbg_hz(dfm::DbgHz::F32, ctx, H, ldH, T, Z, nb, pz, out, 0, hmax_out);
}
// gemmh_zrm_split_kernel:
extern "C" int dfm_debug_hz_split(dfm_ctx *ctx, const double *H, int64_t ldH, int T, const double *Z, int nb, int pz,
                                  double *out, double *hmax_out) {
  return dfm::dbg_hz(dfm::DbgHz::Split, ctx, H, ldH, T, Z, nb, pz, out, 0, hmax_out);
}
// ... through its fp64 epilogue (tests/test_gpu_split_last.py): out has row stride ldo >= nb pz, and nothing of it but
// the T x nb pz elements is written
extern "C" int dfm_debug_hz_split_rows(dfm_ctx *ctx, const double *H, int64_t ldH, int T, const double *Z, int nb, int pz,
                                       double *out, int64_t ldo, double *hmax_out) {
  return dfm::dbg_hz(dfm::DbgHz::SplitRows, ctx, H, ldH, T, Z, nb, pz, out, ldo, hmax_out);
}
// ... as three terms on planes h and m (launch_gemm_zrm_split, terms = 3): out = double(C32), not rescaled by hmax.
// poison_l != 0: plane l of the packed H and Z holds NaNs when the product runs
extern "C" int dfm_debug_hz_split3(dfm_ctx *ctx, const double *H, int64_t ldH, int T, const double *Z, int nb, int pz,
                                   double *out, double *hmax_out, int poison_l) {
  return dfm::dbg_hz(dfm::DbgHz::Split3, ctx, H, ldH, T, Z, nb, pz, out, 0, hmax_out, poison_l != 0);
}
