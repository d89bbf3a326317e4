// Dev microbenchmark for dfm_gemm.hip: the row-major H.Z kernel (the library's
// LDS-DMA running-pointer gemmh_kernel, and the fragment-double-buffered
// gemmh_db_kernel at several ring depths / occupancies) over the bootstrap's
// shapes, with a max-abs-difference check of every db variant against
// gemmh_kernel's output (the same products in the same order: 0 expected).
// Measured (round 2, M = K = 500, Nc = 160000): run3/3 0.695 of peak; the
// double-buffered kernel needs 219-226 VGPRs, so it runs at 2 workgroups per CU
// (db4/2, db3/2: 0.58) or spills at 3 (db3/3, db2/3: 0.09) -- rejected, kept
// here as the record.
// hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/gemm_bench tools/gemm_bench.hip
#include "../dynamicfactormodels.jl_amd/csrc/dfm_gemm.hip"
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <cstdio>
#include <vector>
using namespace dfm;
namespace dfm {
// ---------------------------------------------------------------------------
// gemmh_db_kernel: gemmh_kernel with the MFMA fragments double-
// buffered in two register sets.  A wave no longer waits on its own fragment
// reads at the top of every stage: the barrier that publishes stage s+1 (and
// retires every wave's reads of stage s, whose ring slot is refilled right
// after it) comes before stage s's MFMAs, and stage s+1's fragment reads are
// issued ahead of them.  The stage loop is unrolled by two so the sets
// alternate without register moves (tools/mfma4_occupancy_probe.hip: the 8x8
// fragment loop from LDS runs at 0.84 of peak with one set, 0.92 with two;
// operands in registers 0.95).  The prologue fills all NBUF ring slots.
DFM_DEV void g2_vmwait(int ahead) {   // own DMAs: at most `ahead` later stages (4 per stage) outstanding
  if (ahead >= 3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if (ahead == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if (ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The double-buffered stage loop shared by the LDS-DMA kernels: issue(s)
// starts stage s's DMAs into ring slot s % NBUF (4 per wave), frags(s, af, bf)
// reads this lane's 8 + 8 fragments of stage s.
template <int NBUF, class Issue, class Frags>
DFM_DEV void g2_db_mainloop(int nst, double (&acc)[8][8], Issue &issue, Frags &frags) {
  static_assert(NBUF >= 2 && NBUF <= 4, "ring depth");
  auto publish = [&](int s) {   // stage s+1 visible, every wave's reads of stage s retired
    g2_vmwait(min(NBUF - 2, nst - s - 2));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (s + NBUF < nst) issue(s + NBUF);
  };
  for (int s = 0; s < NBUF && s < nst; ++s) issue(s);
  g2_vmwait(min(NBUF, nst) - 1);
  __builtin_amdgcn_s_barrier();
  double ax[8], bx[8], ay[8], by[8];
  frags(0, ax, bx);
  for (int s = 0; s < nst; s += 2) {
    if (s + 1 < nst) {
      publish(s);
      frags(s + 1, ay, by);
    }
    tile_mfma(acc, ax, bx);
    if (s + 1 >= nst) break;
    if (s + 2 < nst) {
      publish(s + 1);
      frags(s + 2, ax, bx);
    }
    tile_mfma(acc, ay, by);
  }
}

template <int NBUF, int MINB>
__global__ __launch_bounds__(256, MINB) void gemmh_db_kernel(const double *__restrict__ A, int64_t lda,
                                                          const double *__restrict__ B, int64_t ldb,
                                                          double *__restrict__ C, int64_t ldc, int M, int Nc, int K,
                                                          int nrb, int ncb) {
  __shared__ __attribute__((aligned(16))) double lds[NBUF * G2_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int bid = blockIdx.x, xcd = bid & 7, j = bid >> 3;
  const int rb = j % nrb, cb = (j / nrb) * 8 + xcd;
  if (cb >= ncb) return;
  const int abase = rb * GT, bbase = cb * GT;
  double acc[8][8];
  tile_zero(acc);
  const int nst = (K + G2_KS - 1) / G2_KS;
  const double *pa[2], *pb[2];   // gemmh_kernel's DMA sources
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = 2 * wave + h;
    const int a = 8 * c + (lane >> 3);
    const int ka = (2 * (lane & 7)) ^ (((a >> 1) & 1) << 3);
    pa[h] = A + (int64_t)min(abase + a, M - 1) * lda + ka;
    const int kc = 2 * c + (lane >> 5);
    const int x = bbase + ((2 * (lane & 31)) ^ ((kc & 7) << 2));
    pb[h] = B + (int64_t)kc * ldb + min(x, Nc - 2);
  }
  const int64_t bstep = (int64_t)G2_KS * ldb;
  const int c0 = (2 * wave) * 128, c1 = c0 + 128;
  auto issue = [&](int s) {
    double *la = lds + (s % NBUF) * G2_STAGE, *lb = la + GT * G2_KS;
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pa[0], (lds_void_t *)(la + c0), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pb[0], (lds_void_t *)(lb + c0), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pa[1], (lds_void_t *)(la + c1), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pb[1], (lds_void_t *)(lb + c1), 16, 0, 0);
    pa[0] += G2_KS; pa[1] += G2_KS; pb[0] += bstep; pb[1] += bstep;
  };
  auto frags = [&](int s, double (&af)[8], double (&bf)[8]) {
    const double *la = lds + (s % NBUF) * G2_STAGE;
    tile_frags<g2_offA, g2_offB>(la, la + GT * G2_KS, wr, wc, lane, af, bf);
  };
  g2_db_mainloop<NBUF>(nst, acc, issue, frags);
  tile_epilogue(acc, abase, bbase, wr, wc, lane, [&](int row, int col, double v) {
    if (row < M && col < Nc) C[(int64_t)row * ldc + col] = v;
  });
}

}  // namespace dfm
__global__ void fill(double *p, size_t n, double s, int64_t ld, int valid) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) p[i] = ((int64_t)(i % ld) < valid) ? ((i * 2654435761ull) % 1000) * 1e-3 * s - 0.5 : 0.0;
}
__global__ void maxdiff(const double *a, const double *b, size_t n, unsigned long long *out) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) {
    const double d = fabs(a[i] - b[i]);
    atomicMax(out, (unsigned long long)__double_as_longlong(d));
  }
}

__global__ void fill32(float *p, size_t n, float s) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) p[i] = ((i * 2654435761ull) % 1000) * 1e-3f * s - 0.5f * s;
}

// bf16 planes of random values in [-s/2, s/2) (the upper half of the float: timing only)
__global__ void fillbf(uint16_t *p, size_t n, float s) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i < n) p[i] = (uint16_t)(__float_as_uint(((i * 2654435761ull) % 1000) * 1e-3f * s - 0.5f * s) >> 16);
}

// Round 8: gemmh_zrm_f32_kernel (the fp32 middle products) in isolation, at
// the C3 shape (T = 500, pz = 12, 9 999 replicates) and two smaller batches,
// beside gemmh_zrm_kernel on the same shape in fp64.  Operands in the chunk
// layout, every element set (pad rows included: timing only).  Round 15:
// gemmh_zrm_split_kernel (the same products as six bf16 terms) beside them, on
// random planes.  Round 19: the split kernel's fp64 epilogue (zrm_split64: the same
// product stored as fp64 rows of the column-interleaved HZ, launch_gemm_zrm_split_rows).  Round 21: the three-term
// form on planes h and m (16 KB stages), as a 3-deep ring at 3 workgroups per CU (split3_r3w3) and a 4-deep ring at 2
// (split3_r4w2); the library launches the one named by kSplit3Nbuf / kSplit3Wgs.
static void bench_f32() {
  const int T = 500, pz = 12;
  const int64_t lda = (T + 15) / 16 * 16, zrs = lda * pz;
  for (int nb : {9999, 2500, 1250}) {
    const int Nc = nb * pz;
    float *A, *Z, *C;
    double *A64, *Z64, *C64;
    uint16_t *Hs, *Zs;
    hipMalloc(&Hs, hsplit_bytes(T)); hipMalloc(&Zs, (size_t)nb * zrs * 8);
    fillbf<<<(hsplit_bytes(T) / 2 + 255) / 256, 256>>>(Hs, hsplit_bytes(T) / 2, 1.0f);
    fillbf<<<((size_t)nb * zrs * 4 + 255) / 256, 256>>>(Zs, (size_t)nb * zrs * 4, 2.0f);
    hipMalloc(&A, (size_t)T * lda * 4); hipMalloc(&Z, (size_t)nb * zrs * 4); hipMalloc(&C, (size_t)nb * zrs * 4);
    hipMalloc(&A64, (size_t)T * lda * 8); hipMalloc(&Z64, (size_t)nb * zrs * 8); hipMalloc(&C64, (size_t)T * Nc * 8);
    fill32<<<((size_t)T * lda + 255) / 256, 256>>>(A, (size_t)T * lda, 1.0f);
    fill32<<<((size_t)nb * zrs + 255) / 256, 256>>>(Z, (size_t)nb * zrs, 2.0f);
    fill<<<((size_t)T * lda + 255) / 256, 256>>>(A64, (size_t)T * lda, 1.0, lda, T);
    fill<<<((size_t)nb * zrs + 255) / 256, 256>>>(Z64, (size_t)nb * zrs, 2.0, 1, 1);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    for (int v = 0; v < 6; ++v) {
      auto run = [&]() {
        if (v == 5) launch_split<false, 3, 4, 2>(Hs, Zs, pz, zrs, C, 0, 1.0, T, Nc, T, 0);
        else if (v == 4) launch_split<false, 3, 3, 3>(Hs, Zs, pz, zrs, C, 0, 1.0, T, Nc, T, 0);
        else if (v == 3) launch_gemm_zrm_split_rows(Hs, Zs, pz, zrs, C64, Nc, 3.0, T, Nc, T, 0);
        else if (v == 2) launch_gemm_zrm_split(Hs, Zs, pz, zrs, C, T, Nc, T, 6, 0);
        else if (v == 0) launch_gemm_zrm_f32(A, lda, Z, pz, zrs, C, T, Nc, T, 0);
        else launch_gemm_zrm(A64, lda, Z64, pz, zrs, C64, Nc, T, Nc, T, 0, nullptr, nullptr, nullptr);
      };
      for (int w = 0; w < 3; ++w) run();
      const int reps = 10;
      hipEventRecord(e0);
      for (int w = 0; w < reps; ++w) run();
      hipEventRecord(e1); hipEventSynchronize(e1);
      float ms; hipEventElapsedTime(&ms, e0, e1);
      const double t = ms / reps * 1e-3, fl = 2.0 * T * (double)Nc * T, peak = v == 1 ? 78.6 : 157.3;
      // (zrm_split, split3: the fp32-equivalent rate, one product's flops; they issue six and three times as many on the bf16 path)
      printf("%s M=K=%d pz=%d nb=%5d : %8.3f ms  %6.2f TF/s (%.1f%% of %.1f)  [%s]\n",
             v == 0   ? "zrm_f32    "
             : v == 1 ? "zrm_f64    "
             : v == 2 ? "zrm_split  "
             : v == 3 ? "zrm_split64"
             : v == 4 ? "split3_r3w3"
                      : "split3_r4w2",
             T,
             pz, nb, t * 1e3, fl / t / 1e12, fl / t / 1e12 / peak * 100, peak, hipGetErrorString(hipGetLastError()));
    }
    hipFree(Hs); hipFree(Zs);
    hipFree(A); hipFree(Z); hipFree(C); hipFree(A64); hipFree(Z64); hipFree(C64);
  }
}

int main(int argc, char **argv) {
  bench_f32();
  if (argc > 1 && !strcmp(argv[1], "--f32")) return 0;
  struct Cfg { int M, K, Nc; };
  std::vector<Cfg> cfgs = {{500, 500, 160000}, {512, 512, 160000}, {500, 500, 40000}, {1024, 1024, 40000},
                           {2000, 2000, 16000}};
  for (auto c : cfgs) {
    const int64_t lda = (c.K + 15) / 16 * 16;
    const size_t na = (size_t)c.M * lda;
    const int64_t ldb = c.Nc, ldc = c.Nc;
    double *A, *B, *C, *C2;
    hipMalloc(&A, na * 8); hipMalloc(&B, (size_t)((c.K + 15) / 16 * 16) * ldb * 8); hipMemset(B, 0, (size_t)((c.K + 15) / 16 * 16) * ldb * 8);
    hipMalloc(&C, (size_t)c.M * ldc * 8); hipMalloc(&C2, (size_t)c.M * ldc * 8);
    fill<<<(na + 255) / 256, 256>>>(A, na, 1.0, lda, c.K);
    fill<<<((size_t)c.K * ldb + 255) / 256, 256>>>(B, (size_t)c.K * ldb, 2.0, ldb, c.Nc);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    const int nrb = (c.M + GT - 1) / GT, ncb = (c.Nc + GT - 1) / GT, ncb8 = (ncb + 7) / 8 * 8;
    const dim3 grid(nrb * ncb8);
    for (int v = 0; v < 5; ++v) {   // v = 0: the library's kernel, the reference of the others
      auto run = [&](double *Cout) {
        if (v == 0) {   // a rejected reference launch would leave C unwritten under every comparison below
          const hipError_t e = launch_gemm(A, lda, B, ldb, Cout, ldc, c.M, c.Nc, c.K, 0);
          if (e != hipSuccess) { fprintf(stderr, "launch_gemm: %s\n", hipGetErrorString(e)); exit(1); }
        }
        else if (v == 1) hipLaunchKernelGGL((gemmh_db_kernel<3, 3>), grid, dim3(256), 0, 0, A, lda, B, ldb, Cout, ldc, c.M, c.Nc, c.K, nrb, ncb);
        else if (v == 2) hipLaunchKernelGGL((gemmh_db_kernel<4, 2>), grid, dim3(256), 0, 0, A, lda, B, ldb, Cout, ldc, c.M, c.Nc, c.K, nrb, ncb);
        else if (v == 3) hipLaunchKernelGGL((gemmh_db_kernel<3, 2>), grid, dim3(256), 0, 0, A, lda, B, ldb, Cout, ldc, c.M, c.Nc, c.K, nrb, ncb);
        else hipLaunchKernelGGL((gemmh_db_kernel<2, 3>), grid, dim3(256), 0, 0, A, lda, B, ldb, Cout, ldc, c.M, c.Nc, c.K, nrb, ncb);
      };
      double *Cout = v == 0 ? C : C2;
      if (v > 0) hipMemset(C2, 0, (size_t)c.M * ldc * 8);
      for (int w = 0; w < 3; ++w) run(Cout);
      const int reps = 10;
      hipEventRecord(e0);
      for (int w = 0; w < reps; ++w) run(Cout);
      hipEventRecord(e1); hipEventSynchronize(e1);
      float ms; hipEventElapsedTime(&ms, e0, e1);
      const double t = ms / reps * 1e-3, fl = 2.0 * c.M * (double)c.Nc * c.K;
      static const char *names[] = {"run3/3  ", "db3/3   ", "db4/2   ", "db3/2   ", "db2/3   "};
      printf("%s M=%5d K=%5d Nc=%6d : %8.3f ms  %6.2f TF/s (%.1f%% of 78.6)\n", names[v], c.M, c.K, c.Nc, t * 1e3,
             fl / t / 1e12, fl / t / 1e12 / 78.6 * 100);
      if (v > 0) {
        unsigned long long *d, h = 0;
        hipMalloc(&d, 8); hipMemset(d, 0, 8);
        const size_t n = (size_t)c.M * ldc;
        maxdiff<<<(n + 255) / 256, 256>>>(C, C2, n, d);
        hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
        double md; memcpy(&md, &h, 8);
        printf("     max |run3/3 - db| = %.3e\n", md);
        hipFree(d);
      }
    }
    hipFree(A); hipFree(B); hipFree(C); hipFree(C2);
  }
  return 0;
}
