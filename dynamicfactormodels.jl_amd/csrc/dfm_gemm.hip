// dfm_gemm.hip — the LDS-DMA GEMMs on MFMA: every kernel here stages its
// operands with global_load_lds_dwordx4 (no VGPR staging, no ds_write pass)
// through a ring of 16-deep stages (dfm_tile.h: ring_wait).
//
// This is the compute core of the factored bootstrap (dfm_fact.hip): one
// fixed, cache-resident left operand (H = E E' or E') shared by every
// replicate of a batch, so the per-replicate eigen-iterations and the
// loadings pass become single large MFMA GEMMs instead of nb memory-bound
// skinny products.  The fp64 kernels compute one 64 x 64 tile per workgroup
// (v_mfma_f64_4x4x4_4b) and differ in what they stage and where they store:
//   gemmh_kernel          C = A B, B row-major (gram_wk's Q = W K)
//   gemmh_zrm_kernel      C = H Z, Z replicate-major chunks, column compaction
//   gram_dma_kernel       G = alpha X X', lower tiles, split-K
//   gemm_loadings_kernel  L* = [E' | L] [ZF ; M1] / T
// The first three take the tile (accumulators, k step, epilogue) from
// dfm_tile.h; gemm_loadings_kernel shares only ring_wait and writes the same
// tile out itself (on the shared k step it measured 3.6 % slower).
// Grid order is XCD-aware: the row blocks of one column block are issued to
// one XCD so a B tile is fetched from HBM once and re-read from that XCD's L2.
// Two kernels are not fp64, both for the middle products of a warm
// eigenvalue-rule solve's first filter: gemmh_zrm_split_kernel (six bf16 terms
// on v_mfma_f32_32x32x16_bf16, three in the products two or more short of the
// filter's last: the default) and gemmh_zrm_f32_kernel
// (v_mfma_f32_32x32x2_f32, DFM_FACT_SPLIT=0).
#include "dfm_internal.h"
#include "dfm_tile.h"

namespace dfm {

// All of a kernel's LDS is one __shared__ array (a second object makes hipcc
// drain vmcnt before ds_reads).  The two 64 x 16 images of a stage, as
// dfm_gram.hip's: [a][k] with 128-B rows, k XOR-swizzled by 8 ((a >> 1) & 1);
// [k][a] with 512-B rows, a XOR-swizzled by 4 (k & 7).  DMA writes are
// lane-linear, so the swizzle is applied to the per-lane SOURCE address.
namespace {
constexpr int GT = 64, G2_KS = 16, G2_STAGE = 2 * GT * G2_KS;   // doubles per stage (A + B)
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;
DFM_DEV int g2_offA(int a, int kc) { return a * G2_KS + (kc ^ (((a >> 1) & 1) << 3)); }   // [a][k]
DFM_DEV int g2_offB(int a, int kc) { return kc * GT + (a ^ ((kc & 7) << 2)); }           // [k][a]
}  // namespace

// Ring/occupancy choice of gram_dma_kernel by output height: rows >= 1024
// run the 3-deep ring at 3 workgroups per CU (more resident waves beat a
// deeper ring there: tools/gemm_bench.hip, M = 2000).
static bool gemm_ring3(int M) { return M >= 1024; }

// ---------------------------------------------------------------------------
// gemmh_kernel: C (M x Nc) = A B.  A: M x K row-major in an [a][k] image,
// lda >= round_up(K, 16) with zero k-padding; B: K x Nc row-major in a [k][a]
// image, zero rows up to round_up(K, 16), so the DMA sources are running
// pointers advanced by one stage per issue (no per-stage 64-bit address
// arithmetic, no k-tail clamp).  Out-of-range rows / columns read clamped
// (finite) data that only reaches discarded outputs.  3-deep ring at 3
// workgroups per CU (tools/gemm_bench.hip: 0.62 of peak at the C3 shape, 0.75
// at M = K = 2000).
__global__ __launch_bounds__(256, 3) void gemmh_kernel(const double *__restrict__ A, int64_t lda,
                                                      const double *__restrict__ B, int64_t ldb,
                                                      double *__restrict__ C, int64_t ldc, int M, int Nc, int K,
                                                      int nrb, int ncb) {
  constexpr int NBUF = 3;
  __shared__ __attribute__((aligned(16))) double lds[NBUF * G2_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  // XCD-aware mapping: blocks b and b+8 share an XCD (round-robin dispatch)
  const int bid = blockIdx.x, xcd = bid & 7, j = bid >> 3;
  const int rb = j % nrb, cb = (j / nrb) * 8 + xcd;
  if (cb >= ncb) return;
  const int abase = rb * GT, bbase = cb * GT;
  double acc[8][8];
  tile_zero(acc);
  const int nst = (K + G2_KS - 1) / G2_KS;
  // per-lane DMA sources: A chunk rows 8c..8c+7 (lane pair lane & 7), B chunk
  // k-rows 2c, 2c+1 (lane pair lane & 31), the images' swizzle on the source column
  const double *pa[2], *pb[2];
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
  for (int s = 0; s < NBUF - 1 && s < nst; ++s) issue(s);
  for (int s = 0; s < nst; ++s) {
    ring_wait<NBUF>(s, nst);
    if (s + NBUF - 1 < nst) issue(s + NBUF - 1);   // ring slot (s-1)%NBUF: its readers all passed this barrier
    const double *la = lds + (s % NBUF) * G2_STAGE;
    tile_step<g2_offA, g2_offB>(acc, la, la + GT * G2_KS, wr, wc, lane);
  }
  tile_epilogue(acc, abase, bbase, wr, wc, lane, [&](int row, int col, double v) {
    if (row < M && col < Nc) C[(int64_t)row * ldc + col] = v;
  });
}

// C (M x Nc, ldc) = A B on gemmh_kernel.  hipErrorInvalidValue unless A has
// its zero k-padding (lda >= round_up(K, 16)), Nc is even (a lane's 16-B
// column pair) and the strides keep the pairs 16-B aligned; B must hold
// round_up(K, 16) rows, the ones past K zero.
hipError_t launch_gemm(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int M,
                       int Nc, int K, hipStream_t st) {
  if (M < 1 || K < 1 || Nc < 2 || (Nc & 1) || lda < (K + G2_KS - 1) / G2_KS * G2_KS || (lda & 1) || ldb < Nc ||
      (ldb & 1) || ldc < Nc)
    return hipErrorInvalidValue;
  const int nrb = (M + GT - 1) / GT, ncb = (Nc + GT - 1) / GT;
  const int ncb8 = (ncb + 7) / 8 * 8;
  hipLaunchKernelGGL(gemmh_kernel, dim3(nrb * ncb8), dim3(256), 0, st, A, lda, B, ldb, C, ldc, M, Nc, K, nrb, ncb);
  return hipGetLastError();
}

// clist: column compaction by indirection — compact column x of Z / C is
// column x % cg of replicate clist[x / cg] (x / cg < ccount).
DFM_DEV int64_t g2_phys_col(int x, const int *__restrict__ clist, int ccount, int cg) {
  const int slot = min(x / cg, ccount - 1);   // past the list: finite data, discarded outputs
  return (int64_t)clist[slot] * cg + (x - (x / cg) * cg);
}

// ---------------------------------------------------------------------------
// gemmh_zrm_kernel: the factored solver's H.Z with Z replicate-major (round 6).
// Z holds replicate rep's T x pz block as 16-row chunks, each chunk column-
// major: element (s, c) at rep zrs + (s >> 4) 16 pz + 16 c + (s & 15)
// (zrs = round_up(T, 16) pz, the chunk rows past T zero).  A 16-deep k stage
// of one B column is then ONE 128-B line, so the B operand is staged like A
// (and like gram_dma_kernel's second operand): an [a][k] LDS image, 8 columns
// per DMA instruction, each column's 16 k values one line — a 64-column tile
// spanning 5.33 replicates reads whole lines, where the column-interleaved
// T x nb pz layout read one 512-B k-row segment and a replicate-major
// [rep][T][pz] layout six 96-B pieces per k-row (round 5: +5.6 % GEMM).
// The passes that write Z (zscatter_tail, boot_cheb_mid_kernel) then write
// each replicate's 16-row tile as one contiguous 16 pz x 8-B chunk.  The
// fragments hold the same elements as with a row-major Z in gemmh_kernel, so
// HZ has the same bits; C (HZ) keeps the column-interleaved layout (its rows
// are gathered by idx).  A = H as gemmh_kernel's (lda >= round_up(K, 16), zero
// k-padding); 3-deep ring at 3 workgroups per CU; column compaction by clist.
__global__ __launch_bounds__(256, 3) void gemmh_zrm_kernel(const double *__restrict__ A, int64_t lda,
                                                          const double *__restrict__ Z, int pz, int64_t zrs,
                                                          double *__restrict__ C, int64_t ldc, int M, int Nc, int K,
                                                          int nrb, int ncb, const int *__restrict__ col_done,
                                                          const int *__restrict__ clist, const int *__restrict__ ccount_p) {
  constexpr int NBUF = 3;
  __shared__ __attribute__((aligned(16))) double lds[NBUF * G2_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int bid = blockIdx.x, xcd = bid & 7, j = bid >> 3;
  const int rb = j % nrb, cb = (j / nrb) * 8 + xcd;
  if (cb >= ncb) return;
  const int abase = rb * GT, bbase = cb * GT, col_group = pz;
  // compacted launch (straggler phase): column block cb of the listed
  // replicates' column groups only.  The list is rebuilt on the device after
  // every convergence check; compaction applies once it holds < 1/8 of the
  // batch (Nc / col_group replicates), decided here from its device-side
  // count, so the host never waits for it.  Either way a column's sum runs in
  // the same order: the bits do not depend on the mode.
  const int ccount = clist ? *ccount_p : 0;
  const bool compact = clist && (int64_t)ccount * 8 < Nc / col_group;
  clist = compact ? clist : nullptr;
  if (compact) {
    if (bbase >= ccount * col_group) return;
    if (col_done) {   // every listed replicate of the block retired since the list was built
      bool all = true;
      const int s0 = bbase / col_group, s1 = min(ccount - 1, (bbase + GT - 1) / col_group);
      for (int q = s0; q <= s1; ++q) all = all && col_done[clist[q]];
      if (all) return;
    }
  } else if (col_done) {
    bool all = true;
    const int r0 = bbase / col_group, r1 = min(Nc - 1, bbase + GT - 1) / col_group;
    for (int q = r0; q <= r1; ++q) all = all && col_done[q];
    if (all) return;
  }
  double acc[8][8];
  tile_zero(acc);
  const int nst = (K + G2_KS - 1) / G2_KS;
  // per-lane DMA sources: rows a of the A block and columns a of the B block,
  // 16 k per row in 8 lane pairs (the [a][k] images' XOR swizzle on the source k)
  const double *pa[2], *pb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = 2 * wave + h;
    const int a = 8 * c + (lane >> 3);
    const int ka = (2 * (lane & 7)) ^ (((a >> 1) & 1) << 3);
    pa[h] = A + (int64_t)min(abase + a, M - 1) * lda + ka;
    const int x = bbase + a;
    int rep, cc;
    if (clist) {   // compact column x: replicate clist[x / pz] (past the list: finite, discarded)
      const int slot = min(x / pz, ccount - 1);
      rep = clist[slot];
      cc = x - (x / pz) * pz;
    } else {
      const int xc = min(x, Nc - 1);   // past Nc: finite data, discarded outputs
      rep = xc / pz;
      cc = xc - rep * pz;
    }
    pb[h] = Z + (int64_t)rep * zrs + 16 * cc + ka;
  }
  const int64_t bstep = (int64_t)G2_KS * pz;
  const int c0 = (2 * wave) * 128, c1 = c0 + 128;
  auto issue = [&](int s) {
    double *la = lds + (s % NBUF) * G2_STAGE, *lb = la + GT * G2_KS;
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pa[0], (lds_void_t *)(la + c0), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pb[0], (lds_void_t *)(lb + c0), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pa[1], (lds_void_t *)(la + c1), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pb[1], (lds_void_t *)(lb + c1), 16, 0, 0);
    pa[0] += G2_KS; pa[1] += G2_KS; pb[0] += bstep; pb[1] += bstep;
  };
  for (int s = 0; s < NBUF - 1 && s < nst; ++s) issue(s);
  for (int s = 0; s < nst; ++s) {
    ring_wait<NBUF>(s, nst);
    if (s + NBUF - 1 < nst) issue(s + NBUF - 1);
    const double *la = lds + (s % NBUF) * G2_STAGE;
    tile_step<g2_offA, g2_offA>(acc, la, la + GT * G2_KS, wr, wc, lane);
  }
  if (clist)
    tile_epilogue(acc, abase, bbase, wr, wc, lane, [&](int row, int col, double v) {
      if (row < M && col < ccount * col_group)
        C[(int64_t)row * ldc + g2_phys_col(col, clist, ccount, col_group)] = v;
    });
  else
    tile_epilogue(acc, abase, bbase, wr, wc, lane, [&](int row, int col, double v) {
      if (row < M && col < Nc) C[(int64_t)row * ldc + col] = v;
    });
}

// H (M x K, lda >= round_up(K, 16), zero k-padding) times the replicate-major
// chunked Z of nb = Nc / pz replicates (gemmh_zrm_kernel) -> C (M x Nc, ldc)
hipError_t launch_gemm_zrm(const double *A, int64_t lda, const double *Z, int pz, int64_t zrs, double *C,
                           int64_t ldc, int M, int Nc, int K, hipStream_t st, const int *col_done, const int *clist,
                           const int *ccount) {
  if (lda < (K + G2_KS - 1) / G2_KS * G2_KS || pz < 2 || (pz & 1) || Nc % pz) return hipErrorInvalidValue;
  const int nrb = (M + GT - 1) / GT, ncb = (Nc + GT - 1) / GT;
  const int ncb8 = (ncb + 7) / 8 * 8;
  hipLaunchKernelGGL(gemmh_zrm_kernel, dim3(nrb * ncb8), dim3(256), 0, st, A, lda, Z, pz, zrs, C, ldc, M, Nc, K, nrb,
                     ncb, col_done, clist, ccount);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// gemmh_zrm_f32_kernel: C32 = H32 Z32 in fp32 (v_mfma_f32_32x32x2_f32) for the middle products of a warm solve's
// filter-only first step under the eigenvalue rule (dfm_fact_plan.h: HzProduct::F32).  H32 is the model's H in float,
// divided by its largest diagonal entry (|H32| <= 1; lda >= round_up(K, 16), zero k-padding); Z32 and C32 both use the
// replicate-major 16-row chunk indexing of gemmh_zrm_kernel's Z with float elements (element (s, c) of replicate rep
// at rep zrs + (s >> 4) 16 pz + 16 c + (s & 15), chunk rows past the matrix zero in Z32, unspecified in C32).
// 128 x 128 workgroup tile, each wave 64 x 64 as 2 x 2 MFMA tiles (64 accumulator VGPRs); 16-deep k stages by LDS-DMA
// through a 3-deep ring at 3 workgroups per CU (16 KB per stage), one barrier per stage as gemmh_zrm_kernel.  Both
// LDS images are [a][k] with 64-B rows; the 16-B piece q of row a sits at piece q ^ ((a >> 2) & 3), so the
// ds_read_b128 fragment reads (32 rows x one piece per half-wave) touch 16 distinct 16-B slots in each of the
// instruction's 16-lane groups.  Lane half h reads k = 8h .. 8h+7 of its row in two 16-B pieces and MFMA step e pairs
// k = e (h = 0) with k = 8 + e (h = 1): a column's sum runs over k in one fixed order whatever its tile, its place in
// the batch or nb.  The epilogue stores the accumulator's four consecutive rows per register group as one 16-B piece
// of the column's chunk.  No col_done / clist: every replicate is active in step 0.
namespace {
constexpr int F32_GT = 128, F32_KS = 16, F32_STAGE = 2 * F32_GT * F32_KS;   // floats per stage (A + B)
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
}  // namespace

__global__ __launch_bounds__(256, 3) void gemmh_zrm_f32_kernel(const float *__restrict__ A, int64_t lda,
                                                              const float *__restrict__ Z, int pz, int64_t zrs,
                                                              float *__restrict__ C, int M, int Nc, int K, int nrb,
                                                              int ncb) {
  constexpr int NBUF = 3;
  __shared__ __attribute__((aligned(16))) float lds[NBUF * F32_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int bid = blockIdx.x, xcd = bid & 7, j = bid >> 3;
  const int rb = j % nrb, cb = (j / nrb) * 8 + xcd;
  if (cb >= ncb) return;
  const int abase = rb * F32_GT, bbase = cb * F32_GT;
  const int nst = (K + F32_KS - 1) / F32_KS;
  // per-lane DMA sources: 16 rows (columns) per instruction, four 16-B pieces
  // per row, the images' XOR swizzle on the source piece
  const float *pa[2], *pb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int a = 16 * (2 * wave + h) + (lane >> 2);
    const int kq = 4 * ((lane & 3) ^ ((a >> 2) & 3));
    pa[h] = A + (int64_t)min(abase + a, M - 1) * lda + kq;   // rows past M: finite data, discarded outputs
    const int xc = min(bbase + a, Nc - 1);                    // columns past Nc likewise
    const int rep = xc / pz, cc = xc - rep * pz;
    pb[h] = Z + (int64_t)rep * zrs + 16 * cc + kq;
  }
  const int64_t bstep = (int64_t)F32_KS * pz;
  const int c0 = (2 * wave) * 256, c1 = c0 + 256;
  auto issue = [&](int s) {
    float *la = lds + (s % NBUF) * F32_STAGE, *lb = la + F32_GT * F32_KS;
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pa[0], (lds_void_t *)(la + c0), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pb[0], (lds_void_t *)(lb + c0), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pa[1], (lds_void_t *)(la + c1), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pb[1], (lds_void_t *)(lb + c1), 16, 0, 0);
    pa[0] += F32_KS; pa[1] += F32_KS; pb[0] += bstep; pb[1] += bstep;
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[ti][tj][v] = 0.0f;
  // fragment offsets (floats) inside an image: row r32 of tile t, pieces 2h and 2h + 1
  const int r32 = lane & 31, hh = lane >> 5;
  int fo[2][2][2];   // [operand][tile][piece]
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int ra = wr * 64 + 32 * t + r32, rbx = wc * 64 + 32 * t + r32;
      fo[0][t][q] = ra * F32_KS + 4 * ((2 * hh + q) ^ ((ra >> 2) & 3));
      fo[1][t][q] = rbx * F32_KS + 4 * ((2 * hh + q) ^ ((rbx >> 2) & 3));
    }
  for (int s = 0; s < NBUF - 1 && s < nst; ++s) issue(s);
  for (int s = 0; s < nst; ++s) {
    ring_wait<NBUF>(s, nst);
    if (s + NBUF - 1 < nst) issue(s + NBUF - 1);
    const float *la = lds + (s % NBUF) * F32_STAGE, *lb = la + F32_GT * F32_KS;
    f32x4 af[2][2], bf[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        af[t][q] = *reinterpret_cast<const f32x4 *>(la + fo[0][t][q]);
        bf[t][q] = *reinterpret_cast<const f32x4 *>(lb + fo[1][t][q]);
      }
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int tj = 0; tj < 2; ++tj)
            acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[ti][q][e], bf[tj][q][e], acc[ti][tj], 0, 0, 0);
  }
  // accumulator register v of lane l: row 8 (v >> 2) + 4 (l >> 5) + (v & 3), column l & 31
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
    const int x = bbase + wc * 64 + 32 * tj + r32;
    if (x >= Nc) continue;
    const int rep = x / pz, cc = x - rep * pz;
    float *cp = C + (int64_t)rep * zrs + 16 * cc;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = abase + wr * 64 + 32 * ti + 8 * g + 4 * hh;
        if (row < M)   // (rows row .. row + 3 stay inside the chunk: its pad rows take discarded values)
          *reinterpret_cast<f32x4 *>(cp + (int64_t)(row >> 4) * (16 * pz) + (row & 15)) =
              f32x4{acc[ti][tj][4 * g], acc[ti][tj][4 * g + 1], acc[ti][tj][4 * g + 2], acc[ti][tj][4 * g + 3]};
      }
  }
}

// H32 (M x K floats, lda >= round_up(K, 16), zero k-padding) times the
// replicate-major chunked Z32 of nb = Nc / pz replicates -> C32 in the same
// chunk layout (gemmh_zrm_f32_kernel); zrs = round_up(K, 16) pz = round_up(M, 16) pz
hipError_t launch_gemm_zrm_f32(const float *A, int64_t lda, const float *Z, int pz, int64_t zrs, float *C, int M,
                               int Nc, int K, hipStream_t st) {
  const int64_t kpad = (K + F32_KS - 1) / F32_KS * F32_KS;
  if (M < 1 || lda < kpad || (lda & 3) || pz < 1 || Nc < pz || Nc % pz || M != K || zrs < kpad * pz || (zrs & 3))
    return hipErrorInvalidValue;
  const int nrb = (M + F32_GT - 1) / F32_GT, ncb = (Nc + F32_GT - 1) / F32_GT;
  const int ncb8 = (ncb + 7) / 8 * 8;
  hipLaunchKernelGGL(gemmh_zrm_f32_kernel, dim3(nrb * ncb8), dim3(256), 0, st, A, lda, Z, pz, zrs, C, M, Nc, K, nrb,
                     ncb);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// gemmh_zrm_split_kernel: the same product, C32 ~ (H / hmax) Z, as six bf16 MFMA terms (HzProduct::Split).  Both
// operands arrive split into three bf16 planes, x ~ h + m + l (dfm_internal.h: Hs, Zs; the GEMM converts nothing), and
// C32 = sum over the plane pairs of weight >= 2^-18 — (l,h) (h,l) (m,m) (m,h) (h,m) (h,h), the small terms first — on
// v_mfma_f32_32x32x16_bf16 with fp32 accumulators: a product of two bf16 numbers is exact in fp32, and the dropped
// pairs and split remainders are below 2^-25 |H| |Z|.
// Tile, waves, XCD order and epilogue are gemmh_zrm_f32_kernel's.  One k = 16 stage is 24 KB: per operand six
// [128 rows] images of 16-B pieces, one per (plane, k half) — piece (pi, kh, a) at (2 pi + kh) 128 + a, so a wave's
// 1 KB DMA instruction fills 64 consecutive rows of one image from 64 consecutive pieces of Hs (or one image's pieces
// of consecutive Z columns), and a ds_read_b128 fragment read (lane: row l & 31, k half l >> 5) touches 16 distinct
// 16-B slots in each of its 16-lane groups with no swizzle.  The six terms share one set of fragments per stage: 12
// reads per 24 MFMAs.  3-deep ring at 2 workgroups per CU (72 KB), six DMA instructions per wave and stage.  Every
// output element adds its six terms in that order stage by stage, whatever its tile, its place in the batch, nb or
// the lane.
// ROWS64 (HzProduct::SplitRows, the warm filter's last product): the same accumulators leave as fp64 rows scale * C32
// of the column-interleaved HZ (row stride ldc) that gemmh_zrm_kernel writes, instead of float chunk pieces;
// everything before the epilogue is the same code.
namespace {
constexpr int SP_GT = 128, SP_KS = 16, SP_IMG = SP_GT * 16;   // bytes
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
template <int NBUF, int PER>
DFM_DEV void split_ring_wait(int s, int nst) {   // ring_wait at PER DMA instructions per wave and stage
  static_assert(NBUF == 3 || NBUF == 4, "ring depth");
  if (NBUF == 4 && nst - 1 - s >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PER) : "memory");
  else if (nst - 1 - s >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}
}  // namespace

// TERMS = 3 (the warm filter's split products two or more short of its last, dfm_fact_plan.h note (7); float chunks
// only): the pairs (m,h) (h,m) (h,h) on planes h and m alone.  A stage holds only the images of planes 0 and 1 of both
// operands — 8 images, 16 KB, four DMA instructions per wave — and gives 8 fragment reads per 12 MFMAs.  Hs and Zs
// are the six-term form's: plane l's pieces, a third of every k-stage of Hs and the last 32 pz bytes of every Zs
// chunk, are never addressed, so whatever they hold (nothing, where the pass in front wrote two planes) is unread.
// The ring is NBUF deep at WGS workgroups per CU; the library's instance is kSplit3Nbuf / kSplit3Wgs (tools/
// gemm_bench.hip times both candidates, profiles/r21_c3_ab.txt).  The TERMS = 6 instances are what they were.
template <bool ROWS64, int TERMS = 6, int NBUF = 3, int WGS = 2>
__global__ __launch_bounds__(256, WGS) void gemmh_zrm_split_kernel(const char *__restrict__ Hs, int mrows,
                                                                  const char *__restrict__ Zs, int pz, int64_t zrs,
                                                                  std::conditional_t<ROWS64, double, float> *__restrict__ C,
                                                                  int M, int Nc, int K, int nrb, int ncb, int64_t ldc,
                                                                  double scale) {
  static_assert(TERMS == 6 || (TERMS == 3 && !ROWS64), "three terms leave as float chunks only");
  constexpr int NPL = TERMS == 6 ? 3 : 2;            // planes staged per operand
  constexpr int OPB = 2 * NPL * SP_IMG;              // one operand's images of a stage (bytes)
  constexpr int SP_STAGE = 2 * OPB;
  __shared__ __attribute__((aligned(16))) char lds[NBUF * SP_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int bid = blockIdx.x, xcd = bid & 7, j = bid >> 3;
  const int rb = j % nrb, cb = (j / nrb) * 8 + xcd;
  if (cb >= ncb) return;
  const int abase = rb * SP_GT, bbase = cb * SP_GT;
  const int nst = (K + SP_KS - 1) / SP_KS;
  // The stage's 8 NPL DMA instructions, (operand, image q = 2 pi + kh, row half):
  // wave w issues numbers NPL w .. NPL w + NPL - 1 of each operand.  Rows past M are
  // zero in Hs (mrows = hsplit_rows(M) rows), columns past Nc read column
  // Nc - 1 (finite data, discarded outputs).
  const char *pa[NPL], *pb[NPL];
  int lo[NPL];
#pragma unroll
  for (int u = 0; u < NPL; ++u) {
    const int n = NPL * wave + u, q = n >> 1, half = n & 1;
    lo[u] = (q * SP_GT + 64 * half) * 16;
    pa[u] = Hs + ((int64_t)q * mrows + abase + 64 * half + lane) * 16;
    const int xc = min(bbase + 64 * half + lane, Nc - 1);
    const int rep = xc / pz, cc = xc - rep * pz;
    pb[u] = Zs + (int64_t)rep * zrs * 8 + ((int64_t)q * pz + cc) * 16;
  }
  const int64_t astep = (int64_t)6 * mrows * 16, bstep = (int64_t)96 * pz;   // (the layouts' k-stage, three planes)
  auto issue = [&](int s) {
    char *la = lds + (s % NBUF) * SP_STAGE, *lb = la + OPB;
#pragma unroll
    for (int u = 0; u < NPL; ++u) {
      __builtin_amdgcn_global_load_lds((gbl_void_t *)pa[u], (lds_void_t *)(la + lo[u]), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gbl_void_t *)pb[u], (lds_void_t *)(lb + lo[u]), 16, 0, 0);
      pa[u] += astep; pb[u] += bstep;
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[ti][tj][v] = 0.0f;
  // fragment offsets (bytes) inside plane 0's images: row r32 of tile t, k half hh
  const int r32 = lane & 31, hh = lane >> 5;
  int fa[2], fb[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    fa[t] = (hh * SP_GT + wr * 64 + 32 * t + r32) * 16;
    fb[t] = OPB + (hh * SP_GT + wc * 64 + 32 * t + r32) * 16;
  }
  for (int s = 0; s < NBUF - 1 && s < nst; ++s) issue(s);
  for (int s = 0; s < nst; ++s) {
    split_ring_wait<NBUF, 2 * NPL>(s, nst);
    if (s + NBUF - 1 < nst) issue(s + NBUF - 1);
    const char *ls = lds + (s % NBUF) * SP_STAGE;
    bf16x8 af[2][NPL], bf[2][NPL];   // [tile][plane]
#pragma unroll
    for (int pi = NPL - 1; pi >= 0; --pi)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        af[t][pi] = *reinterpret_cast<const bf16x8 *>(ls + fa[t] + 2 * pi * SP_IMG);
        bf[t][pi] = *reinterpret_cast<const bf16x8 *>(ls + fb[t] + 2 * pi * SP_IMG);
      }
    // (H plane, Z plane), small terms first
    constexpr int TA6[6] = {2, 0, 1, 1, 0, 0}, TB6[6] = {0, 2, 1, 0, 1, 0}, TA3[3] = {1, 0, 0}, TB3[3] = {0, 1, 0};
#pragma unroll
    for (int e = 0; e < TERMS; ++e) {
      const int pa_ = TERMS == 6 ? TA6[e] : TA3[e % 3], pb_ = TERMS == 6 ? TB6[e] : TB3[e % 3];
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
          acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ti][pa_], bf[tj][pb_], acc[ti][tj], 0, 0, 0);
    }
  }
  // accumulator register v of lane l: row 8 (v >> 2) + 4 (l >> 5) + (v & 3), column l & 31
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
    const int x = bbase + wc * 64 + 32 * tj + r32;
    if (x >= Nc) continue;
    if constexpr (ROWS64) {
      // hmax C32 as fp64 rows of HZ: a half-wave's 32 lanes write 32 consecutive columns of one row (256 B).  HZ
      // has exactly M rows and no chunk pad rows, so every element has its own row test.
      double *cp = C + x;
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int row = abase + wr * 64 + 32 * ti + 8 * (v >> 2) + 4 * hh + (v & 3);
          if (row < M) cp[(int64_t)row * ldc] = scale * (double)acc[ti][tj][v];
        }
    } else {
      const int rep = x / pz, cc = x - rep * pz;
      float *cp = C + (int64_t)rep * zrs + 16 * cc;
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int row = abase + wr * 64 + 32 * ti + 8 * g + 4 * hh;
          if (row < M)   // (rows row .. row + 3 stay inside the chunk: its pad rows take discarded values)
            *reinterpret_cast<f32x4 *>(cp + (int64_t)(row >> 4) * (16 * pz) + (row & 15)) =
                f32x4{acc[ti][tj][4 * g], acc[ti][tj][4 * g + 1], acc[ti][tj][4 * g + 2], acc[ti][tj][4 * g + 3]};
        }
    }
  }
}
// the three-term instance the library launches: ring depth and workgroups per CU
constexpr int kSplit3Nbuf = 3, kSplit3Wgs = 3;

// Hs (hsplit_bytes(M), launch_fact_hsplit) times the split Z of nb = Nc / pz replicates (dfm_internal.h: Zs; zrs =
// round_up(M, 16) pz, the fp64 Z's replicate stride): one checked launcher for both epilogues of
// gemmh_zrm_split_kernel (ldc and scale are the fp64 rows' alone) ...
template <bool ROWS64, int TERMS, int NBUF, int WGS, class CT>
static hipError_t launch_split(const void *Hs, const void *Zs, int pz, int64_t zrs, CT *C, int64_t ldc, double scale,
                               int M, int Nc, int K, hipStream_t st) {
  const int64_t kpad = (K + SP_KS - 1) / SP_KS * SP_KS;
  if (!Hs || !Zs || !C || M < 1 || pz < 1 || Nc < pz || Nc % pz || M != K || zrs < kpad * pz || (zrs & 3) ||
      (ROWS64 && ldc < Nc))
    return hipErrorInvalidValue;
  const int nrb = (M + SP_GT - 1) / SP_GT, ncb = (Nc + SP_GT - 1) / SP_GT;
  const int ncb8 = (ncb + 7) / 8 * 8;
  hipLaunchKernelGGL((gemmh_zrm_split_kernel<ROWS64, TERMS, NBUF, WGS>), dim3(nrb * ncb8), dim3(256), 0, st,
                     (const char *)Hs, hsplit_rows(M), (const char *)Zs, pz, zrs, C, M, Nc, K, nrb, ncb, ldc, scale);
  return hipGetLastError();
}
// ... -> C32 in launch_gemm_zrm_f32's layout, from terms = 6 plane pairs or from the 3 of planes h and m alone
hipError_t launch_gemm_zrm_split(const void *Hs, const void *Zs, int pz, int64_t zrs, float *C, int M, int Nc, int K,
                                 int terms, hipStream_t st) {
  if (terms == 6) return launch_split<false, 6, 3, 2>(Hs, Zs, pz, zrs, C, 0, 1.0, M, Nc, K, st);
  if (terms == 3) return launch_split<false, 3, kSplit3Nbuf, kSplit3Wgs>(Hs, Zs, pz, zrs, C, 0, 1.0, M, Nc, K, st);
  return hipErrorInvalidValue;
}
// ... or delivered as fp64 rows, C (M x Nc, row stride ldc >= Nc) = scale C32 in launch_gemm_zrm's column-interleaved
// layout: the last product of a warm filter (scale = hmax), whose rows the last Horner step gathers as it gathers an
// fp64 product's.  Nothing outside rows < M and columns < Nc is written.
hipError_t launch_gemm_zrm_split_rows(const void *Hs, const void *Zs, int pz, int64_t zrs, double *C, int64_t ldc,
                                      double scale, int M, int Nc, int K, hipStream_t st) {
  return launch_split<true, 6, 3, 2>(Hs, Zs, pz, zrs, C, ldc, scale, M, Nc, K, st);
}

// ---------------------------------------------------------------------------
// Loadings GEMM of the factored bootstrap:
//   L*[rep][n][j] = ( [E' | L] [ZF ; M1] )[n][rep rp + j] / T
// (src/DynamicFactorModel.jl:90 for every replicate: L* = X*' F* / T with
// X*' F* = E' P' D F* + L (F'F*)): the r x r blocks M1 = F'F* sit under ZF
// as r extra k-rows and L' under E, so the whole finish is K = T + r MFMA
// depth (+1.6 %) and the epilogue a plain scaled store.  A^T operand
// [E; L'] (Kpad x lda, Kpad = round_up(T + r, 16), zero rows past T + r).
// B operand replicate-major: replicate rep's [ZF; M1; 0] is one contiguous
// Kpad x rp block (rp = r rounded up to even, column r zero when r is odd),
// so boot_zf writes whole lines; column x of the GEMM is (rep, j) =
// (x / rp, x % rp), and a lane's 16-B DMA pair (x, x + 1), x even, never
// straddles two replicates.  Both operands staged by LDS-DMA into [k][a]
// images (4-deep ring).  Grid: the row blocks (64 variables)
// are spread over the XCDs — XCD x owns row blocks x, x+8, ... whose E slabs
// (64 x T x 8 B each) stay in its L2 — and every XCD walks the column blocks
// in the same order, so a ZF tile is fetched from HBM once and served to the
// other XCDs from the Infinity Cache.
template <int NBUF, int MINB>
__global__ __launch_bounds__(256, MINB) void gemm_loadings_kernel(const double *__restrict__ A, int64_t lda,
                                                                  const double *__restrict__ B, int Kp, int rp, int M,
                                                                  int Nc, int K, int nrb, int ncb, int r, double invT,
                                                                  double *__restrict__ Lout, int nrep) {
  __shared__ __attribute__((aligned(16))) double lds[NBUF * G2_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int nrb8 = (nrb + 7) / 8;
  const int bid = blockIdx.x, xcd = bid & 7, j = bid >> 3;
  const int rb = (j % nrb8) * 8 + xcd, cb = j / nrb8;
  if (rb >= nrb || cb >= ncb) return;
  const int abase = rb * GT, bbase = cb * GT;
  double acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[i][q] = 0.0;
  const int fi = lane & 3, fkc = 4 * (lane >> 4) + ((lane >> 2) & 3);
  const int nst = (K + G2_KS - 1) / G2_KS;
  // running DMA pointers (both operands hold zero k-rows up to
  // round_up(K, 16), so the last stage needs no clamp)
  const double *pa[2], *pb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int kc = 2 * (2 * wave + h) + (lane >> 5);
    const int sw = (2 * (lane & 31)) ^ ((kc & 7) << 2);
    pa[h] = A + (int64_t)kc * lda + min(abase + sw, (int)lda - 2);
    const int x = min(bbase + sw, Nc - 2), rep = x / rp;   // past Nc: finite, discarded
    pb[h] = B + ((int64_t)rep * Kp + kc) * rp + (x - rep * rp);
  }
  const int64_t astep = (int64_t)G2_KS * lda, bstep = (int64_t)G2_KS * rp;
  auto issue = [&](int s) {
    double *la = lds + (s % NBUF) * G2_STAGE, *lb = la + GT * G2_KS;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = 2 * wave + h;
      __builtin_amdgcn_global_load_lds((gbl_void_t *)pa[h], (lds_void_t *)(la + c * 128), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gbl_void_t *)pb[h], (lds_void_t *)(lb + c * 128), 16, 0, 0);
      pa[h] += astep;
      pb[h] += bstep;
    }
  };
  for (int s = 0; s < NBUF - 1 && s < nst; ++s) issue(s);
  for (int s = 0; s < nst; ++s) {
    ring_wait<NBUF>(s, nst);
    if (s + NBUF - 1 < nst) issue(s + NBUF - 1);
    const double *la = lds + (s % NBUF) * G2_STAGE, *lb = la + GT * G2_KS;
    double af[8], bf[8];
#pragma unroll
    for (int f = 0; f < 8; ++f) {
      af[f] = la[g2_offB(wr * 32 + 4 * f + fi, fkc)];
      bf[f] = lb[g2_offB(wc * 32 + 4 * f + fi, fkc)];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[i][q] = mfma4(af[i], bf[q], acc[i][q]);
  }
  // (accumulators, k step and epilogue written out: on dfm_tile.h's this
  // kernel measured 3.6 % slower per launch, profiles/r09_tile_ab.txt section 4)
  const int b1 = (lane >> 2) & 1, b2 = (lane >> 3) & 1, blk = (lane >> 2) & 3;
  const int oi = lane >> 4, oj = lane & 3;
#pragma unroll
  for (int fa = 0; fa < 8; ++fa)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const double a0 = acc[fa][4 * q], a1 = acc[fa][4 * q + 1], a2 = acc[fa][4 * q + 2],
                   a3 = acc[fa][4 * q + 3];
      double k01 = (b1 ? a1 : a0) + __shfl_xor(b1 ? a0 : a1, 4);
      double k23 = (b1 ? a3 : a2) + __shfl_xor(b1 ? a2 : a3, 4);
      const double v = (b2 ? k23 : k01) + __shfl_xor(b2 ? k01 : k23, 8);
      const int n = abase + wr * 32 + 4 * fa + oi;
      const int col = bbase + wc * 32 + 16 * q + 4 * blk + oj;
      const int rep = col / rp, jj = col - rep * rp;
      if (n < M && rep < nrep && jj < r) Lout[((int64_t)rep * M + n) * r + jj] = v * invT;
    }
}

// ZF: nrep replicate blocks of Kp x rp (see gemm_loadings_kernel); K = T + r.
hipError_t launch_gemm_loadings(const double *Eaug, int64_t lda, const double *ZF, int Kp, int rp, int N, int nrep,
                                int K, int r, double invT, double *Lout, hipStream_t st) {
  const int Nc = nrep * rp;
  const int nrb = (N + GT - 1) / GT, ncb = (Nc + GT - 1) / GT;
  const int nrb8 = (nrb + 7) / 8;
  // (the 3-deep ring at 3 workgroups per CU measured 20 % slower here, with
  // running pointers still 23 % slower: 4-deep at 2 per CU stays)
  hipLaunchKernelGGL((gemm_loadings_kernel<4, 2>), dim3(8 * nrb8 * ncb), dim3(256), 0, st, Eaug, lda, ZF, Kp, rp, N,
                     Nc, K, nrb, ncb, r, invT, Lout, nrep);
  return hipGetLastError();
}

// resident gram_dma_kernel workgroups on the chip for an m-row Gram
int gram_dma_slots(int m) { return (gemm_ring3(m) ? 3 : 2) * 256; }

// ---------------------------------------------------------------------------
// gram_dma_kernel: G = X X' of a plain row-major panel (m x K, ld % 16 == 0,
// zero columns K..ld-1) — the N > T Gram of principal_components
// (src/DynamicFactorModel.jl:87 `x*x'`) when no resample gather is fused: the
// base fit's H = E E' and the expanding windows' one prefix Gram
// (src/utils.jl:59-65 through the prefix identity).  Both
// operands are row blocks of X in [a][k] images, staged by LDS-DMA through a
// 4-deep ring (3-deep at 3 workgroups per CU for the large Grams:
// gemm_ring3); only lower-triangular 64 x 64 tiles run, the epilogue writes
// both halves.  Split-K over blockIdx-derived z (partial
// images summed in fixed order by the caller).  XCD-aware order: the work
// list (z-major, then column tile J, then row tile I >= J) is cut into 8
// contiguous spans, XCD x taking span x, so the workgroups resident on one XCD
// share one k-range and a few column blocks (operands re-read from its L2).

template <int NBUF, int MINB>
__global__ __launch_bounds__(256, MINB) void gram_dma_kernel(const double *__restrict__ X, int64_t ld, int m, int K,
                                                             int nt, int tiles, int items, int span, int ksteps,
                                                             double *__restrict__ G, int64_t ldg, int64_t strideZ,
                                                             double alpha) {
  __shared__ __attribute__((aligned(16))) double lds[NBUF * G2_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int item = (blockIdx.x & 7) * span + (blockIdx.x >> 3);
  if (item >= items) return;
  const int z = item / tiles;
  int u = item - z * tiles, J = 0;
  while (u >= nt - J) { u -= nt - J; ++J; }
  const int I = J + u;
  const int abase = I * GT, bbase = J * GT;
  double acc[8][8];
  tile_zero(acc);
  const int s0 = z * ksteps;
  const int nst = min((K + G2_KS - 1) / G2_KS, s0 + ksteps) - s0;   // the k tail reads ld's zero padding
  const int kbase = s0 * G2_KS;
  // per-lane DMA sources: A chunk rows of block I, B chunk rows of block J,
  // as running pointers (one 64-bit add per operand and stage)
  const double *pa[2], *pb[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = 2 * wave + h;
    const int a = 8 * c + (lane >> 3);
    const int ka = (2 * (lane & 7)) ^ (((a >> 1) & 1) << 3);
    pa[h] = X + (int64_t)min(abase + a, m - 1) * ld + ka + kbase;   // rows past m: finite, discarded outputs
    pb[h] = X + (int64_t)min(bbase + a, m - 1) * ld + ka + kbase;
  }
  const int c0 = (2 * wave) * 128, c1 = c0 + 128;
  auto issue = [&](int s) {
    double *la = lds + (s % NBUF) * G2_STAGE, *lb = la + GT * G2_KS;
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pa[0], (lds_void_t *)(la + c0), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pb[0], (lds_void_t *)(lb + c0), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pa[1], (lds_void_t *)(la + c1), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gbl_void_t *)pb[1], (lds_void_t *)(lb + c1), 16, 0, 0);
    pa[0] += G2_KS; pa[1] += G2_KS; pb[0] += G2_KS; pb[1] += G2_KS;
  };
  for (int s = 0; s < NBUF - 1 && s < nst; ++s) issue(s);
  for (int s = 0; s < nst; ++s) {
    ring_wait<NBUF>(s, nst);
    if (s + NBUF - 1 < nst) issue(s + NBUF - 1);
    const double *la = lds + (s % NBUF) * G2_STAGE;
    tile_step<g2_offA, g2_offA>(acc, la, la + GT * G2_KS, wr, wc, lane);
  }
  const bool diag = I == J;
  double *Gz = G + (int64_t)z * strideZ;
  tile_epilogue(acc, abase, bbase, wr, wc, lane, [&](int row, int col, double f) {
    const double v = f * alpha;   // alpha = 1: exact
    if (row < m && col < m) {
      Gz[(int64_t)row * ldg + col] = v;
      if (!diag) Gz[(int64_t)col * ldg + row] = v;
    }
  });
}

// One launch of gram_dma_kernel over split-K partial images: S images of
// strideZ elements at G (S == 1: G is the output itself).
hipError_t launch_gram_dma(const double *X, int64_t ld, int m, int K, int S, int ksteps, double *G, int64_t ldg,
                           int64_t strideZ, hipStream_t st, double alpha) {
  const int nt = (m + GT - 1) / GT, tiles = nt * (nt + 1) / 2, items = tiles * S;
  const int span = (items + 7) / 8;
  // 3-deep ring at 3 workgroups per CU for the large Grams (more resident
  // waves beat a deeper ring there: tools/gemm_bench.hip, M = 2000)
  if (gemm_ring3(m))
    hipLaunchKernelGGL((gram_dma_kernel<3, 3>), dim3(8 * span), dim3(256), 0, st, X, ld, m, K, nt, tiles, items, span,
                       ksteps, G, ldg, strideZ, alpha);
  else
    hipLaunchKernelGGL((gram_dma_kernel<4, 2>), dim3(8 * span), dim3(256), 0, st, X, ld, m, K, nt, tiles, items, span,
                       ksteps, G, ldg, strideZ, alpha);
  return hipGetLastError();
}

}  // namespace dfm
