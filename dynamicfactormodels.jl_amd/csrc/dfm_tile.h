// dfm_tile.h — the 64 x 64 fp64 workgroup tile on v_mfma_f64_4x4x4_4b, shared
// by gemmh_kernel, gemmh_zrm_kernel and gram_dma_kernel (dfm_gemm.hip) and by
// tools/gemm_bench.hip.  gemm_loadings_kernel and dfm_gram.hip's register-
// staged gram_kernel compute the same tile with their own copies, which
// measured faster there (profiles/r09_tile_ab.txt).  256 threads: wave w owns the 32 x 32 sub-tile
// (wr, wc) = (w >> 1, w & 1) as 8 x 8 fragments of 4 x 4.  A 16-deep k step
// is 64 MFMA per wave; the instruction's four blocks split the 16 k four
// ways and are summed once, in the epilogue.  A kernel brings its own
// staging (what fills the two 64 x 16 LDS images and how they are laid out)
// and its own store; the accumulators, the k step and the epilogue are here,
// so every kernel sums a tile's products in the same order.
#pragma once
#include "dfm_common.h"

namespace dfm {

DFM_DEV void tile_zero(double (&acc)[8][8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[i][q] = 0.0;
}

// This lane's 8 + 8 operand fragments of one 16-deep stage.  la / lb: the
// stage's two LDS images; OFFA(a, kc) / OFFB(a, kc): element offset of row
// (column) a of the tile at k index kc in each.
template <int (*OFFA)(int, int), int (*OFFB)(int, int)>
DFM_DEV void tile_frags(const double *la, const double *lb, int wr, int wc, int lane, double (&af)[8],
                        double (&bf)[8]) {
  const int fi = lane & 3, fkc = 4 * (lane >> 4) + ((lane >> 2) & 3);
#pragma unroll
  for (int f = 0; f < 8; ++f) {
    af[f] = la[OFFA(wr * 32 + 4 * f + fi, fkc)];
    bf[f] = lb[OFFB(wc * 32 + 4 * f + fi, fkc)];
  }
}

DFM_DEV void tile_mfma(double (&acc)[8][8], const double (&af)[8], const double (&bf)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[i][q] = mfma4(af[i], bf[q], acc[i][q]);
}

// One k step: fragments, then the 64 MFMA.
template <int (*OFFA)(int, int), int (*OFFB)(int, int)>
DFM_DEV void tile_step(double (&acc)[8][8], const double *la, const double *lb, int wr, int wc, int lane) {
  double af[8], bf[8];
  tile_frags<OFFA, OFFB>(la, lb, wr, wc, lane, af, bf);
  tile_mfma(acc, af, bf);
}

// Epilogue: fold the four blocks (mm4_fold) and hand this lane's 16 results
// to store(row, col, v); abase / bbase: the tile's first row / column.  A
// store that depends on a wave-uniform mode is chosen outside: one call per
// mode.
template <class Store>
DFM_DEV void tile_epilogue(const double (&acc)[8][8], int abase, int bbase, int wr, int wc, int lane, Store store) {
  const int blk = (lane >> 2) & 3, oi = lane >> 4, oj = lane & 3;
#pragma unroll
  for (int fa = 0; fa < 8; ++fa)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const double v = mm4_fold(acc[fa][4 * q], acc[fa][4 * q + 1], acc[fa][4 * q + 2], acc[fa][4 * q + 3], lane);
      store(abase + wr * 32 + 4 * fa + oi, bbase + wc * 32 + 16 * q + 4 * blk + oj, v);
    }
}

// The LDS-DMA ring's wait before stage s of nst is read.  Every wave issues 4
// DMAs (global_load_lds_dwordx4) per stage, NBUF - 1 stages ahead: it waits
// only for its own DMAs of stage s (counted vmcnt, 0 only when no later stage
// is in flight) and its LDS reads, then ONE raw s_barrier orders them for
// every reader and retires the ring slot (s - 1) % NBUF, read one iteration
// earlier, which the caller refills right after.
template <int NBUF>
DFM_DEV void ring_wait(int s, int nst) {
  static_assert(NBUF == 3 || NBUF == 4, "ring depth");
  const int ahead = min(NBUF - 2, nst - 1 - s);   // later stages already issued
  if (ahead >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if (ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

}  // namespace dfm
