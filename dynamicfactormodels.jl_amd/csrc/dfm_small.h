// dfm_small.h — workgroup-level small dense linear algebra in LDS (n <= 64).
// Every thread of the block must call these (they contain __syncthreads()).
#pragma once
#include "dfm_common.h"

namespace dfm {

// Inverse of an SPD matrix A (n x n, LDS, row stride S) via Cholesky:
// A = L L', Ai = L^-T L^-1.  Lw, Tw: LDS scratch n x S.  *bad |= 1 on a
// non-positive pivot (the reference's inv() would return Inf/garbage).
DFM_DEV void block_spd_inverse(const double *A, double *Ai, double *Lw, double *Tw, int n, int S,
                               int *bad) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int e = tid; e < n * S; e += nt) Lw[e] = 0.0;
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    if (tid == 0) {
      double s = A[j * S + j];
      for (int p = 0; p < j; ++p) s -= Lw[j * S + p] * Lw[j * S + p];
      if (!(s > 0.0)) { *bad = 1; s = 1.0; }
      Lw[j * S + j] = sqrt(s);
    }
    __syncthreads();
    for (int i = j + 1 + tid; i < n; i += nt) {
      double s = A[i * S + j];
      for (int p = 0; p < j; ++p) s -= Lw[i * S + p] * Lw[j * S + p];
      Lw[i * S + j] = s / Lw[j * S + j];
    }
    __syncthreads();
  }
  for (int c = tid; c < n; c += nt)
    for (int i = 0; i < n; ++i) {
      double s = (i == c) ? 1.0 : 0.0;
      for (int p = c; p < i; ++p) s -= Lw[i * S + p] * Tw[p * S + c];
      Tw[i * S + c] = i < c ? 0.0 : s / Lw[i * S + i];
    }
  __syncthreads();
  for (int e = tid; e < n * n; e += nt) {
    const int a = e / n, c = e % n;
    double s = 0.0;
    for (int p = (a > c ? a : c); p < n; ++p) s = fma(Tw[p * S + a], Tw[p * S + c], s);
    Ai[a * S + c] = s;
  }
  __syncthreads();
}

// Inverse of a general matrix by Gauss-Jordan elimination with partial
// pivoting (the first largest |entry| of the column).  W: the augmented
// [A | I] (n x 2n, LDS, row stride S >= 2n); on return its right half holds
// A^-1 and *logdet = log|det A|.  colj (n), rowj (2n), logdet, piv: LDS.
// *bad |= 2 on a zero or non-finite pivot (the elimination then goes on with
// a unit pivot: the flag, not the result, reports it).
DFM_DEV void block_gj_inverse(double *W, int n, int S, double *colj, double *rowj, double *logdet, int *piv,
                              int *bad) {
  const int tid = threadIdx.x, nt = blockDim.x, n2 = 2 * n;
  if (tid == 0) *logdet = 0.0;
  for (int j = 0; j < n; ++j) {
    if (tid == 0) {
      int p = j;
      double best = fabs(W[j * S + j]);
      for (int i = j + 1; i < n; ++i) {
        const double v = fabs(W[i * S + j]);
        if (v > best) { best = v; p = i; }
      }
      *piv = p;
      if (!(best > 0.0) || isinf(best)) *bad |= 2;
      else *logdet += log(best);
    }
    __syncthreads();
    const int p = *piv;
    if (p != j)
      for (int c = tid; c < n2; c += nt) {
        const double a = W[j * S + c];
        W[j * S + c] = W[p * S + c];
        W[p * S + c] = a;
      }
    __syncthreads();
    double pv = W[j * S + j];
    if (!(fabs(pv) > 0.0) || isinf(pv)) pv = 1.0;
    for (int c = tid; c < n2 + n; c += nt) {
      if (c < n2) rowj[c] = W[j * S + c] / pv;
      else colj[c - n2] = W[(c - n2) * S + j];
    }
    __syncthreads();
    for (int e = tid; e < n * n2; e += nt) {
      const int i = e / n2, c = e % n2;
      W[i * S + c] = (i == j) ? rowj[c] : W[i * S + c] - colj[i] * rowj[c];
    }
    __syncthreads();
  }
}

// block_spd_inverse on ONE wave (lanes, no barriers: every LDS write is
// waited for before the lanes that read it issue their reads) — the same
// operations in the same order, so several small inverses run side by side
// on different waves of a workgroup.  A, Ai, Lw, Tw MUST be LDS (__shared__)
// memory: they are cast to the LDS address space here, so every access is a
// ds_* instruction and `s_waitcnt lgkmcnt(0)` is the complete wait (a flat or
// global pointer would need vmcnt too — and is undefined after the cast).
// `bad` (LDS) is raised with an atomic OR: several waves may report at once.
typedef __attribute__((address_space(3))) double lds_double;
DFM_DEV void wave_spd_inverse(const double *A_, double *Ai_, double *Lw_, double *Tw_, int n, int S, int *bad) {
  const lds_double *A = (const lds_double *)A_;
  lds_double *Ai = (lds_double *)Ai_, *Lw = (lds_double *)Lw_, *Tw = (lds_double *)Tw_;
  const int lane = threadIdx.x & 63;
  auto sync = [] { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };
  for (int e = lane; e < n * S; e += 64) Lw[e] = 0.0;
  sync();
  for (int j = 0; j < n; ++j) {
    if (lane == 0) {
      double s = A[j * S + j];
      for (int p = 0; p < j; ++p) s -= Lw[j * S + p] * Lw[j * S + p];
      if (!(s > 0.0)) { atomicOr(bad, 1); s = 1.0; }
      Lw[j * S + j] = sqrt(s);
    }
    sync();
    for (int i = j + 1 + lane; i < n; i += 64) {
      double s = A[i * S + j];
      for (int p = 0; p < j; ++p) s -= Lw[i * S + p] * Lw[j * S + p];
      Lw[i * S + j] = s / Lw[j * S + j];
    }
    sync();
  }
  for (int c = lane; c < n; c += 64)
    for (int i = 0; i < n; ++i) {
      double s = (i == c) ? 1.0 : 0.0;
      for (int p = c; p < i; ++p) s -= Lw[i * S + p] * Tw[p * S + c];
      Tw[i * S + c] = i < c ? 0.0 : s / Lw[i * S + i];
    }
  sync();
  for (int e = lane; e < n * n; e += 64) {
    const int a = e / n, c = e % n;
    double s = 0.0;
    for (int p = (a > c ? a : c); p < n; ++p) s = fma(Tw[p * S + a], Tw[p * S + c], s);
    Ai[a * S + c] = s;
  }
  sync();
}

}  // namespace dfm
