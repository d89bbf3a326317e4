// dfm_eig.hip — K2: batched top-k symmetric eigensolver (block subspace
// iteration with Rayleigh–Ritz), replacing the full-spectrum LAPACK `eig` of
// principal_components (src/DynamicFactorModel.jl:78-79, :87-88) whose
// trailing columns the reference never consumes (only [:, 1:r], :33, :131).
//
// Per replicate b (G_b is m x m, row-major, ldg):
//   gq    : Y = G Q  (v_mfma_f64_4x4x4_4b, 64 rows / workgroup) + per-row-block
//           partials of Q'Y, Y'Y, Q'Q; first checks the previous iteration's
//           explicit residuals and retires converged replicates.
//   small : one wave per replicate.  Q'Q = LL' (the basis is re-orthonormalised
//           implicitly: CholQR folded into the Rayleigh–Ritz step), H~ =
//           L^-1 (Q'Y) L^-T, parallel cyclic Jacobi on p x p, A = L^-T S,
//           Z'Z = A'(Y'Y)A = L2 L2', Bm = A L2^-T.
//   apply : U = Q A (Ritz vectors), Q <- Y Bm (next orthonormal basis),
//           W = Y A - U diag(theta) -> per-block residual partials.
//   final : sign canonicalisation (largest-|.| entry positive, first index).
// Converged when ||G u_j - theta_j u_j|| <= tol * |theta_1| for j < k.
// Deterministic: fixed-order reductions only, no float atomics.
#include "dfm_eig.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace dfm {

#define SMALL_STAMP(i) do { if (w.dbg && rep == 0 && lane == 0) w.dbg[i] = (long long)wall_clock64(); } while (0)
constexpr int SMALL_CHOL1_DONE = 0x100;   // small_rr: R4 already holds chol(Q'Q)^-1 (eig_fused forms it during Y = G Q)
constexpr int SMALL_STAGE_A = 0x200;      // small_rr: stop once A (R2), theta and Z'Z (R3) are formed
constexpr int SMALL_STAGE_B = 0x400;      // small_rr: only chol(Z'Z) and Bm (eig_fused: beside the U pass)
constexpr int SMALL_CHOL_OWN = 0x800;     // small_rr: chol(Q'Q)'s dead pivots by the column's own diagonal entry (eig_run; the
                                          // factored solver's launch of eig_small_kernel keeps the largest-entry rule)

// Upper end b of the Chebyshev filter's damped interval [0, b]: theta_p, the
// block's last Ritz value, but no higher than 0.95 theta_k.  |T_d| = 1 at b,
// at b / 2 and at 0, so with theta_k at b (theta_k tied with every guard
// column, or k == p) the filter amplifies the wanted vector no more than the
// whole unwanted spectrum and only the Rayleigh-Ritz step works on it: a tie
// of p - k + 3 values across the k | k+1 boundary took 165 to more than 400
// steps.  At 0.95 theta_k the last wanted vector gains T_2(2 / 0.95 - 1) =
// 1.44 per degree-2 filter over everything in [0, b]; what lies between b and
// theta_k grows by less than theta_k does.  theta_k <= 0: theta_p (b <= 0,
// the callers' plain power steps).
DFM_DEV double filter_top(const double *th, int k, int p) {
  const double b = th[p - 1], tk = th[k - 1];
  return tk > 0.0 ? fmin(b, 0.95 * tk) : b;
}
// A Ritz vector u = Q A e is a unit vector when chol(Q'Q) is sound.  Where Q'Q
// is numerically singular (every filtered column of an exact-rank G lies in
// its range) the factor is noise or has dead rows, and a column of U comes
// out at norm ~ 0 — exactly 0 for a dead row, with theta = 0.  Such a pair has
// a residual |G u - theta u| near 0 whatever theta is, and passed: zero
// vectors for wanted null directions, or a Ritz value above lambda_1.  A pair
// whose |u|^2 (us) is not within [1/2, 2] is not judged: residual infinite; its
// column of Z is dead in chol(Z'Z) and is re-seeded by the apply step.
DFM_DEV double judged_residual(double rs, double us) { return us > 0.5 && us < 2.0 ? rs : INFINITY; }

// ----------------------------------------------------------------- init
template <int P>
__global__ void eig_init_kernel(double *__restrict__ Q, int m, int p, const double *__restrict__ warm,
                                int kw, int *__restrict__ done, uint64_t seed, int64_t rep0, int ps) {
  const int rep = blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)m * ps) return;
  const int row = (int)(e / ps), c = (int)(e % ps);
  double v = 0.0;
  if (c < kw) v = warm[(int64_t)row * kw + c];
  else if (c < p) v = hash_unit(seed, row, c);   // same start for every replicate: call/batch/shard-invariant
  Q[(int64_t)rep * m * ps + e] = v;
  if (e == 0) done[rep] = 0;
}

__global__ void eig_trace_kernel(const double *__restrict__ G, int64_t ldg, int64_t strideG, int m,
                                 double *__restrict__ trace) {
  const int rep = blockIdx.x, lane = threadIdx.x;
  const double *g = G + (int64_t)rep * strideG;
  double s = 0.0;
  for (int i = lane; i < m; i += 64) s += g[(int64_t)i * ldg + i];
  s = wave_sum(s);
  if (lane == 0) trace[rep] = s;
}

// Convergence test of iteration it-1's Ritz pairs (explicit residual partials
// written by eig_apply).  Every workgroup of a replicate evaluates it on the
// same data (so they agree); row block 0 records the verdict.  Called by one
// whole wave: lane (j, r) loads one partial, the sum over r is a fixed-order
// shuffle tree — no serial chain of dependent global loads.
// tail: the small record's tail (theta[P], dead[P], residual history 2 x P);
// rp: the nrb row-block residual partials (P apart); d: the replicate's done flag.
template <int P>
DFM_DEV int check_converged(EigWork &w, double *tail, const double *rp, const double *up, double tr, int d, int rep, int rb,
                            int nrb, int k, int p, double tol, int it, int check_only) {
  const int lane = threadIdx.x & 63;
  if (!d && it > 0) {
    // the rule is column_verdict / energy_converged (dfm_eig.h)
    const double *th = tail;
    const double *prev = tail + 2 * P + ((it - 1) & 1) * P;
    double *next = tail + 2 * P + (it & 1) * P;
    const double th0 = fabs(th[0]);
    bool ok = true;
    if (tol < 0.0) {
      double bsum = 0.0, tsum = 0.0;
      bool okall = true, floor_ok = true;
      for (int j = lane; j < k; j += 64) {
        double rs = 0.0;
        for (int r = 0; r < nrb; ++r) rs += rp[r * P + j];
        if (up) {   // (the fused kernel folds the norm into rp itself)
          double us = 0.0;
          for (int r = 0; r < nrb; ++r) us += up[r * P + j];
          rs = judged_residual(rs, us);
        }
        const ColumnVerdict v = column_verdict(rs, j, th, th0, prev, k, p, tol, it, w.subspace);
        bsum += v.bnd;
        tsum += th[j];
        okall = okall && v.ok;
        floor_ok = floor_ok && v.floor;
        if (rb == 0) next[j] = v.res;
      }
      bsum = wave_sum(bsum);
      tsum = wave_sum(tsum);
      ok = !__any(!okall) && energy_converged(bsum, tsum, tr, tol, floor_ok);
    } else
    for (int j0 = 0; j0 < k; j0 += 64) {
      // lanes: j = j0 + lane / G, r = lane % G   with G = power of two >= nrb
      // (capped at 64: past 64 row blocks — m > 4096 — lane r also sums
      // blocks r + 64, r + 128, ... in order before the shuffle tree)
      int G = 1;
      while (G < nrb && G < 64) G <<= 1;
      const int per = 64 / G;   // residual columns handled per pass
      for (int jj = 0; jj < 64 && j0 + jj < k; jj += per) {
        const int j = j0 + jj + lane / G, r = lane % G;
        double v = 0.0, us = 0.0;   // us: |u_j|^2 by the same tree (the fused kernel folds the norm into rp itself)
        if (j < k)
          for (int rr = r; rr < nrb; rr += G) {
            v += rp[rr * P + j];
            if (up) us += up[rr * P + j];
          }
        for (int o = G / 2; o >= 1; o >>= 1) { v += __shfl_xor(v, o); us += __shfl_xor(us, o); }
        // lanes with r == 0 hold the column sums
        bool okj = true;
        if (j < k && r == 0) {
          if (up) v = judged_residual(v, us);
          const ColumnVerdict cv = column_verdict(v, j, th, th0, prev, k, p, tol, it, w.subspace);
          okj = cv.ok;
          if (rb == 0) next[j] = cv.res;
        }
        ok = ok && !__any(!okj);
      }
    }
    if (ok) {
      d = 1;
      if (rb == 0 && lane == 0) { w.done[rep] = 1; w.iters[rep] = it; }
    }
  }
  if (rb == 0 && lane == 0 && !d) {
    atomicAdd(&w.active[it], 1);
    if (check_only) w.iters[rep] = it;   // not converged: all maxit steps were taken (status 1)
  }
  return d || check_only;
}

// Partial Q'Y, Y'Y, Q'Q over one 64-row block (fixed order), LDS images sQ/sY.
template <int P, int SQ>
DFM_DEV void emit_partials(const double *sQ, const double *sY, double *pp) {
  for (int e = threadIdx.x; e < 3 * P * P; e += blockDim.x) {
    const int which = e / (P * P), a = (e / P) % P, c = e % P;
    const double *X1 = (which == 1) ? sY : sQ;
    const double *X2 = (which == 2) ? sQ : sY;
    double s = 0.0;
    for (int r = 0; r < EROWS; ++r) s = fma(X1[r * SQ + a], X2[r * SQ + c], s);
    pp[e] = s;
  }
}

// ------------------------------------------------------------------- gq
template <int P>
__global__ __launch_bounds__(256) void eig_gq_kernel(const double *__restrict__ G, int64_t ldg,
                                                     int64_t strideG, EigWork w, int m, int k,
                                                     int p, double tol, int it, int check_only) {
  constexpr int SQ = P + 4;  // padded LDS row stride (conflict-free B-fragment reads)
  __shared__ __attribute__((aligned(16))) double sQ[EROWS * SQ];
  __shared__ __attribute__((aligned(16))) double sY[EROWS * SQ];
  __shared__ int s_skip;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rep = blockIdx.y, rb = blockIdx.x, nrb = gridDim.x;
  double *small = w.small + (int64_t)rep * small_stride<P>();
  if (tid < 64) {
    const int d = check_converged<P>(w, small + 2 * P * P, w.rpart + (int64_t)rep * nrb * P, w.upart + (int64_t)rep * nrb * P, w.trace[rep], w.done[rep],
                                     rep, rb, nrb, k, p, tol, it, check_only);
    if (tid == 0) s_skip = d;
  }
  __syncthreads();
  if (s_skip) return;

  const double *Gr = G + (int64_t)rep * strideG;
  const double *Qr = w.Q + (int64_t)rep * m * P;
  const int fi = lane & 3, fkc = 4 * (lane >> 4) + ((lane >> 2) & 3);
  const int row0 = rb * EROWS + wave * 16;
  double acc[4][P / 4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < P / 4; ++b) acc[a][b] = 0.0;

  for (int kc0 = 0; kc0 < m; kc0 += EROWS) {
    for (int e = tid; e < EROWS * P; e += 256) {
      const int r = e / P, c = e % P;
      sQ[r * SQ + c] = (kc0 + r < m) ? Qr[(int64_t)(kc0 + r) * P + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < EROWS / 16; ++ks) {
      // wave-uniform: rows past m (m = 130: 3 of 12 waves) and k steps past m
      // only ever added zero products
      if (row0 >= m || kc0 + ks * 16 >= m) continue;
      const int kg = kc0 + ks * 16 + fkc;
      double af[4], bf[P / 4];
#pragma unroll
      for (int fa = 0; fa < 4; ++fa) {
        const int row = row0 + 4 * fa + fi;
        af[fa] = (row < m && kg < m) ? Gr[(int64_t)row * ldg + kg] : 0.0;
      }
#pragma unroll
      for (int fb = 0; fb < P / 4; ++fb) bf[fb] = sQ[(ks * 16 + fkc) * SQ + 4 * fb + fi];
#pragma unroll
      for (int fa = 0; fa < 4; ++fa)
#pragma unroll
        for (int fb = 0; fb < P / 4; ++fb) acc[fa][fb] = mfma4(af[fa], bf[fb], acc[fa][fb]);
    }
    __syncthreads();
  }
  // transpose-reduce, write Y (global + LDS)
  // (mm4_fold written out here and in eig_cheb_kernel: through the helper
  // these kernels' instruction streams change)
  const int b1 = (lane >> 2) & 1, b2 = (lane >> 3) & 1, blk = (lane >> 2) & 3;
  const int oi = lane >> 4, oj = lane & 3;
  double *Yr = w.Y + (int64_t)rep * m * P;
#pragma unroll
  for (int fa = 0; fa < 4; ++fa)
#pragma unroll
    for (int q = 0; q < P / 16; ++q) {
      const double a0 = acc[fa][4 * q], a1 = acc[fa][4 * q + 1], a2 = acc[fa][4 * q + 2],
                   a3 = acc[fa][4 * q + 3];
      double k01 = (b1 ? a1 : a0) + __shfl_xor(b1 ? a0 : a1, 4);
      double k23 = (b1 ? a3 : a2) + __shfl_xor(b1 ? a2 : a3, 4);
      const double v = (b2 ? k23 : k01) + __shfl_xor(b2 ? k01 : k23, 8);
      const int lr = wave * 16 + 4 * fa + oi, col = 16 * q + 4 * blk + oj;
      const int row = rb * EROWS + lr;
      sY[lr * SQ + col] = v;
      if (row < m) Yr[(int64_t)row * P + col] = v;
    }
  // Q rows of this block
  for (int e = tid; e < EROWS * P; e += 256) {
    const int r = e / P, c = e % P, row = rb * EROWS + r;
    sQ[r * SQ + c] = row < m ? Qr[(int64_t)row * P + c] : 0.0;
  }
  __syncthreads();
  // partial Q'Y, Y'Y, Q'Q over this block's rows (fixed order)
  emit_partials<P, SQ>(sQ, sY, w.part + ((int64_t)rep * nrb + rb) * 3 * P * P);
}

// One Horner step of the direct path's Chebyshev filter (the factored path's
// boot_cheb_kernel on an explicit Gram): eig_apply leaves V0 = Q Bm in w.Q and
// S_{d-1} = (a_d/b) G V0 + a_{d-1} V0 in w.Y; step i reads S_{i+1} (Sin, every
// row) and writes S_i = G S_{i+1} / b + a_i V0 (Sout: w.S / w.Y alternately,
// w.Q for S_0, the next basis; a thread reads its V0 entry before it writes
// S_0 over it).  b = theta_p; dead (re-randomised) columns keep V0.  Rows of
// one 64-row block per workgroup.
template <int P>
__global__ __launch_bounds__(256) void eig_cheb_kernel(const double *__restrict__ G, int64_t ldg,
                                                       int64_t strideG, EigWork w, int m, int k, int p,
                                                       const double *Sin, double *Sout, double fai) {
  constexpr int SQ = P + 4;
  __shared__ __attribute__((aligned(16))) double sV[EROWS * SQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rep = blockIdx.y, rb = blockIdx.x;
  if (w.done[rep]) return;
  const double *small = w.small + (int64_t)rep * small_stride<P>();
  const double b = filter_top(small + 2 * P * P, k, p);
  // b <= 0 (a degenerate block): plain power steps
  const double cb = b > 0.0 ? 1.0 / b : 1.0, cv0 = b > 0.0 ? fai : 0.0;
  const double *Gr = G + (int64_t)rep * strideG;
  const double *Vr = Sin + (int64_t)rep * m * P;
  double *So = Sout + (int64_t)rep * m * P;
  const double *V0 = w.Q + (int64_t)rep * m * P;
  const int fi = lane & 3, fkc = 4 * (lane >> 4) + ((lane >> 2) & 3);
  const int row0 = rb * EROWS + wave * 16;
  double acc[4][P / 4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int bb = 0; bb < P / 4; ++bb) acc[a][bb] = 0.0;
  for (int kc0 = 0; kc0 < m; kc0 += EROWS) {
    for (int e = tid; e < EROWS * P; e += 256) {
      const int r = e / P, c = e % P;
      sV[r * SQ + c] = (kc0 + r < m) ? Vr[(int64_t)(kc0 + r) * P + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < EROWS / 16; ++ks) {
      // wave-uniform: rows past m (m = 130: 3 of 12 waves) and k steps past m
      // only ever added zero products
      if (row0 >= m || kc0 + ks * 16 >= m) continue;
      const int kg = kc0 + ks * 16 + fkc;
      double af[4], bf[P / 4];
#pragma unroll
      for (int fa = 0; fa < 4; ++fa) {
        const int row = row0 + 4 * fa + fi;
        af[fa] = (row < m && kg < m) ? Gr[(int64_t)row * ldg + kg] : 0.0;
      }
#pragma unroll
      for (int fb = 0; fb < P / 4; ++fb) bf[fb] = sV[(ks * 16 + fkc) * SQ + 4 * fb + fi];
#pragma unroll
      for (int fa = 0; fa < 4; ++fa)
#pragma unroll
        for (int fb = 0; fb < P / 4; ++fb) acc[fa][fb] = mfma4(af[fa], bf[fb], acc[fa][fb]);
    }
    __syncthreads();
  }
  const int b1 = (lane >> 2) & 1, b2 = (lane >> 3) & 1, blk = (lane >> 2) & 3;
  const int oi = lane >> 4, oj = lane & 3;
#pragma unroll
  for (int fa = 0; fa < 4; ++fa)
#pragma unroll
    for (int q = 0; q < P / 16; ++q) {
      const double a0 = acc[fa][4 * q], a1 = acc[fa][4 * q + 1], a2 = acc[fa][4 * q + 2],
                   a3 = acc[fa][4 * q + 3];
      double k01 = (b1 ? a1 : a0) + __shfl_xor(b1 ? a0 : a1, 4);
      double k23 = (b1 ? a3 : a2) + __shfl_xor(b1 ? a2 : a3, 4);
      const double gv = (b2 ? k23 : k01) + __shfl_xor(b2 ? k01 : k23, 8);
      const int lr = wave * 16 + 4 * fa + oi, col = 16 * q + 4 * blk + oj;
      const int row = rb * EROWS + lr;
      if (row < m) {
        const bool dead = small[2 * P * P + P + col] != 0.0;
        const double v0 = V0[(int64_t)row * P + col];
        double sn = dead ? v0 : fma(cb, gv, cv0 * v0);
        if (col >= p) sn = 0.0;
        So[(int64_t)row * P + col] = sn;
      }
    }
}

// ---------------------------------------------------------------- small
// One wave per replicate, all p x p algebra in LDS, written for latency:
// Cholesky + triangular inverse in registers (every solve becomes a parallel
// matrix product), and a parallel cyclic Jacobi whose round is ONE phase: with
// the pairs of a round disjoint, every 2x2 block (pair s1 rows, pair s2 cols)
// is rotated J1' B J2 by one lane.
template <int P>
struct SmallLds {
  static constexpr int S = P + 1;
  // four P x (P+1) regions, reused as the matrices' lifetimes end (the
  // kernel is latency-bound and one wave per workgroup, so the LDS image sets
  // the occupancy: 4 regions = 9.2 KB at P = 16, 16 waves per CU, where the 6
  // of the unshared layout held it to 11):
  //   R1  H~ (Q'Y, then Li Q'Y Li', Jacobi)      -> W = V[:, perm] -> Y'Y A -> Bm
  //   R2  Q'Q -> Li Q'Y -> V (Jacobi vectors)    -> A = Li' W
  //   R3  Y'Y                                    -> Z'Z = A' Y'Y A
  //   R4  Li = chol(Q'Q)^-1                      -> chol(Z'Z)^-1
  double R1[P * S], R2[P * S], R3[P * S], R4[P * S];
  double rc[P / 2], rs[P / 2];
  int ra[P / 2], rb[P / 2], perm[P];
  int dead[P];
};

// LDS hand-off inside the ONE wave that runs the p x p algebra (eig_small's
// single-wave workgroups; in eig_fused the other waves wait at a barrier):
// a wave's LDS accesses complete in issue order, so waiting for its own
// outstanding ones (and fencing the compiler) is the whole synchronisation.
DFM_DEV void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// reciprocal and reciprocal square root: hardware seed + two Newton steps
// (full double precision to within an ulp or so; the Jacobi rotations only
// need c^2 + s^2 = 1 to rounding, which c = rsq(1 + t^2), s = t c keep)
DFM_DEV double nr_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  return fma(fma(-x, r, 1.0), r, r);
}
DFM_DEV double nr_rsq(double x) {
  double y = __builtin_amdgcn_rsq(x);
  const double hx = 0.5 * x;
  y = y * fma(-hx * y, y, 1.5);
  return y * fma(-hx * y, y, 1.5);
}

DFM_DEV double rl64(double x, int l) {   // lane l's x (l wave-uniform: a compile-time constant in unrolled loops)
  const long long b = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// Li = Lo^-1 of the lower Cholesky factor M = Lo Lo' (p x p): lane i < P
// holds row i in registers.  Right-looking factorisation (step j: pivot by
// readlane, column j scaled by one reciprocal square root, the trailing rows
// updated), then lane c forward-substitutes column c of the inverse.  M is
// dead once its rows are in registers, so it holds the columns of Lo as they
// are formed (column j in M's row j): every lane reads the values it needs
// from there as same-address LDS broadcasts, one instruction per double
// where a readlane pair plus its hazard wait took three or four (this
// wave's own writes, in LDS order).  Tiny pivots -> dead (unit diagonal,
// zero column, zero row of Li).  Tiny is 1e-22 of the largest diagonal entry
// (Z'Z: the columns of Z = G U scale with their Ritz values, and a wanted
// zero is dead), or with OWN of the column's own diagonal entry (Q'Q: the
// filter leaves the columns of Q with norms T_d(theta_j / theta_p), 2^67 apart
// on a spectrum that falls by 2^15 across the block, so only a column that is
// linearly dependent on those before it, to 1e-11, is dead; against the
// largest entry every short column was, and came back as theta = 0, u = 0).
template <int P, bool OWN = false>
DFM_DEV void wave_chol_inv(double *M, double *Li, int *dead, int p) {
  constexpr int S = P + 1;
  const int lane = threadIdx.x & 63;
  double mx = 0.0;
  for (int j = lane; j < p; j += 64) mx = fmax(mx, fabs(M[j * S + j]));
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
  const double thresh = 1e-22 * mx;
  double r[P];
#pragma unroll
  for (int k = 0; k < P; ++k) r[k] = (lane < p && k < p) ? M[min(lane, P - 1) * S + k] : 0.0;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // M's rows are in registers before M is overwritten
  double inv_l = 1.0;
  int dead_l = 0;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    if (j < p) {
      const double sj = rl64(r[j], j);
      const bool dd = !(sj > (OWN ? 1e-22 * M[j * S + j] : thresh));   // (row j of M is still the input's)
      const double inv = dd ? 1.0 : rsqrt(sj);
      double lij = (lane > j && lane < p) ? (dd ? 0.0 : r[j] * inv) : 0.0;
      if (lane == j) { lij = dd ? 1.0 : sj * inv; inv_l = inv; dead_l = dd; }
      r[j] = lij;
      if (lane < P) M[j * S + lane] = lij;          // column j of Lo
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int k = j + 1; k < P; ++k) r[k] = r[k] - lij * M[j * S + k];
    }
  }
  if (lane < P) dead[lane] = lane < p ? dead_l : 0;
  if (lane < P) M[(P - 1) * S + lane] = inv_l;   // 1 / Lo[i][i], over column P-1 of Lo (the substitution never reads it)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  double x[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    double sacc = (i == lane) ? 1.0 : 0.0;
#pragma unroll
    for (int q = 0; q < i; ++q) sacc = sacc - M[q * S + i] * x[q];
    x[i] = (i < p) ? sacc * M[(P - 1) * S + i] : 0.0;
  }
  const bool dl = lane < p;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const bool di = dead[i] != 0;
    if (lane < P) Li[i * S + lane] = (i < p && dl && !di) ? x[i] : 0.0;
  }
  wave_lds_sync();
}

// C = op(A) op(B) for P x P LDS matrices (TA/TB transpose flags; C distinct
// from A and B); padded entries are zero so the full P x P product is exact.
// One wave of v_mfma_f64_16x16x4 per 16 x 16 output tile: A operand = row
// (lane & 15), k (lane >> 4); B operand = k (lane >> 4), column (lane & 15);
// accumulator register g = row 4g + (lane >> 4), column (lane & 15).
template <int P, bool TA, bool TB>
DFM_DEV void wave_mm(const double *A, const double *B, double *C) {
  constexpr int S = P + 1, NT = P / 16;
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int rt = 0; rt < NT; ++rt)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
      const int i = 16 * rt + li, j = 16 * ct + li;
      dv4 acc = dv4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < P / 4; ++kk) {
        const int q = 4 * kk + lk;
        acc = mfma16(TA ? A[q * S + i] : A[i * S + q], TB ? B[j * S + q] : B[q * S + j], acc);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) C[(16 * rt + 4 * g + lk) * S + 16 * ct + li] = acc[g];
    }
  wave_lds_sync();
}

template <int P>
DFM_DEV void wave_sym(double *M) {
  constexpr int S = P + 1;
  for (int e = threadIdx.x & 63; e < P * P; e += 64) {
    const int i = e / P, j = e % P;
    if (i < j) { const double v = 0.5 * (M[i * S + j] + M[j * S + i]); M[i * S + j] = v; M[j * S + i] = v; }
  }
  wave_lds_sync();
}

// The Rayleigh-Ritz step on ONE wave (any wave of the workgroup): in, R1 =
// Q'Y, R3 = Y'Y, R2 = Q'Q (entries >= p zero; with SMALL_CHOL1_DONE in
// jsweeps, R4 = chol(Q'Q)^-1 and sm.dead already formed instead); out, A in R2 and Bm in R1
// (also copied to ab[0, P^2) and ab[P^2, 2 P^2) when ab is given) and the
// small record's tail: theta[P], then the dead flags[P].
template <int P>
DFM_DEV void small_rr(SmallLds<P> &sm, EigWork &w, int rep, int p, int jsweeps, double *ab, double *tail) {
  constexpr int S = P + 1;
  double *const Hq = sm.R1, *const Yq = sm.R3;   // region map: SmallLds
  // opaque lane and p: called inside eig_fused's iteration loop, whose
  // optimiser would otherwise hoist this step's lane-derived indices out of
  // the loop and keep them live through every other phase
  int lane = threadIdx.x & 63;
  asm volatile("" : "+v"(lane));
  asm volatile("" : "+s"(p));
  SMALL_STAMP(1);
  if (!(jsweeps & SMALL_STAGE_B)) {
  wave_sym<P>(Hq);
  // 2. Q'Q = L L',  Li = L^-1;  H~ = Li (Q'Y) Li'
  if (!(jsweeps & SMALL_CHOL1_DONE)) {
    if (jsweeps & SMALL_CHOL_OWN) wave_chol_inv<P, true>(sm.R2, sm.R4, sm.dead, p);
    else wave_chol_inv<P>(sm.R2, sm.R4, sm.dead, p);
  }
  SMALL_STAMP(2);
  SMALL_STAMP(3);
  wave_mm<P, false, false>(sm.R4, Hq, sm.R2);   // Q'Q is dead once Li is formed
  wave_mm<P, false, true>(sm.R2, sm.R4, Hq);
  wave_sym<P>(Hq);
  SMALL_STAMP(4);
  for (int e = lane; e < P * S; e += 64) sm.R2[e] = ((e / S) == (e % S)) ? 1.0 : 0.0;   // V
  wave_lds_sync();
  double *const V = sm.R2;
  // 3. parallel cyclic Jacobi (circle-method pairs; index p is a dummy when p is odd)
  const int n = p + (p & 1), h = n / 2;
  // A pair is rotated only while |h_ab| > 4 eps sqrt(|h_aa h_bb|) (the classic
  // Jacobi threshold: a smaller off-diagonal moves the eigenvalues by
  // O(eps^2)); the sweep loop ends at the first sweep that rotates nothing.
  // (A Frobenius off-diagonal test sits at the rounding floor for these
  // matrices and ran every sweep to the cap.)
  // every lane's 2x2 blocks and V entries are the same in every round: their
  // (s1, s2) and (k, sI) indices are computed once here, and the circle-method
  // positions advance by a wrapped increment (no integer division per round)
  constexpr int NHB = ((P / 2) * (P / 2) + 63) / 64, NVE = (P * (P / 2) + 63) / 64;
  int hb1[NHB], hb2[NHB], vk[NVE], vs[NVE];
#pragma unroll
  for (int u = 0; u < NHB; ++u) {
    const int e = lane + 64 * u;
    hb1[u] = (h > 0 && e < h * h) ? e / h : -1;
    hb2[u] = (h > 0 && e < h * h) ? e % h : 0;
  }
#pragma unroll
  for (int u = 0; u < NVE; ++u) {
    const int e = lane + 64 * u;
    vk[u] = (h > 0 && e < p * h) ? e / h : -1;
    vs[u] = (h > 0 && e < p * h) ? e % h : 0;
  }
  const int n1 = n - 1, pa = lane, pb = n - 1 - lane;
  for (int sweep = 0; sweep < (jsweeps & 0xff); ++sweep) {
    bool rotated = false;
    int xa = pa - 1, xb = pb - 1;   // position - 1 + r, wrapped into [0, n - 1)
    for (int r = 0; r < n1; ++r, ++xa, ++xb) {
      if (xa >= n1) xa -= n1;
      if (xb >= n1) xb -= n1;
      bool rot = false;
      if (lane < h) {
        int a = pa == 0 ? 0 : 1 + xa;
        int b = pb == 0 ? 0 : 1 + xb;
        if (a > b) { const int t = a; a = b; b = t; }
        double c = 1.0, sn = 0.0;
        if (b < p) {
          const double hab = Hq[a * S + b], haa = Hq[a * S + a], hbb = Hq[b * S + b];
          // |h_ab| > 4 eps sqrt(|h_aa h_bb|), squared; the rotation from the
          // hardware reciprocal / reciprocal-square-root seeds plus Newton
          // steps (the round's critical path: three divisions and three
          // square roots in correctly rounded form)
          if (fabs(hab) > 1e-300 && hab * hab > 7.921e-31 * fabs(haa * hbb)) {
            const double zeta = (hbb - haa) * nr_rcp(2.0 * hab), az = fabs(zeta);
            const double y = fma(zeta, zeta, 1.0);
            const double rt = az > 1e150 ? az : y * nr_rsq(y);   // sqrt(1 + zeta^2)
            const double t = (zeta >= 0.0 ? 1.0 : -1.0) * nr_rcp(az + rt);
            c = nr_rsq(fma(t, t, 1.0));
            sn = t * c;
            rot = true;
          }
        }
        sm.ra[lane] = a; sm.rb[lane] = b; sm.rc[lane] = c; sm.rs[lane] = sn;
      }
      const bool any = __any(rot);
      rotated = rotated || any;
      if (!any) continue;   // wave-uniform: nothing to apply this round
      wave_lds_sync();
      // H <- J' H J by 2x2 blocks; V <- V J
#pragma unroll
      for (int u = 0; u < NHB; ++u) {
        if (hb1[u] < 0) continue;
        const int s1 = hb1[u], s2 = hb2[u];
        const int i0 = sm.ra[s1], i1 = sm.rb[s1], j0 = sm.ra[s2], j1 = sm.rb[s2];
        const double c1 = sm.rc[s1], n1 = sm.rs[s1], c2 = sm.rc[s2], n2 = sm.rs[s2];
        const double b00 = Hq[i0 * S + j0], b01 = Hq[i0 * S + j1];
        const double b10 = Hq[i1 * S + j0], b11 = Hq[i1 * S + j1];
        const double t00 = c1 * b00 - n1 * b10, t01 = c1 * b01 - n1 * b11;
        const double t10 = n1 * b00 + c1 * b10, t11 = n1 * b01 + c1 * b11;
        Hq[i0 * S + j0] = c2 * t00 - n2 * t01;
        Hq[i0 * S + j1] = n2 * t00 + c2 * t01;
        Hq[i1 * S + j0] = c2 * t10 - n2 * t11;
        Hq[i1 * S + j1] = n2 * t10 + c2 * t11;
      }
#pragma unroll
      for (int u = 0; u < NVE; ++u) {
        if (vk[u] < 0) continue;
        const int k = vk[u], sI = vs[u];
        const int a = sm.ra[sI], b = sm.rb[sI];
        const double c = sm.rc[sI], sn = sm.rs[sI];
        const double va = V[k * S + a], vb = V[k * S + b];
        V[k * S + a] = c * va - sn * vb;
        V[k * S + b] = sn * va + c * vb;
      }
      wave_lds_sync();
    }
    if (w.dbg && rep == 0 && lane == 0) w.dbg[15] = sweep + 1;
    if (!rotated) break;
  }
  SMALL_STAMP(5);
  // 4. sort descending (stable): lane j computes the rank of diagonal j
  for (int j = lane; j < p; j += 64) {
    const double v = Hq[j * S + j];
    int rank = 0;
    for (int i = 0; i < p; ++i) {
      const double u = Hq[i * S + i];
      rank += (u > v || (u == v && i < j)) ? 1 : 0;
    }
    sm.perm[rank] = j;
  }
  wave_lds_sync();
  for (int j = lane; j < P; j += 64) tail[j] = j < p ? Hq[sm.perm[j] * S + sm.perm[j]] : 0.0;
  wave_lds_sync();   // the Ritz values are read from R1 before W overwrites it
  // W = V[:, perm] (zero-padded), into R1
  double *const W = sm.R1;
  for (int e = lane; e < P * P; e += 64) {
    const int i = e / P, c = e % P;
    W[i * S + c] = (i < p && c < p) ? V[i * S + sm.perm[c]] : 0.0;
  }
  wave_lds_sync();
  SMALL_STAMP(6);
  // 5. A = L^-T Vs = Li' W ;  Z'Z = A' (Y'Y) A ;  L2 = chol ;  Bm = A L2^-T
  double *const A = sm.R2;
  wave_mm<P, true, false>(sm.R4, W, A);       // V is dead once permuted
  wave_mm<P, false, false>(Yq, A, sm.R1);     // Y'Y A (W is dead)
  wave_mm<P, true, false>(A, sm.R1, sm.R3);   // Z'Z (Y'Y is dead)
  wave_sym<P>(sm.R3);
  SMALL_STAMP(7);
  }
  if (jsweeps & SMALL_STAGE_A) return;
  double *const A = sm.R2;
  wave_chol_inv<P>(sm.R3, sm.R4, sm.dead, p);
  SMALL_STAMP(8);
  SMALL_STAMP(9);
  wave_mm<P, false, true>(A, sm.R4, sm.R1);   // Bm = A Li'
  if (ab)
    for (int e = lane; e < P * P; e += 64) {
      const int a = e / P, c = e % P;
      ab[e] = (a < p && c < p) ? A[a * S + c] : 0.0;
      ab[P * P + e] = (a < p && c < p) ? sm.R1[a * S + c] : 0.0;
    }
  for (int j = lane; j < P; j += 64) tail[P + j] = (j < p && sm.dead[j]) ? 1.0 : 0.0;
  wave_lds_sync();
  SMALL_STAMP(10);
}

template <int P>
__global__ __launch_bounds__(64) void eig_small_kernel(EigWork w, int p, int nrb, int jsweeps) {
  constexpr int S = P + 1;
  __shared__ SmallLds<P> sm;
  const int lane = threadIdx.x, rep = blockIdx.x;
  if (w.done[rep]) return;
  SMALL_STAMP(0);
  // 1. sum partials in fixed order (entries >= p are zero: Q columns >= p are zero)
  const double *pp = w.part + (int64_t)rep * nrb * 3 * P * P;
  constexpr int PER = 3 * P * P / 64;   // entries per lane (12 for P = 16)
  {
    double acc[PER];
#pragma unroll
    for (int u = 0; u < PER; ++u) acc[u] = 0.0;
    for (int r = 0; r < nrb; ++r) {   // all PER loads of a block issue together
      double v[PER];
#pragma unroll
      for (int u = 0; u < PER; ++u) v[u] = pp[(int64_t)r * 3 * P * P + lane + 64 * u];
#pragma unroll
      for (int u = 0; u < PER; ++u) acc[u] += v[u];
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = lane + 64 * u;
      const int which = e / (P * P), a = (e / P) % P, c = e % P;
      double *M = which == 0 ? sm.R1 : (which == 1 ? sm.R3 : sm.R2);
      M[a * S + c] = acc[u];
    }
  }
  wave_lds_sync();
  double *small = w.small + (int64_t)rep * small_stride<P>();
  small_rr<P>(sm, w, rep, p, jsweeps, small, small + 2 * P * P);
}

// ---------------------------------------------------------------- apply
template <int P>
// cheb = 1: the next basis is formed by eig_cheb_kernel; here V = Y Bm goes
// to w.Y and Q Bm to w.Q (both over this block's own rows, already staged).
__global__ __launch_bounds__(256) void eig_apply_kernel(EigWork w, int m, int p, int k, int it,
                                                        uint64_t seed, int64_t rep0, int cheb, double fa1,
                                                        double fa0) {
  constexpr int SQ = P + 1;
  __shared__ double sQ[EROWS * SQ], sY[EROWS * SQ], sW[EROWS * P];
  __shared__ double sA[P * P], sB[P * P], sT[2 * P], sUn[256];
  const int tid = threadIdx.x, rep = blockIdx.y, rb = blockIdx.x, nrb = gridDim.x;
  double un = 0.0;   // this thread's rows' share of |u_c|^2, c = tid % P (256 % P == 0: one column per thread)
  if (w.done[rep]) return;
  const double *small = w.small + (int64_t)rep * small_stride<P>();
  double *Qr = w.Q + (int64_t)rep * m * P;
  double *Yr = w.Y + (int64_t)rep * m * P;
  double *Ur = w.U + (int64_t)rep * m * P;
  for (int e = tid; e < EROWS * P; e += 256) {
    const int r = e / P, c = e % P, row = rb * EROWS + r;
    sQ[r * SQ + c] = row < m ? Qr[(int64_t)row * P + c] : 0.0;
    sY[r * SQ + c] = row < m ? Yr[(int64_t)row * P + c] : 0.0;
  }
  for (int e = tid; e < P * P; e += 256) { sA[e] = small[e]; sB[e] = small[P * P + e]; }
  for (int e = tid; e < 2 * P; e += 256) sT[e] = small[2 * P * P + e];
  __syncthreads();
  for (int e = tid; e < EROWS * P; e += 256) {
    const int r = e / P, c = e % P, row = rb * EROWS + r;
    double u = 0.0, ya = 0.0, qn = 0.0, qb = 0.0;
    for (int a = 0; a < p; ++a) {
      u = fma(sQ[r * SQ + a], sA[a * P + c], u);
      ya = fma(sY[r * SQ + a], sA[a * P + c], ya);
      qn = fma(sY[r * SQ + a], sB[a * P + c], qn);
      if (cheb) qb = fma(sQ[r * SQ + a], sB[a * P + c], qb);
    }
    if (c < p && sT[P + c] != 0.0) qn = hash_unit(seed, row, 1000003ull * (it + 1) + c);
    if (c >= p) { qn = 0.0; qb = 0.0; }
    if (c < k) { const double wv = ya - sT[c] * u; sW[r * P + c] = row < m ? wv * wv : 0.0; }
    if (row < m) un = fma(u, u, un);
    if (row < m) {
      Ur[(int64_t)row * P + c] = u;
      if (cheb) {   // the filter's first Horner term S = (a_d/b) V + a_{d-1} Q Bm, and V0 = Q Bm (dead: V)
        const double bch = filter_top(sT, k, p);
        const bool dead = c < p && sT[P + c] != 0.0;
        const double sv = dead ? qn : (bch > 0.0 ? fma(fa1 / bch, qn, fa0 * qb) : qn);
        Yr[(int64_t)row * P + c] = c >= p ? 0.0 : sv;
        Qr[(int64_t)row * P + c] = c >= p ? 0.0 : (dead ? qn : qb);
      } else {
        Qr[(int64_t)row * P + c] = qn;
      }
    }
  }
  sUn[tid] = un;
  __syncthreads();
  if (tid < k) {
    double s = 0.0, us = 0.0;
    for (int r = 0; r < EROWS; ++r) s += sW[r * P + tid];
    for (int q = tid; q < 256; q += P) us += sUn[q];
    w.rpart[((int64_t)rep * nrb + rb) * P + tid] = s;
    w.upart[((int64_t)rep * nrb + rb) * P + tid] = us;
  }
}

// ---------------------------------------------------------------- final
// lam: nb x k, Uk: nb x m x k (row-major), status: nb (0 ok, 1 not converged)
// Ur: the replicate's Ritz vectors (m x P), theta its Ritz values; 256 threads.
template <int P>
DFM_DEV void eig_final_body(const double *Ur, const double *theta, int done, int rep, int m, int k,
                            double *__restrict__ lam, double *__restrict__ Uk, int *__restrict__ status) {
  if (!Uk) {   // eigenvalue-only statistics: no vectors wanted, no pass over U
    if (threadIdx.x < k) lam[(int64_t)rep * k + threadIdx.x] = theta[threadIdx.x];
    if (threadIdx.x == 0) status[rep] = done ? 0 : 1;
    return;
  }
  // one pass over U: each thread keeps the running max |U[r][j]| (first row
  // on ties) of its rows for every column j, then a shuffle reduction per
  // wave and a fixed-order combine of the four waves (smaller row index wins
  // ties: the same pick as a serial scan)
  __shared__ double sv[P][4];
  __shared__ int si[P][4];
  __shared__ double ssign[P];
  const int tid = threadIdx.x, wv = tid >> 6;
  double best[P];
  int bi[P];
#pragma unroll
  for (int j = 0; j < P; ++j) { best[j] = -1.0; bi[j] = 0; }
  for (int r = tid; r < m; r += 256) {
    double v[P];
#pragma unroll
    for (int j = 0; j < P; j += 2) {
      const double2 x = *reinterpret_cast<const double2 *>(Ur + (int64_t)r * P + j);
      v[j] = x.x; v[j + 1] = x.y;
    }
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const double a = fabs(v[j]);
      if (j < k && a > best[j]) { best[j] = a; bi[j] = r; }
    }
  }
#pragma unroll
  for (int j = 0; j < P; ++j) {
    if (j >= k) continue;
    double a = best[j];
    int ai = bi[j];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const double b = __shfl_xor(a, o);
      const int bj = __shfl_xor(ai, o);
      if (b > a || (b == a && bj < ai)) { a = b; ai = bj; }
    }
    if ((tid & 63) == 0) { sv[j][wv] = a; si[j][wv] = ai; }
  }
  __syncthreads();
  if (tid < k) {
    double a = sv[tid][0];
    int ai = si[tid][0];
    for (int q = 1; q < 4; ++q)
      if (sv[tid][q] > a || (sv[tid][q] == a && si[tid][q] < ai)) { a = sv[tid][q]; ai = si[tid][q]; }
    si[tid][0] = ai;
  }
  __syncthreads();
  if (tid < k) ssign[tid] = Ur[(int64_t)si[tid][0] * P + tid] < 0.0 ? -1.0 : 1.0;
  __syncthreads();
  if (tid < k) lam[(int64_t)rep * k + tid] = theta[tid];
  if (tid == 0) status[rep] = done ? 0 : 1;
  for (int64_t e = tid; e < (int64_t)m * k; e += 256) {
    const int r = (int)(e / k), j = (int)(e % k);
    Uk[(int64_t)rep * m * k + e] = ssign[j] * Ur[(int64_t)r * P + j];
  }
}

DFM_DEV void count_iters_body(const int *__restrict__ active, int last_gemm, int last_cheb, int nb, long long *cnt,
                              int cp0, int cp1, int skip0);
template <int P>
__global__ __launch_bounds__(256) void eig_final_kernel(EigWork w, int m, int k, double *__restrict__ lam,
                                                        double *__restrict__ Uk, int *__restrict__ status,
                                                        double *__restrict__ trace_out, long long *cnt, int last_gemm,
                                                        int last_cheb, int cp0, int cp1, int skip0) {
  const int rep = blockIdx.x;
  if (trace_out && threadIdx.x == 0) trace_out[rep] = w.trace[rep];   // (the caller's copy of trace(G))
  // the factored run's iteration / product counts
  if (cnt && rep == 0 && threadIdx.x == 0) count_iters_body(w.active, last_gemm, last_cheb, gridDim.x, cnt, cp0, cp1, skip0);
  eig_final_body<P>(w.U + (int64_t)rep * m * P, w.small + (int64_t)rep * small_stride<P>() + 2 * P * P, w.done[rep],
                    rep, m, k, lam, Uk, status);
}

// ------------------------------------------------------------- host driver
size_t eig_workspace_bytes(int m, int nb, int P, int maxit) {
  const int nrb = (m + EROWS - 1) / EROWS;
  size_t s = 0;
  s += 4 * (size_t)nb * m * P * 8;               // Q, Y, U, S
  s += (size_t)nb * nrb * 3 * P * P * 8;         // part
  s += (size_t)nb * nrb * P * 8;                 // rpart
  s += (size_t)nb * (2 * P * P + 4 * P) * 8;     // small
  s += (size_t)nb * 8;                           // trace
  s += (size_t)(2 * nb + maxit + 2) * 4 + 256;   // done, iters, active
  s += (size_t)nb * nrb * P * 8 + 256;           // upart
  return s;
}

EigWork carve(char *base, int m, int nb, int P, int maxit) {
  const int nrb = (m + EROWS - 1) / EROWS;
  EigWork w;
  auto take = [&](size_t bytes) { char *p = base; base += (bytes + 255) & ~size_t(255); return p; };
  w.Q = (double *)take((size_t)nb * m * P * 8);
  w.Y = (double *)take((size_t)nb * m * P * 8);
  w.U = (double *)take((size_t)nb * m * P * 8);
  w.S = (double *)take((size_t)nb * m * P * 8);
  w.part = (double *)take((size_t)nb * nrb * 3 * P * P * 8);
  w.rpart = (double *)take((size_t)nb * nrb * P * 8);
  w.small = (double *)take((size_t)nb * (2 * P * P + 4 * P) * 8);
  w.trace = (double *)take((size_t)nb * 8);
  w.done = (int *)take((size_t)nb * 4);
  w.iters = (int *)take((size_t)nb * 4);
  w.active = (int *)take((size_t)(maxit + 2) * 4);
  w.upart = (double *)take((size_t)nb * nrb * P * 8);   // last: the members before it keep their places
  w.dbg = nullptr;
  w.subspace = 0;
  w.no_vectors = 0;
  return w;
}

// per-replicate Rayleigh-Ritz steps of the last solve carved from ws (diagnostic stat)
const int *eig_iters_ptr(char *ws, int m, int nb, int P, int maxit) { return carve(ws, m, nb, P, maxit).iters; }

size_t eig_workspace_bytes_padded(int m, int nb, int P, int maxit) {
  return eig_workspace_bytes(m, nb, P, maxit) + 16 * 256;
}

// Jacobi sweeps per Rayleigh-Ritz step of the fused solver: ONE (C2: the
// same 4.99 steps per replicate as two sweeps, 458k vs 423k rep/s — the
// inner sweeps accumulate across outer steps).  DFM_EIG_JSWEEPS overrides.
static int fused_sweeps() {
  static const int v = [] {
    const char *a = getenv("DFM_EIG_JSWEEPS");
    return a ? std::max(1, std::min(8, atoi(a))) : 1;
  }();
  return v;
}
thread_local int g_last_iters = 0;   // iterations run by the last eig_run / eig_run_factored (host stat)
// replicate-iterations of the last run's dominant product (G.Q in eig_gq, or
// the H.Z GEMM in the factored solver) that still had an unconverged
// replicate: the algorithmic work the roofline figure is priced on.
thread_local int64_t g_last_rep_iters = 0;
thread_local int64_t g_last_gemm_products_f32 = 0;   // of g_last_gemm_products, those run in fp32 (factored solver only)
thread_local int64_t g_last_gemm_products_split_last = 0;   // the warm filter's last products run as bf16 terms (factored solver only)
thread_local int64_t g_last_gemm_products_split3 = 0;   // of the fp32 ones, those run as three bf16 terms (factored solver only)
thread_local int64_t g_last_gemm_products = 0;   // replicate-products of the last run: H . Z (factored, both Chebyshev GEMMs) or G S (fused direct solver)

// Sum of the unconverged-replicate counts seen by the products of iterations
// 0..last (shift = 1: the product of iteration it runs before that
// iteration's convergence check, so it sees active[it-1]; active[-1] = nb).
// Device-side form of count_rep_iters for the factored run: adds the
// replicate-iterations (GEMM launches 0..last_gemm, shift 1) and the GEMM
// replicate-products (those plus the Chebyshev GEMMs 0..last_cheb, shift 0)
// to cnt[0], cnt[1] — no host synchronisation after the eigen loop.
// skip0: step 0 was a filter alone (a warm solve without a first
// Rayleigh-Ritz step; active[0] = nb, q0_guards_kernel): its first product counts as a product
// but not as a replicate-iteration.
DFM_DEV void count_iters_body(const int *__restrict__ active, int last_gemm, int last_cheb, int nb, long long *cnt,
                              int cp0, int cp1, int skip0) {
  long long a = 0, b = 0;
  for (int it = 0; it <= last_gemm; ++it) a += it - 1 < 0 ? nb : active[it - 1];
  // Chebyshev products: cp0 after the first Rayleigh-Ritz step, cp1 after the others
  for (int it = 0; it <= last_cheb; ++it) b += (long long)active[it] * (it == 0 ? cp0 : cp1);
  // device-scope atomics: a model's two bootstrap lanes count into one context
  atomicAdd(reinterpret_cast<unsigned long long *>(cnt), (unsigned long long)(a - (skip0 && last_gemm >= 0 ? nb : 0)));
  atomicAdd(reinterpret_cast<unsigned long long *>(cnt + 1), (unsigned long long)(a + b));
}
int64_t count_rep_iters(const int *active_dev, int last, int shift, int nb, hipStream_t st) {
  if (last < 0) return 0;
  std::vector<int> a((size_t)last + 2, 0);
  hipMemcpyAsync(a.data(), active_dev, a.size() * 4, hipMemcpyDeviceToHost, st);
  hipStreamSynchronize(st);
  int64_t s = 0;
  for (int it = 0; it <= last; ++it) s += (it - shift < 0) ? nb : a[it - shift];
  return s;
}

constexpr int kChebDirectStrict = 4;
// Shifted Chebyshev coefficients T*_d(y) = T_d(2y - 1) = sum_i a_i y^i
// (T*_0 = 1, T*_1 = 2y - 1, T*_{n+1} = 2 (2y - 1) T*_n - T*_{n-1}).
void shifted_cheb(int d, double *a) {   // a[0..kChebDMax]
  double t0[kChebDMax + 1] = {1.0}, t1[kChebDMax + 1] = {-1.0, 2.0};
  if (d == 0) { for (int i = 0; i <= kChebDMax; ++i) a[i] = t0[i]; return; }
  for (int n = 1; n < d; ++n) {
    double t2[kChebDMax + 1];
    for (int i = 0; i <= kChebDMax; ++i) t2[i] = -2.0 * t1[i] - t0[i] + (i > 0 ? 4.0 * t1[i - 1] : 0.0);
    for (int i = 0; i <= kChebDMax; ++i) { t0[i] = t1[i]; t1[i] = t2[i]; }
  }
  for (int i = 0; i <= kChebDMax; ++i) a[i] = t1[i];
}

// ---------------------------------------------------------------- fused
// The whole direct solve of ONE replicate in ONE workgroup (4 waves), P = 16
// and m <= 16 NGW: the basis Q and the product Y stay in LDS for the whole
// solve (2 x m x 16 doubles: 37 KB at m = 130, three workgroups per CU), G
// streams from L2 / MALL once per product.  Each iteration runs the same
// algebra as the kernel sequence gq -> small -> apply -> cheb:
//   check    wave 0: iteration it-1's residuals (check_converged), retire / count
//   Y = G Q  v_mfma_f64_4x4x4_4b; 4-row groups dealt round-robin to the waves
//   Q'Y, Y'Y, Q'Q   waves 0..2, one product each over all m rows
//   small_rr wave 0 (the other waves wait at the barrier)
//   apply    U = Q A -> global (eig_final reads it), residual sums, V0 = Q Bm
//            and the filter's first Horner term S = (a_d/b) Y Bm + a_{d-1} V0
//   cheb     dg - 1 times S <- G S / b + a_i V0; S_0 (into Q) is the next basis
// The multi-kernel path's launch chain, its host polls and its per-row-block
// partial records are gone: a replicate leaves the loop the moment it
// converges, the others keep iterating.  Sums run in a fixed order.
struct ChebCo { double c2[kChebDMax + 1], c4[kChebDMax + 1]; };

// LDS image of an m x 16 block, row r, column c: the 4-column block is
// XOR-swizzled by (r >> 1) & 3, so the MFMA operand reads (rows 4 (lane >> 4)
// + ((lane >> 2) & 3), columns 4 fb + (lane & 3)) hit 8 distinct 8-bank
// groups per half-wave.
// x, opaque to the optimiser: lane-derived offsets recomputed per phase
// instead of hoisted out of the iteration loop (every phase's hoisted
// offsets live at once otherwise — hundreds of VGPRs, spilled)
DFM_DEV int fz_opaque(int x) { asm volatile("" : "+v"(x)); return x; }

DFM_DEV int fz_ix(int r, int c) { return (r << 4) | ((((c >> 2) ^ ((r >> 1) & 3)) << 2) | (c & 3)); }

// acc[q] = rows of 4-row group g = wave + NW q (NW waves share the rows) of G S (G: m x m in global, S:
// the LDS image, rows m..mpad-1 zero).  Lane: row 4 g + (lane & 3), k index
// k0 + 4 (lane >> 4) + ((lane >> 2) & 3) — a G row's 16 k values per chunk are
// one 128-byte line.  G comes from L2 / MALL (a batch's Grams outgrow the
// L2): a register ring holds FZ_DEPTH chunks in flight (3; 2 when a wave
// owns more than 9 groups — registers), the loads of chunk c + FZ_DEPTH - 1
// issue before chunk c's MFMAs.
template <int NGW, int NW, int FZ_DEPTH = (NGW > 9 ? 2 : 3)>
DFM_DEV void fz_gemm(const double *__restrict__ Gr, int64_t ldg, int m, int ng, const double *S, int wave, int lane,
                     double (&acc)[NGW][4]) {
  const int fi = lane & 3, fkc = 4 * (lane >> 4) + ((lane >> 2) & 3);
  const int ld = (int)ldg;   // m <= 256: element offsets fit 32 bits (SGPR base + VGPR offset loads)
  const int nch = (m + 15) >> 4;
#pragma unroll
  for (int q = 0; q < NGW; ++q)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[q][b] = 0.0;
  unsigned off[NGW];   // the lane's G row offset + k of chunk 0
#pragma unroll
  for (int q = 0; q < NGW; ++q) off[q] = (unsigned)((4 * (wave + NW * q) + fi) * ld + fkc);
  double ring[FZ_DEPTH][NGW];
  auto load = [&](int c, double (&dst)[NGW]) {
    const int kg = 16 * c + fkc;
#pragma unroll
    for (int q = 0; q < NGW; ++q) {
      const int g = wave + NW * q, row = 4 * g + fi;
      dst[q] = (g < ng && row < m && kg < m) ? Gr[off[q] + 16 * c] : 0.0;
    }
  };
#pragma unroll
  for (int s = 0; s < FZ_DEPTH - 1; ++s) load(s, ring[s]);
#pragma unroll 1
  for (int c0 = 0; c0 < nch; c0 += FZ_DEPTH) {
#pragma unroll
    for (int s = 0; s < FZ_DEPTH; ++s) {
      const int c = c0 + s;
      load(c + FZ_DEPTH - 1, ring[(s + FZ_DEPTH - 1) % FZ_DEPTH]);
      if (c < nch) {   // wave-uniform
        double bf[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) bf[fb] = S[fz_ix(16 * c + fkc, 4 * fb + fi)];
#pragma unroll
        for (int q = 0; q < NGW; ++q) {
          if (wave + NW * q >= ng) continue;   // wave-uniform
#pragma unroll
          for (int fb = 0; fb < 4; ++fb) acc[q][fb] = mfma4(ring[s][q], bf[fb], acc[q][fb]);
        }
      }
    }
  }
}

// Out (P x P, stride P + 1) = X1' X2 over the mpad rows of two LDS images,
// on ONE wave: output 4-row groups g = 0..3 of v_mfma_f64_4x4x4_4b.
DFM_DEV void fz_xtx(const double *X1, const double *X2, double *Out, int mpad, int lane) {
  constexpr int S = 17;
  const int fi = lane & 3, fkc = 4 * (lane >> 4) + ((lane >> 2) & 3);
  double a4[4][4];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int b = 0; b < 4; ++b) a4[g][b] = 0.0;
#pragma unroll 1
  for (int k0 = 0; k0 < mpad; k0 += 16) {
    const int kr = k0 + fkc;
    double af[4], bf[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) af[g] = X1[fz_ix(kr, 4 * g + fi)];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) bf[fb] = X2[fz_ix(kr, 4 * fb + fi)];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int fb = 0; fb < 4; ++fb) a4[g][fb] = mfma4(af[g], bf[fb], a4[g][fb]);
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const double v = mm4_fold(a4[g], lane);
    Out[(4 * g + (lane >> 4)) * S + (lane & 15)] = v;
  }
}

// OVL: Y = G Q on waves 0..2 (NG3 groups each) while wave 3 forms Q'Q and
// its inverse Cholesky factor — the Rayleigh-Ritz step's first factorisation
// leaves the critical path.
template <int NGW, int NG3, bool OVL>
__global__ __launch_bounds__(256, NGW <= 9 ? 2 : 1) void eig_fused_kernel(
    const double *__restrict__ G, int64_t ldg, int64_t strideG, EigWork w, int m, int k, int p, double tol,
    int maxit, const double *__restrict__ warm, int kw, uint64_t seed, int warm_strict, int jsweeps, ChebCo cc,
    double *__restrict__ lam, double *__restrict__ Uk, int *__restrict__ status, long long *__restrict__ prof) {
  constexpr int P = 16, S = P + 1;
  __shared__ SmallLds<P> sm;
  __shared__ double s_tail[4 * P];   // the small record's tail: theta[P], dead[P], residual history 2 x P
  __shared__ double s_rw[4][P];      // per-wave residual sums of one apply
  __shared__ double s_uw[4][P];      // and of |u_c|^2 (judged_residual)
  __shared__ double s_res[P];        // their fixed-order total (check_converged's one "row block")
  __shared__ int s_done;
  __shared__ double s_ca[2][kChebDMax + 1];   // filter coefficients, degree 2 | 4 (indexed at run time: LDS, not the kernarg struct)
  extern __shared__ double s_dyn[];  // Q | Y, mpad x 16 each (fz_ix images)
  const int rep = blockIdx.x;
  const int mpad = (m + 15) & ~15, ng = (m + 3) >> 2;
  double *const sQ = s_dyn, *const sY = s_dyn + mpad * P;
  const double *Gr = G + (int64_t)rep * strideG;
  double *Ur = w.U + (int64_t)rep * m * P;
  // Every phase derives its thread coordinates from an opaque copy of
  // threadIdx.x: the lane's MFMA operand coordinates (fi, fkc), its element of
  // a folded 4 x 16 group result (orow, oc).  Coordinates derived once would
  // be hoisted out of the iteration loop with everything computed from them,
  // and all phases' offsets would stay live at once (hundreds of VGPRs).
#define FZ_THREAD                                                    \
  const int tid = fz_opaque(threadIdx.x), lane = tid & 63;          \
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);         \
  const int fi = lane & 3, fkc = 4 * (lane >> 4) + ((lane >> 2) & 3); \
  const int orow = lane >> 4, oc = lane & 15;                        \
  (void)wave; (void)fi; (void)fkc; (void)orow; (void)oc

  double tr = 0.0;   // trace (eig_trace_kernel's order); wave 0 keeps it for the checks
  {
    FZ_THREAD;
    // start basis (eig_init_kernel's)
    for (int e = tid; e < mpad * P; e += 256) {
      const int row = e >> 4, c = e & 15;
      double v = 0.0;
      if (row < m) {
        if (c < kw) v = warm[(int64_t)row * kw + c];
        else if (c < p) v = hash_unit(seed, row, c);
      }
      sQ[fz_ix(row, c)] = v;
      sY[fz_ix(row, c)] = 0.0;
    }
    if (tid < 4 * P) s_tail[tid] = 0.0;
    if (tid < P) s_res[tid] = 0.0;
    if (tid <= kChebDMax) { s_ca[0][tid] = cc.c2[tid]; s_ca[1][tid] = cc.c4[tid]; }
    if (wave == 0) {
      for (int i = lane; i < m; i += 64) tr += Gr[(int64_t)i * ldg + i];
      tr = wave_sum(tr);
      if (lane == 0) { w.trace[rep] = tr; w.done[rep] = 0; }
    }
  }
  __syncthreads();
  // phase profile of replicate 0 (DFM_EIG_PROF): thread 0's wall clock at the
  // phase-ending barriers, summed per phase over the iterations
  const bool pf = prof && rep == 0;   // workgroup-uniform: the sums stay in SGPRs
  long long pt = pf ? wall_clock64() : 0, pacc[6] = {0, 0, 0, 0, 0, 0};
#define FZ_MARK(i)                                           \
  do {                                                       \
    if (pf) { const long long t_ = wall_clock64(); pacc[i] += t_ - pt; pt = t_; } \
  } while (0)

  int it = 0;
  for (;; ++it) {
    {
      FZ_THREAD;
      if (wave == 0) {
        const int d = check_converged<P>(w, s_tail, s_res, nullptr, tr, 0, rep, 0, 1, k, p, tol, it, 0);
        if (lane == 0) s_done = d;
      }
    }
    __syncthreads();
    FZ_MARK(0);
    if (s_done || it == maxit) break;   // converged, or the check-only pass after maxit steps

    {   // Y = G Q
      FZ_THREAD;
      constexpr int NG = OVL ? NG3 : NGW, NW = OVL ? 3 : 4;
      if (!OVL || wave < 3) {
        double acc[NG][4];
        fz_gemm<NG, NW>(Gr, ldg, m, ng, sQ, wave, lane, acc);
#pragma unroll
        for (int q = 0; q < NG; ++q) {
          const int g = wave + NW * q;
          if (g >= ng) continue;
          const double v = mm4_fold(acc[q], lane);
          const int row = 4 * g + orow;
          if (row < m) sY[fz_ix(row, oc)] = v;
        }
      } else {
        fz_xtx(sQ, sQ, sm.R2, mpad, lane);   // Q'Q
        wave_lds_sync();
        wave_chol_inv<P, true>(sm.R2, sm.R4, sm.dead, p);
      }
    }
    __syncthreads();
    FZ_MARK(1);

    {   // Q'Y -> R1, Y'Y -> R3 (and Q'Q -> R2 unless OVL formed it), stride P + 1, over all mpad rows
      FZ_THREAD;
      if (wave < (OVL ? 2 : 3)) {
        const double *X1 = wave == 1 ? sY : sQ, *X2 = wave == 2 ? sQ : sY;
        fz_xtx(X1, X2, wave == 0 ? sm.R1 : (wave == 1 ? sm.R3 : sm.R2), mpad, lane);
      }
    }
    __syncthreads();
    FZ_MARK(2);

    {
      FZ_THREAD;
      if (wave == 0) {
        if (pf) {   // stamps of the Rayleigh-Ritz stages (the last step's) after the phase sums
          EigWork wd = w;
          wd.dbg = prof + 8;
          small_rr<P>(sm, wd, rep, p, jsweeps | (OVL ? SMALL_CHOL1_DONE : SMALL_CHOL_OWN) | SMALL_STAGE_A, nullptr, s_tail);
        } else {
          small_rr<P>(sm, w, rep, p, jsweeps | (OVL ? SMALL_CHOL1_DONE : SMALL_CHOL_OWN) | SMALL_STAGE_A, nullptr, s_tail);
        }
      }
    }
    __syncthreads();
    FZ_MARK(3);

    // U pass (waves 1..3; A = R2, theta): U = Q A -> global, residual sums
    // of W = Y A - U diag(theta) — beside wave 0's chol(Z'Z) and Bm = R1
    {
      FZ_THREAD;
      if (wave == 0) {
        if (pf) {
          EigWork wd = w;
          wd.dbg = prof + 8;
          small_rr<P>(sm, wd, rep, p, jsweeps | SMALL_STAGE_B, nullptr, s_tail);
        } else {
          small_rr<P>(sm, w, rep, p, jsweeps | SMALL_STAGE_B, nullptr, s_tail);
        }
        if (lane < P) { s_rw[0][lane] = 0.0; s_uw[0][lane] = 0.0; }
      } else {
        double bA[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) bA[fb] = sm.R2[fkc * S + 4 * fb + fi];
        const double th_c = s_tail[oc];
        double rs = 0.0, us = 0.0;
#pragma unroll 1
        for (int g = wave - 1; g < ng; g += 3) {
          const int ra = 4 * g + fi;
          const double aq = sQ[fz_ix(ra, fkc)], ay = sY[fz_ix(ra, fkc)];
          double u4[4], ya4[4];
#pragma unroll
          for (int fb = 0; fb < 4; ++fb) {
            u4[fb] = mfma4(aq, bA[fb], 0.0);
            ya4[fb] = mfma4(ay, bA[fb], 0.0);
          }
          const double u = mm4_fold(u4, lane), ya = mm4_fold(ya4, lane);
          const int row = 4 * g + orow;
          if (row < m) {
            if (oc < k) { const double wv = ya - th_c * u; rs += wv * wv; us = fma(u, u, us); }
            Ur[(int64_t)row * P + oc] = u;
          }
        }
        rs += __shfl_xor(rs, 16);
        rs += __shfl_xor(rs, 32);
        us += __shfl_xor(us, 16);
        us += __shfl_xor(us, 32);
        if (lane < P) { s_rw[wave][lane] = rs; s_uw[wave][lane] = us; }
      }
    }
    __syncthreads();
    FZ_MARK(4);

    // next basis: V = Y Bm, V0 = Q Bm -> the filter's first Horner term S =
    // (a_d / b) V + a_{d-1} V0 into Y, V0 into Q (dead columns re-randomised)
    const int dg = (warm_strict && it < 4) ? kChebDirectStrict : 2;
    const double *ca = s_ca[dg == 2 ? 0 : 1];
    const double bch = filter_top(s_tail, k, p);
    {
      FZ_THREAD;
      if (tid < P)
        s_res[tid] = judged_residual(((s_rw[0][tid] + s_rw[1][tid]) + s_rw[2][tid]) + s_rw[3][tid],
                                     tid < k ? ((s_uw[0][tid] + s_uw[1][tid]) + s_uw[2][tid]) + s_uw[3][tid] : 1.0);
      const bool dead_c = oc < p && s_tail[P + oc] != 0.0;
      double bB[4];
#pragma unroll
      for (int fb = 0; fb < 4; ++fb) bB[fb] = sm.R1[fkc * S + 4 * fb + fi];
      const double fa1 = ca[dg], fa0 = ca[dg - 1];
#pragma unroll 1
      for (int g = wave; g < ng; g += 4) {
        const int ra = 4 * g + fi;
        const double aq = sQ[fz_ix(ra, fkc)], ay = sY[fz_ix(ra, fkc)];
        double qn4[4], qb4[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
          qn4[fb] = mfma4(ay, bB[fb], 0.0);
          qb4[fb] = mfma4(aq, bB[fb], 0.0);
        }
        double qn = mm4_fold(qn4, lane), qb = mm4_fold(qb4, lane);
        const int row = 4 * g + orow;
        if (dead_c) qn = hash_unit(seed, row, 1000003ull * (it + 1) + oc);
        if (oc >= p) { qn = 0.0; qb = 0.0; }
        if (row < m) {
          const double sv = dead_c ? qn : (bch > 0.0 ? fma(fa1 / bch, qn, fa0 * qb) : qn);
          sY[fz_ix(row, oc)] = oc >= p ? 0.0 : sv;
          sQ[fz_ix(row, oc)] = oc >= p ? 0.0 : (dead_c ? qn : qb);
        }
      }
    }
    __syncthreads();

    // Chebyshev filter: S_{dg-1} in Y; S_i = G S_{i+1} / b + a_i V0; S_0 into Q
    const double cb = bch > 0.0 ? 1.0 / bch : 1.0;
    for (int j = 1; j < dg; ++j) {
      const double cv0 = bch > 0.0 ? ca[dg - 1 - j] : 0.0;
      const bool last = j == dg - 1;
      double *So = last ? sQ : sY;
      FZ_THREAD;
      double acc[NGW][4];
      fz_gemm<NGW, 4>(Gr, ldg, m, ng, sY, wave, lane, acc);
      if (!last) __syncthreads();   // every wave has read S_{i+1} before S_i overwrites it
      const bool dead_c = oc < p && s_tail[P + oc] != 0.0;
#pragma unroll
      for (int q = 0; q < NGW; ++q) {
        const int g = wave + 4 * q;
        if (g >= ng) continue;
        const double gv = mm4_fold(acc[q], lane);
        const int row = 4 * g + orow;
        if (row < m) {
          const int ix = fz_ix(row, oc);
          const double v0 = sQ[ix];
          double sn = dead_c ? v0 : fma(cb, gv, cv0 * v0);
          if (oc >= p) sn = 0.0;
          So[ix] = sn;
        }
      }
      __syncthreads();
    }
    FZ_MARK(5);
  }
  // the last apply's Ritz vectors (this workgroup's own global writes: the
  // barrier that ended the iteration makes them visible) -> signs, outputs
  if (!s_done && threadIdx.x == 0) w.iters[rep] = it;   // not converged: it == maxit (check_converged's check-only record)
  eig_final_body<P>(Ur, s_tail, s_done, rep, m, k, lam, Uk, status);
  if (pf && threadIdx.x == 0) {
    for (int i = 0; i < 6; ++i) prof[i] = pacc[i];
    prof[6] = it;
    prof[7] = wall_clock64() - pt;   // the final step
  }
#undef FZ_MARK
#undef FZ_THREAD
}

static int fused_ngw(int m) { return m <= 64 ? 4 : (m <= 144 ? 9 : (m <= 256 ? 16 : 0)); }
static bool fused_enabled() {
  static const bool on = [] { const char *e = getenv("DFM_EIG_FUSED"); return !(e && atoi(e) == 0); }();
  return on;
}

// Solve nb problems.  Returns 0 ok, 1 not converged (status per replicate),
// negative on bad args, or a hipError_t (>1000).
template <int P>
static int eig_run_t(const double *G, int64_t ldg, int64_t strideG, int m, const EigArgs &a, int *iters_host,
                     int64_t rep0) {
  const int nb = a.nb, k = a.k, p = a.p, kw = a.kw, maxit = a.maxit, poll = a.poll;
  const double *warm = a.warm;
  const double tol = a.tol;
  double *lam = a.lam, *Uk = a.Uk, *trace_out = a.trace_out;
  int *status = a.status;
  hipStream_t st = a.st;
  const int nrb = (m + EROWS - 1) / EROWS;
  EigWork w = carve(a.ws, m, nb, P, maxit);
  w.subspace = a.subspace;
  hipMemsetAsync(w.active, 0, (size_t)(maxit + 2) * 4, st);
  hipMemsetAsync(w.iters, 0, (size_t)nb * 4, st);
  const uint64_t seed = 0x5eed0000ull + (uint64_t)m * 131 + k;
  // degree: 4 for the first four filters of a warm-started batch or a single
  // fit under the strict eigenvector rule (C2's Chow statistics: 8-9
  // Rayleigh-Ritz steps with degree 2, 5 with degree 4 in tools/eig_proto.py),
  // 2 for the polishing steps after them and for eigenvalue-only solves
  // (single fits, nb = 1, too: cold-started, polished to 1e-14 by run_eig)
  const bool warm_strict = tol >= 0.0 && ((warm && kw >= k) || nb == 1);
  if constexpr (P == 16) {
    const int ngw = (a.fused < 0 ? fused_enabled() : a.fused != 0) ? fused_ngw(m) : 0;
    if (ngw) {
      ChebCo cc;
      shifted_cheb(kChebDirectStrict, cc.c4);
      shifted_cheb(2, cc.c2);
      const size_t lds = (size_t)2 * ((m + 15) & ~15) * P * sizeof(double);
      // DFM_EIG_PROF=1: phase profile of replicate 0 of every fused solve -> stderr
      static const bool want_prof = [] { const char *e = getenv("DFM_EIG_PROF"); return e && atoi(e) != 0; }();
      long long *prof = nullptr;
      if (want_prof) {
        static thread_local long long *buf = nullptr;
        if (!buf && hipMalloc((void **)&buf, 24 * sizeof(long long)) != hipSuccess) buf = nullptr;
        prof = buf;
      }
#define DFM_FUSED(...)                                                                                          \
  hipFuncSetAttribute((const void *)eig_fused_kernel<__VA_ARGS__>, hipFuncAttributeMaxDynamicSharedMemorySize,    \
                      (int)lds);                                                                                  \
  hipLaunchKernelGGL((eig_fused_kernel<__VA_ARGS__>), dim3(nb), dim3(256), lds, st, G, ldg, strideG, w, m, k, p, tol, \
                     maxit, warm, kw, seed, (int)warm_strict, fused_sweeps(), cc, lam, Uk, status, prof)
      { TimerScope ts(a, DFM_KC_EIG_GQ);
        if (ngw == 4) { DFM_FUSED(4, 6, true); }
        else if (ngw == 9) { DFM_FUSED(9, 12, true); }
        else { DFM_FUSED(16, 22, false); }
      }
#undef DFM_FUSED
      // iteration statistics from the per-iteration unconverged counts
      std::vector<int> act((size_t)maxit + 2, 0);
      hipMemcpyAsync(act.data(), w.active, act.size() * 4, hipMemcpyDeviceToHost, st);
      hipError_t e = hipStreamSynchronize(st);
      if (e != hipSuccess) return 1000 + (int)e;
      int last = maxit;
      for (int i = 0; i <= maxit; ++i)
        if (act[i] == 0) { last = i; break; }
      g_last_iters = last;
      // act[i] replicates took Rayleigh-Ritz step i, each with dg(i) products
      // G S (Y = G Q and the filter's dg - 1 Horner steps)
      int64_t s = 0, prods = 0;
      for (int i = 0; i <= std::min(last, maxit - 1); ++i) {
        s += act[i];
        prods += (int64_t)act[i] * ((warm_strict && i < 4) ? kChebDirectStrict : 2);
      }
      g_last_rep_iters = s;
      g_last_gemm_products = prods;
      g_last_gemm_products_f32 = g_last_gemm_products_split_last = g_last_gemm_products_split3 = 0;
      if (prof) {
        long long h[24];
        hipMemcpy(h, prof, sizeof(h), hipMemcpyDeviceToHost);
        const long long *d = h + 8;   // small_rr stamps 1..10, sweeps at 15
        fprintf(stderr, "eig_fused small stages us: chol1=%.2f mm=%.2f jacobi(%lld sweeps)=%.2f sort=%.2f mm3=%.2f "
                "chol2=%.2f mm=%.2f\n", (d[2] - d[1]) / 100.0, (d[4] - d[3]) / 100.0, d[15], (d[5] - d[4]) / 100.0,
                (d[6] - d[5]) / 100.0, (d[7] - d[6]) / 100.0, (d[8] - d[7]) / 100.0, (d[10] - d[9]) / 100.0);
        fprintf(stderr, "eig_fused m=%d nb=%d rep0: iters=%lld us check=%.1f gq=%.1f part=%.1f small=%.1f apply=%.1f "
                "cheb=%.1f final=%.1f\n", m, nb, h[6], h[0] / 100.0, h[1] / 100.0, h[2] / 100.0, h[3] / 100.0,
                h[4] / 100.0, h[5] / 100.0, h[7] / 100.0);
      }
      if (trace_out) hipMemcpyAsync(trace_out, w.trace, (size_t)nb * 8, hipMemcpyDeviceToDevice, st);
      if (iters_host) hipMemcpyAsync(iters_host, w.iters, (size_t)nb * 4, hipMemcpyDeviceToHost, st);
      e = hipGetLastError();
      if (e != hipSuccess) return 1000 + (int)e;
      return 0;
    }
  }
  { TimerScope ts(a, DFM_KC_EIG_OTHER);
    const int64_t n = (int64_t)m * P;
    dim3 grid((unsigned)((n + 255) / 256), nb);
    hipLaunchKernelGGL(eig_init_kernel<P>, grid, dim3(256), 0, st, w.Q, m, p, warm, kw, w.done, seed, rep0);
    hipLaunchKernelGGL(eig_trace_kernel, dim3(nb), dim3(64), 0, st, G, ldg, strideG, m, w.trace);
  }
  int it = 0;
  const int cheb = 1;   // Chebyshev filter between Rayleigh-Ritz steps
  double ca4[kChebDMax + 1], ca2[kChebDMax + 1];
  shifted_cheb(kChebDirectStrict, ca4);
  shifted_cheb(2, ca2);
  int next_poll = poll;
  for (; it <= maxit; ++it) {
    const int dg = warm_strict && it < 4 ? kChebDirectStrict : 2;
    const double *ca = dg == 2 ? ca2 : ca4;
    const int check_only = (it == maxit);
    { TimerScope ts(a, DFM_KC_EIG_GQ);
      hipLaunchKernelGGL(eig_gq_kernel<P>, dim3(nrb, nb), dim3(256), 0, st, G, ldg, strideG, w, m, k,
                         p, tol, it, check_only);
    }
    if (check_only) break;
    { TimerScope ts(a, DFM_KC_EIG_SMALL);
      hipLaunchKernelGGL(eig_small_kernel<P>, dim3(nb), dim3(64), 0, st, w, p, nrb, kJacobiSweeps | SMALL_CHOL_OWN);
    }
    { TimerScope ts(a, DFM_KC_EIG_APPLY);
      hipLaunchKernelGGL(eig_apply_kernel<P>, dim3(nrb, nb), dim3(256), 0, st, w, m, p, k, it, seed, rep0, cheb,
                         ca[dg], ca[dg - 1]);
      for (int j = 1; cheb && j < dg; ++j) {   // S_{dg-1-j}: in w.Y / w.S alternately, S_0 into w.Q
        const double *sin = (j & 1) ? w.Y : w.S;
        double *sout = j == dg - 1 ? w.Q : ((j & 1) ? w.S : w.Y);
        hipLaunchKernelGGL(eig_cheb_kernel<P>, dim3(nrb, nb), dim3(256), 0, st, G, ldg, strideG, w, m, k, p, sin, sout,
                           ca[dg - 1 - j]);
      }
    }
    if (it == next_poll) {
      int act = -1;
      hipMemcpyAsync(&act, w.active + it, 4, hipMemcpyDeviceToHost, st);
      hipError_t e = hipStreamSynchronize(st);
      if (e != hipSuccess) return 1000 + (int)e;
      if (act == 0) break;
      // a straggler tail (< 1/8 of the batch active): poll every step, so the
      // empty iterations after its last replicate retires are not launched
      next_poll = it + ((int64_t)act * 8 < nb ? 1 : poll);
    }
  }
  g_last_iters = it;
  g_last_rep_iters = count_rep_iters(w.active, std::min(it, maxit - 1), 0, nb, st);
  g_last_gemm_products = g_last_rep_iters;
  g_last_gemm_products_f32 = g_last_gemm_products_split_last = g_last_gemm_products_split3 = 0;
  { TimerScope ts(a, DFM_KC_EIG_OTHER);
    hipLaunchKernelGGL(eig_final_kernel<P>, dim3(nb), dim3(256), 0, st, w, m, k, lam, Uk, status, trace_out);
  }
  if (iters_host) {
    hipMemcpyAsync(iters_host, w.iters, (size_t)nb * 4, hipMemcpyDeviceToHost, st);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return 1000 + (int)e;
  return 0;
}

// A requested block below k + 1 is raised to k + 1: the Chebyshev filter's
// interval [0, theta_p] must lie below every wanted eigenvalue, so the block
// needs at least one guard vector (p == k: theta_p is the k-th WANTED value
// and the filter stops amplifying it — the k-th vector then never converges)
int eig_block_p(int m, int k, int req) {
  int p = req > 0 ? std::max(req, k + 1) : std::max(k + 8, 16);
  p = std::min(p, m);
  return p;
}

// Block of the factored bootstrap solver (N > T, eig_run_fact2_t): k + 4
// columns, at least 8 (C3: 12 instead of the explicit-Gram solvers' 16).  The
// H.Z GEMM's work and the Z / HZ traffic scale with the block (Z, HZ hold it
// compactly, rounded up to even), and the Chebyshev filter does the damping
// that extra guard vectors would otherwise buy: tools/eig_proto.py at C3
// (warm start + the degree-6 first filter) retires 94 % of replicates at the
// 2nd Rayleigh-Ritz step with 12 columns (7.12 products) as with 16 (7.00).
// A requested block (dfm_ctx_set_eig_params) is taken as for the other
// solvers; DFM_FACT_GUARD (A/B) overrides the 4.
int fact_block_p(int m, int k, int req) {
  if (req > 0) return eig_block_p(m, k, req);
  static const int guard = [] { const char *e = getenv("DFM_FACT_GUARD"); return e ? atoi(e) : 4; }();
  if (guard <= 0) return eig_block_p(m, k, 0);
  return std::min(m, std::max(k + guard, 8));
}

int eig_run(const double *G, int64_t ldg, int64_t strideG, int m, const EigArgs &a, int *iters_host, int64_t rep0) {
  if (a.p < a.k || a.p > 32 || a.p > m) return -1;
  if (a.p <= 16) return eig_run_t<16>(G, ldg, strideG, m, a, iters_host, rep0);
  return eig_run_t<32>(G, ldg, strideG, m, a, iters_host, rep0);
}

// the kernels the factored solver (dfm_fact.hip) launches too
DFM_EIG_SHARED_KERNELS(template, 16)
DFM_EIG_SHARED_KERNELS(template, 32)

}  // namespace dfm
