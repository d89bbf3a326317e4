// dfm_chow.hip — Breitung–Eickmeier (2011) Chow tests for ALL variables at
// once (src/chowtest.jl:4-42), and hard-threshold targeted predictors
// (src/targeted_predictors.jl:9-30).
//
// Chow, per replicate, with F (T x r), break period bp (rows < bp | >= bp),
// d_t = 1{t >= bp}, D = [F, F.*d]:
//   A1 = F1'F1, A2 = F2'F2, D'D = M = [[A1+A2, A2], [A2, A2]]      (shared)
//   per variable i (one thread): g_j = F_j' x_i^(j), two passes over x_i
//   LR  = T (ln ||E_i||^2 - ln(SSR_1 + SSR_2)), SSR_j of x_i on F_j     (:19-23)
//   LM  = T (D'E_i)' M^-1 (D'E_i) / ||E_i||^2, D'E_i = [F'E_i; c],
//         c = g2 - A2 l_i: the uncentred R^2 of :35-42.  F'E_i = 0 only for
//         exact eigenvectors; the eigensolver leaves a residual, so the
//         first block is kept (cf = g1 + g2 - (A1 + A2) l_i)
//   ||E_i||^2 and the subperiod SSRs are summed explicitly (no cancellation)
//   A model fitted with break_indices (src/DynamicFactorModel.jl:73, :98)
//   has one loadings matrix per break block: E_i = x_i - F_t l_i^(block(t)),
//   and F = vcat(F_j) (defect D1): D'E_i = [sum_t f_t e_ti; sum_{t >= bp}
//   f_t e_ti], both summed explicitly.
//   Wald: beta = M^-1 [g1+g2; g2]; HC0 meat; with W = M^-1[:, r:] = [Wa; Wb]
//         Cov22 = sum_t u_t^2 z_t z_t',  z_t = Wa'f_t (t < bp), (Wa+Wb)'f_t
//         (t >= bp) — one r x r accumulator per variable instead of the
//         reference's T x T diagm sandwich (:25-33).
#include <algorithm>

#include "dfm_internal.h"
#include "dfm_small.h"

namespace dfm {

constexpr int CH_RMAX = 16;
constexpr int CH_BMAX = 64;   // break blocks of a Chow call

// Row ranges of the model's break blocks: block j is rows a[j] .. a[j+1]-1,
// its loadings at Lm + j * lbs (+ replicate stride N r).
struct ChowBlocks {
  int n;
  int a[CH_BMAX + 1];
  int64_t lbs;
};

// Per replicate, written by chow_prep_kernel: nine RC x RC matrices (RC =
// the Chow kernel's padded factor count 4 / 8 / 16, zero outside r),
// back to back — A1^-1, A2^-1, A2, A1 + A2 and the blocks of M^-1 below —
// so the kernel reads them at small immediate offsets from one base (the
// 16 x 16-padded layout of round 3 needed a 64-bit address per element and
// the compiler spilled them).
enum { CP_A1I = 0, CP_A2I, CP_A2, CP_APS, CP_VA, CP_VC, CP_WA, CP_WC, CP_WB, CP_NMAT };
constexpr size_t CH_PREP_BYTES = (size_t)CP_NMAT * CH_RMAX * CH_RMAX * 8;

size_t chow_workspace_bytes(int T, int N, int r, int nb) {
  return (size_t)nb * CH_PREP_BYTES + (size_t)nb * T * r * 8 + (size_t)3 * nb * N * 8 + 4096;
}

__global__ __launch_bounds__(256) void chow_prep_kernel(const double *__restrict__ F, int T, int r,
                                                        int bp, int RC, double *__restrict__ prep,
                                                        double *__restrict__ Z) {
  constexpr int S = 2 * CH_RMAX + 1;
  __shared__ double A1[CH_RMAX * S], A2s[CH_RMAX * S], M[2 * CH_RMAX * S], Mi[2 * CH_RMAX * S],
      Lw[2 * CH_RMAX * S], Tw[2 * CH_RMAX * S], A1i[CH_RMAX * S], A2i[CH_RMAX * S], Lw1[CH_RMAX * S],
      Tw1[CH_RMAX * S], Lw2[CH_RMAX * S], Tw2[CH_RMAX * S];
  __shared__ int bad;
  const int tid = threadIdx.x, rep = blockIdx.x;
  const double *Fr = F + (int64_t)rep * T * r;
  if (tid == 0) bad = 0;
  // A1 = F1'F1, A2 = F2'F2: the 2 r^2 entries x ns row strips over the
  // threads (C2, r = 3: 18 entries x 14 strips — one entry per thread made 18
  // T/2-long dependent chains the whole workgroup waited on); each strip's
  // partial sum in LDS, then the strips summed in order (fixed order:
  // per-replicate, batch-invariant)
  const int ne = 2 * r * r, ns = ne >= 256 ? 1 : 256 / ne, nst = ne < 256 ? ne : 256;
  for (int e0 = 0; e0 < ne; e0 += 256) {
    const int e = e0 + tid % ne, sp = tid / ne;
    if (e0 + tid < ne * ns && (ns > 1 || e < ne)) {
      const int which = e / (r * r), a = (e / r) % r, c = e % r;
      const int t0 = which ? bp : 0, t1 = which ? T : bp, len = t1 - t0;
      const int q0 = t0 + (int)((int64_t)len * sp / ns), q1 = t0 + (int)((int64_t)len * (sp + 1) / ns);
      // 16 rows' operands loaded before their (in-order) products
      constexpr int PU = 16;
      double sacc = 0.0;
      for (int tb = q0; tb < q1; tb += PU) {
        double fa[PU], fc[PU];
#pragma unroll
        for (int u = 0; u < PU; ++u) {
          const int t = min(tb + u, q1 - 1);
          fa[u] = Fr[(int64_t)t * r + a];
          fc[u] = Fr[(int64_t)t * r + c];
        }
#pragma unroll
        for (int u = 0; u < PU; ++u)
          if (tb + u < q1) sacc = fma(fa[u], fc[u], sacc);
      }
      Tw[sp * nst + e - e0] = sacc;   // (Tw: scratch until the inverses below; < 256 entries)
    }
    __syncthreads();
    if (tid < min(256, ne - e0)) {
      const int e = e0 + tid;
      const int which = e / (r * r), a = (e / r) % r, c = e % r;
      double sacc = 0.0;
      for (int q = 0; q < ns; ++q) sacc += Tw[q * nst + tid];
      (which ? A2s : A1)[a * S + c] = sacc;
    }
    __syncthreads();
  }
  __syncthreads();
  const int n2 = 2 * r;
  for (int e = tid; e < n2 * n2; e += 256) {
    const int a = e / n2, c = e % n2;
    const double v = (a < r && c < r) ? A1[a * S + c] + A2s[a * S + c] : A2s[(a % r) * S + (c % r)];
    M[a * S + c] = v;
  }
  __syncthreads();
  // the three inverses side by side on waves 0..2 (one after another across
  // the workgroup they were ~40 barriers)
  {
    const int wv = tid >> 6;
    if (wv == 0) wave_spd_inverse(M, Mi, Lw, Tw, n2, S, &bad);
    else if (wv == 1) wave_spd_inverse(A1, A1i, Lw1, Tw1, r, S, &bad);
    else if (wv == 2) wave_spd_inverse(A2s, A2i, Lw2, Tw2, r, S, &bad);
  }
  __syncthreads();
  double *P = prep + (size_t)rep * CP_NMAT * RC * RC;
  // every entry is written (zeros outside r): the main kernel reads RC x RC blocks
  for (int e = tid; e < RC * RC; e += 256) {
    const int a = e / RC, c = e % RC;
    const bool in = a < r && c < r;
    const int q = RC * RC;
    P[CP_A1I * q + e] = in ? A1i[a * S + c] : 0.0;
    P[CP_A2I * q + e] = in ? A2i[a * S + c] : 0.0;
    P[CP_A2 * q + e] = in ? A2s[a * S + c] : 0.0;
    P[CP_APS * q + e] = in ? A1[a * S + c] + A2s[a * S + c] : 0.0;
    // Mi = [[P11, P12], [P21, P22]]:  beta1 = P11 g1 + (P11 + P12) g2,
    // beta2 = P21 g1 + (P21 + P22) g2 (stored transposed-ready, see kernel)
    P[CP_VA * q + e] = in ? Mi[a * S + c] : 0.0;
    P[CP_VC * q + e] = in ? Mi[a * S + c] + Mi[(r + a) * S + c] : 0.0;
    P[CP_WA * q + e] = in ? Mi[a * S + r + c] : 0.0;
    P[CP_WC * q + e] = in ? Mi[a * S + r + c] + Mi[(r + a) * S + r + c] : 0.0;
    P[CP_WB * q + e] = in ? Mi[(r + a) * S + r + c] : 0.0;
  }
  (void)bad;   // (a singular M leaves inf / NaN statistics, as the reference's inv)
  // z_t = Wa' f_t (t < bp) or Wc' f_t (t >= bp)
  for (int e = tid; e < T * r; e += 256) {
    const int t = e / r, j = e % r;
    double s = 0.0;
    for (int a = 0; a < r; ++a) {
      const double wv = (t < bp) ? Mi[a * S + r + j] : Mi[a * S + r + j] + Mi[(r + a) * S + r + j];
      s = fma(wv, Fr[(int64_t)t * r + a], s);
    }
    Z[(int64_t)rep * T * r + e] = s;
  }
}

// FLAT = false: one thread per variable, grid (variable blocks, replicate);
// the block is sized to the panel width (64 .. 256).  FLAT = true (R <= 8, N
// wide enough that a block spans <= CH_FLAT_REPS replicates): one
// thread per (replicate, variable) pair in replicate-major order, so the lanes
// of a 256-thread block run on into the next replicate's variables instead of
// idling at the panel edge (C2, N = 130: 3 waves per replicate of which 62
// lanes idle -> 2.03 waves); a block spans at most CH_FLAT_REPS replicates,
// each with its own staged F, Z, eta and idx rows.  Both read the small
// prep matrices from global memory (L1/L2).  Per (replicate, variable) the
// arithmetic and its order are the same in both forms.
constexpr int CH_FLAT_REPS = 4;   // flat when ceil(256 / KS / N) + 1 <= 4 (N >= 86 at KS = 1)
//
// KS > 1 (R <= 4): KS lanes per (replicate, variable), lane k taking rows
// t = t0 + k, t0 + k + KS, ... of every staged tile; the per-lane partial sums
// (pass A's F'x, ||E_i||^2, pass B's SSR and HC0 block) are combined across
// the KS lanes by xor shuffles in a fixed order before they are used.  A
// C2-sized job (500 replicates x 130 variables) is then 4 waves per SIMD
// instead of one — the kernel is latency-bound (a dependent chain per
// accumulator over T rows), not VALU-bound.
#ifndef DFM_CH_KS   // (A/B builds: make EXTRA="-DDFM_CH_KS=1 -DDFM_CH_WAVES=2")
#define DFM_CH_KS 2
#endif
#ifndef DFM_CH_WAVES
#define DFM_CH_WAVES 3
#endif
constexpr int CH_KS = DFM_CH_KS;
template <int R, int KS>
constexpr int chow_waves() { return (R <= 4 && KS > 1) ? DFM_CH_WAVES : (R <= 8 ? 2 : 1); }
// x[a] / x[a] := v for a runtime a, by compile-time indices (no scratch)
template <int R>
DFM_DEV double rsel(const double (&x)[R], int a) {
  double v = x[0];
#pragma unroll
  for (int j = 1; j < R; ++j) v = a == j ? x[j] : v;
  return v;
}
template <int R>
DFM_DEV void rput(double (&x)[R], int a, double v) {
#pragma unroll
  for (int j = 0; j < R; ++j) x[j] = a == j ? v : x[j];
}
template <int KS>
DFM_DEV double ks_sum(double v) {
  if constexpr (KS >= 2) v += __shfl_xor(v, 1);
  if constexpr (KS >= 4) v += __shfl_xor(v, 2);
  return v;
}

template <int R, bool HAS_C, bool HAS_ETA, bool HAS_IDX, bool BRK, bool FLAT = false, int KS = 1>
__global__ __launch_bounds__(256, (chow_waves<R, KS>())) void chow_all_kernel(PanelSrc src, ChowBlocks blk, int T, int N, int r, int bp,
                                                       int nb, const double *__restrict__ F,
                                                       const double *__restrict__ Z,
                                                       const double *__restrict__ prep,
                                                       const double *__restrict__ Lm,
                                                       double *__restrict__ LR,
                                                       double *__restrict__ LM,
                                                       double *__restrict__ WD, double *__restrict__ LRo,
                                                       double *__restrict__ LMo, double *__restrict__ WDo,
                                                       int64_t os) {
#ifndef DFM_CH_TR   // (A/B builds: rows per staged tile)
#define DFM_CH_TR 128
#endif
  constexpr int TR = DFM_CH_TR;
  // rows whose gathered values are in flight together: 16, or 8 at R = 8,
  // whose per-variable state (36 HC0 sums, four R-vectors of coefficients)
  // already fills most of the 2-wave register budget.  The launch bound keeps
  // R <= 8 at 2 waves per SIMD (256 registers): what the per-variable state
  // does not fit is spilled once per thread around pass B, not inside the row
  // loops — unbounded, the compiler took 256 VGPRs + 76 AGPRs at R = 4 and ran
  // one wave per SIMD
#ifndef DFM_CH_CU   // (A/B builds: rows per gather round at KS > 1)
#define DFM_CH_CU 8
#endif
  constexpr int CU = KS > 1 ? DFM_CH_CU : (R <= 4 ? 16 : (R <= 8 ? 8 : 16));
  constexpr int NR = FLAT ? CH_FLAT_REPS : 1;   // replicates staged per block
  __shared__ double sF[NR][TR * R], sZ[NR][TR * R], sE[NR][TR];
  __shared__ unsigned sI[NR][TR];   // byte offset of the row's E row (idx_t ld 8)
  const int tid = threadIdx.x, nth = blockDim.x, ks = tid % KS;
  int rep, i, rep0, nrw;
  if constexpr (FLAT) {   // (replicate, variable) pairs, KS threads each
    const int64_t g = ((int64_t)blockIdx.x * nth + tid) / KS, g0 = (int64_t)blockIdx.x * nth / KS;
    rep = (int)(g / N); i = (int)(g % N);
    rep0 = (int)(g0 / N);
    nrw = min(nb - 1, (int)((g0 + nth / KS - 1) / N)) - rep0 + 1;
  } else {
    rep = blockIdx.y; i = (blockIdx.x * nth + tid) / KS; rep0 = rep; nrw = 1;
  }
  const bool ok = FLAT ? rep < nb : i < N;
  const int lr = FLAT ? (ok ? rep - rep0 : 0) : 0;   // this thread's staged replicate
  if (!ok) i = 0;   // (idle lanes gather a valid column; they write nothing)
  const unsigned ld8 = (unsigned)src.ld * 8u, i8 = (unsigned)i * 8u;
  // this pair's replicate's prep block (matrix m at Pc + m R^2, row-major R x R)
  const double *Pc = prep + (size_t)(ok ? rep : rep0) * CP_NMAT * R * R;
  auto PM = [&](int m, int a, int c) -> double { return Pc[m * R * R + a * R + c]; };
  auto stage = [&](int t0) {
    for (int e = tid; e < nrw * TR * R; e += nth) {
      const int q = e / (TR * R), f = e % (TR * R), rr = f / R, j = f % R, t = t0 + rr;
      const int64_t base = (int64_t)(rep0 + q) * T * r;
      sF[q][f] = (t < T && j < r) ? F[base + (int64_t)t * r + j] : 0.0;
      sZ[q][f] = (t < T && j < r) ? Z[base + (int64_t)t * r + j] : 0.0;
    }
    for (int e = tid; e < nrw * TR; e += nth) {
      const int q = e / TR, rr = e % TR, t = t0 + rr;
      const int64_t ro = (int64_t)(rep0 + q) * src.rs;
      sE[q][rr] = (HAS_ETA && t < T) ? src.eta[ro + t] : 1.0;
      sI[q][rr] = t < T ? (unsigned)(HAS_IDX ? src.idx[ro + t] : t) * ld8 : 0u;
    }
  };
  // CU rows' gathered values x = C + eta E[idx]: the staged row indices
  // first, then every row's loads, then the arithmetic — all 2 CU loads in
  // flight together (computing each row's x as its loads arrive made the
  // compiler wait for every row's loads before the next row's issued)
  // (this lane's rows of the tile: rb, rb + KS, ..., rb + (CU - 1) KS)
  // Addresses: 32-bit byte offsets from the uniform panel bases (the launcher
  // checks T ld 8 < 2^32) — the staged E-row offsets plus 8 i, the C row
  // offsets stepping by KS ld 8 — so a row costs two 32-bit adds, not the
  // 64-bit index products that were a third of the loop's instructions.
  auto load_rows = [&](int t0, int rb, int tn, double *xs) {
    unsigned ro[CU];
    double ee[CU], cc[CU];
#pragma unroll
    for (int u = 0; u < CU; ++u) ro[u] = sI[lr][min(rb + KS * u, tn - 1)] + i8;
    unsigned co = (unsigned)(t0 + rb) * ld8 + i8;
#pragma unroll
    for (int u = 0; u < CU; ++u) {
      ee[u] = *(const double *)((const char *)src.E + ro[u]);
      if (HAS_C) cc[u] = *(const double *)((const char *)src.C + (rb + KS * u < tn ? co : (unsigned)(t0 + tn - 1) * ld8 + i8));
      co += KS * ld8;
    }
#pragma unroll
    for (int u = 0; u < CU; ++u) {
      double x = ee[u];
      if (HAS_ETA) x *= sE[lr][min(rb + KS * u, tn - 1)];
      if (HAS_C) x += cc[u];
      xs[u] = x;
    }
  };
  // 1: every row of this wave's batch (rows rb, rb + KS, .. of the tile) is
  // before bp, 2: every row at or after bp, 0: mixed (a wave vote)
  auto batch_side = [&](int t0, int rb, int tn) {
    const int ta = t0 + rb, tb = t0 + min(rb + KS * (CU - 1), tn - 1);
    if (!__any(ok && tb >= bp)) return 1;
    if (!__any(ok && ta < bp)) return 2;
    return 0;
  };
  // loadings of variable i (src/chowtest.jl uses dfm.factor_residuals = x - F L')
  // (break models: block b's loadings for rows a[b] .. a[b+1]-1)
  double l[R];
  auto load_l = [&](int b) {
#pragma unroll
    for (int j = 0; j < R; ++j) l[j] = (ok && j < r) ? Lm[b * blk.lbs + ((int64_t)rep * N + i) * r + j] : 0.0;
  };
  load_l(0);
  int cb = 0, next = BRK ? blk.a[1] : T;
  // ---- pass A: g_j = F_j' x^(j), e2 = ||x - F l||^2 (BRK: cx = sum_{t>=bp} f_t e_t)
  // gc: the accumulator of the current side — g1's until the first batch
  // wholly at or after bp, then (g1 saved) g2's — so the all-pre and all-post
  // batches share one loop body with no branch; only the one mixed batch
  // selects per row.  (One per-row if / else over the three cases compiled
  // to a divergent branch whose arms shuttled g1 / g2 through ~15 register
  // copies per row.)  Same sums in the same order.
  double g1[R], g2[R], gc[R], cx[R], cf[R], e2 = 0.0;
  bool post_a = false;
#pragma unroll
  for (int j = 0; j < R; ++j) { g1[j] = 0.0; g2[j] = 0.0; gc[j] = 0.0; cx[j] = 0.0; cf[j] = 0.0; }
  for (int t0 = 0; t0 < T; t0 += TR) {
    __syncthreads();
    stage(t0);
    __syncthreads();
    if (!ok) continue;
    const int tn = min(TR, T - t0);
    // CU rows per round: every row's gathered x loaded before the sums (CU
    // loads in flight per thread).  (Prefetching the next round's rows into a
    // second register set was measured: at 3 waves per SIMD it spills, and a
    // copy between the sets waits for the prefetched loads.)
    for (int rb = ks; rb < tn; rb += KS * CU) {
      double xs[CU];
      load_rows(t0, rb, tn, xs);
      const int side = batch_side(t0, rb, tn);   // wave-uniform
      if (side == 2 && !post_a) {
#pragma unroll
        for (int j = 0; j < R; ++j) { g1[j] = gc[j]; gc[j] = g2[j]; }
        post_a = true;
      }
      if (side == 0) {   // the mixed batch (gc holds g1's sums)
#pragma unroll
        for (int u = 0; u < CU; ++u) {
          const int rr = rb + KS * u;
          if (rr < tn) {   // (a guard, not a break: the loop must unroll)
          const int t = t0 + rr;
          if (BRK && t >= next) { while (t >= next) { ++cb; next = blk.a[cb + 1]; } load_l(cb); }
          const double x = xs[u];
          double fr[R];
#pragma unroll
          for (int j = 0; j < R; ++j) fr[j] = sF[lr][rr * R + j];
          double ev = x;
#pragma unroll
          for (int j = 0; j < R; ++j) ev -= fr[j] * l[j];
          e2 = fma(ev, ev, e2);
          if (BRK) {
#pragma unroll
            for (int j = 0; j < R; ++j) cf[j] = fma(ev, fr[j], cf[j]);
          }
          if (BRK && t >= bp) {
#pragma unroll
            for (int j = 0; j < R; ++j) cx[j] = fma(ev, fr[j], cx[j]);
          }
          const bool pre = t < bp;
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const double a1 = fma(x, fr[j], gc[j]), a2 = fma(x, fr[j], g2[j]);
            gc[j] = pre ? a1 : gc[j];
            g2[j] = pre ? g2[j] : a2;
          }
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < CU; ++u) {
          const int rr = rb + KS * u;
          if (rr < tn) {
          const int t = t0 + rr;
          if (BRK && t >= next) { while (t >= next) { ++cb; next = blk.a[cb + 1]; } load_l(cb); }
          const double x = xs[u];
          double fr[R];
#pragma unroll
          for (int j = 0; j < R; ++j) fr[j] = sF[lr][rr * R + j];
          double ev = x;
#pragma unroll
          for (int j = 0; j < R; ++j) ev -= fr[j] * l[j];
          e2 = fma(ev, ev, e2);
          if (BRK) {
#pragma unroll
            for (int j = 0; j < R; ++j) cf[j] = fma(ev, fr[j], cf[j]);
          }
          if (BRK && t >= bp) {
#pragma unroll
            for (int j = 0; j < R; ++j) cx[j] = fma(ev, fr[j], cx[j]);
          }
#pragma unroll
          for (int j = 0; j < R; ++j) gc[j] = fma(x, fr[j], gc[j]);
          }
        }
      }
    }
  }
  if (post_a) {
#pragma unroll
    for (int j = 0; j < R; ++j) g2[j] = gc[j];
  } else {
#pragma unroll
    for (int j = 0; j < R; ++j) g1[j] = gc[j];
  }
  if constexpr (KS > 1) {   // the KS lanes' partial sums, in a fixed order
#pragma unroll
    for (int j = 0; j < R; ++j) {
      g1[j] = ks_sum<KS>(g1[j]); g2[j] = ks_sum<KS>(g2[j]);
      if (BRK) { cx[j] = ks_sum<KS>(cx[j]); cf[j] = ks_sum<KS>(cf[j]); }
    }
    e2 = ks_sum<KS>(e2);
  }
  // subperiod OLS coefficients gamma_j = A_j^-1 g_j, Wald beta = M^-1 [g1+g2; g2],
  // LM vector D'E_i = [F'E_i; F2'E_i] = [cf; c]: c = g2 - A2 l, cf = g1 + g2 -
  // (A1 + A2) l (break models: both summed explicitly in pass A).  F'E_i
  // vanishes only to the eigensolver's residual, so it is kept, not assumed 0
  double ga1[R], ga2[R], b1[R], b2[R], cv[R];
  // rows a in a loop that is NOT unrolled, register arrays read and written
  // by compile-time index only (rsel / rput): the prep-matrix reads of row a
  // are then issued per row — unrolled, the compiler hoisted all 7 R^2 of
  // them above the row loop (the matrices are read-only) and spilled them
#pragma unroll 1
  for (int a = 0; a < R; ++a) {
    const double g1a = rsel<R>(g1, a), g2a = rsel<R>(g2, a);
    double u1 = 0.0, u2 = 0.0, v1 = 0.0, v2 = 0.0, c = g2a, cs = g1a + g2a;
#pragma unroll
    for (int c2 = 0; c2 < R; ++c2) {
      u1 = fma(PM(CP_A1I, a, c2), g1[c2], u1);
      u2 = fma(PM(CP_A2I, a, c2), g2[c2], u2);
      v1 = fma(PM(CP_VA, c2, a), g1[c2], fma(PM(CP_VC, c2, a), g2[c2], v1));
      v2 = fma(PM(CP_WA, c2, a), g1[c2], fma(PM(CP_WC, c2, a), g2[c2], v2));
      if (!BRK) { c -= PM(CP_A2, a, c2) * l[c2]; cs -= PM(CP_APS, a, c2) * l[c2]; }
    }
    rput<R>(ga1, a, u1); rput<R>(ga2, a, u2); rput<R>(b1, a, v1); rput<R>(b2, a, v2);
    rput<R>(cv, a, BRK ? rsel<R>(cx, a) : c);
    if (!BRK) rput<R>(cf, a, cs);
  }
  // lmq = [cf; c]' M^-1 [cf; c]; M^-1 = [[Va, Wa], [Wa', Wb]] (r x r blocks)
  double lmq = 0.0;
#pragma unroll 1
  for (int a = 0; a < R; ++a) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int c2 = 0; c2 < R; ++c2) {
      s1 = fma(PM(CP_VA, a, c2), cf[c2], fma(PM(CP_WA, a, c2), cv[c2], s1));
      s2 = fma(PM(CP_WA, c2, a), cf[c2], fma(PM(CP_WB, a, c2), cv[c2], s2));
    }
    lmq = fma(rsel<R>(cf, a), s1, fma(rsel<R>(cv, a), s2, lmq));
  }
  // ---- pass B: subperiod SSRs and the HC0 block sum_t u_t^2 z_t z_t'
  double S[R * (R + 1) / 2], ssr = 0.0, bq[R];
  bool post_set = false;
#pragma unroll
  for (int j = 0; j < R; ++j) bq[j] = b1[j] + b2[j];
#pragma unroll
  for (int e = 0; e < R * (R + 1) / 2; ++e) S[e] = 0.0;
  for (int t0 = 0; t0 < T; t0 += TR) {
    __syncthreads();
    stage(t0);
    __syncthreads();
    if (!ok) continue;
    const int tn = min(TR, T - t0);
    for (int rb = ks; rb < tn; rb += KS * CU) {
      double xs[CU];
      load_rows(t0, rb, tn, xs);
      const int side = batch_side(t0, rb, tn);   // wave-uniform
      // rows ascend, so once a batch lies wholly at or after bp every later
      // one does: the post-break coefficients then replace the pre-break ones
      // (b1 and ga1 are not read after pass B) and the rows run without the
      // per-row selects, which only the one mixed batch keeps
      if (side == 2 && !post_set) {
#pragma unroll
        for (int j = 0; j < R; ++j) { b1[j] = bq[j]; ga1[j] = ga2[j]; }
        post_set = true;
      }
      if (side == 0) {   // the mixed batch: per-row subperiod selects
#pragma unroll
        for (int uq = 0; uq < CU; ++uq) {
          const int rr = rb + KS * uq;
          if (rr < tn) {
          const int t = t0 + rr;
          const double x = xs[uq];
          const bool post = t >= bp;
          double u = x, rs = x;
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const double f = sF[lr][rr * R + j];
            u -= f * (post ? bq[j] : b1[j]);
            rs -= f * (post ? ga2[j] : ga1[j]);
          }
          ssr = fma(rs, rs, ssr);
          const double u2 = u * u;
          double zs[R];
#pragma unroll
          for (int j = 0; j < R; ++j) zs[j] = u2 * sZ[lr][rr * R + j];
          int e = 0;
#pragma unroll
          for (int a = 0; a < R; ++a)
#pragma unroll
            for (int c2 = 0; c2 <= a; ++c2) { S[e] = fma(zs[a], sZ[lr][rr * R + c2], S[e]); ++e; }
          }
        }
      } else {
#pragma unroll
        for (int uq = 0; uq < CU; ++uq) {
          const int rr = rb + KS * uq;
          if (rr < tn) {
          const double x = xs[uq];
          double u = x, rs = x;
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const double f = sF[lr][rr * R + j];
            u -= f * b1[j];
            rs -= f * ga1[j];
          }
          ssr = fma(rs, rs, ssr);
          const double u2 = u * u;
          double zs[R];
#pragma unroll
          for (int j = 0; j < R; ++j) zs[j] = u2 * sZ[lr][rr * R + j];
          int e = 0;
#pragma unroll
          for (int a = 0; a < R; ++a)
#pragma unroll
            for (int c2 = 0; c2 <= a; ++c2) { S[e] = fma(zs[a], sZ[lr][rr * R + c2], S[e]); ++e; }
          }
        }
      }
    }
  }
  if constexpr (KS > 1) {
    ssr = ks_sum<KS>(ssr);
#pragma unroll
    for (int e = 0; e < R * (R + 1) / 2; ++e) S[e] = ks_sum<KS>(S[e]);
  }
  if (!ok || ks != 0) return;
  // Wald = b2' S^-1 b2 via in-register Cholesky of S (packed lower; padded
  // dimensions r..R-1 are an identity block)
  double wv = 0.0;
  {
    double Lc[R * (R + 1) / 2];
    int e = 0;
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
      for (int c2 = 0; c2 <= a; ++c2) {
        double s = (a < r && c2 < r) ? S[e] : (a == c2 ? 1.0 : 0.0);
#pragma unroll
        for (int p = 0; p < c2; ++p) s -= Lc[a * (a + 1) / 2 + p] * Lc[c2 * (c2 + 1) / 2 + p];
        Lc[e] = (a == c2) ? sqrt(s) : s / Lc[c2 * (c2 + 1) / 2 + c2];
        ++e;
      }
    double yv[R];
#pragma unroll
    for (int a = 0; a < R; ++a) {
      double s = (a < r) ? b2[a] : 0.0;
#pragma unroll
      for (int p = 0; p < a; ++p) s -= Lc[a * (a + 1) / 2 + p] * yv[p];
      yv[a] = s / Lc[a * (a + 1) / 2 + a];
      wv = fma(yv[a], yv[a], wv);
    }
  }
  const int64_t o = (int64_t)rep * N + i, oo = (int64_t)rep * os + i;
  const double vlr = T * (log(e2) - log(ssr)), vlm = T * lmq / e2;
  LR[o] = vlr;
  LM[o] = vlm;
  WD[o] = wv;
  // the caller's strided rows directly (three 2-D copy launches per job before)
  if (LRo) LRo[oo] = vlr;
  if (LMo) LMo[oo] = vlm;
  if (WDo) WDo[oo] = wv;
}

template <int R>
static void launch_chow_r(const PanelSrc &src, const ChowBlocks &blk, int T, int N, int r, int bp, int nb,
                          const double *F, const double *Z, const double *prep, const double *Lm, double *LR,
                          double *LM, double *WD, double *LRo, double *LMo, double *WDo, int64_t os,
                          hipStream_t st) {
  const bool c = src.C, e = src.eta, x = src.idx;
  constexpr int KS = R <= 4 ? CH_KS : 1;   // lanes per (replicate, variable)
  // flat: a 256-thread block (256 / KS pairs) spans at most CH_FLAT_REPS replicates
  const bool flat = R <= 8 && (256 / KS + N - 1) / N + 1 <= CH_FLAT_REPS;
  // non-flat: narrow panels get a block of round_up(N KS, 64) threads, not a half-idle 256
  const int nth = flat ? 256 : std::min(256, (N * KS + 63) / 64 * 64);
  dim3 grid(flat ? (unsigned)(((int64_t)nb * N * KS + 255) / 256) : (unsigned)((N * KS + nth - 1) / nth),
            flat ? 1 : nb),
      block(nth);
#define DFM_CH(C_, E_, X_, B_)                                                                                  \
  do {                                                                                                          \
    if (flat)                                                                                                   \
      hipLaunchKernelGGL((chow_all_kernel<R, C_, E_, X_, B_, (R <= 8), KS>), grid, block, 0, st, src, blk, T, N, \
                         r, bp, nb, F, Z, prep, Lm, LR, LM, WD, LRo, LMo, WDo, os);                             \
    else                                                                                                        \
      hipLaunchKernelGGL((chow_all_kernel<R, C_, E_, X_, B_, false, KS>), grid, block, 0, st, src, blk, T, N, r, \
                         bp, nb, F, Z, prep, Lm, LR, LM, WD, LRo, LMo, WDo, os);                                \
  } while (0)
  if (blk.n > 1) {
    if (c && e && x) DFM_CH(true, true, true, true);
    else if (c && !e && x) DFM_CH(true, false, true, true);
    else DFM_CH(false, false, false, true);
  } else {
    if (c && e && x) DFM_CH(true, true, true, false);
    else if (c && !e && x) DFM_CH(true, false, true, false);
    else DFM_CH(false, false, false, false);
  }
#undef DFM_CH
}

// scratch layout in ws: [prep blocks: nb x CH_PREP_BYTES][Z: nb x T x r] ... [3][nb][N] at the END.
// Break models: nblk > 1 blocks with first rows brow[0..nblk-1] (brow[0] = 0),
// loadings of block j at Lm + j * lbs.
hipError_t launch_chow(int orient, const PanelSrc &src, int T, int N, int r, int bp, int nb,
                       const double *F, const double *Lm, double *LRo, double *LMo, double *WDo,
                       int64_t out_stride, char *ws, size_t ws_bytes, hipStream_t st, int nblk,
                       const int *brow, int64_t lbs) {
  (void)orient;
  if (r < 1 || r > CH_RMAX || nblk < 1 || nblk > CH_BMAX) return hipErrorInvalidValue;
  if ((int64_t)T * src.ld * 8 >= ((int64_t)1 << 32)) return hipErrorInvalidValue;   // 32-bit gather offsets
  ChowBlocks blk{};
  blk.n = nblk;
  blk.lbs = lbs;
  for (int j = 0; j < nblk; ++j) blk.a[j] = nblk > 1 ? brow[j] : 0;
  blk.a[nblk] = T;
  double *prep = (double *)ws;
  double *Z = (double *)(ws + (size_t)nb * CH_PREP_BYTES);
  double *scr = (double *)(ws + ws_bytes) - (size_t)3 * nb * N;
  const int RC = r <= 4 ? 4 : (r <= 8 ? 8 : 16);   // the main kernel's padded R (below)
  hipLaunchKernelGGL(chow_prep_kernel, dim3(nb), dim3(256), 0, st, F, T, r, bp, RC, prep, Z);
  double *LR = scr, *LM = scr + (size_t)nb * N, *WD = scr + (size_t)2 * nb * N;
  // R = padded factor count of the per-variable register blocks (zero
  // padding: r <= 4 runs 4-wide, 10 HC0 accumulators instead of 36)
  if (r <= 4) launch_chow_r<4>(src, blk, T, N, r, bp, nb, F, Z, prep, Lm, LR, LM, WD, LRo, LMo, WDo, out_stride, st);
  else if (r <= 8) launch_chow_r<8>(src, blk, T, N, r, bp, nb, F, Z, prep, Lm, LR, LM, WD, LRo, LMo, WDo, out_stride, st);
  else launch_chow_r<16>(src, blk, T, N, r, bp, nb, F, Z, prep, Lm, LR, LM, WD, LRo, LMo, WDo, out_stride, st);
  // (the kernel wrote the caller's strided output rows itself)
  return hipGetLastError();
}

// ------------------------------------------------------ targeted predictors
// PER_CANDIDATE (Bai–Ng 2008 / defect D8 extension): for each column i,
// OLS of y on [w x_i] with White HC0.  By Frisch–Waugh–Lovell the x_i
// coefficient and its HC0 variance equal those of y~ on x~_i, where ~ is
// the residual after projecting on w:  beta = Sxy/Sxx,
// var = sum_t u_t^2 x~_t^2 / Sxx^2,  u = y~ - beta x~.
// Wp: q x q inverse of w'w and yt = M_w y are precomputed per call.
constexpr int TP_QMAX = 16;
__global__ __launch_bounds__(256) void tp_candidate_kernel(const double *__restrict__ Xp, int64_t ld,
                                                           int T, int N, const double *__restrict__ w,
                                                           int q, const double *__restrict__ Wi,
                                                           const double *__restrict__ yt, double cv,
                                                           double *__restrict__ tstat,
                                                           uint8_t *__restrict__ mask) {
  __shared__ double sW[128 * TP_QMAX], sy[128], sWi[TP_QMAX * TP_QMAX];
  const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
  const bool ok = i < N;
  for (int e = tid; e < q * q; e += 256) sWi[e] = Wi[e];
  // pass 1: w'x_i
  double wx[TP_QMAX];
#pragma unroll
  for (int a = 0; a < TP_QMAX; ++a) wx[a] = 0.0;
  for (int t0 = 0; t0 < T; t0 += 128) {
    __syncthreads();
    for (int e = tid; e < 128 * q; e += 256) {
      const int rr = e / q, a = e % q, t = t0 + rr;
      sW[rr * TP_QMAX + a] = t < T ? w[(int64_t)a * T + t] : 0.0;
    }
    __syncthreads();
    if (!ok) continue;
    const int tn = min(128, T - t0);
    for (int rr = 0; rr < tn; ++rr) {
      const double x = Xp[(int64_t)(t0 + rr) * ld + i];
#pragma unroll
      for (int a = 0; a < TP_QMAX; ++a)
        if (a < q) wx[a] = fma(sW[rr * TP_QMAX + a], x, wx[a]);
    }
  }
  double cfs[TP_QMAX];
#pragma unroll
  for (int a = 0; a < TP_QMAX; ++a) {
    double s = 0.0;
    for (int b = 0; b < q; ++b) s = fma(sWi[a * q + b], wx[b], s);
    cfs[a] = a < q ? s : 0.0;
  }
  // pass 2: Sxy, Sxx ; pass 3: sum u^2 x~^2
  double sxy = 0.0, sxx = 0.0, beta = 0.0, meat = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int t0 = 0; t0 < T; t0 += 128) {
      __syncthreads();
      for (int e = tid; e < 128 * q; e += 256) {
        const int rr = e / q, a = e % q, t = t0 + rr;
        sW[rr * TP_QMAX + a] = t < T ? w[(int64_t)a * T + t] : 0.0;
      }
      for (int e = tid; e < 128; e += 256) sy[e] = (t0 + e < T) ? yt[t0 + e] : 0.0;
      __syncthreads();
      if (!ok) continue;
      const int tn = min(128, T - t0);
      for (int rr = 0; rr < tn; ++rr) {
        double xt = Xp[(int64_t)(t0 + rr) * ld + i];
#pragma unroll
        for (int a = 0; a < TP_QMAX; ++a)
          if (a < q) xt -= sW[rr * TP_QMAX + a] * cfs[a];
        if (pass == 0) { sxy = fma(xt, sy[rr], sxy); sxx = fma(xt, xt, sxx); }
        else { const double u = sy[rr] - beta * xt; meat = fma(u * u, xt * xt, meat); }
      }
    }
    beta = sxy / sxx;
  }
  if (!ok) return;
  const double tv = beta / sqrt(fabs(meat / (sxx * sxx)));
  tstat[i] = tv;
  mask[i] = fabs(tv) > cv ? 1 : 0;
}

// JOINT (the reference, q + N < T): D = [w x], beta = (D'D)^-1 D'y, HC0,
// |diag| (:15-24).  Dense n x n inverse in LDS: n = q + N <= TPJ_MAX.
constexpr int TPJ_MAX = 64;
__global__ __launch_bounds__(256) void tp_joint_kernel(const double *__restrict__ Xp, int64_t ld, int T,
                                                       int N, const double *__restrict__ w, int q,
                                                       const double *__restrict__ y, double cv,
                                                       double *__restrict__ tstat,
                                                       uint8_t *__restrict__ mask, int *bad_out) {
  constexpr int S = TPJ_MAX + 1;
  __shared__ double M[TPJ_MAX * S], Mi[TPJ_MAX * S], Lw[TPJ_MAX * S], Tw[TPJ_MAX * S];
  __shared__ double Dy[TPJ_MAX], beta[TPJ_MAX], dg[TPJ_MAX];
  __shared__ int bad;
  const int tid = threadIdx.x, n = q + N;
  auto D = [&](int t, int c) { return c < q ? w[(int64_t)c * T + t] : Xp[(int64_t)t * ld + (c - q)]; };
  if (tid == 0) bad = 0;
  for (int e = tid; e < n * n; e += 256) {
    const int a = e / n, c = e % n;
    double s = 0.0;
    for (int t = 0; t < T; ++t) s = fma(D(t, a), D(t, c), s);
    M[a * S + c] = s;
  }
  for (int a = tid; a < n; a += 256) {
    double s = 0.0;
    for (int t = 0; t < T; ++t) s = fma(D(t, a), y[t], s);
    Dy[a] = s;
  }
  __syncthreads();
  block_spd_inverse(M, Mi, Lw, Tw, n, S, &bad);
  for (int a = tid; a < n; a += 256) {
    double s = 0.0;
    for (int c = 0; c < n; ++c) s = fma(Mi[a * S + c], Dy[c], s);
    beta[a] = s;
  }
  __syncthreads();
  // diag(cov)_j = sum_t u_t^2 (Mi d_t)_j^2
  for (int j = tid; j < n; j += 256) dg[j] = 0.0;
  __syncthreads();
  for (int j = tid; j < n; j += 256) {
    double s = 0.0;
    for (int t = 0; t < T; ++t) {
      double fit = 0.0, kj = 0.0;
      for (int c = 0; c < n; ++c) {
        const double dv = D(t, c);
        fit = fma(dv, beta[c], fit);
        kj = fma(Mi[j * S + c], dv, kj);
      }
      const double u = y[t] - fit;
      s = fma(u * u, kj * kj, s);
    }
    dg[j] = s;
  }
  __syncthreads();
  for (int i = tid; i < N; i += 256) {
    const double tv = beta[q + i] / sqrt(fabs(dg[q + i]));
    tstat[i] = tv;
    mask[i] = fabs(tv) > cv ? 1 : 0;
  }
  if (tid == 0) *bad_out = bad;
}

size_t targeted_workspace_bytes(int mode, int T, int N, int q) {
  (void)mode; (void)N;
  return (size_t)TP_QMAX * TP_QMAX * 8 + (size_t)T * 8 + 4096 + (size_t)q * 0;
}

hipError_t launch_targeted(int mode, const double *y, const double *w, int q, const double *Xp,
                           int64_t ld, int T, int N, double cv, double *tstat, uint8_t *mask, char *ws,
                           size_t ws_bytes, hipStream_t st, int *bad) {
  (void)ws_bytes;
  if (mode == 0) {
    if (q + N > TPJ_MAX) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tp_joint_kernel, dim3(1), dim3(256), 0, st, Xp, ld, T, N, w, q, y, cv, tstat,
                       mask, bad);
    return hipGetLastError();
  }
  if (q > TP_QMAX) return hipErrorInvalidValue;
  double *Wi = (double *)ws;
  double *yt = Wi + TP_QMAX * TP_QMAX;
  // host computes nothing: the q x q inverse of w'w and y~ are produced by a
  // one-workgroup kernel below
  extern __global__ void tp_prep_kernel(const double *, int, const double *, int, double *, double *, int *);
  hipLaunchKernelGGL(tp_prep_kernel, dim3(1), dim3(256), 0, st, w, q, y, T, Wi, yt, bad);
  hipLaunchKernelGGL(tp_candidate_kernel, dim3((N + 255) / 256), dim3(256), 0, st, Xp, ld, T, N, w, q,
                     Wi, yt, cv, tstat, mask);
  return hipGetLastError();
}

// (w'w)^-1 and y~ = y - w (w'w)^-1 w'y
__global__ __launch_bounds__(256) void tp_prep_kernel(const double *__restrict__ w, int q,
                                                      const double *__restrict__ y, int T,
                                                      double *__restrict__ Wi, double *__restrict__ yt,
                                                      int *bad_out) {
  constexpr int S = TP_QMAX + 1;
  __shared__ double M[TP_QMAX * S], Mi[TP_QMAX * S], Lw[TP_QMAX * S], Tw[TP_QMAX * S], wy[TP_QMAX],
      c[TP_QMAX];
  __shared__ int bad;
  const int tid = threadIdx.x;
  if (tid == 0) bad = 0;
  for (int e = tid; e < q * q; e += 256) {
    const int a = e / q, b = e % q;
    double s = 0.0;
    for (int t = 0; t < T; ++t) s = fma(w[(int64_t)a * T + t], w[(int64_t)b * T + t], s);
    M[a * S + b] = s;
  }
  for (int a = tid; a < q; a += 256) {
    double s = 0.0;
    for (int t = 0; t < T; ++t) s = fma(w[(int64_t)a * T + t], y[t], s);
    wy[a] = s;
  }
  __syncthreads();
  block_spd_inverse(M, Mi, Lw, Tw, q, S, &bad);
  for (int a = tid; a < q; a += 256) {
    double s = 0.0;
    for (int b = 0; b < q; ++b) s = fma(Mi[a * S + b], wy[b], s);
    c[a] = s;
  }
  for (int e = tid; e < q * q; e += 256) Wi[e] = Mi[(e / q) * S + e % q];
  __syncthreads();
  for (int t = tid; t < T; t += 256) {
    double s = y[t];
    for (int a = 0; a < q; ++a) s -= w[(int64_t)a * T + t] * c[a];
    yt[t] = s;
  }
  if (tid == 0) *bad_out = bad;
}

}  // namespace dfm
