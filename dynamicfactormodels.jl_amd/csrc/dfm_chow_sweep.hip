// dfm_chow_sweep.hip — the Breitung–Eickmeier (2011) Chow statistics of
// dfm_chow.hip (src/chowtest.jl:19-42) for EVERY variable at EVERY break
// period bp_lo..bp_hi of a replicate batch in one device pass, reduced over bp
// to the sup statistics and their arg-max dates (Andrews 1993).  r <= 16,
// models fitted without breaks.
//
// The [F, F.*d] regression of the header of dfm_chow.hip is the two sub-period
// regressions.  With the full-sample residuals e_t = x_ti - f_t' l_i and
//   c1 = sum_{t<bp} f_t e_t,  c2 = sum_{t>=bp} f_t e_t  ([cf; c] = [c1 + c2; c2]),
//   A1 = F1'F1, A2 = F2'F2,   delta_j = A_j^-1 c_j   (gamma_j = l_i + delta_j)
// the statistics of one (bp, i) are
//   LM   = T [cf; c]' M^-1 [cf; c] / ||E_i||^2 = T (c1'A1^-1 c1 + c2'A2^-1 c2) / ||E_i||^2
//          — the same quadratic form in the block-diagonal basis [F.*(1-d), F.*d]
//          (M^-1 = [[A1^-1, -A1^-1], [-A1^-1, A1^-1 + A2^-1]]); F'E_i is kept
//   LR   = T (ln ||E_i||^2 - ln(SSR_1 + SSR_2)),  SSR_1 + SSR_2 = ||E_i||^2 - q,
//          q = c1'delta_1 + c2'delta_2 (exact for any l_i), so LR = -T log1p(-q / ||E_i||^2):
//          the small correction q is formed from the explicit residuals, never
//          as a difference of two sums of squares of x
//   Wald = b' Cov22^-1 b,  b = delta_2 - delta_1,  Cov22 = sum_t u_t^2 z_t z_t',
//          u_t = e_t - f_t' delta_side(t),  z_t = A_side(t)^-1 f_t  (Wa = -A1^-1, Wa + Wb = A2^-1)
//
// Five steps per chunk of replicates, each one timed DFM_KC_CHOW launch:
//   resid   e = C + eta E[idx] - F l   (T x N per replicate, read by every date)
//   prep    A1(bp)^-1, A2(bp)^-1 for every date: a forward and a backward running
//           sum of f f' per replicate, then one wave per (bp, replicate) inverts
//   lm      pass A only: LR and LM curves       (O(T r) per (bp-tile, i))
//   wald    pass A + the HC0 pass: Wald curve   (O(T r^2) per (bp, i)); launched
//           only when a Wald output is wanted
//   reduce  sup / first arg-max over bp of each wanted curve
// One lane per variable, the break periods of a block uniform across the
// wave: F and z rows are LDS broadcasts, the residual column loads coalesce
// over i, and a thread carries BPT consecutive dates so a residual load and
// its f row serve BPT accumulator sets.  c1 of consecutive dates is one
// running prefix sum, snapshotted at each date.  Every sum runs in a fixed
// order per (replicate, bp, i): results do not depend on batch or chunk.
#include <algorithm>

#include "dfm_internal.h"
#include "dfm_small.h"

namespace dfm {

constexpr int SW_RMAX = 16;
constexpr int SW_TR = 128;                        // rows per staged F tile
constexpr size_t SW_CHUNK_BYTES = (size_t)512 << 20;   // workspace bound of one chunk of replicates
constexpr int SW_CHUNK_MAX = 4096;                // grid.z

static int sweep_rc(int r) { return r <= 4 ? 4 : (r <= 8 ? 8 : 16); }
// per replicate: residuals, two RC x RC inverses per date, three curves
static size_t sweep_rep_bytes(int T, int N, int r, int nbp) {
  const int RC = sweep_rc(r);
  return ((size_t)T * N + (size_t)nbp * 2 * RC * RC + (size_t)3 * nbp * N) * 8;
}
static int sweep_chunk(int T, int N, int r, int nbp, int nb) {
  const size_t cap = std::max<size_t>(1, SW_CHUNK_BYTES / sweep_rep_bytes(T, N, r, nbp));
  return (int)std::min<size_t>(std::min<size_t>(cap, SW_CHUNK_MAX), (size_t)std::max(nb, 1));
}
size_t chow_sweep_workspace_bytes(int T, int N, int r, int nbp, int nb) {
  return (size_t)sweep_chunk(T, N, r, nbp, nb) * sweep_rep_bytes(T, N, r, nbp) + 4096;
}

// e[t][i] = x_ti - f_t' l_i,  x = C + eta E[idx]  (dfm_chow.hip's gathered row)
__global__ __launch_bounds__(256) void chow_sweep_resid_kernel(PanelSrc src, int T, int N, int r,
                                                               const double *__restrict__ F,
                                                               const double *__restrict__ Lm,
                                                               double *__restrict__ Er) {
  const int rep = blockIdx.y;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)T * N) return;
  const int t = (int)(e / N), i = (int)(e % N);
  const int64_t ro = (int64_t)rep * src.rs;
  const int64_t row = src.idx ? src.idx[ro + t] : t;
  double x = src.E[row * src.ld + i];
  if (src.eta) x *= src.eta[ro + t];
  if (src.C) x += src.C[(int64_t)t * src.ld + i];
  const double *f = F + ((int64_t)rep * T + t) * r, *l = Lm + ((int64_t)rep * N + i) * r;
  double ev = x;
  for (int j = 0; j < r; ++j) ev -= f[j] * l[j];
  Er[(int64_t)rep * T * N + e] = ev;
}

// A1(bp) = sum_{t<bp} f_t f_t' and A2(bp) = sum_{t>=bp} f_t f_t' of every date of
// one replicate: entry (a, c) on one lane, a forward and a backward running sum
// over the rows (each a plain in-order sum, staged F tiles), snapshotted at
// each date into the date's two RC x RC slots at prep + ((rep nbp + k) 2) RC^2
// — O(T r^2) per replicate, where a sum per date was O(nbp T r^2) of
// latency-bound loads.
__global__ __launch_bounds__(256) void chow_sweep_scan_kernel(const double *__restrict__ F, int T, int r, int bp_lo,
                                                              int nbp, int RC, double *__restrict__ prep) {
  constexpr int TR = SW_TR;
  __shared__ double sF[TR * SW_RMAX];   // row stride r
  const int tid = threadIdx.x, rep = blockIdx.x, bp_hi = bp_lo + nbp - 1;
  const double *Fr = F + (int64_t)rep * T * r;
  const bool act = tid < r * r;
  const int a = act ? tid / r : 0, c = act ? tid % r : 0;
  double *P = prep + (int64_t)rep * nbp * 2 * RC * RC + a * RC + c;
  auto stage = [&](int t0) {
    __syncthreads();
    for (int e = tid; e < TR * r; e += 256) sF[e] = t0 + e / r < T ? Fr[(int64_t)t0 * r + e] : 0.0;
    __syncthreads();
  };
  double s = 0.0;
  for (int t0 = 0; t0 <= bp_hi; t0 += TR) {   // rows 0 .. bp_hi, ascending
    stage(t0);
    if (!act) continue;
    const int tn = min(TR, bp_hi + 1 - t0);
    for (int rr = 0; rr < tn; ++rr) {
      const int k = t0 + rr - bp_lo;
      if (k >= 0) P[(int64_t)(k * 2) * RC * RC] = s;   // (k < nbp: t <= bp_hi)
      s = fma(sF[rr * r + a], sF[rr * r + c], s);
    }
  }
  s = 0.0;
  for (int t0 = (T - 1) / TR * TR; t0 >= 0 && t0 + TR > bp_lo; t0 -= TR) {   // rows T-1 .. bp_lo, descending
    stage(t0);
    if (!act) continue;
    for (int rr = min(TR, T - t0) - 1; rr >= 0 && t0 + rr >= bp_lo; --rr) {
      s = fma(sF[rr * r + a], sF[rr * r + c], s);
      const int k = t0 + rr - bp_lo;
      if (k < nbp) P[(int64_t)(k * 2 + 1) * RC * RC] = s;
    }
  }
}

// The two sums of a date inverted in place, one wave per (date, replicate),
// SW_IW of them per block: RC x RC each, zero outside r.
constexpr int SW_IW = 4;
static size_t sweep_inv_lds(int RC) { return (size_t)SW_IW * 6 * RC * (RC + 1) * 8; }
__global__ __launch_bounds__(64 * SW_IW) void chow_sweep_inv_kernel(int r, int64_t ndates, int RC,
                                                                    double *__restrict__ prep) {
  extern __shared__ double sw_inv_lds[];
  __shared__ int bad;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, S = RC + 1, M = RC * S;
  const int64_t d = (int64_t)blockIdx.x * SW_IW + wv;   // (replicate, date) pair
  double *A1 = sw_inv_lds + (size_t)wv * 6 * M, *A2 = A1 + M, *A1i = A2 + M, *A2i = A1i + M, *Lw = A2i + M,
         *Tw = Lw + M;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  if (d >= ndates) return;   // (whole waves; no barrier below)
  double *P = prep + d * 2 * RC * RC;
  for (int e = lane; e < r * r; e += 64) {
    const int a = e / r, c = e % r;
    A1[a * S + c] = P[a * RC + c];
    A2[a * S + c] = P[RC * RC + a * RC + c];
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // this wave's LDS writes before its reads
  wave_spd_inverse(A1, A1i, Lw, Tw, r, S, &bad);
  wave_spd_inverse(A2, A2i, Lw, Tw, r, S, &bad);
  (void)bad;   // (a singular block leaves inf / NaN statistics, as the reference's inv)
  for (int e = lane; e < RC * RC; e += 64) {
    const int a = e / RC, c = e % RC;
    const bool in = a < r && c < r;
    P[e] = in ? A1i[a * S + c] : 0.0;
    P[RC * RC + e] = in ? A2i[a * S + c] : 0.0;
  }
}

// Dates per thread: a residual load and its F row feed BPT accumulator sets in
// the Wald pass (R = 4: 10 HC0 sums and two coefficient vectors per date); the
// LR / LM pass keeps one snapshot of the running sum per date, so it takes
// more dates per read of the residual column.
template <int R, bool WALD>
constexpr int sweep_bpt() { return WALD ? (R <= 4 ? 4 : 1) : (R <= 4 ? 8 : (R <= 8 ? 4 : 2)); }

// grid (date tiles, variable tiles of 64, replicates), one wave per block.
// WALD = false: writes the LR and LM curves; true: the Wald curve only.
// Curves: [replicate][date][N].
// Waves per SIMD the register budget is held to: the LR / LM pass waits on its
// residual loads and wants waves (unbounded, the compiler hoisted the block's
// inverses out of LDS into 256 registers); the Wald pass holds BPT HC0 blocks.
template <int R, bool WALD>
constexpr int sweep_waves() { return WALD ? (R <= 8 ? 2 : 1) : (R <= 8 ? 3 : 2); }
template <int R, int BPT, bool WALD>
__global__ __launch_bounds__(64, (sweep_waves<R, WALD>())) void chow_sweep_kernel(int T, int N, int r, int bp_lo, int nbp,
                                                        const double *__restrict__ F,
                                                        const double *__restrict__ Er,
                                                        const double *__restrict__ prep,
                                                        double *__restrict__ cLR, double *__restrict__ cLM,
                                                        double *__restrict__ cWD) {
  constexpr int TR = SW_TR, CU = 8, NS = R * (R + 1) / 2;
  __shared__ double sF[TR * R], sZ[WALD ? BPT * TR * R : 1], sAi[BPT * 2 * R * R];
  const int lane = threadIdx.x, rep = blockIdx.z, k0 = blockIdx.x * BPT, b0 = bp_lo + k0;
  const int nk = min(BPT, nbp - k0);
  int i = blockIdx.y * 64 + lane;
  const bool ok = i < N;
  if (!ok) i = N - 1;   // (idle lanes read a valid column; they write nothing)
  const double *Fr = F + (int64_t)rep * T * r, *Ei = Er + (int64_t)rep * T * N + i;
  // this block's dates' inverses (dates past the range: zeros, never written out)
  for (int e = lane; e < BPT * 2 * R * R; e += 64)
    sAi[e] = e / (2 * R * R) < nk ? prep[((int64_t)rep * nbp + k0) * 2 * R * R + e] : 0.0;
  auto stage = [&](int t0) {
    for (int e = lane; e < TR * R; e += 64) {
      const int rr = e / R, j = e % R, t = t0 + rr;
      sF[e] = (t < T && j < r) ? Fr[(int64_t)t * r + j] : 0.0;
    }
  };
  // CU rows' residuals in flight together
  auto load_rows = [&](int t0, int rb, int tn, double *es) {
#pragma unroll
    for (int u = 0; u < CU; ++u) es[u] = Ei[(int64_t)(t0 + min(rb + u, tn - 1)) * N];
  };
  // ---- pass A: cp = running sum_t f_t e_t, snapshotted at each date; e2 = ||E_i||^2
  double cp[R], c1[BPT][R], e2 = 0.0;
#pragma unroll
  for (int j = 0; j < R; ++j) {
    cp[j] = 0.0;
#pragma unroll
    for (int k = 0; k < BPT; ++k) c1[k][j] = 0.0;
  }
  for (int t0 = 0; t0 < T; t0 += TR) {
    __syncthreads();
    stage(t0);
    __syncthreads();
    const int tn = min(TR, T - t0);
    for (int rb = 0; rb < tn; rb += CU) {
      double es[CU];
      load_rows(t0, rb, tn, es);
#pragma unroll
      for (int u = 0; u < CU; ++u) {
        const int rr = rb + u;
        if (rr < tn) {
          const int t = t0 + rr;
#pragma unroll
          for (int k = 0; k < BPT; ++k)
            if (t == b0 + k) {   // (uniform)
#pragma unroll
              for (int j = 0; j < R; ++j) c1[k][j] = cp[j];
            }
          const double ev = es[u];
          e2 = fma(ev, ev, e2);
#pragma unroll
          for (int j = 0; j < R; ++j) cp[j] = fma(sF[rr * R + j], ev, cp[j]);
        }
      }
    }
  }
  // delta_j = A_j^-1 c_j of date k (the inverses from LDS), q = c1'delta_1 + c2'delta_2
  auto deltas = [&](int k, const double (&c1k)[R], double (&d1k)[R], double (&d2k)[R]) {
    double c2[R], qs = 0.0;
#pragma unroll
    for (int j = 0; j < R; ++j) c2[j] = cp[j] - c1k[j];
#pragma unroll
    for (int a = 0; a < R; ++a) {
      double u1 = 0.0, u2 = 0.0;
#pragma unroll
      for (int c = 0; c < R; ++c) {
        u1 = fma(sAi[(k * 2) * R * R + a * R + c], c1k[c], u1);
        u2 = fma(sAi[(k * 2 + 1) * R * R + a * R + c], c2[c], u2);
      }
      d1k[a] = u1;
      d2k[a] = u2;
      qs = fma(c1k[a], u1, fma(c2[a], u2, qs));
    }
    return qs;
  };
  if constexpr (!WALD) {
    // the dates one after another in a loop that is NOT unrolled (c1[k] picked
    // by compile-time indices): unrolled, the compiler hoisted all BPT 2 R^2
    // LDS reads above the loop and spilled them
#pragma unroll 1
    for (int k = 0; k < nk; ++k) {
      double c1k[R], d1k[R], d2k[R];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        c1k[j] = c1[0][j];
#pragma unroll
        for (int kk = 1; kk < BPT; ++kk) c1k[j] = k == kk ? c1[kk][j] : c1k[j];
      }
      const double rho = deltas(k, c1k, d1k, d2k) / e2;
      if (!ok) continue;
      const int64_t o = ((int64_t)rep * nbp + k0 + k) * N + i;
      if (cLR) cLR[o] = -(double)T * log1p(-rho);
      if (cLM) cLM[o] = (double)T * rho;
    }
    return;
  } else {
    double d1[BPT][R], d2[BPT][R];
#pragma unroll
    for (int k = 0; k < BPT; ++k) deltas(k, c1[k], d1[k], d2[k]);
    // ---- pass B: Cov22 = sum_t u_t^2 z_t z_t'
    double Sm[BPT][NS];
#pragma unroll
    for (int k = 0; k < BPT; ++k)
#pragma unroll
      for (int e = 0; e < NS; ++e) Sm[k][e] = 0.0;
    for (int t0 = 0; t0 < T; t0 += TR) {
      __syncthreads();
      stage(t0);
      __syncthreads();
      // z_t = A_side^-1 f_t of every date of the block (the inverses are symmetric)
      for (int e = lane; e < BPT * TR * R; e += 64) {
        const int k = e / (TR * R), rr = (e / R) % TR, j = e % R;
        const double *A = sAi + (k * 2 + (t0 + rr >= b0 + k ? 1 : 0)) * R * R + j * R;
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < R; ++a) s = fma(A[a], sF[rr * R + a], s);
        sZ[e] = s;
      }
      __syncthreads();
      const int tn = min(TR, T - t0);
      for (int rb = 0; rb < tn; rb += CU) {
        double es[CU];
        load_rows(t0, rb, tn, es);
#pragma unroll
        for (int u = 0; u < CU; ++u) {
          const int rr = rb + u;
          if (rr < tn) {
            const int t = t0 + rr;
            double fr[R];
#pragma unroll
            for (int j = 0; j < R; ++j) fr[j] = sF[rr * R + j];
#pragma unroll
            for (int k = 0; k < BPT; ++k) {
              const bool pre = t < b0 + k;   // (uniform)
              double uv = es[u];
#pragma unroll
              for (int j = 0; j < R; ++j) uv -= fr[j] * (pre ? d1[k][j] : d2[k][j]);
              const double u2 = uv * uv;
              double z[R], zs[R];
#pragma unroll
              for (int j = 0; j < R; ++j) { z[j] = sZ[(k * TR + rr) * R + j]; zs[j] = u2 * z[j]; }
              int e = 0;
#pragma unroll
              for (int a = 0; a < R; ++a)
#pragma unroll
                for (int c = 0; c <= a; ++c) { Sm[k][e] = fma(zs[a], z[c], Sm[k][e]); ++e; }
            }
          }
        }
      }
    }
    // Wald = b' Cov22^-1 b by an in-register Cholesky (packed lower; the padded
    // dimensions r..R-1 are an identity block), as chow_all_kernel's
#pragma unroll
    for (int k = 0; k < BPT; ++k) {
      double wv = 0.0, Lc[NS], yv[R];
      int e = 0;
#pragma unroll
      for (int a = 0; a < R; ++a)
#pragma unroll
        for (int c = 0; c <= a; ++c) {
          double s = (a < r && c < r) ? Sm[k][e] : (a == c ? 1.0 : 0.0);
#pragma unroll
          for (int p = 0; p < c; ++p) s -= Lc[a * (a + 1) / 2 + p] * Lc[c * (c + 1) / 2 + p];
          Lc[e] = (a == c) ? sqrt(s) : s / Lc[c * (c + 1) / 2 + c];
          ++e;
        }
#pragma unroll
      for (int a = 0; a < R; ++a) {
        double s = (a < r) ? d2[k][a] - d1[k][a] : 0.0;
#pragma unroll
        for (int p = 0; p < a; ++p) s -= Lc[a * (a + 1) / 2 + p] * yv[p];
        yv[a] = s / Lc[a * (a + 1) / 2 + a];
        wv = fma(yv[a], yv[a], wv);
      }
      if (ok && k < nk) cWD[((int64_t)rep * nbp + k0 + k) * N + i] = wv;
    }
  }
}

// sup over the dates and its first arg-max, per (statistic, replicate, variable)
struct SweepReduce {
  const double *cur[3];
  double *sup[3];
  int64_t *arg[3];
};
__global__ __launch_bounds__(256) void chow_sweep_reduce_kernel(SweepReduce a, int nbp, int N, int nrep, int bp_lo,
                                                                int64_t os) {
  const int s = blockIdx.y;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (!a.cur[s] || g >= (int64_t)nrep * N) return;
  const int64_t rep = g / N, i = g % N;
  const double *c = a.cur[s] + rep * nbp * N + i;
  double best = c[0];
  int bi = 0;
#pragma unroll 8
  for (int k = 1; k < nbp; ++k) {   // (unrolled: eight dates' loads in flight, compared in order)
    const double v = c[(int64_t)k * N];
    if (v > best) { best = v; bi = k; }
  }
  if (a.sup[s]) a.sup[s][rep * os + i] = best;
  if (a.arg[s]) a.arg[s][rep * N + i] = bp_lo + bi;
}

template <int R, bool WALD>
static void launch_sweep_rw(dim3 grid, int T, int N, int r, int bp_lo, int nbp, const double *F,
                           const double *Er, const double *prep, double *cLR, double *cLM, double *cWD,
                           hipStream_t st) {
  constexpr int BPT = sweep_bpt<R, WALD>();
  grid.x = (unsigned)((nbp + BPT - 1) / BPT);
  hipLaunchKernelGGL((chow_sweep_kernel<R, BPT, WALD>), grid, dim3(64), 0, st, T, N, r, bp_lo, nbp, F, Er, prep, cLR,
                     cLM, cWD);
}
template <int R>
static void launch_sweep_r(bool wald, dim3 grid, int T, int N, int r, int bp_lo, int nbp, const double *F,
                           const double *Er, const double *prep, double *cLR, double *cLM, double *cWD,
                           hipStream_t st) {
  if (wald) launch_sweep_rw<R, true>(grid, T, N, r, bp_lo, nbp, F, Er, prep, cLR, cLM, cWD, st);
  else launch_sweep_rw<R, false>(grid, T, N, r, bp_lo, nbp, F, Er, prep, cLR, cLM, cWD, st);
}

// ws: chow_sweep_workspace_bytes(T, N, r, nbp, nb) or more; the replicates run
// in chunks of as many as ws holds.  Per chunk: [residuals][inverses][3 curves].
hipError_t launch_chow_sweep(const PanelSrc &src, int T, int N, int r, int bp_lo, int bp_hi, int nb, const double *F,
                             const double *Lm, const ChowSweepOut &out, char *ws, size_t ws_bytes, hipStream_t st,
                             timer_fn tf, void *tctx) {
  if (r < 1 || r > SW_RMAX || bp_lo > bp_hi || bp_lo < r || bp_hi > T - r || nb < 1) return hipErrorInvalidValue;
  const int nbp = bp_hi - bp_lo + 1, RC = sweep_rc(r);
  bool want[3];
  for (int s = 0; s < 3; ++s) want[s] = out.sup[s] || out.argsup[s] || out.curve[s];
  if (!want[0] && !want[1] && !want[2]) return hipSuccess;
  const size_t per = sweep_rep_bytes(T, N, r, nbp);
  if (ws_bytes < per + 4096) return hipErrorInvalidValue;
  const int nc = (int)std::min<size_t>(std::min<size_t>((ws_bytes - 4096) / per, SW_CHUNK_MAX), (size_t)nb);
  double *Er = (double *)ws, *prep = Er + (size_t)nc * T * N, *cur = prep + (size_t)nc * nbp * 2 * RC * RC;
  const size_t cs = (size_t)nc * nbp * N;   // one statistic's curves
  auto timed = [&](int begin) { if (tf) tf(tctx, DFM_KC_CHOW, begin); };
  for (int c0 = 0; c0 < nb; c0 += nc) {
    const int n = std::min(nc, nb - c0);
    PanelSrc ps = src;
    if (ps.idx) ps.idx += (int64_t)c0 * src.rs;
    if (ps.eta) ps.eta += (int64_t)c0 * src.rs;
    const double *Fc = F + (size_t)c0 * T * r, *Lc = Lm + (size_t)c0 * N * r;
    timed(1);
    hipLaunchKernelGGL(chow_sweep_resid_kernel, dim3((unsigned)(((int64_t)T * N + 255) / 256), n), dim3(256), 0, st, ps,
                       T, N, r, Fc, Lc, Er);
    timed(0);
    timed(1);
    hipLaunchKernelGGL(chow_sweep_scan_kernel, dim3(n), dim3(256), 0, st, Fc, T, r, bp_lo, nbp, RC, prep);
    hipLaunchKernelGGL(chow_sweep_inv_kernel, dim3((unsigned)(((int64_t)n * nbp + SW_IW - 1) / SW_IW)),
                       dim3(64 * SW_IW), sweep_inv_lds(RC), st, r, (int64_t)n * nbp, RC, prep);
    timed(0);
    const dim3 grid(1, (N + 63) / 64, n);
    for (int pass = 0; pass < 2; ++pass) {   // 0: LR / LM, 1: Wald
      if (pass == 0 ? !(want[0] || want[1]) : !want[2]) continue;
      double *cLR = want[0] ? cur : nullptr, *cLM = want[1] ? cur + cs : nullptr, *cWD = cur + 2 * cs;
      timed(1);
      if (RC == 4) launch_sweep_r<4>(pass, grid, T, N, r, bp_lo, nbp, Fc, Er, prep, cLR, cLM, cWD, st);
      else if (RC == 8) launch_sweep_r<8>(pass, grid, T, N, r, bp_lo, nbp, Fc, Er, prep, cLR, cLM, cWD, st);
      else launch_sweep_r<16>(pass, grid, T, N, r, bp_lo, nbp, Fc, Er, prep, cLR, cLM, cWD, st);
      timed(0);
    }
    SweepReduce ra{};
    bool any = false;
    for (int s = 0; s < 3; ++s) {
      if (!want[s]) continue;
      if (out.curve[s]) {
        const hipError_t e = hipMemcpyAsync(out.curve[s] + (size_t)c0 * nbp * N, cur + s * cs, (size_t)n * nbp * N * 8,
                                            hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return e;
      }
      if (!out.sup[s] && !out.argsup[s]) continue;
      ra.cur[s] = cur + s * cs;
      ra.sup[s] = out.sup[s] ? out.sup[s] + (int64_t)c0 * out.os : nullptr;
      ra.arg[s] = out.argsup[s] ? out.argsup[s] + (int64_t)c0 * N : nullptr;
      any = true;
    }
    if (any) {
      timed(1);
      hipLaunchKernelGGL(chow_sweep_reduce_kernel, dim3((unsigned)(((int64_t)n * N + 255) / 256), 3), dim3(256), 0, st,
                         ra, nbp, N, n, bp_lo, out.os);
      timed(0);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace dfm
