// dfm_fact.hip — the factored bootstrap top-k solver (eig_run_factored): the
// replicate Grams G* are never formed.  It shares the workspace record, the
// init / small / final kernels and the filter coefficients with the
// explicit-Gram solver of dfm_eig.hip through dfm_eig.h.
//
// Factored bootstrap (N > T).  With X* = F L' + D P E  (F = F_r, L = L_r of the
// base fit, D = diag(eta), P the row selection of idx; src/bootstrap.jl:45):
//   G* Q = X* X*' Q = F [S a + (EL)' Z] + D P [(EL) a + H Z]
//   a = F'Q (r x p), Z = P' D Q (T x p, scatter through a CSR of idx),
//   S = L'L, EL = E L (T x r), H = E E' (T x T)  — S, EL, H shared by all
// replicates.  H Z for a whole batch is ONE MFMA GEMM (dfm_gemm.hip) with H
// resident in L2; everything else is O(T r p) per replicate.
#include "dfm_eig.h"
#include "dfm_fact_plan.h"
#include "dfm_fact_ws.h"
#include <algorithm>
#include <cmath>
#include <type_traits>

namespace dfm {

static_assert(kFilterDMax == kChebDMax, "the plan's products and shifted_cheb's coefficients share one highest degree");

// waves per replicate workgroup of the factored passes (prep, y2, ap2, Chebyshev)
constexpr int BW = 4;

// (Z's replicate-major chunk indexing, zrm_ix, is in dfm_internal.h; the fp32
// middle products' Z32 and HZ32 use it with float elements, Z32 in the first
// half of Z's region, HZ32 in HZ's)
typedef float zf4 __attribute__((ext_vector_type(4)));

// A staged 16-row Z chunk (st: 16 pz doubles, element 16 c + row, this wave's LDS) to replicate rep's chunk `tile` of
// Zc as whole 16-B pieces, in the format the next H.Z product reads: fp64, float (round to nearest, the same chunk
// indexing with float elements) or the chunk's 6 pz pieces of the three bf16 planes (dfm_internal.h: Zs; planes = 2:
// the 4 pz pieces of planes h and m alone).
template <int P>
DFM_DEV void zchunk_store(ZFmt zf, const double *st, double *__restrict__ Zc, int rep, int64_t zrs, int tile, int pz,
                          int lane, int planes) {
  if (zf == ZFmt::Split) {
    zsplit_store_chunk<P == 16>(st, pz, lane, reinterpret_cast<char *>(Zc + (int64_t)rep * zrs) +
                                                  (int64_t)__builtin_amdgcn_readfirstlane(tile) * 96 * pz, planes);
  } else if (zf != ZFmt::F64) {
    zf4 *zc4 = reinterpret_cast<zf4 *>(reinterpret_cast<float *>(Zc) + (int64_t)rep * zrs + (int64_t)tile * 16 * pz);
    for (int e = lane; e < 4 * pz; e += 64)
      zc4[e] = zf4{(float)st[4 * e], (float)st[4 * e + 1], (float)st[4 * e + 2], (float)st[4 * e + 3]};
  } else {
    double2 *zc2 = reinterpret_cast<double2 *>(Zc + (int64_t)rep * zrs + (int64_t)tile * 16 * pz);
    for (int e = lane; e < 8 * pz; e += 64) zc2[e] = double2{st[2 * e], st[2 * e + 1]};
  }
}

// a = F'Q0 of the first product for the whole batch: F and the warm start Q0
// are shared by every replicate, so this one workgroup forms the 16 x P block
// once, into apre in ab's layout; boot_prep_kernel copies it into every
// replicate's ab.  Tiles per wave and the wave sums run in the order of the
// per-replicate passes' a = F'Qn (boot_ap2_kernel, boot_cheb_kernel).
template <int P>
__global__ __launch_bounds__(64 * BW) void prep_a_kernel(FactBase fb, const double *__restrict__ Q0, int ps,
                                                         double *__restrict__ apre) {
  constexpr int NT = P / 16;
  __shared__ double sred[NT * 256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4, T = fb.T, r = fb.r;
  const int ntile = (T + 15) >> 4;
  dv4 aacc[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) aacc[ct] = dv4{0.0, 0.0, 0.0, 0.0};
  for (int tile = wave; tile < ntile; tile += BW) {
    const int t0 = tile * 16;
    double fa[4], qv[NT][4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int t = t0 + 4 * g + lk;
      const int tc = min(t, T - 1);
      fa[g] = (t < T && li < r) ? fb.F[(int64_t)tc * r + li] : 0.0;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct)
        qv[ct][g] = (t < T && 16 * ct + li < ps) ? Q0[(int64_t)tc * ps + 16 * ct + li] : 0.0;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) aacc[ct] = mfma16(fa[g], qv[ct][g], aacc[ct]);
  }
  // (the four-wave sum of wave_block_store, written out: see there)
  for (int wv = 0; wv < BW; ++wv) {
    if (wave == wv)
#pragma unroll
      for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int e = (ct * 4 + g) * 64 + lane;
          sred[e] = (wv ? sred[e] : 0.0) + aacc[ct][g];
        }
    __syncthreads();
  }
  for (int e = tid; e < NT * 256; e += 64 * BW) {
    const int l = e & 63, g = (e >> 6) & 3, ct = e >> 8;
    apre[(4 * g + (l >> 4)) * P + 16 * ct + (l & 15)] = sred[e];
  }
}

// Shared tail of prep, ap2 and the last Horner step: Z = P' D Qn by CSR gather (bucket s lists t ascending),
// cc = EL' Z, and ab[rep] = [a (16 x P); cc (16 x P)], a = F' Qn, with fixed-order wave sums.
// From ap2 / the last Horner step (PREP = false) a is the caller's accumulator aacc and Z is stored directly.  From
// prep (PREP = true) a is copied from apre (prep_a_kernel), a tile's Z chunk (16 rows x pz, contiguous in the
// replicate-major layout) leaves through this wave's LDS stage zst (16 pz doubles) as 16-B pieces instead of one
// 128-B-strided element per lane, in the format zf (zchunk_store), and the same rows go to pvr (PV) if set.
// The staged store measured -3 % in prep and +0.3 % in ap2 / the last Horner step (profiles/r06_c3_ab.txt item 13),
// so those store directly.
struct PrepTail {   // PREP = true
  const double *apre;
  double *zst, *pvr;
  ZFmt zf;
  int planes;   // of a Split Z0 (FilterPlan::z0_planes)
};
struct AccTail {   // PREP = false
  const dv4 *aacc;
};
template <bool PREP> using TailSrc = std::conditional_t<PREP, PrepTail, AccTail>;
template <int P, bool PREP>
DFM_DEV void zscatter_tail(const FactBase &fb, int T, int r, int ntile, int tid, int wave, int lane,
                           const double *set, const int *so, const int *sl, const double *Qn,
                           double *__restrict__ Zc, int pz, int rep, double *__restrict__ ab, double *sred, int ps,
                           TailSrc<PREP> src) {
  const int64_t zrs = zrm_stride(T, pz);
  constexpr int NT = P / 16;
  const int li = lane & 15, lk = lane >> 4;
  dv4 cacc[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) cacc[ct] = dv4{0.0, 0.0, 0.0, 0.0};
  for (int tile = wave; tile < ntile; tile += BW) {
    const int s0 = tile * 16;
    // all four row groups' first GU bucket entries are fetched together
    // (independent loads in flight); longer buckets finish serially
    constexpr int GU = 3;
    double z[4][NT];
    int qn0[4], qn1[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int s = s0 + 4 * g + lk;
      qn0[g] = s < T ? so[s] : 0;
      qn1[g] = s < T ? so[s + 1] : 0;
    }
    double val[4][GU][NT], ev[4][GU];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int u = 0; u < GU; ++u) {
        const int q = qn0[g] + u;
        const bool ok = q < qn1[g];
        const int t = sl[ok ? q : 0];
        ev[g][u] = ok ? set[t] : 0.0;
        // (lanes past their bucket issue no load: most second / third entries
        // are empty, and these passes are bound by the texture-address unit)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
          val[g][u][ct] = (ok && 16 * ct + li < ps) ? Qn[(int64_t)t * ps + 16 * ct + li] : 0.0;
      }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        double acc = 0.0;
#pragma unroll
        for (int u = 0; u < GU; ++u) acc = fma(ev[g][u], val[g][u][ct], acc);
        z[g][ct] = acc;
      }
      for (int q = qn0[g] + GU; q < qn1[g]; ++q) {
        const int t = sl[q];
        const double e = set[t];
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
          z[g][ct] = fma(e, 16 * ct + li < ps ? Qn[(int64_t)t * ps + 16 * ct + li] : 0.0, z[g][ct]);
      }
    }
    if constexpr (PREP) {
      if (src.pvr) {   // the same rows as PV = P'D Qn in boot_cheb_mid_kernel's layout (compact rows, ps columns)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int s = s0 + 4 * g + lk;
          if (s < T)
#pragma unroll
            for (int ct = 0; ct < NT; ++ct)
              if (16 * ct + li < ps) src.pvr[(int64_t)s * ps + 16 * ct + li] = z[g][ct];
        }
      }
      // (rows past T: 0, the chunk's pad-row value the H.Z GEMM's k-padding needs)
      double *zst = src.zst;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the previous tile's staged reads are done
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
          if (16 * ct + li < pz) zst[16 * (16 * ct + li) + 4 * g + lk] = s0 + 4 * g + lk < T ? z[g][ct] : 0.0;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      zchunk_store<P>(src.zf, zst, Zc, rep, zrs, tile, pz, lane, src.planes);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int s = s0 + 4 * g + lk;
      const bool v = s < T;
      const double ea = (v && li < r) ? fb.EL[(int64_t)s * r + li] : 0.0;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        if (!PREP && v && 16 * ct + li < pz) Zc[zrm_ix(rep, s, 16 * ct + li, pz, zrs)] = z[g][ct];
        cacc[ct] = mfma16(ea, z[g][ct], cacc[ct]);
      }
    }
  }
  double *abr = ab + (int64_t)rep * 32 * P;
  if constexpr (PREP)
    for (int e = tid; e < 16 * P; e += 64 * BW) abr[e] = src.apre[e];
  // (the four-wave sum of wave_block_store, written out: see there)
  for (int pass = PREP ? 1 : 0; pass < 2; ++pass) {
    for (int wv = 0; wv < BW; ++wv) {
      if (wave == wv)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int e = (ct * 4 + g) * 64 + lane;
            double v = cacc[ct][g];
            if constexpr (!PREP) v = pass ? v : src.aacc[ct][g];
            sred[e] = (wv ? sred[e] : 0.0) + v;
          }
      __syncthreads();
    }
    for (int e = tid; e < NT * 256; e += 64 * BW) {
      const int l = e & 63, g = (e >> 6) & 3, ct = e >> 8;
      abr[pass * 16 * P + (4 * g + (l >> 4)) * P + 16 * ct + (l & 15)] = sred[e];
    }
    __syncthreads();
  }
}

// Per replicate: CSR of idx (bucket s lists t ascending — fixed summation order, bit-reproducible), PF = P'D F and e2
// = P'D^2 1 for the middle Horner steps, and trace(G*) = sum_t ||x*_t||^2 = sum_t [F_t S F_t' + 2 eta_t
// F_t.(EL)_idx_t + eta_t^2 H_idx_t,idx_t]; then, from the CSR it still holds in LDS, the first H.Z product's operand
// Z0 = P'D Q0 and the first step's ab = [a; cc] (a = F'Q0 from apre, prep_a_kernel; cc = EL'Z0) through
// zscatter_tail.  Q0, Zc, ab and apre are required; PF, E2, PV, FV are optional outputs.
template <int P>
__global__ __launch_bounds__(64 * BW) void boot_prep_kernel(FactBase fb, const int32_t *__restrict__ idx,
                                                            const double *__restrict__ eta, int *__restrict__ off,
                                                            int *__restrict__ lst, double *__restrict__ trace,
                                                            double *__restrict__ PF, double *__restrict__ E2,
                                                            const double *__restrict__ Q0, int ps,
                                                            double *__restrict__ Zc, int64_t ldz, int pz,
                                                            double *__restrict__ ab, const double *__restrict__ apre,
                                                            double *__restrict__ PV, double *__restrict__ FV, ZFmt zf,
                                                            int zplanes) {
  // zf: the format Z0 leaves in (the first product's operand, FilterPlan::z0; zplanes: the planes of a Split one,
  // FilterPlan::z0_planes); PV, FV, a, cc stay fp64
  static_assert(64 * BW == 256, "the scans and the tree sum below are written for 256 threads");
  constexpr int NT = P / 16;
  __shared__ double sred[NT * 256];
  __shared__ double zst[BW][16 * P];   // per-wave Z chunk staging (zscatter_tail)
  extern __shared__ int sh[];   // cnt[T+1], six[T], sorted list L[T] (+ so[T+1], eta[T]: Zc)
  __shared__ double red[256];
  __shared__ int scan[256];
  const int tid = threadIdx.x, rep = blockIdx.x, T = fb.T, r = fb.r;
  const int32_t *ix = idx + (int64_t)rep * T;
  const double *et = eta ? eta + (int64_t)rep * T : nullptr;
  int *cnt = sh, *six = sh + T + 1;
  for (int s = tid; s <= T; s += 256) cnt[s] = 0;
  for (int t = tid; t < T; t += 256) six[t] = ix[t];
  __syncthreads();
  for (int t = tid; t < T; t += 256) atomicAdd(&cnt[six[t] + 1], 1);
  __syncthreads();
  // inclusive scan of cnt[0..T]: per-thread chunks, a 256-wide scan of the chunk sums
  const int per = (T + 1 + 255) / 256, c0 = min(T + 1, tid * per), c1 = min(T + 1, c0 + per);
  int run = 0;
  for (int s = c0; s < c1; ++s) run += cnt[s];
  scan[tid] = run;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int v = tid >= o ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  run = scan[tid] - run;
  for (int s = c0; s < c1; ++s) { run += cnt[s]; cnt[s] = run; }   // cnt[s] = start of bucket s
  __syncthreads();
  for (int s = tid; s <= T; s += 256) off[(int64_t)rep * (T + 1) + s] = cnt[s];
  __syncthreads();
  // placement: LDS atomics hand out slots inside each bucket (any order), then each bucket is insertion-sorted by t —
  // ascending t per bucket, the serial counting sort's order, in O(T) work (buckets are short) (in LDS, then one
  // coalesced copy out: the shifts of a sort in global memory were chains of dependent global round trips)
  int *L = sh + 2 * T + 1;
  for (int t = tid; t < T; t += 256) L[atomicAdd(&cnt[six[t]], 1)] = t;
  __syncthreads();   // cnt[s] is now the END of bucket s; L visible workgroup-wide
  for (int s = tid; s < T; s += 256) {
    const int b0 = s ? cnt[s - 1] : 0, b1 = cnt[s];
    for (int i = b0 + 1; i < b1; ++i) {
      const int v = L[i];
      int j = i - 1;
      while (j >= b0 && L[j] > v) { L[j + 1] = L[j]; --j; }
      L[j + 1] = v;
    }
  }
  __syncthreads();
  for (int t = tid; t < T; t += 256) lst[(int64_t)rep * T + t] = L[t];
  // LDS after the sorted list: bucket starts so[0..T] and eta_t (PF below, zscatter_tail)
  int *so = sh + 3 * T + 1;
  double *set = reinterpret_cast<double *>(sh + ((4 * T + 2 + 1) & ~1));
  for (int q = tid; q <= T; q += 256) so[q] = q ? cnt[q - 1] : 0;
  for (int t = tid; t < T; t += 256) set[t] = et ? et[t] : 1.0;
  __syncthreads();
  if (E2 && !PF)   // P'D^2 1 alone: the middle steps take P'D F from PV's rows (boot_cheb_mid_kernel's NOPF)
    for (int s = tid; s < T; s += 256) {   // the same walk and sums as below, LDS only
      const int b0 = s ? cnt[s - 1] : 0, b1 = cnt[s];
      double a2 = 0.0;
      for (int q = b0; q < b1; ++q) {
        const double h = set[L[q]];
        a2 = fma(h, h, a2);
      }
      E2[(int64_t)rep * T + s] = a2;
    }
  if (PF)   // P'D F (row stride r) and P'D^2 1 of the middle Horner steps (boot_cheb_mid_kernel):
    for (int s = tid; s < T; s += 256) {   // this thread's own sorted buckets, t ascending
      const int b0 = s ? cnt[s - 1] : 0, b1 = cnt[s];
      double a[16], a2 = 0.0;
#pragma unroll
      for (int j = 0; j < 16; ++j) a[j] = 0.0;
      for (int q = b0; q < b1; ++q) {
        const int t = L[q];
        const double h = set[t];
        a2 = fma(h, h, a2);
        if ((r & 1) == 0) {   // 16-B loads of the F row (F rows start 16-B aligned)
          const double2 *f2 = reinterpret_cast<const double2 *>(fb.F + (int64_t)t * r);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (2 * j < r) {
              const double2 f = f2[j];
              a[2 * j] = fma(h, f.x, a[2 * j]);
              a[2 * j + 1] = fma(h, f.y, a[2 * j + 1]);
            }
        } else {
#pragma unroll
          for (int j = 0; j < 16; ++j)
            if (j < r) a[j] = fma(h, fb.F[(int64_t)t * r + j], a[j]);
        }
      }
      double *pf = PF + ((int64_t)rep * T + s) * r;
      if ((r & 1) == 0) {   // 16-B stores (rows start 16-B aligned for even r)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (2 * j < r) reinterpret_cast<double2 *>(pf)[j] = double2{a[2 * j], a[2 * j + 1]};
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
          if (j < r) pf[j] = a[j];
      }
      E2[(int64_t)rep * T + s] = a2;
    }
  {
    const int lane = tid & 63, wave = tid >> 6;
    const int ntile = (T + 15) >> 4;
    // the last chunk's rows past T (the H.Z GEMM's zero k-padding of B)
    {
      const int64_t zrs = zrm_stride(T, pz);
      const int npad = ((T + 15) & ~15) - T;
      if (zf == ZFmt::Split) {   // (the staged store writes the whole last chunk, its zero pad rows included)
      } else if (zf != ZFmt::F64)
        for (int e = tid; e < npad * pz; e += 256)
          reinterpret_cast<float *>(Zc)[zrm_ix(rep, T + e / pz, e % pz, pz, zrs)] = 0.0f;
      else
        for (int e = tid; e < npad * pz; e += 256) Zc[zrm_ix(rep, T + e / pz, e % pz, pz, zrs)] = 0.0;
    }
    __syncthreads();   // so / set visible
    // (PV, FV: a warm solve without a first Rayleigh-Ritz step filters V0 = Q0 itself, so the middle Horner
    // steps' PV = P'D V0 is Z0 row by row and FV = F'V0 is a)
    zscatter_tail<P, true>(fb, T, r, ntile, tid, wave, lane, set, so, L, Q0, Zc, pz, rep, ab, sred, ps,
                           PrepTail{apre, zst[wave], PV ? PV + (int64_t)rep * T * P : nullptr, zf, zplanes});
    if (FV)
      for (int e = tid; e < 16 * P; e += 256) FV[(int64_t)rep * 16 * P + e] = apre[e];
  }
  double acc = 0.0;
  for (int t = tid; t < T; t += 256) {
    const int i = ix[t];
    const double e = et ? et[t] : 1.0;
    double fe = 0.0;
    if ((r & 1) == 0) {   // F and EL rows as 16-B pieces (half the load instructions; same fma order)
      const double2 *f2 = reinterpret_cast<const double2 *>(fb.F + (int64_t)t * r);
      const double2 *e2 = reinterpret_cast<const double2 *>(fb.EL + (int64_t)i * r);
      double2 fv[8], ev[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (2 * j < r) { fv[j] = f2[j]; ev[j] = e2[j]; }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (2 * j < r) { fe = fma(fv[j].x, ev[j].x, fe); fe = fma(fv[j].y, ev[j].y, fe); }
    } else {
      for (int j = 0; j < r; ++j) fe = fma(fb.F[(int64_t)t * r + j], fb.EL[(int64_t)i * r + j], fe);
    }
    acc += fb.cF[t] + 2.0 * e * fe + e * e * fb.hd[i];
  }
  red[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
  if (tid == 0) trace[rep] = red[0];
}

size_t fact_workspace_bytes(int T, int nb, int P) { return fact_ws_layout(T, nb, P, P).total; }

// ================================================= fused factored iteration
// For T <= F2_T_MAX and r <= 16 (C3: T = 500, r = 8) one iteration of
// the factored solver is four launches instead of five, with no per-row-block
// partial arrays and no separate convergence pass:
//   GEMM  HZ = H Z                          (shared H, all unconverged replicates)
//   y2    Y = F (S a + cc) + D (EL[idx] a + HZ[idx]),  Q'Y, Y'Y, Q'Q   (one WG / replicate)
//   small Rayleigh-Ritz on p x p            (eig_small_kernel, nrb = 1)
//   ap2   U = Q A, Qn = Y Bm, residuals ||Y A - U diag(theta)|| -> converged?
//         else Z = P' D Qn (CSR gather from an LDS image), a = F'Qn, cc = EL'Z
// Every T x P product is a v_mfma_f64_16x16x4 chain whose operands are the
// rows a lane already holds: A[i][k] at lane i + 16k, B[k][j] at lane j + 16k,
// C[row][col] at lane col + 16 (row % 4), register row / 4
// (tools/mfma16_layout.hip).  An accumulator register g holds rows
// 4g .. 4g+3 in exactly the B-operand layout, so Q'Y etc. need no lane movement.
// Reductions over waves run in a fixed order: bit-reproducible, batch-invariant.
constexpr int F2_T_MAX = 4096;

// Convergence verdict from per-column squared residuals res2[j] (j < k), on
// one whole wave: the rule is column_verdict / energy_converged (dfm_eig.h).
DFM_DEV bool decide_converged(const double *res2, const double *th, const double *prev, double *next,
                              int k, int p, double tol, double trace, int itc, int subspace) {
  const int lane = threadIdx.x & 63;
  const double th0 = fabs(th[0]);
  bool okall = true, floor_ok = true;
  double bsum = 0.0, tsum = 0.0;
  for (int j = lane; j < k; j += 64) {
    const ColumnVerdict v = column_verdict(res2[j], j, th, th0, prev, k, p, tol, itc, subspace);
    if (tol < 0.0) {
      bsum += v.bnd;
      tsum += th[j];
    }
    floor_ok = floor_ok && v.floor;
    okall = okall && v.ok;
    next[j] = v.res;
  }
  bool ok = !__any(!okall);
  if (tol < 0.0) {
    bsum = wave_sum(bsum);
    tsum = wave_sum(tsum);
    ok = ok && energy_converged(bsum, tsum, trace, tol, floor_ok);
  }
  return ok;
}

#ifdef DFM_DIAG_X
// diagnostic build only (tools/c3_excess.py): how far each replicate's
// eigenvalue-bound test is from passing at Rayleigh-Ritz step it + 1
__device__ double g_diag_x[4][16384];
DFM_DEV void diag_excess(const double *res2, const double *th, int k, int p, double tol, double trace, int rep,
                         int it) {
  const int lane = threadIdx.x & 63;
  double r1 = 0.0, bsum = 0.0, tsum = 0.0;
  for (int j = lane; j < k; j += 64) {
    const double gap = fmin(j > 0 ? fabs(th[j] - th[j - 1]) : INFINITY, j + 1 < p ? fabs(th[j] - th[j + 1]) : INFINITY);
    const double bnd = res2[j] / (0.5 * gap);
    bsum += bnd; tsum += th[j];
    r1 = fmax(r1, bnd / (-tol * fabs(th[j])));
  }
  bsum = wave_sum(bsum); tsum = wave_sum(tsum);
  for (int o = 32; o >= 1; o >>= 1) r1 = fmax(r1, __shfl_xor(r1, o));
  const double vnum = fmax(fabs(trace - tsum), 1e-6 * fabs(trace));
  const double x = fmax(r1, bsum / (-tol * vnum));
  if (lane == 0 && it >= 0 && it < 4 && rep < 16384) g_diag_x[it][rep] = x;
}
extern "C" int dfm_diag_read_x(double *out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag_x), sizeof(g_diag_x)) == hipSuccess ? 0 : -1;
}
#endif

// One 16-row tile's operands for y2: F / EL[idx] rows in A-operand layout
// (row t0 + (lane & 15), factor 4kk + (lane >> 4)), HZ[idx] and Q in the
// accumulator layout (row t0 + 4g + (lane >> 4), column 16ct + (lane & 15)).
// Rows >= T load row T-1 and are masked by the consumer.
template <int P>
struct Y2Tile {
  double fA[4], eA[4], hz[P / 16][4], q[P / 16][4];
};
// STG (P = 16, even r <= 8, pz <= 16; y2 and the last Horner step — y2
// reads its MFMA B operands from LDS per tile when staged, else the staged
// form spills: 128 VGPRs + 52 B of scratch, y2 60 % slower, profiles/
// r06_c3_ab.txt items 19 and 23): every
// operand of the tile arrives as 16-B pieces through this wave's LDS stage
// (stg, Y2_STG doubles) — the F rows as one contiguous range, each EL[idx]
// and HZ[idx] row as r / 2 and pz / 2 pieces, the Q rows as one contiguous
// range — and is transposed to its register layout there: half the load
// requests of one-double-per-lane loads, for passes bound by the texture-
// address unit.  Stage layout: F rows [0, 144) (kept for the
// caller's accumulator-layout read of F, fa), EL rows [144, 288), then HZ
// and Q rows over [144, 688) once the EL reads are done.
constexpr int Y2_STG = 16 * 9 + 2 * 16 * 17;
template <int P, bool STG = false>
DFM_DEV void y2_load(Y2Tile<P> &L, int tile, int T, int r, int KR, int lane, const int *six, const FactBase &fb,
                     const double *__restrict__ HZ, int64_t ldz, int pz, int rep, const double *__restrict__ Qr,
                     int ps, double *stg = nullptr) {
  constexpr int NT = P / 16;
  const int li = lane & 15, lk = lane >> 4, t0 = tile * 16;
  const int ta = min(t0 + li, T - 1);
  if constexpr (STG) {
    static_assert(P == 16, "the staged loader covers one 16-column block");
    const int nrow = min(16, T - t0), hr = r >> 1, hp = pz >> 1, hq = ps >> 1;
    // issue every piece first (F, EL: 8 r <= 64 pieces; HZ, Q: 8 pz, 8 ps <= 128)
    double2 fv, ev, hv[2], qv[2];
    {
      const int row = hr ? lane / hr : 0, jp = lane - row * hr;
      const bool ok = lane < nrow * hr;
      fv = ok ? reinterpret_cast<const double2 *>(fb.F + (int64_t)t0 * r)[lane] : double2{0.0, 0.0};
      ev = ok ? reinterpret_cast<const double2 *>(fb.EL + (int64_t)six[t0 + row] * r)[jp] : double2{0.0, 0.0};
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = u * 64 + lane;
      const int row = e / hp, jp = e - row * hp;
      const bool okh = e < nrow * hp;
      hv[u] = okh ? reinterpret_cast<const double2 *>(HZ + (int64_t)six[t0 + row] * ldz + (int64_t)rep * pz)[jp]
                  : double2{0.0, 0.0};
      const bool okq = e < nrow * hq;
      qv[u] = okq ? reinterpret_cast<const double2 *>(Qr + (int64_t)t0 * ps)[e] : double2{0.0, 0.0};
    }
    const int RF = r + 1, RH = pz + 1, RQ = ps + 1;
    double *sF = stg, *sE = stg + 16 * 9;         // (RF <= 9)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the previous tile's staged reads are done
    if (lane < 16 * hr) {
      const int row = lane / hr, j = 2 * (lane - row * hr);
      sF[row * RF + j] = fv.x; sF[row * RF + j + 1] = fv.y;
      sE[row * RF + j] = ev.x; sE[row * RF + j + 1] = ev.y;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const bool ok = kk < KR && 4 * kk + lk < r && t0 + li < T;
      L.fA[kk] = ok ? sF[li * RF + 4 * kk + lk] : 0.0;
      L.eA[kk] = ok ? sE[li * RF + 4 * kk + lk] : 0.0;
    }
    double *sH = stg + 16 * 9, *sQ = sH + 16 * 17;   // over EL (read above), after F (kept for fa)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int e = u * 64 + lane;
      if (e < 16 * hp) {
        const int row = e / hp, j = 2 * (e - row * hp);
        sH[row * RH + j] = hv[u].x; sH[row * RH + j + 1] = hv[u].y;
      }
      if (e < 16 * hq) {
        const int row = e / hq, j = 2 * (e - row * hq);
        sQ[row * RQ + j] = qv[u].x; sQ[row * RQ + j + 1] = qv[u].y;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      L.hz[0][g] = li < pz ? sH[(4 * g + lk) * RH + li] : 0.0;
      L.q[0][g] = li < ps ? sQ[(4 * g + lk) * RQ + li] : 0.0;
    }
    return;
  } else {
    const int ia = six[ta];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int j = max(0, min(4 * kk + lk, r - 1));   // never index -1 (r = 0: expanding windows)
      L.fA[kk] = (kk < KR && 4 * kk + lk < r && t0 + li < T) ? fb.F[(int64_t)ta * r + j] : 0.0;
      L.eA[kk] = (kk < KR && 4 * kk + lk < r && t0 + li < T) ? fb.EL[(int64_t)ia * r + j] : 0.0;
    }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int t = min(t0 + 4 * g + lk, T - 1);
    const int i = six[t];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
      const int c = 16 * ct + li;
      L.hz[ct][g] = c < pz ? HZ[(int64_t)i * ldz + (int64_t)rep * pz + c] : 0.0;   // compact Z / HZ: pz columns
      L.q[ct][g] = c < ps ? Qr[(int64_t)t * ps + c] : 0.0;   // compact rows: ps columns
    }
  }
}

// sa = a, sb = S a + cc (16 x P each, rows >= r of S a zero) from ab[rep] =
// [a; cc]: the B operands of the tile products of y2 and the Horner steps.
// Ends on a barrier.
template <int P>
DFM_DEV void load_ab(const FactBase &fb, const double *abr, double *sa, double *sb, int tid, int r) {
  for (int e = tid; e < 16 * P; e += 64 * BW) sa[e] = abr[e];
  __syncthreads();
  for (int e = tid; e < 16 * P; e += 64 * BW) {
    const int j = e / P, c = e % P;
    double v = abr[16 * P + e];
    if (j < r)
      for (int i = 0; i < r; ++i) v = fma(fb.S[j * r + i], sa[i * P + c], v);
    sb[e] = v;
  }
  __syncthreads();
}

// A replicate's image in dynamic LDS: eta (T doubles; 1 without eta), then
// idx (T ints) if IDX, then the CSR — bucket starts (T + 1 ints) and the
// sorted list (T ints) — if CSR; the pointers of an absent piece are passed
// as null.  No barrier: the caller's next one publishes it.
// (The pieces are template flags, not tests of the pointers: with the tests
// at run time y2 and the last Horner step grew by 12 and 51 instructions,
// profiles/r11_fact_refactor.txt section 1.)
struct RepLds {
  double *set;
  int *six, *so, *sl;
};
template <bool IDX, bool CSR>
DFM_DEV RepLds load_rep_lds(double *sdyn, int T, int tid, int rep, const int32_t *__restrict__ idx,
                            const double *__restrict__ eta, const int *__restrict__ off,
                            const int *__restrict__ lst) {
  RepLds s;
  s.set = sdyn;
  s.six = (int *)(sdyn + T);
  s.so = IDX ? s.six + T : s.six;
  s.sl = s.so + T + 1;
  const int32_t *ixg = IDX ? idx + (int64_t)rep * T : nullptr;
  const double *etg = eta ? eta + (int64_t)rep * T : nullptr;
  const int *o = CSR ? off + (int64_t)rep * (T + 1) : nullptr;
  const int *L = CSR ? lst + (int64_t)rep * T : nullptr;
  for (int e = tid; e < T; e += 64 * BW) {
    if constexpr (IDX) s.six[e] = ixg[e];
    s.set[e] = etg ? etg[e] : 1.0;
    if constexpr (CSR) { s.so[e] = o[e]; s.sl[e] = L[e]; }
  }
  if (CSR && tid == 0) s.so[T] = o[T];
  return s;
}

// One tile's yF = F bB and yE = EL[idx] a (16 x P each): A operands fA / eA of
// the tile (Y2Tile), B operands sb / sa — from registers (bA, bB: the copies
// y2 and the last Horner step hold) or, LDSB, re-read from LDS per tile.
template <int P, bool LDSB>
DFM_DEV void tile_yfe(const Y2Tile<P> &t, int KR, int li, int lk, const double *sa, const double *sb,
                      const double (*bA)[P / 16], const double (*bB)[P / 16], dv4 *yF, dv4 *yE) {
  constexpr int NT = P / 16;
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) { yF[ct] = dv4{0.0, 0.0, 0.0, 0.0}; yE[ct] = yF[ct]; }
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    if (kk < KR) {
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        if constexpr (LDSB) {
          yF[ct] = mfma16(t.fA[kk], sb[(4 * kk + lk) * P + 16 * ct + li], yF[ct]);
          yE[ct] = mfma16(t.eA[kk], sa[(4 * kk + lk) * P + 16 * ct + li], yE[ct]);
        } else {
          yF[ct] = mfma16(t.fA[kk], bB[kk][ct], yF[ct]);
          yE[ct] = mfma16(t.eA[kk], bA[kk][ct], yE[ct]);
        }
      }
    }
  }
}

// y2: one workgroup (4 waves) per replicate; wave w takes 16-row tiles w, w+4, ...
template <int P, bool STG>
// 4 workgroups per CU (~113 VGPRs, no spills; a tile is loaded at the top of
// its own iteration, no register prefetch of the next): these per-replicate
// passes are HBM-latency-bound, and resident waves buy more bandwidth than
// per-wave prefetch did (2 -> 4 WGs/CU: y2 -24 %, ap2 -13 %)
__global__ __launch_bounds__(64 * BW, 4) void boot_y2_kernel(FactBase fb, EigWork w, int T, const int32_t *__restrict__ idx,
                                                      const double *__restrict__ eta,
                                                      const double *__restrict__ HZ, int64_t ldz, int pz,
                                                      const double *__restrict__ ab,
                                                      const double *__restrict__ Qc, int64_t qs,
                                                      double *__restrict__ Yo, int ps) {
  constexpr int NT = P / 16;
  const int rep = blockIdx.x;
  if (w.done[rep]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = fb.r;
  const int li = lane & 15, lk = lane >> 4;
  __shared__ double sa[16 * P], sb[16 * P];          // a = F'Q, S a + cc  (rows >= r zero)
  __shared__ double red[3 * NT * NT * 256];
  extern __shared__ double sdyn[];                   // eta (T doubles), idx (T ints)
  __shared__ double stgy[STG ? BW : 1][STG ? Y2_STG : 1];   // per-wave operand staging (y2_load)
  const RepLds rl = load_rep_lds<true, false>(sdyn, T, tid, rep, idx, eta, nullptr, nullptr);
  const double *set = rl.set;
  const int *six = rl.six;
  load_ab<P>(fb, ab + (int64_t)rep * 32 * P, sa, sb, tid, r);
  const int KR = (r + 3) >> 2;
  double bA[4][NT], bB[4][NT];   // (STG: read from LDS per tile instead, to make room for the staged loader)
  if constexpr (!STG) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        bA[kk][ct] = sa[(4 * kk + lk) * P + 16 * ct + li];
        bB[kk][ct] = sb[(4 * kk + lk) * P + 16 * ct + li];
      }
  }
  dv4 acc[3][NT][NT];
#pragma unroll
  for (int m3 = 0; m3 < 3; ++m3)
#pragma unroll
    for (int a = 0; a < NT; ++a)
#pragma unroll
      for (int b = 0; b < NT; ++b) acc[m3][a][b] = dv4{0.0, 0.0, 0.0, 0.0};
  const double *Qr = Qc + (int64_t)rep * qs;   // qs = 0: the shared warm start (first step)
  double *Yr = Yo + (int64_t)rep * T * P;
  const int ntile = (T + 15) >> 4;
  // each tile's operands load at the top of its iteration (occupancy hides the latency)
  Y2Tile<P> cur;
  for (int tile = wave; tile < ntile; tile += BW) {
    y2_load<P, STG>(cur, tile, T, r, KR, lane, six, fb, HZ, ldz, pz, rep, Qr, ps, stgy[STG ? wave : 0]);
    const int t0 = tile * 16;
    dv4 yF[NT], yE[NT];
    tile_yfe<P, STG>(cur, KR, li, lk, sa, sb, bA, bB, yF, yE);
    double Yv[NT][4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int t = t0 + 4 * g + lk;
      const bool v = t < T;
      const double e = v ? set[t] : 0.0;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const int c = 16 * ct + li;
        const double y = v ? fma(e, yE[ct][g] + cur.hz[ct][g], yF[ct][g]) : 0.0;
        if (v && c < ps) Yr[(int64_t)t * ps + c] = y;
        Yv[ct][g] = y;
        if (!v) cur.q[ct][g] = 0.0;   // clamped row: no contribution to Q'Y, Q'Q
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int a = 0; a < NT; ++a)
#pragma unroll
        for (int b = 0; b < NT; ++b) {
          acc[0][a][b] = mfma16(cur.q[a][g], Yv[b][g], acc[0][a][b]);
          acc[1][a][b] = mfma16(Yv[a][g], Yv[b][g], acc[1][a][b]);
          acc[2][a][b] = mfma16(cur.q[a][g], cur.q[b][g], acc[2][a][b]);
        }
  }
  // fixed-order sum over the four waves (wave_block_store's, over 3 NT^2 blocks)
  for (int wv = 0; wv < BW; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int m3 = 0; m3 < 3; ++m3)
#pragma unroll
        for (int a = 0; a < NT; ++a)
#pragma unroll
          for (int b = 0; b < NT; ++b)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              const int e = ((m3 * NT + a) * NT + b) * 256 + g * 64 + lane;
              red[e] = (wv ? red[e] : 0.0) + acc[m3][a][b][g];
            }
    }
    __syncthreads();
  }
  double *pp = w.part + (int64_t)rep * 3 * P * P;
  for (int e = tid; e < 3 * NT * NT * 256; e += 64 * BW) {
    const int l = e & 63, g = (e >> 6) & 3, blk = e >> 8;
    const int b = blk % NT, a = (blk / NT) % NT, m3 = blk / (NT * NT);
    pp[m3 * P * P + (16 * a + 4 * g + (l >> 4)) * P + 16 * b + (l & 15)] = red[e];
  }
}

// End b of the Chebyshev filter's damping interval [0, b]: theta_p, the
// block's smallest Ritz value (above every unwanted eigenvalue once the block
// has converged a little), or after the first Rayleigh-Ritz step of a warm
// start at least bbeta * theta_k: there the guard columns' Ritz values are
// still far below lambda_p (C3: theta_16 ~ 0.8e3 vs lambda_17 ~ 8e3) and
// [0, theta_p] would leave most of the unwanted spectrum undamped, while the
// wanted theta_k is already accurate (b < theta_k keeps every wanted
// eigenvalue amplified; a b short of lambda_{p+1} only slows the filter).
template <int P>
DFM_DEV double filter_end(const double *small, int k, int p, double bbeta) {
  const double tp = small[2 * P * P + p - 1];
  return bbeta > 0.0 ? fmax(tp, bbeta * small[2 * P * P + k - 1]) : tp;
}

// One 16-row tile's operands for ap2 (ap2_load_lds): Q and Y rows in A-operand layout
// (row t0 + (lane & 15), column 4kk + (lane >> 4)) and F rows for a = F'Qn in
// A-operand layout per row group g (row t0 + 4g + (lane >> 4), factor lane & 15).
// Rows >= T read row T-1 (masked later).
template <int P>
struct Ap2Tile {
  double qa[P / 4], yo[P / 4], fa[4];
};

// The tile's Q and Y rows (16 x P each) through a wave-private LDS
// transpose: read with coalesced 16-B loads (4 lanes per 128-B row) and
// re-read from LDS in the MFMA A-operand layout (row lane & 15, column
// 4 kk + (lane >> 4)), instead of 2 P/4 loads that each touch 16 rows.
// Row stride P + 1: conflict-free A-layout reads.
template <int P>
DFM_DEV void ap2_load_lds(Ap2Tile<P> &L, int tile, int T, int r, int lane, const double *__restrict__ Qr,
                          const double *Yr, const FactBase &fb, double *tq, double *ty, int ps, bool ldf = true) {
  constexpr int KP = P / 4, PER = P / 4;   // doubles per lane per matrix
  const int li = lane & 15, lk = lane >> 4, t0 = tile * 16;
  {
    const int rr = lane >> 2, c0 = (lane & 3) * PER, t = t0 + rr;
    const bool ok = t < T;
    const int tc = ok ? t : T - 1;
    double2 qv[PER / 2], yv[PER / 2];
#pragma unroll
    for (int j = 0; j < PER / 2; ++j) {
      // compact rows (ps columns, ps even): pairs past ps are the zero columns
      const bool in = c0 + 2 * j < ps;
      qv[j] = in ? *reinterpret_cast<const double2 *>(Qr + (int64_t)tc * ps + c0 + 2 * j) : double2{0.0, 0.0};
      yv[j] = in ? *reinterpret_cast<const double2 *>(Yr + (int64_t)tc * ps + c0 + 2 * j) : double2{0.0, 0.0};
    }
#pragma unroll
    for (int j = 0; j < PER / 2; ++j) {
      tq[rr * (P + 1) + c0 + 2 * j] = ok ? qv[j].x : 0.0;
      tq[rr * (P + 1) + c0 + 2 * j + 1] = ok ? qv[j].y : 0.0;
      ty[rr * (P + 1) + c0 + 2 * j] = ok ? yv[j].x : 0.0;
      ty[rr * (P + 1) + c0 + 2 * j + 1] = ok ? yv[j].y : 0.0;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's writes land before its reads
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) {
      L.qa[kk] = tq[li * (P + 1) + 4 * kk + lk];
      L.yo[kk] = ty[li * (P + 1) + 4 * kk + lk];
    }
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int t = t0 + 4 * g + lk;
    const int tc = min(t, T - 1);
    // only lanes holding a factor column of a row < T load (r = 0, the
    // expanding windows' case without base factors, loads nothing)
    // (ldf = false, ap2's probe pass: no a = F'Qn there, no F rows)
    L.fa[g] = (ldf && t < T && li < r) ? fb.F[(int64_t)tc * r + li] : 0.0;
  }
}

// ap2: one workgroup per replicate, after the Rayleigh-Ritz step's eig_small.
// Qn goes to global memory (over the Y rows this wave just read)
// and is gathered back through the CSR after the barrier: same-CU L1, so the
// workgroup-scope fence of __syncthreads makes it visible.  Dynamic LDS:
// eta (T doubles), off (T+1 ints), lst (T ints) of this replicate.
// probe: decide before writing.  A first pass over the
// tiles forms only u = Q A, Y A and the residuals (Q and Y tiles in, the sAm
// MFMAs, no stores); the verdict follows as in the one-pass form.  A
// replicate that retires (or a last launch) takes the exit without ever
// having written V0 and Qn; one that goes on then runs the one-pass tile
// loop, its residuals discarded.  Every value that leaves the kernel is
// formed by the same instructions in the same order from the same inputs in
// both forms: rows, done, iters, the active counters and the residual record
// do not depend on probe.  The host sets it on the steps replicates are
// expected to retire at (eig_run_fact2_t).
template <int P>
// 4 workgroups per CU (see boot_y2_kernel)
__global__ __launch_bounds__(64 * BW, 4) void boot_ap2_kernel(FactBase fb, EigWork w, int T, int k, int p, double tol,
                                                       int it, int last, double fa1,
                                                       double fa0, double bbeta, const double *__restrict__ eta,
                                                       const int *__restrict__ off, const int *__restrict__ lst,
                                                       const double *__restrict__ Qc, int64_t qs,
                                                       double *__restrict__ Yq, double *__restrict__ Zc, int64_t ldz,
                                                       int pz, double *__restrict__ ab, uint64_t seed, int ps,
                                                       int probe) {
  constexpr int NT = P / 16, KP = P / 4;
  const int rep = blockIdx.x;
  if (w.done[rep]) return;
  extern __shared__ double sdyn[];
  __shared__ double sred[NT * 256];
  __shared__ double sres[BW][P];
  __shared__ double stile[BW][2][16 * (P + 1)];   // per-wave Q / Y tile transposes (ap2_load_lds)
  __shared__ int s_conv;
  __shared__ double sAm[P * P], sBm[P * P];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = fb.r;
  const int li = lane & 15, lk = lane >> 4;
  const RepLds rl = load_rep_lds<false, true>(sdyn, T, tid, rep, nullptr, eta, off, lst);
  const double *set = rl.set;
  const int *so = rl.so, *sl = rl.sl;
  double *small = w.small + (int64_t)rep * small_stride<P>();
  // the Rayleigh-Ritz step's A and Bm (P x P each) in LDS: the MFMA B
  // operands are read per tile instead of held in 2 KP NT registers (held in
  // registers the kernel sat at 128 VGPRs with 32 B of scratch)
  for (int e = tid; e < P * P; e += 64 * BW) {
    sAm[e] = small[e];
    sBm[e] = small[P * P + e];
  }
  double th[NT];
  bool dd[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    const int c = 16 * ct + li;
    th[ct] = small[2 * P * P + c];
    dd[ct] = small[2 * P * P + P + c] != 0.0;
  }
  __syncthreads();
  const double *Qr = Qc + (int64_t)rep * qs;   // (qs = 0: the warm start Q0, shared by every replicate)
  double *Yr = Yq + (int64_t)rep * T * P;
  // the filter's first Horner term (boot_cheb_kernel): S = (fa1 / b) Y Bm + fa0 Q Bm,
  // fa1 / fa0 = T*_d's y^d / y^(d-1) coefficients, b = filter_end
  const double bch = filter_end<P>(small, k, p, bbeta);
  const double cf1 = bch > 0.0 ? fa1 / bch : 1.0, cf0 = bch > 0.0 ? fa0 : 0.0;
  double res2[NT];
  dv4 aacc[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) { res2[ct] = 0.0; aacc[ct] = dv4{0.0, 0.0, 0.0, 0.0}; }
  const int ntile = (T + 15) >> 4;
  // each tile's operands load at the top of its iteration (occupancy hides the latency)
  Ap2Tile<P> cur;
  // the loaded tile's residuals: u = Q A, Y A, res2 += (Y A - u diag(theta))^2 over the rows < T
  auto tile_residuals = [&](int t0) {
    dv4 u[NT], ya[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) { u[ct] = dv4{0.0, 0.0, 0.0, 0.0}; ya[ct] = u[ct]; }
#pragma unroll
    for (int kk = 0; kk < KP; ++kk)
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const double am = sAm[(4 * kk + lk) * P + 16 * ct + li];
        u[ct] = mfma16(cur.qa[kk], am, u[ct]);
        ya[ct] = mfma16(cur.yo[kk], am, ya[ct]);
      }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const bool v = t0 + 4 * g + lk < T;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const double wr = ya[ct][g] - th[ct] * u[ct][g];
        if (v && 16 * ct + li < k) res2[ct] = fma(wr, wr, res2[ct]);
      }
    }
  };
  // the one-pass tile loop: the residuals, then V0 and Qn out and a = F'Qn
  // (the residuals' u and Y A are done with before V0 = Q Bm and Y Bm start:
  // with all four products in one loop the kernel needs 128 VGPRs and 64 B of
  // scratch, profiles/r11_fact_refactor.txt)
  auto tile_loop = [&]() {
    for (int tile = wave; tile < ntile; tile += BW) {
      ap2_load_lds<P>(cur, tile, T, r, lane, Qr, Yr, fb, stile[wave][0], stile[wave][1], ps);
      const int t0 = tile * 16;
      tile_residuals(t0);
      double qv[NT][4];
      dv4 qn[NT], qb[NT];
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) { qn[ct] = dv4{0.0, 0.0, 0.0, 0.0}; qb[ct] = qn[ct]; }
#pragma unroll
      for (int kk = 0; kk < KP; ++kk)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          const double bm = sBm[(4 * kk + lk) * P + 16 * ct + li];
          qn[ct] = mfma16(cur.yo[kk], bm, qn[ct]);
          qb[ct] = mfma16(cur.qa[kk], bm, qb[ct]);
        }
      {   // V0 = Q Bm for the filter's later steps (boot_cheb_kernel), kept in w.U
        double *Xr = w.U + (int64_t)rep * T * P;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int t = t0 + 4 * g + lk;
          if (t < T)
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
              const int c = 16 * ct + li;
              double x = qb[ct][g];
              if (c < p && dd[ct]) x = hash_unit(seed, t, 1000003ull * (it + 1) + c);   // = S
              if (c >= p) x = 0.0;
              if (c < ps) Xr[(int64_t)t * ps + c] = x;
            }
        }
      }
      // every wave reads only its own tiles' Y rows, loaded (above) before
      // these stores: Qn may overwrite this tile's Y rows
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int t = t0 + 4 * g + lk;
        const bool v = t < T;
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          const int c = 16 * ct + li;
          // the filter's first Horner term S_{d-1} = (a_d / b) K_1 + a_{d-1} V0
          // (K_1 = Y Bm = G* V0; b <= 0, a degenerate block: the plain power step Y Bm)
          double q = fma(cf1, qn[ct][g], cf0 * qb[ct][g]);
          if (c < p && dd[ct]) q = hash_unit(seed, t, 1000003ull * (it + 1) + c);
          if (c >= p || !v) q = 0.0;
          qv[ct][g] = q;
          if (v && c < ps) Yr[(int64_t)t * ps + c] = q;
        }
      }
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) aacc[ct] = mfma16(cur.fa[g], qv[ct][g], aacc[ct]);
    }
  };
  // probe: first only u, Y A and the residuals (no stores); the tile loop after the verdict, if the replicate goes on
  if (probe) {
    for (int tile = wave; tile < ntile; tile += BW) {
      ap2_load_lds<P>(cur, tile, T, r, lane, Qr, Yr, fb, stile[wave][0], stile[wave][1], ps, false);
      tile_residuals(tile * 16);
    }
  } else {
    tile_loop();
  }
  // residuals: sum over the 4 row-lanes of a column, then over waves (fixed order)
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    double v = res2[ct];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (lk == 0) sres[wave][16 * ct + li] = v;
  }
  __syncthreads();
  if (wave == 0) {
    if (lane < P) {
      double v = sres[0][lane];
#pragma unroll
      for (int wv = 1; wv < BW; ++wv) v += sres[wv][lane];
      sres[0][lane] = v;
    }
    __builtin_amdgcn_wave_barrier();
    const int itc = it + 1;
    const double *prev = small + 2 * P * P + 2 * P + ((itc - 1) & 1) * P;
    double *next = small + 2 * P * P + 2 * P + (itc & 1) * P;
    const int conv =
        decide_converged(sres[0], small + 2 * P * P, prev, next, k, p, tol, w.trace[rep], itc, w.subspace) ? 1 : 0;
#ifdef DFM_DIAG_X
    diag_excess(sres[0], small + 2 * P * P, k, p, tol, w.trace[rep], rep, it);
#endif
    if (lane == 0) {
      s_conv = conv;
      if (conv) { w.done[rep] = 1; w.iters[rep] = it + 1; }
      else atomicAdd(&w.active[it], 1);
    }
  }
  __syncthreads();
  if (s_conv || last) {
    if (w.no_vectors) return;   // eigenvalue-only statistics: eig_final reads theta only
    // Ritz vectors U = Q A for the final output (eig_final_kernel)
    double *Ur = w.U + (int64_t)rep * T * P;
    for (int tile = wave; tile < ntile; tile += BW) {
      const int t0 = tile * 16, ta = t0 + li;
      dv4 u[NT];
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) u[ct] = dv4{0.0, 0.0, 0.0, 0.0};
      double qa[KP];
#pragma unroll
      for (int kk = 0; kk < KP; ++kk) qa[kk] = (ta < T && 4 * kk + lk < ps) ? Qr[(int64_t)ta * ps + 4 * kk + lk] : 0.0;
#pragma unroll
      for (int kk = 0; kk < KP; ++kk)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) u[ct] = mfma16(qa[kk], sAm[(4 * kk + lk) * P + 16 * ct + li], u[ct]);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int t = t0 + 4 * g + lk;
        if (t < T)
#pragma unroll
          for (int ct = 0; ct < NT; ++ct) Ur[(int64_t)t * P + 16 * ct + li] = u[ct][g];
      }
    }
    return;
  }
  if (probe) {
    tile_loop();   // (its residuals are not read again)
    __syncthreads();   // every wave's Qn rows visible to the CSR gather (one pass: the verdict's barriers)
  }
  // Z = P' D Qn by CSR gather (bucket s lists t ascending), cc = EL' Z
  zscatter_tail<P, false>(fb, T, r, ntile, tid, wave, lane, set, so, sl, Yr, Zc, pz, rep, ab, sred, ps, AccTail{aacc});
}

// One Horner step of the degree-d Chebyshev filter of the factored solver.
// With V0 = Q Bm and y = G*/b (b = filter_end), the filter is the shifted
// Chebyshev polynomial T*_d(y) = T_d(2y - 1) = sum_i a_i y^i, evaluated as
// S_d = a_d V0, S_i = G* S_{i+1} / b + a_i V0, T*_d(y) V0 = S_0: ap2 leaves
// S_{d-1} = (a_d / b) K_1 + a_{d-1} V0 (K_1 = Y Bm = G* V0, no product) with
// its Z, a, cc, and V0 in w.U; each step gets W = G* S_{i+1} from the GEMM
// H . Z(S_{i+1}) (formed exactly as y2 forms Y) and writes S_i = W / b + a_i V0
// with the Z, a, cc of S_i for the next GEMM (or, S_0, the next Rayleigh-Ritz
// step).  The same step serves the middle and the end of the filter, with
// one running vector (the monomial form also rewrote a running sum per
// step).  Degree 2: T2(2G/b - 1)(Q Bm) = (8/b^2) G*^2 V0 - (8/b) G* V0 + V0.
// The filter damps the unwanted spectrum ~T_d(2 lambda_k/b - 1) times
// relative to the wanted one; the basis is orthonormalised by the next
// Rayleigh-Ritz step (CholQR folded into eig_small).
template <int P, bool STG>
__global__ __launch_bounds__(64 * BW, 4) void boot_cheb_kernel(FactBase fb, EigWork w, int T, int p,
                                                        const int32_t *__restrict__ idx,
                                                        const double *__restrict__ eta,
                                                        const int *__restrict__ off, const int *__restrict__ lst,
                                                        const double *__restrict__ HZ, int64_t ldz, int pz,
                                                        double *__restrict__ ab, double fai, double bbeta, int k,
                                                        double *__restrict__ Qo,
                                                        double *__restrict__ Zc, int ps,
                                                        const double *__restrict__ V0, int64_t v0s, double bfix) {
  // V0, v0s: the filtered block and its replicate stride (w.U, T P after a
  // Rayleigh-Ritz step; the shared warm start Q0, 0, for a filter-only first
  // step).  bfix > 0: the interval end, the same for every replicate, instead
  // of filter_end — no Rayleigh-Ritz step has run, so the small record is
  // not read and no column is deflated.
  constexpr int NT = P / 16;
  const int rep = blockIdx.x;
  if (w.done[rep]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = fb.r;
  const int li = lane & 15, lk = lane >> 4;
  __shared__ double sa[16 * P], sb[16 * P];
  __shared__ double sred[NT * 256];
  __shared__ double stg[STG ? BW : 1][STG ? Y2_STG : 1];   // per-wave operand staging (y2_load)
  extern __shared__ double sdyn[];             // eta, idx and the CSR of idx
  const RepLds rl = load_rep_lds<true, true>(sdyn, T, tid, rep, idx, eta, off, lst);
  const double *set = rl.set;
  const int *six = rl.six, *so = rl.so, *sl = rl.sl;
  load_ab<P>(fb, ab + (int64_t)rep * 32 * P, sa, sb, tid, r);
  const double *small = w.small + (int64_t)rep * small_stride<P>();
  const double b = bfix > 0.0 ? bfix : filter_end<P>(small, k, p, bbeta);
  // b <= 0 (a degenerate block): plain power steps
  const double cb = b > 0.0 ? 1.0 / b : 1.0, cv0 = b > 0.0 ? fai : 0.0;
  bool dd[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) dd[ct] = bfix > 0.0 ? false : small[2 * P * P + P + 16 * ct + li] != 0.0;
  const int KR = (r + 3) >> 2;
  double bA[4][NT], bB[4][NT];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) {
      bA[kk][ct] = sa[(4 * kk + lk) * P + 16 * ct + li];
      bB[kk][ct] = sb[(4 * kk + lk) * P + 16 * ct + li];
    }
  const double *Xr = V0 + (int64_t)rep * v0s;   // V0 = Q Bm (ap2), or the warm start
  double *Qr = Qo + (int64_t)rep * T * P;
  dv4 aacc[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) aacc[ct] = dv4{0.0, 0.0, 0.0, 0.0};
  const int ntile = (T + 15) >> 4;
  Y2Tile<P> cur;
  for (int tile = wave; tile < ntile; tile += BW) {
    y2_load<P, STG>(cur, tile, T, r, KR, lane, six, fb, HZ, ldz, pz, rep, Xr, ps, stg[STG ? wave : 0]);   // cur.q = V0 rows
    const int t0 = tile * 16;
    dv4 yF[NT], yE[NT];
    tile_yfe<P, false>(cur, KR, li, lk, sa, sb, bA, bB, yF, yE);
    double qv[NT][4], fa[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int t = t0 + 4 * g + lk;
      const bool v = t < T;
      const int tc = min(t, T - 1);
      if constexpr (STG)
        fa[g] = (v && li < r) ? stg[wave][(4 * g + lk) * (r + 1) + li] : 0.0;
      else
        fa[g] = (v && li < r) ? fb.F[(int64_t)tc * r + min(li, max(r - 1, 0))] : 0.0;   // never F[-1] (r = 0)
      const double e = v ? set[t] : 0.0;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const int c = 16 * ct + li;
        const double wv = fma(e, yE[ct][g] + cur.hz[ct][g], yF[ct][g]);
        double q = dd[ct] ? cur.q[ct][g] : fma(cb, wv, cv0 * cur.q[ct][g]);
        if (c >= p || !v) q = 0.0;
        qv[ct][g] = q;
        if (v && c < ps) Qr[(int64_t)t * ps + c] = q;
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) aacc[ct] = mfma16(fa[g], qv[ct][g], aacc[ct]);
  }
  __syncthreads();   // every wave's Qn rows visible to the CSR gather
  zscatter_tail<P, false>(fb, T, r, ntile, tid, wave, lane, set, so, sl, Qr, Zc, pz, rep, ab, sred, ps, AccTail{aacc});
}

// The middle Horner steps in row-local form.  With W = G* S_{i+1} = F bB +
// D P u (bB = S a + cc, u = EL a + HZ, a / cc of S_{i+1}) and S_i = W / b +
// a_i V0, the next GEMM operand and the step's reductions need no S_i rows:
//   Z_i = P'D S_i = (PF bB + e2 . u) / b + a_i PV,
//   a_i = F'S_i   = (F'F bB + PF'u) / b + a_i FV,     cc_i = EL'Z_i,
// with PF = P'D F, e2 = P'D^2 1 (boot_prep_kernel, once per solve), PV = P'D V0
// and FV = F'V0 (ap2, once per filter).  Every row s reads HZ[s], PV[s],
// PF[s], e2[s], EL[s] and writes Z[s]: no CSR gather, no S_i write and
// re-read, no barrier between the two (the last step, which must hand S_0 to
// the next Rayleigh-Ritz step, stays boot_cheb_kernel).  Columns that
// deflated (dd) carry V0: Z = PV, a = FV; columns >= p are zero.
// F'F (16 x 16, rows / columns >= r zero), one workgroup: four row quarters
// per entry (t ascending in each), summed in a fixed order
__global__ __launch_bounds__(1024) void ftf_kernel(FactBase fb, double *__restrict__ FtF) {
  __shared__ double part[4][256];
  const int e = threadIdx.x & 255, q = threadIdx.x >> 8, j = e >> 4, i = e & 15, r = fb.r;
  const int t0 = q * ((fb.T + 3) / 4), t1 = min(fb.T, t0 + (fb.T + 3) / 4);
  double acc = 0.0;
  if (j < r && i < r) {
    // 8 rows' loads in flight before their (in-order) products: the one-row
    // loop was ~125 dependent L2 round trips (30-40 us on every lane's stream)
    int t = t0;
    for (; t + 8 <= t1; t += 8) {
      double a[8], b[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { a[u] = fb.F[(int64_t)(t + u) * r + j]; b[u] = fb.F[(int64_t)(t + u) * r + i]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) acc = fma(a[u], b[u], acc);
    }
    for (; t < t1; ++t) acc = fma(fb.F[(int64_t)t * r + j], fb.F[(int64_t)t * r + i], acc);
  }
  part[q][e] = acc;
  __syncthreads();
  if (q == 0) FtF[e] = (part[0][e] + part[1][e]) + (part[2][e] + part[3][e]);
}
hipError_t launch_fact_ftf(const FactBase &fb, double *FtF, hipStream_t st) {
  hipLaunchKernelGGL(ftf_kernel, dim3(1), dim3(1024), 0, st, fb, FtF);
  return hipGetLastError();
}

// fixed-order sum over the waves of a 16 x P accumulator block -> dst (row-major, stride P)
// (used by the middle Horner steps alone.  prep_a, zscatter_tail and y2 keep the same sum written out: those
// kernels and the middle steps sit at 125-128 VGPRs, and with the helper shared the order in which the compiler
// inlines it moves spills between boot_cheb_mid_kernel's instances, profiles/r11_fact_refactor.txt section 1)
template <int P>
DFM_DEV void wave_block_store(const dv4 *acc, double *sred, int wave, int lane, int tid, double *__restrict__ dst) {
  constexpr int NT = P / 16;
  for (int wv = 0; wv < BW; ++wv) {
    if (wave == wv)
#pragma unroll
      for (int ct = 0; ct < NT; ++ct)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int e = (ct * 4 + g) * 64 + lane;
          sred[e] = (wv ? sred[e] : 0.0) + acc[ct][g];
        }
    __syncthreads();
  }
  if (dst)
    for (int e = tid; e < NT * 256; e += 64 * BW) {
      const int l = e & 63, g = (e >> 6) & 3, ct = e >> 8;
      dst[(4 * g + (l >> 4)) * P + 16 * ct + (l & 15)] = sred[e];
    }
}

// PV = P'D V0 and FV = F'V0 for a filter with middle steps, launched between
// the Rayleigh-Ritz step's eig_small and ap2: V0 = Q Bm is linear in Q, so
// PV = Z(Q) Bm and FV = a(Q) Bm from the Z = P'D Q and a = F'Q that the
// previous step left in Zc / ab (ap2 overwrites both) — row-local, no CSR
// gather of V0.  Columns that ap2 refills (dead pivots: V0 = hash_unit) take
// the explicit sums over their buckets / rows.
template <int P>
__global__ __launch_bounds__(64 * BW, 4) void boot_pv_kernel(FactBase fb, EigWork w, int T, int p, int it,
                                                      const double *__restrict__ eta, const int *__restrict__ off,
                                                      const int *__restrict__ lst, const double *__restrict__ Zc,
                                                      int64_t ldz, int pz, const double *__restrict__ ab, uint64_t seed,
                                                      double *__restrict__ PV, double *__restrict__ FV, int ps) {
  constexpr int NT = P / 16, KP = P / 4;
  const int rep = blockIdx.x;
  if (w.done[rep]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = fb.r;
  const int li = lane & 15, lk = lane >> 4;
  const double *small = w.small + (int64_t)rep * small_stride<P>();
  const uint64_t hc = 1000003ull * (it + 1);
  double bBm[KP][NT];
  bool dd[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) {
    const int c = 16 * ct + li;
    dd[ct] = small[2 * P * P + P + c] != 0.0;
#pragma unroll
    for (int kk = 0; kk < KP; ++kk) bBm[kk][ct] = small[P * P + (4 * kk + lk) * P + c];
  }
  const double *et = eta ? eta + (int64_t)rep * T : nullptr;
  const int *o = off + (int64_t)rep * (T + 1);
  const int *L = lst + (int64_t)rep * T;
  double *pvr = PV + (int64_t)rep * T * P;
  const int ntile = (T + 15) >> 4;
  for (int tile = wave; tile < ntile; tile += BW) {
    const int t0 = tile * 16, ta = min(t0 + li, T - 1);
    double za[KP];
#pragma unroll
    for (int kk = 0; kk < KP; ++kk)
      za[kk] = (t0 + li < T && 4 * kk + lk < pz) ? Zc[zrm_ix(rep, ta, 4 * kk + lk, pz, zrm_stride(T, pz))] : 0.0;
    dv4 v[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) v[ct] = dv4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < KP; ++kk)
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) v[ct] = mfma16(za[kk], bBm[kk][ct], v[ct]);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int s = t0 + 4 * g + lk;
      if (s < T)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          const int c = 16 * ct + li;
          double x = v[ct][g];
          if (c < p && dd[ct]) {   // refilled column: sum over bucket s (t ascending)
            x = 0.0;
            for (int q = o[s]; q < o[s + 1]; ++q) {
              const int t = L[q];
              x = fma(et ? et[t] : 1.0, hash_unit(seed, t, hc + c), x);
            }
          }
          if (c >= p) x = 0.0;
          if (c < ps) pvr[(int64_t)s * ps + c] = x;
        }
    }
  }
  const double *aq = ab + (int64_t)rep * 32 * P;
  double *fvr = FV + (int64_t)rep * 16 * P;
  for (int e = tid; e < 16 * P; e += 64 * BW) {
    const int j = e / P, c = e % P;
    double x = 0.0;
    if (j < r && c < p) {
      if (small[2 * P * P + P + c] != 0.0) {
        for (int t = 0; t < T; ++t) x = fma(fb.F[(int64_t)t * r + j], hash_unit(seed, t, hc + c), x);
      } else {
        for (int i = 0; i < P; ++i) x = fma(aq[j * P + i], small[P * P + i * P + c], x);
      }
    }
    fvr[e] = x;
  }
}

// HF, ZF (dfm_fact_plan.h; the reduced-precision products of a warm eigenvalue-rule solve): how HZ arrives and how Z
// leaves.  Rows64: fp64 rows as described.  Chunk32: float HZ32 in Z's replicate-major chunk layout (this replicate's
// 16-row tile one contiguous 64 pz-byte piece, fetched as 16-B pieces and transposed through the EL stage), scaled by
// hscale = hmax on the way in.  Z leaves as zchunk_store writes it: fp64 in the normal layout (behind Chunk32: the
// last middle step in front of an fp64 product), float Z32, rounded to nearest, or the three bf16 planes (the same
// doubles of the stage, split on the way out).  All arithmetic, a and cc stay fp64 in every mode; cc is formed from
// the unrounded Z.
//
// NOPF (a warm solve that starts with the filter, eig_run_fact2_t; selected by DFM_FACT_PF=0 only, FilterPlan::nopf):
// no stored PF.  There V0 = Q0, whose first r columns are the warm vectors bit for bit (eig_init_kernel;
// q0_guards_kernel leaves them), and F = pfs * warm[:, :r] with one rounding per element (FactArgs::fscale), so
//   PF = P'D F = pfs * (P'D Q0)[:, :r] = pfs * PV[:, :r]
// up to the rounding of the bucket sums.  The tile's 16 PV rows — one contiguous range of 16 ps doubles — arrive as
// 16-B pieces in the stage the PF rows take otherwise, and pA, pfa (columns < r, times pfs) and pv are read from
// there: no PF loads, no PV row gathers.  PF and pfr are not read.
//
// ZPL: the planes of the Split Z this step writes (FilterPlan::mid_planes), or 0 for the run-time argument zplanes.
// The P = 16 instances take the argument (wave-uniform; their registers do not move).  At P = 32 the live argument
// costs <32, false, Chunk32, Split, false> 8 B more scratch, so there the count is an instance (ZPL = 3: the
// parent's code; ZPL = 2 beside it) and the argument is dead.
template <int P, bool FAST, HzFmt HF, ZFmt ZF, bool NOPF = false, int ZPL = 0>
__global__ __launch_bounds__(64 * BW, 4) void boot_cheb_mid_kernel(FactBase fb, EigWork w, int T, int p,
                                                            const double *__restrict__ HZ, int64_t ldz, int pz,
                                                            double *__restrict__ ab, double fai, double bbeta, int k,
                                                            const double *__restrict__ PF,
                                                            const double *__restrict__ E2,
                                                            const double *__restrict__ PV,
                                                            const double *__restrict__ FV,
                                                            const double *__restrict__ FtF,
                                                            double *__restrict__ Zc, int ps, double bfix,
                                                            double lead, double hscale, double pfs, int zplanes) {
  // zplanes: see ZPL (read by ZF = Split alone)
  static_assert(ZPL == 0 || (ZF == ZFmt::Split && (ZPL == 2 || ZPL == 3)), "a plane count belongs to a Split Z");
  // bfix > 0: the interval end of a filter-only first step (boot_cheb_kernel); lead: the scale of the incoming
  // S_{i+1} not yet applied to its Z, a, cc — the filter's leading coefficient a_d at the first step of such a filter
  // (S_d = a_d V0 is never formed: prep left the Z, a, cc of V0), else 1
  static_assert(HF == HzFmt::Chunk32 || ZF == ZFmt::F64, "a step fed fp64 rows writes an fp64 Z");
  constexpr int NT = P / 16;
  const int rep = blockIdx.x;
  if (w.done[rep]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = fb.r;
  const int li = lane & 15, lk = lane >> 4;
  __shared__ double sa[16 * P], sb[16 * P];
  __shared__ double sred[NT * 256];
  // per-wave staging (this pass is bound by the texture-address unit, TA_TA_BUSY 0.95 of its cycles): the tile's PF
  // and EL rows arrive as ONE contiguous 16-row range each (16 r doubles) instead of two differently shaped gathers
  // of the same rows, and the tile's Z chunk (16 rows x pz, contiguous in the replicate-major layout) leaves as whole
  // 16-B pieces instead of one 128-B-strided element per lane stage 0 holds the PF rows (16 x (r | 1) <= 16 x 17) and
  // then the Z chunk (16 x pz <= 16 x P) (NOPF: the PV rows instead, 16 x (ps | 1) <= 16 x (P + 1))
  constexpr int MID_STG = NOPF ? 16 * (P + 1) : 16 * (P > 17 ? P : 17);
  static_assert(MID_STG >= 16 * P && MID_STG >= 16 * 17, "the stage holds a Z chunk of pz <= P columns and 16 PF rows");
  static_assert(!NOPF || MID_STG >= 16 * (P | 1), "... or 16 PV rows of ps <= P columns at an odd stride");
  __shared__ double stgP[BW][MID_STG], stgE[BW][16 * 17];
  double *abr = ab + (int64_t)rep * 32 * P;
  // (load_ab, written out: through the helper <32, false, 0, true> spills 8 B more, profiles/r11_fact_refactor.txt)
  // sa = a, sb = S a + cc
  for (int e = tid; e < 16 * P; e += 64 * BW) sa[e] = abr[e];
  __syncthreads();
  for (int e = tid; e < 16 * P; e += 64 * BW) {
    const int j = e / P, c = e % P;
    double v = abr[16 * P + e];
    if (j < r)
      for (int i = 0; i < r; ++i) v = fma(fb.S[j * r + i], sa[i * P + c], v);
    sb[e] = v;
  }
  __syncthreads();
  const double *small = w.small + (int64_t)rep * small_stride<P>();
  const double b = bfix > 0.0 ? bfix : filter_end<P>(small, k, p, bbeta);
  const double cb = b > 0.0 ? lead / b : 1.0, cv0 = b > 0.0 ? fai : 0.0;
  bool dd[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) dd[ct] = bfix > 0.0 ? false : small[2 * P * P + P + 16 * ct + li] != 0.0;
  const int KR = (r + 3) >> 2;
  const double *pfr = PF + (int64_t)rep * T * r, *e2r = E2 + (int64_t)rep * T, *pvr = PV + (int64_t)rep * T * P;
  dv4 aacc[NT], cacc[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct) { aacc[ct] = dv4{0.0, 0.0, 0.0, 0.0}; cacc[ct] = aacc[ct]; }
  const int ntile = (T + 15) >> 4;
  const int RS = r | 1;   // staged row stride (odd: the 16-row reads spread over the banks)
  const int hps = ps >> 1, RP = NOPF ? (ps | 1) : RS;   // NOPF: 16-B pieces per PV row; stage 0's row stride
  double *sP = stgP[wave], *sE = stgE[wave];
  const int64_t zrs = zrm_stride(T, pz);
  for (int tile = wave; tile < ntile; tile += BW) {
    // Split: the lane number is re-read per tile, so the tile's lane-dependent addresses are formed here from one
    // register and not carried through the loop as invariants (the split store below needs their registers: 128 VGPRs)
    int lane_t = lane;
    if constexpr (ZF == ZFmt::Split) asm volatile("" : "+v"(lane_t));
    const int lane = lane_t, li = lane & 15, lk = lane >> 4;
    const int t0 = tile * 16;
    const int nr = min(16, T - t0) * r;   // valid doubles of the tile's contiguous PF / EL range
    double hz[NT][4], pv[NT][4], e2v[4];
    double pst[4], est[4];
    double2 pst2 = double2{0.0, 0.0}, est2 = double2{0.0, 0.0};
    double2 pvp[2 * NT];   // NOPF: the tile's PV rows (16 ps doubles from t0 ps, 16-B aligned: ps even)
    if constexpr (NOPF) {
      const double2 *pc = reinterpret_cast<const double2 *>(pvr + (int64_t)t0 * ps);
      const int npc = min(16, T - t0) * hps;   // pieces of the rows < T; the pad rows stage as zero
#pragma unroll
      for (int u = 0; u < 2 * NT; ++u) pvp[u] = u * 64 + lane < npc ? pc[u * 64 + lane] : double2{0.0, 0.0};
    }
    if constexpr (FAST) {   // even r <= 8: the 8 r <= 64 pieces of 16 B, one round
      const bool ok = 2 * lane < nr;
      if constexpr (!NOPF)
        pst2 = ok ? reinterpret_cast<const double2 *>(pfr + (int64_t)t0 * r)[lane] : double2{0.0, 0.0};
      est2 = ok ? reinterpret_cast<const double2 *>(fb.EL + (int64_t)t0 * r)[lane] : double2{0.0, 0.0};
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {   // 16 r <= 256 doubles: four rounds of 64 lanes
        const int e = u * 64 + lane;
        pst[u] = (!NOPF && e < nr) ? pfr[(int64_t)t0 * r + e] : 0.0;
        est[u] = e < nr ? fb.EL[(int64_t)t0 * r + e] : 0.0;
      }
    }
    const double e2l = t0 + li < T ? e2r[t0 + li] : 0.0;
    zf4 h4[NT];   // Chunk32: the tile's HZ32 chunk, piece e = 64 u + lane: column e >> 2, rows 4 (e & 3) .. + 3
    if constexpr (HF == HzFmt::Chunk32) {
      const zf4 *hc = reinterpret_cast<const zf4 *>(reinterpret_cast<const float *>(HZ) + (int64_t)rep * zrs +
                                                     (int64_t)tile * 16 * pz);
#pragma unroll
      for (int u = 0; u < NT; ++u) h4[u] = u * 64 + lane < 4 * pz ? hc[u * 64 + lane] : zf4{0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int s = t0 + 4 * g + lk;
      const int sc = min(s, T - 1);
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const int c = 16 * ct + li;
        if constexpr (HF == HzFmt::Rows64) hz[ct][g] = c < pz ? HZ[(int64_t)sc * ldz + (int64_t)rep * pz + c] : 0.0;
        if constexpr (!NOPF) pv[ct][g] = c < ps ? pvr[(int64_t)sc * ps + c] : 0.0;
      }
    }
    if constexpr (FAST) {
      if (2 * lane < 16 * r) {
        const int e = 2 * lane, row = e / r, j = e - row * r;
        if constexpr (!NOPF) { sP[row * RS + j] = pst2.x; sP[row * RS + j + 1] = pst2.y; }
        sE[row * RS + j] = est2.x; sE[row * RS + j + 1] = est2.y;
      }
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = u * 64 + lane;
        if (e < 16 * r) {
          const int row = e / r, j = e - row * r;
          if constexpr (!NOPF) sP[row * RS + j] = pst[u];
          sE[row * RS + j] = est[u];
        }
      }
    }
    if constexpr (NOPF) {
#pragma unroll
      for (int u = 0; u < 2 * NT; ++u) {
        const int e = u * 64 + lane;
        if (e < 16 * hps) {
          const int row = e / hps, j = 2 * (e - row * hps);
          sP[row * RP + j] = pvp[u].x; sP[row * RP + j + 1] = pvp[u].y;
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's writes land before its reads
    double pA[4], eA[4], pfa[4], ea[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int j = 4 * kk + lk;
      const bool ok = kk < KR && j < r && t0 + li < T;
      pA[kk] = ok ? (NOPF ? pfs * sP[li * RP + j] : sP[li * RP + j]) : 0.0;
      eA[kk] = ok ? sE[li * RS + j] : 0.0;
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int s = t0 + 4 * g + lk;
      const bool v = s < T;
      e2v[g] = v ? __shfl(e2l, 4 * g + lk, 16) : 0.0;
      pfa[g] = (v && li < r) ? (NOPF ? pfs * sP[(4 * g + lk) * RP + li] : sP[(4 * g + lk) * RP + li]) : 0.0;
      ea[g] = (v && li < r) ? sE[(4 * g + lk) * RS + li] : 0.0;
      if constexpr (NOPF)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) pv[ct][g] = 16 * ct + li < ps ? sP[(4 * g + lk) * RP + 16 * ct + li] : 0.0;
    }
    if constexpr (HF == HzFmt::Chunk32) {
      // HZ32 through the EL stage (its reads above are complete in this wave's LDS order): column c at float offset
      // 17 c (17 pz <= 17 P floats fit the stage's 16 x 17 doubles), read back in the accumulator layout
      static_assert(17 * P <= 2 * 16 * 17, "the EL stage holds the HZ32 chunk");
      float *sH = reinterpret_cast<float *>(sE);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int u = 0; u < NT; ++u) {
        const int e = u * 64 + lane;
        if (e < 4 * pz) {
          float *d = sH + 17 * (e >> 2) + 4 * (e & 3);
          d[0] = h4[u][0]; d[1] = h4[u][1]; d[2] = h4[u][2]; d[3] = h4[u][3];
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          const int c = 16 * ct + li;
          hz[ct][g] = c < pz ? hscale * (double)sH[17 * c + 4 * g + lk] : 0.0;
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // before the next tile's EL rows overwrite the stage
    }
    dv4 yP[NT], yE[NT];
#pragma unroll
    for (int ct = 0; ct < NT; ++ct) { yP[ct] = dv4{0.0, 0.0, 0.0, 0.0}; yE[ct] = yP[ct]; }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (kk < KR) {   // B operands a / bB from LDS (registers are this kernel's limit)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
          yP[ct] = mfma16(pA[kk], sb[(4 * kk + lk) * P + 16 * ct + li], yP[ct]);
          yE[ct] = mfma16(eA[kk], sa[(4 * kk + lk) * P + 16 * ct + li], yE[ct]);
        }
      }
    }
    double uv[NT][4], zv[NT][4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int s = t0 + 4 * g + lk;
      const bool v = s < T;
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const int c = 16 * ct + li;
        const double u = yE[ct][g] + hz[ct][g];
        double z = dd[ct] ? pv[ct][g] : fma(cb, fma(e2v[g], u, yP[ct][g]), cv0 * pv[ct][g]);
        if (c >= p || !v) z = 0.0;
        uv[ct][g] = v ? u : 0.0;
        zv[ct][g] = z;
      }
    }
    // the Z chunk through the PF staging (its reads above are complete in this wave's LDS order): chunk element 16 c
    // + (s & 15); rows past T hold z = 0, the value boot_prep_kernel left in the chunk's pad rows
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const int c = 16 * ct + li;
        if (c < pz) sP[16 * c + 4 * g + lk] = zv[ct][g];
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // (ZFmt::Split leaves below, behind the tile's last MFMAs: their operands' registers are free there)
    // (zchunk_store's other two formats, written out: through the helper these instances spill differently)
    if constexpr (ZF == ZFmt::F32) {
      zf4 *zc4 = reinterpret_cast<zf4 *>(reinterpret_cast<float *>(Zc) + (int64_t)rep * zrs + (int64_t)tile * 16 * pz);
      for (int e = lane; e < 4 * pz; e += 64)
        zc4[e] = zf4{(float)sP[4 * e], (float)sP[4 * e + 1], (float)sP[4 * e + 2], (float)sP[4 * e + 3]};
    } else if constexpr (ZF == ZFmt::F64) {
      double2 *zc2 = reinterpret_cast<double2 *>(Zc + (int64_t)rep * zrs + (int64_t)tile * 16 * pz);
      for (int e = lane; e < 8 * pz; e += 64) zc2[e] = double2{sP[2 * e], sP[2 * e + 1]};
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        aacc[ct] = mfma16(pfa[g], uv[ct][g], aacc[ct]);
        cacc[ct] = mfma16(ea[g], zv[ct][g], cacc[ct]);
      }
    if constexpr (ZF == ZFmt::Split) {   // (the stage is this wave's until the next tile's PF rows, behind these reads in its LDS order)
      asm volatile("" ::: "memory");
      zchunk_store<P>(ZF, sP, Zc, rep, zrs, tile, pz, lane, ZPL ? ZPL : zplanes);
    }
  }
  // a_i = (F'F bB + PF'u) / b + a_i FV  (dd columns: FV; columns >= p: 0)
  wave_block_store<P>(aacc, sred, wave, lane, tid, nullptr);
  const double *fvr = FV + (int64_t)rep * 16 * P;
  for (int e = tid; e < 16 * P; e += 64 * BW) {
    const int j = e / P, c = e % P;
    const int ct = c >> 4, l = ((j & 3) << 4) | (c & 15), g = j >> 2;
    double a = 0.0;
    if (j < r && c < p) {
      if (!(bfix > 0.0) && small[2 * P * P + P + c] != 0.0) a = fvr[e];
      else {
        double f = 0.0;
        for (int i = 0; i < r; ++i) f = fma(FtF[j * 16 + i], sb[i * P + c], f);
        a = fma(cb, f + sred[(ct * 4 + g) * 64 + l], cv0 * fvr[e]);
      }
    }
    abr[e] = a;
  }
  __syncthreads();
  wave_block_store<P>(cacc, sred, wave, lane, tid, abr + 16 * P);
}

__global__ __launch_bounds__(256) void zero_spans_kernel(ZeroSpans z) {
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
#pragma unroll
  for (int s = 0; s < 4; ++s)
    for (int64_t i = i0; i < z.n[s]; i += stride) z.p[s][i] = 0;
}
hipError_t launch_zero_spans(const ZeroSpans &z, hipStream_t st) {
  int64_t mx = 0;
  for (int s = 0; s < 4; ++s) mx = std::max<int64_t>(mx, z.p[s] ? z.n[s] : 0);
  if (mx == 0) return hipSuccess;
  ZeroSpans c = z;
  for (int s = 0; s < 4; ++s)
    if (!c.p[s]) c.n[s] = 0;
  hipLaunchKernelGGL(zero_spans_kernel, dim3((unsigned)std::min<int64_t>(512, (mx + 255) / 256)), dim3(256), 0, st, c);
  return hipGetLastError();
}

// Ascending list of the still-active replicates (done == 0) and their count,
// one 1024-thread workgroup: per-thread chunk counts, an LDS scan, in-order
// writes.  Feeds the compacted H.Z GEMM of the straggler phase.
__global__ __launch_bounds__(1024) void active_list_kernel(const int *__restrict__ done, int nb,
                                                           int *__restrict__ list, int *__restrict__ count) {
  __shared__ int part[1024];
  const int tid = threadIdx.x, per = (nb + 1023) / 1024;
  const int b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
  int c = 0;
  for (int i = b0; i < b1; ++i) c += done[i] ? 0 : 1;
  part[tid] = c;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int v = tid >= off ? part[tid - off] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int pos = part[tid] - c;
  for (int i = b0; i < b1; ++i)
    if (!done[i]) list[pos++] = i;
  if (tid == 1023) *count = part[1023];
}

// Guard columns kw..p-1 of the shared warm start Q0 (m rows of ps columns),
// orthonormalised against the warm columns 0..kw-1 (one projection; the warm
// columns, left bit-for-bit as they are, are orthogonal eigenvectors) and
// against each other (Cholesky of their Gram matrix, a forward substitution
// per row).  One workgroup; every sum runs over fixed row groups in a fixed
// order, so Q0 is the same in every batch, lane and shard.
// The kernel also opens the filter-only step's record: active[0] = nb, what
// a first Rayleigh-Ritz step that retires no replicate would have counted
// (every replicate runs step 0; count_iters_body prices its products from it).
constexpr int Q0G_SUMS = Q0G_PMAX * Q0G_PMAX;       // sums per phase: (ng + 1) kw <= 272 (ng + kw <= 32), ng^2 <= 1024
__global__ __launch_bounds__(1024) void q0_guards_kernel(double *__restrict__ Q0, int m, int ps, int kw, int p,
                                                         int *__restrict__ active, int nb) {
  static_assert(Q0G_SUMS <= 1024, "one thread per sum, one partial per thread");
  __shared__ double part[1024];
  __shared__ double dots[Q0G_SUMS];   // the cross / norm sums, then the guards' ng x ng Gram matrix
  __shared__ double Lc[Q0G_PMAX * Q0G_PMAX];
  const int tid = threadIdx.x, ng = p - kw;
  if (tid == 0) active[0] = nb;
  if (ng <= 0 || kw < 0 || p > Q0G_PMAX) return;
  for (int phase = 0; phase < 2; ++phase) {
    // phase 0: pair e = j kw + i -> <g_j, w_i> (j < ng), j = ng -> <w_i, w_i>;  phase 1: e = j ng + i -> <g_j, g_i>
    const int np = phase == 0 ? (ng + 1) * kw : ng * ng;
    int npp = 1;
    while (npp < np) npp <<= 1;
    const int rg = 1024 / npp;   // row groups (np <= Q0G_SUMS: npp <= 1024, rg >= 1)
    const int e = tid % npp, g = tid / npp;
    double acc = 0.0;
    if (e < np && g < rg) {
      int ca, cb;
      if (phase == 0) { const int j = e / kw, i = e % kw; ca = j < ng ? kw + j : i; cb = i; }
      else { ca = kw + e / ng; cb = kw + e % ng; }
      for (int t = g; t < m; t += rg) acc = fma(Q0[(int64_t)t * ps + ca], Q0[(int64_t)t * ps + cb], acc);
    }
    part[tid] = acc;
    __syncthreads();
    if (tid < np) {
      double s = 0.0;
      for (int q = 0; q < rg; ++q) s += part[q * npp + tid];
      dots[tid] = s;
    }
    __syncthreads();
    if (phase == 0) {
      if (kw > 0)
        for (int x = tid; x < m * ng; x += 1024) {
          const int t = x / ng, j = x % ng;
          double v = Q0[(int64_t)t * ps + kw + j];
          for (int i = 0; i < kw; ++i) {
            const double n = dots[ng * kw + i];
            if (n > 0.0) v = fma(-(dots[j * kw + i] / n), Q0[(int64_t)t * ps + i], v);
          }
          Q0[(int64_t)t * ps + kw + j] = v;
        }
    } else {
      if (tid == 0) {   // Gram = L L' (a column whose pivot is not positive stays as it is)
        for (int j = 0; j < ng; ++j) {
          for (int i = 0; i <= j; ++i) {
            double s = dots[j * ng + i];
            for (int q = 0; q < i; ++q) s -= Lc[j * 32 + q] * Lc[i * 32 + q];
            if (i < j) Lc[j * 32 + i] = Lc[i * 32 + i] > 0.0 ? s / Lc[i * 32 + i] : 0.0;
            else Lc[j * 32 + j] = s > 0.0 ? sqrt(s) : -1.0;
          }
          if (!(Lc[j * 32 + j] > 0.0))
            for (int i = 0; i < j; ++i) Lc[j * 32 + i] = 0.0;
        }
      }
      __syncthreads();
      for (int t = tid; t < m; t += 1024) {   // row t: g L^-T by forward substitution
        double nv[32];
        for (int j = 0; j < ng; ++j) {
          double v = Q0[(int64_t)t * ps + kw + j];
          const double d = Lc[j * 32 + j];
          if (d > 0.0) {
            for (int i = 0; i < j; ++i) v -= Lc[j * 32 + i] * nv[i];
            v /= d;
          }
          nv[j] = v;
          Q0[(int64_t)t * ps + kw + j] = v;
        }
      }
    }
    __syncthreads();
  }
}

// Zero the pad rows T .. round_up(T, 16) - 1 of every replicate's fp64 Z (its last 16-row chunk): gemmh_zrm_kernel
// reads them against H's zero k-padding, so they must be finite.  A step 0 whose last product runs split
// (FilterPlan::zero_zpad) needs it: prep and every middle step wrote bf16 planes there, no pass wrote the fp64 chunks,
// and the last Horner step (zscatter_tail) stores rows < T only.  nb pz doubles per pad row, disjoint from those rows.
__global__ void zpad_zero_kernel(double *__restrict__ Zc, int T, int pz, int64_t zrs, int nb) {
  const int npad = ((T + 15) & ~15) - T;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)nb * pz * npad) return;
  const int rep = (int)(i / (pz * npad)), e = (int)(i - (int64_t)rep * (pz * npad));
  Zc[zrm_ix(rep, T + e % npad, e / npad, pz, zrs)] = 0.0;
}

// The kernel instances eig_run_fact2_t launches.  stg: the loaders staged through LDS (y2_load's STG, the middle
// steps' FAST), which exist for P = 16 only.  hf, zf, nopf: boot_cheb_mid_kernel's HF, ZF and NOPF; the four (hf, zf)
// pairs are the ones a consistent FilterPlan holds.  zplanes: the planes of a Split Z, an instance (ZPL) at P = 32.
template <int P>
static auto y2_instance(bool stg) { return stg ? boot_y2_kernel<P, P == 16> : boot_y2_kernel<P, false>; }
template <int P>
static auto cheb_instance(bool stg) { return stg ? boot_cheb_kernel<P, P == 16> : boot_cheb_kernel<P, false>; }
template <int P, bool FAST, bool NOPF>
static auto cheb_mid_pair(HzFmt hf, ZFmt zf, int zplanes) {
  if (hf == HzFmt::Rows64) return boot_cheb_mid_kernel<P, FAST, HzFmt::Rows64, ZFmt::F64, NOPF>;
  if (zf == ZFmt::F32) return boot_cheb_mid_kernel<P, FAST, HzFmt::Chunk32, ZFmt::F32, NOPF>;
  if (zf == ZFmt::F64) return boot_cheb_mid_kernel<P, FAST, HzFmt::Chunk32, ZFmt::F64, NOPF>;
  if constexpr (P == 16) {
    return boot_cheb_mid_kernel<P, FAST, HzFmt::Chunk32, ZFmt::Split, NOPF>;   // (planes: the argument)
  } else {
    if (zplanes == 2) return boot_cheb_mid_kernel<P, FAST, HzFmt::Chunk32, ZFmt::Split, NOPF, 2>;
    return boot_cheb_mid_kernel<P, FAST, HzFmt::Chunk32, ZFmt::Split, NOPF, 3>;
  }
}
template <int P>
static auto cheb_mid_instance(bool stg, HzFmt hf, ZFmt zf, bool nopf, int zplanes) {
  constexpr bool F = P == 16;
  if (!nopf) return !stg ? cheb_mid_pair<P, false, false>(hf, zf, zplanes) : cheb_mid_pair<P, F, false>(hf, zf, zplanes);
  return !stg ? cheb_mid_pair<P, false, true>(hf, zf, zplanes) : cheb_mid_pair<P, F, true>(hf, zf, zplanes);
}

template <int P>
static int eig_run_fact2_t(const FactBase &fb, const EigArgs &a, const FactArgs &f) {
  const int m = fb.T, nb = a.nb, k = a.k, p = a.p, maxit = a.maxit, poll = a.poll;
  const int32_t *idx = f.idx;
  const double *eta = f.eta;
  int *off = f.off, *lst = f.lst;
  const PollBuf *pb = f.pb;
  hipStream_t st = a.st;
  // Step 0's schedule, kernels and formats (dfm_fact_plan.h): one plan, checked before the first launch
  const FactSwitches sw = read_fact_switches();
  FilterPlanIn pin;
  pin.warm = a.warm; pin.kw = a.kw; pin.k = k; pin.p = p; pin.P = P; pin.r = fb.r; pin.T = m; pin.maxit = maxit;
  pin.tol = a.tol; pin.spread = f.spread; pin.lamk = f.lamk; pin.fscale = f.fscale;
  pin.has_H32 = fb.H32 != nullptr; pin.has_Hs = fb.Hs != nullptr; pin.hmax = fb.hmax;
  const FilterPlan plan = plan_first_filter(pin, sw);
  if (!plan.consistent()) return 1003;
  const bool warm_started = plan.warm_started, mid = plan.mid, skip0 = plan.skip0, stg_ok = plan.stg_ok, nopf = plan.nopf;
  const int d0 = plan.d0;
  EigWork w = carve(a.ws, m, nb, P, maxit);
  w.subspace = a.subspace;
  w.no_vectors = a.Uk == nullptr;
  // Z / HZ hold pz = p rounded up to even columns per replicate (the GEMM's
  // 16-byte DMA pairs): the H.Z GEMM's work scales with the block p, not P
  const int pz = (p + 1) & ~1;
  // (measured and rejected: Z / HZ rows padded to 128-B lines cut the H.Z GEMM's FETCH_SIZE 0.40 -> 0.32 GB per
  // launch — unpadded, a 512-B tile row straddles five lines, one shared with another XCD's column block — but left
  // the GEMM's time unchanged and slowed the gathering passes 2-4 % with an even or an odd number of lines per row:
  // C3 15.09 -> 15.27-15.38 ms)
  const int ncz = nb * pz;
  const int64_t ldz = ncz;           // HZ: T x nb pz, column-interleaved (rows gathered by idx)
  const int64_t zrs = z_rows(m) * pz;   // Z: replicate-major 16-row chunks (zrm_ix), nb zrs <= z_rows ldz
  // the per-replicate T-row buffers (Q, Y, V0 in U, PV in S, the warm start Q0) hold compact rows of ps = pz columns
  // (columns >= p are zero, so the register layouts' columns ps..P-1 load as zero and are never stored): ~20 % fewer
  // bytes in the per-replicate passes at C3 (P = 16, pz = 12). Replicate slots keep the P-column stride (T P
  // doubles), so a retired replicate's final Ritz vectors (U, row stride P, eig_final_kernel) never overlap another
  // replicate's compact rows.
  const int ps = pz;
  const FactWsLayout wl = fact_ws_layout(m, nb, P, pz);
  auto ws_at = [&](size_t o) { return (double *)(f.fws + o); };
  double *Zc = ws_at(wl.Z), *HZ = ws_at(wl.HZ), *ab = ws_at(wl.ab);
  // the middle Horner steps' operands
  double *PFb = ws_at(wl.PF), *E2b = ws_at(wl.e2), *FVb = ws_at(wl.FV), *FtF = ws_at(wl.FtF);
  // dynamic LDS of ap2 and of the last Horner step (eta, idx, CSR: 20 T bytes)
  const size_t ap2_lds = (size_t)m * 8 + (size_t)(2 * m + 1) * 4;
  const size_t cheb_lds = (size_t)m * 8 + (size_t)(3 * m + 1) * 4;
  {   // counters and flags: one launch
    ZeroSpans zs{};
    zs.p[0] = w.active; zs.n[0] = maxit + 2;
    zs.p[1] = w.iters; zs.n[1] = nb;
    zs.p[2] = w.done; zs.n[2] = nb;
    if (launch_zero_spans(zs, st) != hipSuccess) return 1001;
  }
  const uint64_t seed = 0x5eed0000ull + (uint64_t)m * 131 + k;
  double *cur = w.Q, *alt = w.Y;
  // One stream-ordered block of the solve's own:
  //   Q0      the warm start, the same for every replicate: ONE m x P block,
  //           read with replicate stride 0 by prep and the first step's y2 /
  //           ap2 (L2-resident) instead of nb materialised copies
  //   apre    a = F'Q0 (16 x P), the same for every replicate (prep_a_kernel)
  //   alist   straggler phase (< 1/8 of the batch active at a poll): the GEMMs
  //           tile only the listed replicates' column groups (nb ints; list
  //           built once, a superset of the later active sets; replicates
  //           retired since are computed and ignored)
  //   acount  its length (4 ints)
  struct { size_t Q0, apre, alist, acount, total; } ql;
  ql.Q0 = 0;
  ql.apre = ql.Q0 + (size_t)m * P * 8;
  ql.alist = ql.apre + (size_t)16 * P * 8;
  ql.acount = ql.alist + (size_t)nb * 4;
  ql.total = ql.acount + 4 * 4;
  char *qblk = nullptr;
  if (stream_malloc((void **)&qblk, ql.total, st) != hipSuccess) return 1002;
  double *Q0 = (double *)(qblk + ql.Q0), *apre = (double *)(qblk + ql.apre);
  int *alist = (int *)(qblk + ql.alist), *acount = (int *)(qblk + ql.acount);
  bool cl_on = false;
  struct Q0Free { char *q; hipStream_t s; ~Q0Free() { hipFreeAsync(q, s); } } q0free{qblk, st};
  const double *qin = Q0;
  int64_t qs = 0;
  const double bfix = kWarmFixBeta * f.lamk;   // the filter-only step's interval end
  auto chk = cheb_instance<P>(stg_ok);
  auto y2k = y2_instance<P>(stg_ok);
  // dynamic LDS above the default 64 KB cap: prep (24 T + 8 bytes) for T > 2730, the last Horner step (20 T + 4)
  // for T > 3276, ap2 (16 T + 4) at T = F2_T_MAX.  A refused cap is this solve's error, not a later launch's.
  const size_t prep_lds = (size_t)((4 * m + 3) & ~1) * 4 + (size_t)m * 8;
  {
    hipError_t e = hipSuccess;
    if (prep_lds > 65536)
      e = hipFuncSetAttribute((const void *)boot_prep_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)prep_lds);
    if (e == hipSuccess && cheb_lds > 65536)
      e = hipFuncSetAttribute((const void *)chk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cheb_lds);
    if (e == hipSuccess && ap2_lds > 65536)
      e = hipFuncSetAttribute((const void *)boot_ap2_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ap2_lds);
    if (e != hipSuccess) return 1000 + (int)e;
  }
  { TimerScope ts(a, DFM_KC_EIG_OTHER);
    const int64_t n = (int64_t)m * P;
    dim3 grid((unsigned)((n + 255) / 256), 1);
    hipLaunchKernelGGL(eig_init_kernel<P>, grid, dim3(256), 0, st, Q0, m, p, a.warm, a.kw, w.done, seed, (int64_t)0, ps);
    if (skip0) hipLaunchKernelGGL(q0_guards_kernel, dim3(1), dim3(1024), 0, st, Q0, m, ps, a.kw, p, w.active, nb);
    // the CSR, trace, PF / e2 and the first product's Z0 and ab
    hipLaunchKernelGGL(prep_a_kernel<P>, dim3(1), dim3(64 * BW), 0, st, fb, Q0, ps, apre);
    hipLaunchKernelGGL(boot_prep_kernel<P>, dim3(nb), dim3(64 * BW), prep_lds, st,
                       fb, idx, eta, off, lst, w.trace, mid && !nopf ? PFb : nullptr, mid ? E2b : nullptr, Q0, ps, Zc,
                       ldz, pz, ab, apre,
                       skip0 ? w.S : nullptr, skip0 ? FVb : nullptr, plan.z0, plan.z0_planes);
    if (mid && !fb.FtF) hipLaunchKernelGGL(ftf_kernel, dim3(1), dim3(1024), 0, st, fb, FtF);
  }
  const double *ftf = fb.FtF ? fb.FtF : FtF;
  const double beta0 = warm_started ? sw.beta : 0.0;
  double ca0[kChebDMax + 1], ca1[kChebDMax + 1];
  shifted_cheb(d0, ca0);
  shifted_cheb(kChebD, ca1);
  // One H.Z product for the whole batch, by the kernel the plan names:
  //   F64        HZ = H Z in fp64 rows — listed: for the listed replicates' column groups, once the straggler list is on
  //   F32        HZ32 = H32 Z32 in fp32 (Z32 in the first half of Z's region, HZ32 in HZ's, both in Z's chunk layout;
  //              every replicate is active there: no col_done, no list)
  //   Split      the same HZ32 from the bf16 planes of H and Z, Zs in Z's region at the fp64 replicate stride, as
  //              `terms` plane pairs (FilterPlan::terms)
  //   SplitRows  HZ = hmax HZ32 from the same planes, written as F64 writes it
  // zpad: behind it the fp64 Z's pad rows, which no pass of step 0 wrote, are zeroed for the fp64 products that follow
  auto product = [&](HzProduct kind, bool listed, bool zpad = false, int terms = 0) -> int {
    TimerScope ts(a, DFM_KC_GEMM);
    hipError_t e = hipErrorInvalidValue;
    switch (kind) {
      case HzProduct::F64:
        e = launch_gemm_zrm(fb.H, fb.ldH, Zc, pz, zrs, HZ, ldz, m, ncz, m, st, w.done, listed ? alist : nullptr,
                            listed ? acount : nullptr);
        break;
      case HzProduct::F32:
        e = launch_gemm_zrm_f32(fb.H32, fb.ldH, (const float *)Zc, pz, zrs, (float *)HZ, m, ncz, m, st);
        break;
      case HzProduct::Split:
        e = launch_gemm_zrm_split(fb.Hs, Zc, pz, zrs, (float *)HZ, m, ncz, m, terms, st);
        break;
      case HzProduct::SplitRows:
        e = launch_gemm_zrm_split_rows(fb.Hs, Zc, pz, zrs, HZ, ldz, fb.hmax, m, ncz, m, st);
        break;
    }
    if (e == hipSuccess && zpad) {
      const int64_t n = (int64_t)nb * pz * plan.pad_rows;
      hipLaunchKernelGGL(zpad_zero_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, Zc, m, pz, zrs, nb);
      e = hipGetLastError();
    }
    return e == hipSuccess ? 0 : 1000 + (int)e;
  };
  // a middle Horner step S_i = G* S_{i+1} / b + c V0 in row-local form (Z, a, cc only), reading HZ as hf and
  // writing Z as zf (a Split one with zplanes planes) ...
  auto horner_mid = [&](double c, double bbeta, double bfx, double lead, HzFmt hf = HzFmt::Rows64,
                        ZFmt zf = ZFmt::F64, int zplanes = 0) {
    TimerScope ts(a, DFM_KC_EIG_APPLY);
    hipLaunchKernelGGL(cheb_mid_instance<P>(stg_ok, hf, zf, nopf, zplanes), dim3(nb), dim3(64 * BW), 0, st, fb, w, m, p, HZ, ldz,
                       pz, ab, c, bbeta, k, PFb, E2b, w.S, FVb, ftf, Zc, ps, bfx, lead, fb.hmax, f.fscale, zplanes);
  };
  // ... and the last one, S_0: the new basis into cur, with its Z, a, cc
  auto horner_last = [&](double c, double bbeta, const double *V0, int64_t v0s, double bfx) {
    TimerScope ts(a, DFM_KC_EIG_APPLY);
    hipLaunchKernelGGL(chk, dim3(nb), dim3(64 * BW), cheb_lds, st, fb, w, m, p, idx, eta, off, lst, HZ, ldz, pz, ab, c,
                       bbeta, k, cur, Zc, ps, V0, v0s, bfx);
  };

  // Convergence polls from the step most replicates retire at (first_poll) on.  After each such step the device
  // rebuilds the list of active replicates (the GEMMs compact to it once it holds < 1/8 of the batch, decided on the
  // device, so no host round trip sits in front of the straggler phase) and, with a pinned read-back buffer, the
  // active count is copied to host[it] behind an event.  Outside the tail the host does not wait for it: it queues
  // the next step first and reads the previous step's count then (one step of look-ahead — the GPU always has a step
  // queued while the host decides; a step queued after the last replicate retired runs as a no-op and counts for
  // nothing, its active count being 0).  In the straggler tail each step is short and most likely the last, so the
  // count is awaited before the step's Chebyshev products, as a blocking poll (queued no-op steps cost more than the
  // wait: 2.50 -> 2.58 ms per 1 250-replicate shard with look-ahead throughout).  Without the buffer: a blocking poll
  // every `poll` steps, every step in the tail.
  const int first_poll = warm_started ? 1 : poll - 1;
  const bool ahead = pb && pb->host && pb->cap >= maxit + 2;
  const bool probe = !sw.ap2_probe_off;
  int it = 0, last_gemm = -1, last_cheb = -1, next_poll = first_poll, pend = -1, steps = -1;
  bool tail = false;
  if (skip0) {
    // Filter alone: step 0 without its Rayleigh-Ritz step.  S_d = a_d Q0 (prep left the Z, a, cc, PV, FV of Q0; a_d
    // goes into the first step's scale), d0 products, the last step writes the new basis into cur with its Z, a, cc
    // (the kernels of the products and the formats between them: plan, dfm_fact_plan.h)
    for (int sp = 1; sp <= d0; ++sp) {
      if (int rc = product(plan.product[sp], false, sp == d0 && plan.zero_zpad, plan.terms[sp])) return rc;
      if (sp < d0)
        horner_mid(ca0[d0 - sp], 0.0, bfix, sp == 1 ? ca0[d0] : 1.0, plan.mid_in[sp], plan.mid_out[sp],
                   plan.mid_planes[sp]);
      else horner_last(ca0[0], 0.0, Q0, 0, bfix);
    }
    last_gemm = last_cheb = 0;
    qin = cur;
    qs = (int64_t)m * P;
    it = 1;
  }
  for (; it < maxit; ++it) {
    const int dg = it == 0 ? d0 : kChebD;
    const double *ca = it == 0 ? ca0 : ca1;
    const double bb = it == 0 ? beta0 : 0.0;
    hipError_t e;
    // Rayleigh-Ritz step: Y = G* Q, the p x p problem, U / residuals / the next product's operands
    if (int rc = product(HzProduct::F64, cl_on)) return rc;
    last_gemm = it;
    { TimerScope ts(a, DFM_KC_EIG_GQ);
      hipLaunchKernelGGL(y2k, dim3(nb), dim3(64 * BW), (size_t)m * 12, st, fb, w, m, idx, eta, HZ, ldz, pz,
                         ab, qin, qs, alt, ps);
    }
    { TimerScope ts(a, DFM_KC_EIG_SMALL);
      hipLaunchKernelGGL(eig_small_kernel<P>, dim3(nb), dim3(64), 0, st, w, p, 1, kJacobiSweeps);
    }
    { TimerScope ts(a, DFM_KC_EIG_APPLY);
      if (mid && it == 0 && it < maxit - 1)   // before ap2 overwrites Z(Q) and a(Q)
        hipLaunchKernelGGL(boot_pv_kernel<P>, dim3(nb), dim3(64 * BW), 0, st, fb, w, m, p, it, eta, off, lst, Zc, ldz,
                           pz, ab, seed, w.S, FVb, ps);
      hipLaunchKernelGGL(boot_ap2_kernel<P>, dim3(nb), dim3(64 * BW), ap2_lds, st, fb, w, m, k, p, a.tol, it,
                         it == maxit - 1 ? 1 : 0, ca[dg], ca[dg - 1], bb, eta, off, lst, qin, qs, alt, Zc, ldz, pz, ab,
                         seed, ps, probe && it >= first_poll ? 1 : 0);
    }
    if (it >= first_poll) {
      if (ahead) {
        if ((e = hipMemcpyAsync(pb->host + it, w.active + it, 4, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipEventRecord(pb->ev[it & 1], st)) != hipSuccess)
          return 1000 + (int)e;
      }
      hipLaunchKernelGGL(active_list_kernel, dim3(1), dim3(1024), 0, st, w.done, nb, alist, acount);
      cl_on = true;
      if (ahead) {
        if (pend >= 0) {   // the previous step's count: this step is already queued behind it
          if ((e = hipEventSynchronize(pb->ev[pend & 1])) != hipSuccess) return 1000 + (int)e;
          const int act = pb->host[pend];
          if (act == 0) { steps = pend + 1; ++it; break; }   // (this step ran as a no-op)
          tail = (int64_t)act * 8 < nb;
          pend = -1;
        }
        if (tail) {   // in the straggler tail: this step's count now, before its Chebyshev products
          if ((e = hipEventSynchronize(pb->ev[it & 1])) != hipSuccess) return 1000 + (int)e;
          const int act = pb->host[it];
          if (act == 0) { ++it; break; }
        } else {
          pend = it;
        }
      } else if (it == next_poll) {
        int act = -1;
        hipMemcpyAsync(&act, w.active + it, 4, hipMemcpyDeviceToHost, st);
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return 1000 + (int)e;
        if (act == 0) { ++it; break; }
        next_poll = it + ((int64_t)act * 8 < nb ? 1 : poll);
      }
    }
    if (it < maxit - 1) {
      // Filter: d - 1 products G* S_{i+1} and Horner steps S_i, i = d-2 .. 0: the new
      // basis S_0 goes back into cur (Q), Y stays in alt
      for (int sp = 2; sp <= dg; ++sp) {
        if (int rc = product(HzProduct::F64, cl_on)) return rc;
        if (mid && it == 0 && sp < dg) horner_mid(ca[dg - sp], bb, 0.0, 1.0);
        else horner_last(ca[dg - sp], bb, w.U, (int64_t)m * P, 0.0);
      }
      last_cheb = it;
    } else {
      std::swap(cur, alt);
    }
    qin = cur;
    qs = (int64_t)m * P;
  }
  if (steps < 0) steps = it;
  g_last_iters = steps;
  g_last_gemm_products_f32 = (int64_t)plan.products_f32 * nb;
  g_last_gemm_products_split_last = (int64_t)plan.products_split_last * nb;
  g_last_gemm_products_split3 = (int64_t)plan.products_split3 * nb;
  // the Chebyshev GEMM of iteration it runs after that iteration's check
  if (f.cnt) {   // (counted by eig_final_kernel below)
    g_last_rep_iters = g_last_gemm_products = 0;
  } else {
    g_last_rep_iters = count_rep_iters(w.active, last_gemm, 1, nb, st);
    const int64_t c0 = count_rep_iters(w.active, std::min(last_cheb, 0), 0, nb, st);
    const int64_t call = count_rep_iters(w.active, last_cheb, 0, nb, st);
    g_last_gemm_products = g_last_rep_iters + c0 * (d0 - 1) + (call - c0) * (kChebD - 1);
    if (skip0 && last_gemm >= 0) g_last_rep_iters -= nb;   // (step 0's first product belongs to no Rayleigh-Ritz step)
  }
  { TimerScope ts(a, DFM_KC_EIG_OTHER);
    hipLaunchKernelGGL(eig_final_kernel<P>, dim3(nb), dim3(256), 0, st, w, m, k, a.lam, a.Uk, a.status, a.trace_out,
                       f.cnt, last_gemm, last_cheb, d0 - 1, kChebD - 1, skip0 ? 1 : 0);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return 1000 + (int)e;
  return 0;
}

int eig_run_factored(const FactBase &fb, const EigArgs &a, const FactArgs &f) {
  // (r > 16 or T > F2_T_MAX: callers take the direct path)
  if (a.p < a.k || a.p > 32 || a.p > fb.T || fb.r > 16 || fb.T > F2_T_MAX) return -1;
  if (a.p <= 16) return eig_run_fact2_t<16>(fb, a, f);
  return eig_run_fact2_t<32>(fb, a, f);
}
int fact_t_max() { return F2_T_MAX; }

}  // namespace dfm
